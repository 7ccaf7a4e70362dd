// Wave-per-problem kernels of the CartPoleWall model with control limits (Limited<CartPoleWall>): every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

template int mi_host::launch_limited<mi::CartPoleWall>(mi_ilqr*, int, const mi::KArgs&);
