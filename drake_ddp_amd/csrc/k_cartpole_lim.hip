// Wave-per-problem kernels of the CartPole model with control limits (Limited<CartPole>): every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

template int mi_host::launch_limited<mi::CartPole>(mi_ilqr*, int, const mi::KArgs&);
