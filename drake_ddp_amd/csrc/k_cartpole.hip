// Wave-per-problem kernels of the CartPole model: every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

template int mi_host::launch_jac<mi::CartPole>(mi_ilqr*, int, const mi::KArgs&);
