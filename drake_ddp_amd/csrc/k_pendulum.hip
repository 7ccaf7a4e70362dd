// Wave-per-problem kernels of the Pendulum model: every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

template int mi_host::launch_jac<mi::Pendulum>(mi_ilqr*, int, const mi::KArgs&);
