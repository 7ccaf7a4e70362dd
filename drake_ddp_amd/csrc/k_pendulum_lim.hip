// Wave-per-problem kernels of the Pendulum model with control limits (Limited<Pendulum>): every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

template int mi_host::launch_limited<mi::Pendulum>(mi_ilqr*, int, const mi::KArgs&);
