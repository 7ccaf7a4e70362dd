// Wave-per-problem kernels of the Acrobot model with control limits (Limited<Acrobot>): every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

template int mi_host::launch_limited<mi::Acrobot>(mi_ilqr*, int, const mi::KArgs&);
