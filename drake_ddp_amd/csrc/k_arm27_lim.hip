// Workgroup-per-problem kernels of the Arm27 model with control limits (Limited<Arm27>: the mid-size family's box-QP backward pass and
// clamped rollouts): every (Jacobian mode, kernel mode) instantiation.
#include "launch_large.hpp"

template int mi_host::launch_jac_large_limited<mi::Arm27>(mi_ilqr*, int, const mi::KArgs&);
