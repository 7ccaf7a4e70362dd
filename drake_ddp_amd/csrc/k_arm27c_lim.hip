// Workgroup-per-problem kernels of the Arm27C model with control limits (Limited<Arm27C>: the mid-size family's box-QP backward pass and
// clamped rollouts): every (Jacobian mode, kernel mode) instantiation.
#include "launch_large.hpp"

template int mi_host::launch_jac_large_limited<mi::Arm27C>(mi_ilqr*, int, const mi::KArgs&);
