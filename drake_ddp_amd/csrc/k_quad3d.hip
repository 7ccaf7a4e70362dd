// Workgroup-per-problem kernels of the Quad3D model (n = 37: the split tile layout of ilqr_large.hpp): every (Jacobian mode, kernel mode) instantiation.
#include "launch_large.hpp"

template int mi_host::launch_jac_large<mi::Quad3D>(mi_ilqr*, int, const mi::KArgs&);
