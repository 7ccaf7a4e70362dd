// Workgroup-per-problem kernels of the PlanarQuad model: every (Jacobian mode, kernel mode) instantiation.
#include "launch_large.hpp"

template int mi_host::launch_jac_large<mi::PlanarQuad>(mi_ilqr*, int, const mi::KArgs&);
