// Workgroup-per-problem kernels of the Synth36 model: every (Jacobian mode, kernel mode) instantiation.
#include "launch_large.hpp"

template int mi_host::launch_jac_large<mi::Synth36>(mi_ilqr*, int, const mi::KArgs&);
