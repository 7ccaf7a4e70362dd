// Wave-per-problem kernels of the Pendulum model with control limits (Limited<Pendulum>): every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

MI_INTERNAL int launch_pendulum_lim(mi_ilqr* h, int mode, const mi::KArgs& a) { return mi_host::launch_limited<mi::Pendulum>(h, mode, a); }
