// Wave-per-problem kernels of the Acrobot model with control limits (Limited<Acrobot>): every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

MI_INTERNAL int launch_acrobot_lim(mi_ilqr* h, int mode, const mi::KArgs& a) { return mi_host::launch_limited<mi::Acrobot>(h, mode, a); }
