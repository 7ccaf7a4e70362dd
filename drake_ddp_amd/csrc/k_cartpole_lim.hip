// Wave-per-problem kernels of the CartPole model with control limits (Limited<CartPole>): every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

MI_INTERNAL int launch_cartpole_lim(mi_ilqr* h, int mode, const mi::KArgs& a) { return mi_host::launch_limited<mi::CartPole>(h, mode, a); }
