// Wave-per-problem kernels of the CartPoleWall model with control limits (Limited<CartPoleWall>): every (Jacobian mode, kernel mode) instantiation.
#include "launch_small.hpp"

MI_INTERNAL int launch_cartpole_wall_lim(mi_ilqr* h, int mode, const mi::KArgs& a) { return mi_host::launch_limited<mi::CartPoleWall>(h, mode, a); }
