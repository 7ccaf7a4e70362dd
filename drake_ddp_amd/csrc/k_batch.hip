// Lane-per-problem ("throughput") kernels of every small-state model: one translation unit.
#include "launch_batch.hpp"

template int mi_host::launch_batch<mi::Pendulum>(mi_ilqr*, int, const mi::KArgs&);
template int mi_host::launch_batch<mi::Acrobot>(mi_ilqr*, int, const mi::KArgs&);
template int mi_host::launch_batch<mi::CartPole>(mi_ilqr*, int, const mi::KArgs&);
template int mi_host::launch_batch<mi::CartPoleWall>(mi_ilqr*, int, const mi::KArgs&);
