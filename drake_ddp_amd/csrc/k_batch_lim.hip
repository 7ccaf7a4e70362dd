// Lane-per-problem ("throughput") kernels of every small-state model with control limits (Limited<M>): one translation unit.
#include "launch_batch.hpp"

template int mi_host::launch_batch_limited<mi::Pendulum>(mi_ilqr*, int, const mi::KArgs&);
template int mi_host::launch_batch_limited<mi::Acrobot>(mi_ilqr*, int, const mi::KArgs&);
template int mi_host::launch_batch_limited<mi::CartPole>(mi_ilqr*, int, const mi::KArgs&);
template int mi_host::launch_batch_limited<mi::CartPoleWall>(mi_ilqr*, int, const mi::KArgs&);
