// On-device Monte-Carlo kernels (policy_mc.hpp: sampled starts, one lane per sample, per-problem statistics) of every built-in
// model, without noise: one translation unit.
#include "policy_mc.hpp"

template int mi_host::launch_policy_mc<mi::Pendulum>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc<mi::Acrobot>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc<mi::CartPole>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc<mi::CartPoleWall>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc<mi::Synth36>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc<mi::PlanarQuad>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc<mi::Quad3D>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc<mi::Arm27>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc<mi::Arm27C>(mi_ilqr*, const mi_host::PolicyMcArgs&);
