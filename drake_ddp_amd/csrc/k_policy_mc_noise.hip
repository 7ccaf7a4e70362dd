// On-device Monte-Carlo kernels with process and actuation noise (policy_mc.hpp, NZ = true) of every built-in model: a unit of
// their own beside k_policy_mc.hip, so that the two build in parallel.
#include "policy_mc.hpp"

template int mi_host::launch_policy_mc_noise<mi::Pendulum>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc_noise<mi::Acrobot>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc_noise<mi::CartPole>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc_noise<mi::CartPoleWall>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc_noise<mi::Synth36>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc_noise<mi::PlanarQuad>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc_noise<mi::Quad3D>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc_noise<mi::Arm27>(mi_ilqr*, const mi_host::PolicyMcArgs&);
template int mi_host::launch_policy_mc_noise<mi::Arm27C>(mi_ilqr*, const mi_host::PolicyMcArgs&);
