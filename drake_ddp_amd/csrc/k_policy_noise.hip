// Policy-rollout kernels with process and actuation noise (policy_rollout.hpp, NZ = true) of every built-in model: a unit of their
// own beside k_policy.hip, so that the two build in parallel.
#include "policy_rollout.hpp"

template int mi_host::launch_policy_rollout_noise<mi::Pendulum>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout_noise<mi::Acrobot>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout_noise<mi::CartPole>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout_noise<mi::CartPoleWall>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout_noise<mi::Synth36>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout_noise<mi::PlanarQuad>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout_noise<mi::Quad3D>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout_noise<mi::Arm27>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout_noise<mi::Arm27C>(mi_ilqr*, const mi_host::PolicyArgs&);
