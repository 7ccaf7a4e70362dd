// Policy-rollout kernels (policy_rollout.hpp: one lane per sample) of every built-in model: one translation unit.
#include "policy_rollout.hpp"

template int mi_host::launch_policy_rollout<mi::Pendulum>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout<mi::Acrobot>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout<mi::CartPole>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout<mi::CartPoleWall>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout<mi::Synth36>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout<mi::PlanarQuad>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout<mi::Quad3D>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout<mi::Arm27>(mi_ilqr*, const mi_host::PolicyArgs&);
template int mi_host::launch_policy_rollout<mi::Arm27C>(mi_ilqr*, const mi_host::PolicyArgs&);
