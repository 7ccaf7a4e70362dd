// Plant kernels with process and actuation noise (plant_advance.hpp, NZ = true) of every built-in model: a unit of their own
// beside k_plant.hip, so that the two build in parallel.
#include "plant_advance.hpp"

template int mi_host::launch_plant_advance_noise<mi::Pendulum>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance_noise<mi::Acrobot>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance_noise<mi::CartPole>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance_noise<mi::CartPoleWall>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance_noise<mi::Synth36>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance_noise<mi::PlanarQuad>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance_noise<mi::Quad3D>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance_noise<mi::Arm27>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance_noise<mi::Arm27C>(mi_ilqr*, const mi_host::PlantArgs&);
