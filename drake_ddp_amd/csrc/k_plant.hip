// Plant kernels of the closed MPC loop (plant_advance.hpp: one lane per problem) of every built-in model: one translation unit.
#include "plant_advance.hpp"

template int mi_host::launch_plant_advance<mi::Pendulum>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance<mi::Acrobot>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance<mi::CartPole>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance<mi::CartPoleWall>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance<mi::Synth36>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance<mi::PlanarQuad>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance<mi::Quad3D>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance<mi::Arm27>(mi_ilqr*, const mi_host::PlantArgs&);
template int mi_host::launch_plant_advance<mi::Arm27C>(mi_ilqr*, const mi_host::PlantArgs&);
