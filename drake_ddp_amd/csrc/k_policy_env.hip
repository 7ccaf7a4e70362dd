// The on-device Monte-Carlo's envelope and safety-box kernels (policy_env.hpp: per-row statistics over the samples, one lane per
// sample against a box) and their launchers: no model templates, one translation unit for every model.
#include "policy_env.hpp"
