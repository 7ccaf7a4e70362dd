// The multi-start kernel (seeds.hpp: a handle read as groups of K seeds - draw the guesses, pick the best member, reseed around it,
// gather the winners) and its launcher: no model templates, one translation unit for every model.
#include "seeds.hpp"
