// h2s_debug.hip — the CPU chain's debug instances of k_tile (h2s_debug_float).
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(debug)
