// h2s_debug_semi.hip — the CPU chain's debug instances of k_tile for semi-planar frame sets.
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(debug_semi)
