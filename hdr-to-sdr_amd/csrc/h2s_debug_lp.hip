// h2s_debug_lp.hip — the libplacebo branch's debug instances of k_tile.
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(debug_lp)
