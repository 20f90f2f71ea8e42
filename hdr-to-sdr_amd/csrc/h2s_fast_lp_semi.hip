// h2s_fast_lp_semi.hip — the libplacebo branch's product instances of k_tile for semi-planar frame sets.
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(fast_lp_semi)
