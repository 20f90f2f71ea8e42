// h2s_fast_lp_tl.hip — the libplacebo branch's product instances of k_tile for top-left 4:2:0 input.
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(fast_lp_tl)
