// h2s_fast_lp_dv.hip — the Dolby Vision profile-5 product instances of k_tile.
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(fast_lp_dv)
