// h2s_debug_lp_dv.hip — the Dolby Vision profile-5 debug instances of k_tile.
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(debug_lp_dv)
