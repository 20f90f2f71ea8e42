// h2s_fast_semi.hip — the CPU chain's product instances of k_tile for semi-planar frame sets.
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(fast_semi)
