// h2s_fast_sub444.hip — the CPU chain's product instances of k_tile for 4:4:4 input.
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(fast_sub444)
