// h2s_fast_sub422.hip — the CPU chain's product instances of k_tile for 4:2:2 input.
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(fast_sub422)
