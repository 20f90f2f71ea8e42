// h2s_fast_lp.hip — the libplacebo branch's product instances of k_tile: their own unit, so that they compile
// with LLVM's default scheduler, 2-3 % faster for them (profiles/r03/ablations/fast_body_scheduler_*.log).
#include "h2s_tile_sets.h"

H2S_TILE_UNIT(fast_lp)
