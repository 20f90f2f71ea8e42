// h2s_fast_lp_tl.hip — the libplacebo branch's product instances of the tile
// kernel for 4:2:0 input whose chroma is sited top-left (k_tile<..., LP = 1, 0,
// SEMI = true, SUB = 3>: h2s_set_input_tags, H2S_CHROMA_TOPLEFT; planar or
// semi-planar on either side).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(0, 1, true, 3)

}  // namespace h2s
