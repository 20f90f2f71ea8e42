// h2s_fast_tl.hip — the CPU chain's product instances of the tile kernel for
// 4:2:0 input whose chroma is sited top-left (k_tile<..., SEMI = true, SUB = 3>:
// h2s_set_input_tags, H2S_CHROMA_TOPLEFT; planar or semi-planar on either
// side), apart from the left-sited ones so that those stay exactly what they
// were (h2s_tile.h).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(0, 0, true, 3)

}  // namespace h2s
