// h2s_fast_dbg34_semi.hip — debug instances of k_tile (h2s_stage 3, 4) for
// semi-planar input (h2s_debug_float under h2s_set_frame_layout).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(3, 0, true)
H2S_TILE_INSTANCE(3, 1, true)
H2S_TILE_INSTANCE(4, 0, true)
H2S_TILE_INSTANCE(4, 1, true)

}  // namespace h2s
