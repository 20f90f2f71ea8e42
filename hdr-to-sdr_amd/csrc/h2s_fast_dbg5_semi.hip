// h2s_fast_dbg5_semi.hip — debug instances of k_tile (h2s_stage 5) for
// semi-planar input (h2s_debug_float under h2s_set_frame_layout).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(5, 0, true)
H2S_TILE_INSTANCE(5, 1, true)

}  // namespace h2s
