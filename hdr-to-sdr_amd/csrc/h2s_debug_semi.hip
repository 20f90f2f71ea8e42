// h2s_debug_semi.hip — the CPU chain's debug instances of k_tile (DBG = 1, as
// h2s_debug.hip) for semi-planar input (h2s_debug_float under
// h2s_set_frame_layout).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(1, 0, true)

}  // namespace h2s
