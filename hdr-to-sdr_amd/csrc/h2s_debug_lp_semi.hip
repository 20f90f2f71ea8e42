// h2s_debug_lp_semi.hip — the libplacebo branch's debug instances of k_tile
// (DBG = 1, as h2s_debug.hip) for semi-planar input.
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(1, 1, true)

}  // namespace h2s
