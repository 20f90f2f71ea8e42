// h2s_debug.hip — the CPU chain's debug instances of k_tile (DBG = 1): the tile
// kernel's own arithmetic with the planes of one h2s_stage (F.dbg_stage)
// exported (h2s_debug_float).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(1, 0, false)

}  // namespace h2s
