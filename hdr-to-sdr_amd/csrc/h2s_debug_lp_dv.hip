// h2s_debug_lp_dv.hip — the tile kernel's Dolby Vision profile-5 debug instances (DBG = 1), planar sets
// (k_tile<2, TM, 0, 1, ...>: the libplacebo branch's five operators), in a
// translation unit of their own so that the parallel build stays parallel.
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_DV_INSTANCE(1, false)

}  // namespace h2s
