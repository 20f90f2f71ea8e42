// h2s_fast_lp_dv_semi.hip — the tile kernel's Dolby Vision profile-5 product instances for semi-planar frame sets
// (k_tile<2, TM, 0, 1, ...>: the libplacebo branch's five operators), in a
// translation unit of their own so that the parallel build stays parallel.
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_DV_INSTANCE(0, true)

}  // namespace h2s
