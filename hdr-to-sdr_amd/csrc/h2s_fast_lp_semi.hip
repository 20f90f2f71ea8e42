// h2s_fast_lp_semi.hip — the libplacebo branch's product instances of the
// tile kernel for semi-planar frame sets (k_tile<..., LP = 1, 0, SEMI = true>).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(0, 1, true)

}  // namespace h2s
