// h2s_debug_lp.hip — the libplacebo branch's debug instances of k_tile (DBG = 1,
// as h2s_debug.hip).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(1, 1, false)

}  // namespace h2s
