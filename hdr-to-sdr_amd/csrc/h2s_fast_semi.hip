// h2s_fast_semi.hip — the CPU chain's product instances of the tile kernel
// for semi-planar frame sets (k_tile<..., SEMI = true>: nv12 / p010le / p012le
// on either side, h2s_set_frame_layout), apart from the planar ones so that
// those stay exactly what they were (h2s_tile.h).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(0, 0, true)

}  // namespace h2s
