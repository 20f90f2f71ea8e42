// h2s_fast_sub422.hip — the CPU chain's product instances of the tile kernel
// for 4:2:2 input (k_tile<..., SEMI = true, SUB = 1>: yuv422p10le / 12le in,
// h2s_set_input_subsampling; planar or semi-planar 4:2:0 out), apart from the
// 4:2:0 ones so that those stay exactly what they were (h2s_tile.h).
#include <hip/hip_runtime.h>

#include "h2s_tile.h"

namespace h2s {

H2S_TILE_INSTANCE(0, 0, true, 1)

}  // namespace h2s
