// h2s_scale.h — what k_scale420 (h2s_scale.hip) and its host side
// (h2s_api_scale.hip) share: the launch record of the scaled 4:2:0 output and
// the LDS budget both sides size their pieces from.
#pragma once
#include <stdint.h>

namespace h2s {

constexpr int SCALE_COLS = 64;         // output columns of a block's strip
constexpr int SCALE_THREADS = 256;     // four waves: a group of source rows each in the horizontal pass
constexpr int SCALE_MAX_ROWS = 48;     // output rows a block owns at the most
constexpr int SCALE_SEG = 848;         // source samples one wave stages of a row: 63 * 12 + 1 + 49 taps at the ratio
                                       // limit, and a 16-byte chunk's slack at either end
constexpr int SCALE_LDS = 32 * 1024;   // the whole of a block's LDS at the most: at least four blocks a CU
constexpr int SCALE_LDS_SMALL = 24 * 1024;   // what the host prefers (six blocks a CU: measured faster at 2 : 1 and
constexpr int SCALE_ROWS_SMALL = 8;          // 3 : 1) while it still leaves a block this many rows

// the pieces of a block's LDS, in bytes (each a multiple of 16): the four
// waves' source segments, the strip's weights (tap-major), the quantised
// output tile and the horizontal results of `hrows` source rows
struct ScaleLds {
  int wt, ot, hb, total;
};
__host__ __device__ inline ScaleLds scale_lds(int src_bps, int Tx, int rows, int np, int out_bps, int hrows) {
  ScaleLds l;
  l.wt = 4 * SCALE_SEG * src_bps;
  l.ot = l.wt + SCALE_COLS * Tx * 4;
  l.hb = l.ot + (rows * SCALE_COLS * np * out_bps + 15) / 16 * 16;
  l.total = l.hb + hrows * SCALE_COLS * 4;
  return l;
}

// One entry of a launch: a plane of the chain's output (np 1), or the two
// chroma planes that share one interleaved destination (np 2, semi-planar:
// element x of a destination row is the pair (Cb, Cr)).  sw x sh source
// samples -> ow x oh; wx / sx: ow x Tx weights and first taps, wy / sy: oh x Ty
struct ScalePlane {
  const uint8_t* src[2];
  long long sls, sfp;
  uint8_t* dst;
  long long dls, dfp;
  int sw, sh, ow, oh;
  const float *wx, *wy;
  const int *sx, *sy;
  int Tx, Ty;
  int np;
  int rows, hrows;   // output rows a block owns; source rows its LDS holds (the host's choice, scale_lds)
  int nsx, nblk;     // strips across, blocks of the entry in one frame
};

struct ScaleParams {
  ScalePlane pl[3];
  int nplanes;
  int src_shift;     // source code = sample >> src_shift (the chain's shift_out)
  int qmax;          // 2^q - 1
  int shift_out, rep_rs;   // S8: (v << shift_out) | (v >> rep_rs); rep_rs 31: a plain shift
  int out_sh;        // a semi-planar 16-bit word carries the code in its high bits
  int out_bps;
  int vec_out;       // every destination row start is 16-byte aligned
};

}  // namespace h2s
