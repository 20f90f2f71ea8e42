// h2s_repack.h — what k_repack420 (h2s_repack.hip) and its host side
// (h2s_api_ladder.hip) share: the launch record of a rendition ladder's
// source-size rung (h2s_process_ladder).
#pragma once
#include <stdint.h>

namespace h2s {

constexpr int REPACK_THREADS = 256;
constexpr int REPACK_ROWS = 4;      // rows of its 16-byte column a lane copies: that many loads in flight

// One entry of a launch: a plane of the scratch (np 1), or its two chroma
// planes that share one interleaved destination (np 2, semi-planar: element x
// of a destination row is the pair (Cb, Cr)).  A source row is row_bytes bytes,
// nch 16-byte chunks (the last may be ragged: the scratch's rows are padded to
// 16 bytes, so it is loaded whole and stored in part)
struct RepackPlane {
  const uint8_t* src[2];
  long long sls, sfp;
  uint8_t* dst;
  long long dls, dfp;
  int row_bytes, rows;
  int nch, nblk;     // chunks of a row; blocks of the entry in one frame
  int np;
};

struct RepackParams {
  RepackPlane pl[3];
  int nplanes;
  int sh;            // a semi-planar 16-bit word carries the code in its high bits (16 - bits; else 0)
  int vec_out;       // every destination row start is 16-byte aligned
};

}  // namespace h2s
