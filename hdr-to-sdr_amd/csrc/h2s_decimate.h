// h2s_decimate.h — what k_decimate420 (h2s_decimate.hip) and its host side
// (h2s_api_decimate.hip) share: the launch record of the 4:2:0 front-end
// (h2s_set_input_decimation) and the shape of a wave's piece of work.
#pragma once
#include <stdint.h>

namespace h2s {

constexpr int DEC_THREADS = 256;    // four waves, each with a piece of its own (no block barrier)
constexpr int DEC_CHUNK = 8;        // 16-bit words of a lane's 16-byte chunk of a source chroma row
constexpr int DEC_ROWS_STEP = 4;    // a run's output rows are a multiple of this (the 8-row window's period)
constexpr int DEC_ROWS_MAX = 32;    // output rows of a run at the most: 70 source rows read for 64
constexpr int DEC_ROWS_MIN = 4;

// the chunks of a source row that one wave turns into output: every lane's
// (4:2:2: the vertical pass alone), or all but the two edge lanes', which load
// the horizontal pass's halo (4:4:4)
__host__ __device__ constexpr int dec_wave_chunks(int sub444) { return sub444 ? 62 : 64; }

// One launch: the chroma of nframes frames.  A source plane is `rows` rows of
// `nw` 16-bit words (planar: one word a sample; semi-planar: the (Cb, Cr) pairs
// of the one interleaved plane, two words a sample); the output plane has
// rows / 2 rows of `onw` words (4:2:2: nw; 4:4:4: nw / 2).  A word holds its
// code shifted left by sh (semi-planar: 16 - bits), in and out
struct DecimateParams {
  const uint8_t* src[2];
  uint8_t* dst[2];
  long long sls, sfp;      // source row and frame pitch, bytes
  long long dls, dfp;      // output row and frame pitch (rows 16-byte aligned and padded to 16 bytes)
  int nplanes;             // 2 planar, 1 semi-planar
  int nw, onw, rows;
  int sh, vmax;            // 2^bits - 1
  int vec;                 // every source row start is 16-byte aligned
  int run;                 // output rows of a run (a multiple of DEC_ROWS_STEP)
  int nstrips, nruns;      // wave pieces of one plane: strips across x runs down
  float wx[7], wy[8];      // chroma_taps (h2s_resolve.hip)
};

}  // namespace h2s
