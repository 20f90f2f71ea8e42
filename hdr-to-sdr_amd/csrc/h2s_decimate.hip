// h2s_decimate.hip — the 4:2:0 front-end (h2s_set_input_decimation): the
// chroma of a 4:2:2 / 4:4:4 set decimated to 4:2:0 into a context scratch, in
// front of the unchanged conversion, [EXT].  The model is S6's swscale-bicubic
// one (chroma_taps, h2s_resolve.hip): 4:4:4 horizontally wx7 on source columns
// 2k-3 .. 2k+3 (left-sited), both vertically wy8 on source rows 2m-3 .. 2m+4
// (centred), indices clamped to the plane, float32 on the integer codes, each
// pass an ascending fmaf chain from 0, v = floor(acc + 0.5) clamped to the
// code range.  Luma is not touched.
//
// A wave owns a strip of 16-byte chunks of a source chroma row (a lane one
// chunk, 8 words) and a run of output rows, and walks down it with a window of
// 8 source rows in registers as floats: two new rows per output row, loaded
// two output rows ahead.  The window's slot of a source row is fixed (row + 3
// mod 8; a run starts at a multiple of 4 output rows), so nothing is moved.
// 4:2:2 is that alone: no LDS, no barrier; a semi-planar chunk is four pairs
// and the arithmetic is the same per word.  4:4:4: the vertically filtered row
// goes to a wave-private LDS row (9 floats a lane: no bank conflicts), and
// each lane sums its 4 output words from it; the strip's two edge lanes load
// the neighbouring chunks (clamped to the row) and write no output, so the
// halo needs no path of its own.  Output rows are the scratch's: 16-byte
// aligned and padded, so every store is a whole non-temporal 16- or 8-byte one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/h2s.h"
#include "h2s_decimate.h"
#include "h2s_launch.h"

namespace h2s {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// LDS written by some lanes of a wave and read by others of the same wave:
// the LDS runs a wave's accesses in order, the compiler must not move them
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// a lane's chunk of source row y (clamped to the plane): one 16-byte load, or
// (rows not 16-byte aligned, the row's ragged last chunk) its words one by one,
// those past the row's end replicated
__device__ __forceinline__ u32x4 load_chunk(const uint8_t* plane, long long sls, int rows, int y, int chunk, bool whole,
                                            int nw) {
  const uint8_t* row = plane + (long long)clampi(y, 0, rows - 1) * sls;
  if (whole) return *reinterpret_cast<const u32x4*>(row + chunk * 16);
  const uint16_t* w = reinterpret_cast<const uint16_t*>(row);
  u32x4 v;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const unsigned lo = w[min(chunk * DEC_CHUNK + 2 * i, nw - 1)], hi = w[min(chunk * DEC_CHUNK + 2 * i + 1, nw - 1)];
    v[i] = lo | (hi << 16);
  }
  return v;
}

__device__ __forceinline__ void codes_of(u32x4 v, int sh, float* f) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    f[2 * i] = (float)((v[i] & 0xFFFFu) >> sh);
    f[2 * i + 1] = (float)(v[i] >> (16 + sh));
  }
}

__device__ __forceinline__ unsigned word_of(float acc, float vmax, int sh) {
  return (unsigned)fminf(fmaxf(floorf(acc + 0.5f), 0.0f), vmax) << sh;
}

}  // namespace

// SUB: H2S_SUB_422 / H2S_SUB_444.  SEMI: the words are (Cb, Cr) pairs
template <int SUB, bool SEMI>
__global__ __launch_bounds__(DEC_THREADS) void k_decimate420(const DecimateParams P) {
  constexpr bool H = SUB == H2S_SUB_444;           // there is a horizontal pass
  constexpr int NOUT = dec_wave_chunks(H);
  constexpr int LROW = 64 * (DEC_CHUNK + 1);       // a wave's LDS row: 9 floats a lane
  __shared__ float lds[H ? DEC_THREADS / 64 * LROW : 1];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int per_plane = P.nstrips * P.nruns;
  const int piece = blockIdx.x * (DEC_THREADS / 64) + wave;
  if (piece >= P.nplanes * per_plane) return;   // (wave-uniform)
  const int plane = piece / per_plane, rem = piece - plane * per_plane;
  const int run = rem / P.nstrips, strip = rem - run * P.nstrips;
  const int frame = blockIdx.y;

  const int nw = P.nw, rows = P.rows, orows = rows >> 1, sh = P.sh;
  const int nchunks = (nw + DEC_CHUNK - 1) / DEC_CHUNK;
  const int c = strip * NOUT + lane - (H ? 1 : 0);   // the lane's chunk of the row; the edge lanes': the halo
  const int lc = clampi(c, 0, nchunks - 1);
  const bool whole = P.vec && lc * DEC_CHUNK + DEC_CHUNK <= nw;
  const uint8_t* src = P.src[plane] + (long long)frame * P.sfp;
  uint8_t* dst = P.dst[plane] + (long long)frame * P.dfp;
  const float vmax = (float)P.vmax;

  const int m0 = run * P.run, mend = min(m0 + P.run, orows);
  float win[8][DEC_CHUNK];   // source row y in slot (y + 3) & 7
  {
    u32x4 raw[6];
#pragma unroll
    for (int t = 0; t < 6; t++) raw[t] = load_chunk(src, P.sls, rows, 2 * m0 - 3 + t, lc, whole, nw);
#pragma unroll
    for (int t = 0; t < 6; t++) codes_of(raw[t], sh, win[t]);
  }
  // the new rows of the next two output rows, in flight
  u32x4 na = load_chunk(src, P.sls, rows, 2 * m0 + 3, lc, whole, nw);
  u32x4 nb = load_chunk(src, P.sls, rows, 2 * m0 + 4, lc, whole, nw);
  u32x4 na2 = load_chunk(src, P.sls, rows, 2 * m0 + 5, lc, whole, nw);
  u32x4 nb2 = load_chunk(src, P.sls, rows, 2 * m0 + 6, lc, whole, nw);

  for (int mb = m0; mb < mend; mb += DEC_ROWS_STEP) {
#pragma unroll
    for (int j = 0; j < DEC_ROWS_STEP; j++) {
      const int m = mb + j;
      if (m >= mend) break;   // (wave-uniform)
      codes_of(na, sh, win[(2 * j + 6) & 7]);
      codes_of(nb, sh, win[(2 * j + 7) & 7]);
      // two output rows ahead (past the run's last: loaded, unused)
      na = na2, nb = nb2;
      na2 = load_chunk(src, P.sls, rows, 2 * m + 7, lc, whole, nw);
      nb2 = load_chunk(src, P.sls, rows, 2 * m + 8, lc, whole, nw);
      float v[DEC_CHUNK];
#pragma unroll
      for (int i = 0; i < DEC_CHUNK; i++) {
        float acc = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; t++) acc = fmaf(P.wy[t], win[(2 * j + t) & 7][i], acc);
        v[i] = acc;
      }
      if constexpr (!H) {
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = word_of(v[2 * i], vmax, sh) | (word_of(v[2 * i + 1], vmax, sh) << 16);
        if (c < nchunks) __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(dst + (long long)m * P.dls) + c);
      } else {
        float* row = lds + wave * LROW;
#pragma unroll
        for (int i = 0; i < DEC_CHUNK; i++) row[lane * (DEC_CHUNK + 1) + i] = v[i];
        wave_sync();
        // entry e of the wave's row is word e0 + e of the source row
        const int e0 = (strip * NOUT - 1) * DEC_CHUNK;
        unsigned w[4];
#pragma unroll
        for (int o = 0; o < 4; o++) {
          // planar: output column 4c + o; semi-planar: component o & 1 of output pair 2c + (o >> 1)
          const int k = SEMI ? 2 * c + (o >> 1) : 4 * c + o;
          float acc = 0.0f;
#pragma unroll
          for (int i = 0; i < 7; i++) {
            const int x = clampi(2 * k - 3 + i, 0, (SEMI ? nw >> 1 : nw) - 1);
            const int e = clampi((SEMI ? 2 * x + (o & 1) : x) - e0, 0, 64 * DEC_CHUNK - 1);
            acc = fmaf(P.wx[i], row[e + (e >> 3)], acc);
          }
          w[o] = word_of(acc, vmax, sh);
        }
        wave_sync();   // (the next output row overwrites the LDS row)
        u32x2 o2;
        o2[0] = w[0] | (w[1] << 16), o2[1] = w[2] | (w[3] << 16);
        if (lane >= 1 && lane <= NOUT && c < nchunks)
          __builtin_nontemporal_store(o2, reinterpret_cast<u32x2*>(dst + (long long)m * P.dls) + c);
      }
    }
  }
}

// the run: the longest (least re-read halo: 6 source rows a run) that still
// gives the chip two blocks a CU; `run` > 0 forces it (a test's)
hipError_t launch_decimate420(const DecimateParams& P0, int sub, bool semi, int nframes, int run, hipStream_t s) {
  if (nframes <= 0) return hipSuccess;
  DecimateParams P = P0;
  const bool h = sub == H2S_SUB_444;
  const int nchunks = (P.nw + DEC_CHUNK - 1) / DEC_CHUNK, orows = P.rows / 2;
  P.nstrips = (nchunks + dec_wave_chunks(h) - 1) / dec_wave_chunks(h);
  auto blocks = [&](int r) {
    const long long pieces = (long long)P.nplanes * P.nstrips * ((orows + r - 1) / r);
    return (pieces + DEC_THREADS / 64 - 1) / (DEC_THREADS / 64);
  };
  if (run <= 0)
    for (run = DEC_ROWS_MAX; run > DEC_ROWS_MIN && blocks(run) * nframes < 512; run /= 2) {
    }
  if (run % DEC_ROWS_STEP) return hipErrorInvalidValue;
  P.run = run;
  P.nruns = (orows + run - 1) / run;
  const dim3 grid((unsigned)blocks(run), (unsigned)nframes), block(DEC_THREADS);
  // (4:2:2: the vertical pass is per word, so pairs take the planar instance)
  if (!h) hipLaunchKernelGGL((k_decimate420<H2S_SUB_422, false>), grid, block, 0, s, P);
  else if (!semi) hipLaunchKernelGGL((k_decimate420<H2S_SUB_444, false>), grid, block, 0, s, P);
  else hipLaunchKernelGGL((k_decimate420<H2S_SUB_444, true>), grid, block, 0, s, P);
  return hipGetLastError();
}

}  // namespace h2s
