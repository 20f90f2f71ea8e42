// h2s_scale.hip — the scaled 4:2:0 output (h2s_process_scaled): the chain's
// trailing scale= stage on its quantised planes, [EXT].  The chain writes a
// planar scratch at full size; k_scale420 resizes every plane of every frame
// of a chunk in one launch.
//
// A block owns a strip of SCALE_COLS output columns of one plane and a run of
// output rows.  The horizontal pass runs once per source row the run needs:
// a wave stages the source segments of a few rows in LDS with 16-byte loads
// (its own piece, so the four waves walk the rows without a block barrier, and
// the next rows' loads fly while these are summed), then each lane sums one
// output column's taps from them into the float row buffer.  The
// vertical pass sums each output row from that buffer.  Both are ascending
// fmaf chains from 0 in k_resize_u8's order, so the codes are that kernel's.
// The quantised tile goes through LDS once more so that the stores are 16-byte
// wherever the destination rows allow.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "h2s_launch.h"
#include "h2s_scale.h"

namespace h2s {

namespace {

// LDS written by some lanes of a wave and read by others of the same wave:
// the LDS runs a wave's accesses in order, the compiler must not move them
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a lane's two chunks of the row group that starts at source row r0 + rb: chunk
// ka of the group's row ga, chunk kb of row gb (rows past the run's last: none)
__device__ __forceinline__ void fetch_pair(const uint8_t* plane, long long sls, int r0, int rb, int nrows, bool has_a,
                                           int ga, int ka, bool has_b, int gb, int kb, uint4& a, uint4& b) {
  if (has_a && rb + ga < nrows) a = reinterpret_cast<const uint4*>(plane + (long long)(r0 + rb + ga) * sls)[ka];
  if (has_b && rb + gb < nrows) b = reinterpret_cast<const uint4*>(plane + (long long)(r0 + rb + gb) * sls)[kb];
}

__device__ __forceinline__ uint4 codes_of(uint4 v, int shift, unsigned keep) {
  return make_uint4((v.x >> shift) & keep, (v.y >> shift) & keep, (v.z >> shift) & keep, (v.w >> shift) & keep);
}

template <int E>
__device__ __forceinline__ void store_elem(uint8_t* dst, const uint8_t* src) {
  // (a pair word of a 16-bit semi-planar plane is 2-byte aligned only)
  memcpy(dst, src, E);
}

}  // namespace

// BPS: bytes of a source sample (the scratch is at the context's bits_out)
template <int BPS>
__global__ void __launch_bounds__(SCALE_THREADS) k_scale420(const ScaleParams P) {
  extern __shared__ uint4 lds[];
  uint8_t* const base = reinterpret_cast<uint8_t*>(lds);
  constexpr int V = 16 / BPS;   // samples of a 16-byte chunk
  using Sample = typename std::conditional<BPS == 1, uint8_t, uint16_t>::type;

  // which entry, strip and run (all uniform)
  int b = blockIdx.x, e = 0;
  if (b >= P.pl[0].nblk) {
    b -= P.pl[0].nblk, e = 1;
    if (b >= P.pl[1].nblk) b -= P.pl[1].nblk, e = 2;
  }
  const ScalePlane& L = P.pl[e];
  const int Tx = L.Tx, Ty = L.Ty, np = L.np, R = L.rows;
  const int x0 = (b % L.nsx) * SCALE_COLS, y0 = (b / L.nsx) * R;
  const int ncols = min(SCALE_COLS, L.ow - x0), ye = min(y0 + R, L.oh);
  const long long f = blockIdx.y;
  const int tid = threadIdx.x, col = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int colc = min(col, ncols - 1);   // (a lane past a ragged strip repeats the last column; it stores nothing)

  const ScaleLds o = scale_lds(BPS, Tx, R, np, P.out_bps, L.hrows);
  uint4* const seg4 = reinterpret_cast<uint4*>(base + wave * (SCALE_SEG * BPS));
  const Sample* const seg = reinterpret_cast<const Sample*>(seg4);
  float* const wt = reinterpret_cast<float*>(base + o.wt);
  uint8_t* const ot = base + o.ot;
  float* const hb = reinterpret_cast<float*>(base + o.hb);

  // the strip's source columns [lo, hi), staged from the chunk boundary g0 on;
  // the run's source rows [r0, r1].  A tap outside them is the edge sample
  const int c0 = L.sx[x0], c1 = L.sx[x0 + ncols - 1] + Tx;
  const int lo = clampi(c0, 0, L.sw - 1), hi = clampi(c1, lo + 1, L.sw);
  const int g0 = lo & ~(V - 1);
  const int nch = min((hi - g0 + V - 1) / V, SCALE_SEG / V);
  const int r0 = clampi(L.sy[y0], 0, L.sh - 1);
  const int r1 = clampi(L.sy[ye - 1] + Ty - 1, r0, L.sh - 1);
  const int nrows = min(r1 - r0 + 1, L.hrows);

  // the weights, tap-major: lane `col` reads wt[i * 64 + col], one bank each
  for (int i = wave; i < Tx; i += 4) wt[i * SCALE_COLS + col] = L.wx[(long long)(x0 + colc) * Tx + i];
  const int s0 = L.sx[x0 + colc];
  __syncthreads();

  // A wave stages G source rows at a time, as many as its segment holds (a
  // 2 : 1 strip of 16-bit samples is 18 chunks: one row would leave 46 lanes
  // without a load).  Lane slots t = col and col + 64: chunk t % nch of the
  // group's row t / nch, kept in seg4[t]
  const int G = clampi((SCALE_SEG / V) / nch, 1, 8);
  int ga = 0, gb = 0;
#pragma unroll
  for (int g = 1; g <= 8; g++) ga += col >= g * nch, gb += col + 64 >= g * nch;
  const int ka = col - ga * nch, kb = col + 64 - gb * nch;
  const bool has_a = ga < G, has_b = gb < G;
  // the chain's q-bit code of every sample of a chunk: sample >> src_shift, two (four) to a dword
  const unsigned keep = BPS == 2 ? (0xffffu >> P.src_shift) * 0x10001u : (0xffu >> P.src_shift) * 0x1010101u;

  for (int q = 0; q < np; q++) {
    // ---- horizontal: wave w takes the row groups w, w + 4, ...; the next
    // group's loads are in flight while this one's taps are summed ----
    const uint8_t* const plane = L.src[q] + f * L.sfp + (long long)g0 * BPS;
    uint4 cur_a = make_uint4(0, 0, 0, 0), cur_b = cur_a;
    fetch_pair(plane, L.sls, r0, wave * G, nrows, has_a, ga, ka, has_b, gb, kb, cur_a, cur_b);
    for (int rb = wave * G; rb < nrows; rb += 4 * G) {
      uint4 nxt_a = cur_a, nxt_b = cur_b;
      fetch_pair(plane, L.sls, r0, rb + 4 * G, nrows, has_a, ga, ka, has_b, gb, kb, nxt_a, nxt_b);
      wave_sync();   // (the last group's taps are read)
      if (has_a) seg4[col] = codes_of(cur_a, P.src_shift, keep);
      if (has_b) seg4[col + 64] = codes_of(cur_b, P.src_shift, keep);
      cur_a = nxt_a, cur_b = nxt_b;
      wave_sync();
      // (one weight and one index per tap serve the group's rows; a row past
      // the run's last sums whatever its piece of the segment holds and is dropped)
      float h[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 3
      for (int i = 0; i < Tx; i++) {
        const int c = clampi(s0 + i, lo, hi - 1) - g0;
        const float w = wt[i * SCALE_COLS + colc];
#pragma unroll
        for (int g = 0; g < 8; g++)
          if (g < G) h[g] = fmaf(w, (float)seg[g * nch * V + c], h[g]);
      }
#pragma unroll
      for (int g = 0; g < 8; g++)
        if (g < G && rb + g < nrows) hb[(rb + g) * SCALE_COLS + col] = h[g];
    }
    __syncthreads();
    // ---- vertical: wave w takes output rows y0 + w, y0 + w + 4, ... ----
    for (int y = y0 + wave; y < ye; y += 4) {
      const int sy = L.sy[y];
      const float* wy = L.wy + (long long)y * Ty;
      float acc = 0.0f;
#pragma unroll 3
      for (int j = 0; j < Ty; j++) {
        const int r = clampi(sy + j - r0, 0, nrows - 1);   // ([r0, r0 + nrows) lies inside the plane)
        acc = fmaf(wy[j], hb[r * SCALE_COLS + col], acc);
      }
      float v = floorf(acc + 0.5f);
      v = v < 0.0f ? 0.0f : (v > (float)P.qmax ? (float)P.qmax : v);
      const int c = (int)v;
      const unsigned code = (unsigned)(((c << P.shift_out) | (c >> P.rep_rs)) << P.out_sh);
      const int at = ((y - y0) * SCALE_COLS + col) * np + q;
      if (P.out_bps == 1) ot[at] = (uint8_t)code;
      else reinterpret_cast<uint16_t*>(ot)[at] = (uint16_t)code;
    }
    __syncthreads();   // (the next plane's horizontal pass rewrites hb; the stores read ot)
  }

  // ---- stores: the tile's rows, ncols elements of E bytes each ----
  const int E = np * P.out_bps, tile_ls = SCALE_COLS * E, valid = ncols * E, nr = ye - y0;
  uint8_t* const dst = L.dst + f * L.dfp + (long long)y0 * L.dls + (long long)x0 * E;
  if (P.vec_out) {
    const int lc = E == 1 ? 2 : (E == 2 ? 3 : 4);   // 4, 8 or 16 chunks a row
    for (int k = tid; k < nr << lc; k += SCALE_THREADS) {
      const int row = k >> lc, cb = (k - (row << lc)) * 16;
      const uint8_t* s = ot + row * tile_ls + cb;
      uint8_t* d = dst + (long long)row * L.dls + cb;
      if (cb + 16 <= valid) {
        *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
      } else {
        for (int j = 0; cb + j < valid; j += E) {
          if (E == 1) store_elem<1>(d + j, s + j);
          else if (E == 2) store_elem<2>(d + j, s + j);
          else store_elem<4>(d + j, s + j);
        }
      }
    }
  } else {
    for (int k = tid; k < nr * SCALE_COLS; k += SCALE_THREADS) {
      const int row = k >> 6, c = k & 63;
      if (c >= ncols) continue;
      const uint8_t* s = ot + row * tile_ls + c * E;
      uint8_t* d = dst + (long long)row * L.dls + (long long)c * E;
      if (E == 1) store_elem<1>(d, s);
      else if (E == 2) store_elem<2>(d, s);
      else store_elem<4>(d, s);
    }
  }
}

hipError_t launch_scale420(const ScaleParams& P, int src_bps, int nframes, hipStream_t s) {
  int nblk = 0, bytes = 0;
  for (int e = 0; e < P.nplanes; e++) {
    const ScalePlane& L = P.pl[e];
    nblk += L.nblk;
    bytes = std::max(bytes, scale_lds(src_bps, L.Tx, L.rows, L.np, P.out_bps, L.hrows).total);
  }
  if (bytes > SCALE_LDS) return hipErrorInvalidValue;
  const dim3 grid((unsigned)nblk, (unsigned)nframes);
  if (src_bps == 1) hipLaunchKernelGGL(k_scale420<1>, grid, dim3(SCALE_THREADS), (size_t)bytes, s, P);
  else hipLaunchKernelGGL(k_scale420<2>, grid, dim3(SCALE_THREADS), (size_t)bytes, s, P);
  return hipGetLastError();
}

}  // namespace h2s
