// h2s_repack.hip — a rendition ladder's source-size rung (h2s_process_ladder):
// the scaled output's scratch already holds the chain's finished bits_out codes
// as planar 4:2:0 with 16-byte aligned rows, so the rung is a copy of them into
// the caller's layout and pitches.  k_repack420 copies every plane of every
// frame of a chunk in one launch.
//
// A lane owns one 16-byte column of a plane and REPACK_ROWS rows of it: that
// many 16-byte loads are issued before the first store.  A planar destination
// takes the chunk as it is, at its own pitch.  A semi-planar one takes the Cb
// and the Cr chunk of one column as two chunks of (Cb, Cr) pairs, and a 16-bit
// word carries its code in the high bits (code << (16 - bits), luma too).
// Stores are whole non-temporal 16-byte ones where every destination row start
// is 16-byte aligned (a launch-uniform flag); otherwise, and in a row's ragged
// last chunk, they are per sample.  No LDS, no barrier; nothing past a row's
// last sample is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "h2s_launch.h"
#include "h2s_repack.h"

namespace h2s {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the first `valid` bytes of a chunk, sample by sample (16-bit planes are 2-byte aligned: check_frames)
template <int BPS>
__device__ __forceinline__ void store_samples(uint8_t* d, u32x4 v, int valid) {
#pragma unroll
  for (int j = 0; j < 16 / BPS; j++) {
    if (j * BPS < valid) {
      if (BPS == 1) d[j] = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
      else reinterpret_cast<uint16_t*>(d)[j] = (uint16_t)(v[j >> 1] >> (16 * (j & 1)));
    }
  }
}

template <int BPS>
__device__ __forceinline__ void store_chunk(uint8_t* d, u32x4 v, int valid, bool vec) {
  if (valid <= 0) return;
  if (vec && valid >= 16) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(d));
  else store_samples<BPS>(d, v, valid);
}

// half h (0, 1) of the 32 bytes of pairs that the chunks cb and cr make
template <int BPS>
__device__ __forceinline__ u32x4 pairs_of(u32x4 cb, u32x4 cr, int h, int sh) {
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (BPS == 2) {
      // word 4h + k of either chunk
      const unsigned b = cb[2 * h + (k >> 1)] >> (16 * (k & 1)) & 0xFFFFu;
      const unsigned r = cr[2 * h + (k >> 1)] >> (16 * (k & 1)) & 0xFFFFu;
      o[k] = (b | (r << 16)) << sh;
    } else {
      // bytes 8h + 2k, 8h + 2k + 1 of either chunk
      const unsigned b = cb[2 * h + (k >> 1)] >> (16 * (k & 1)), r = cr[2 * h + (k >> 1)] >> (16 * (k & 1));
      o[k] = (b & 0xFFu) | ((r & 0xFFu) << 8) | ((b & 0xFF00u) << 8) | ((r & 0xFF00u) << 16);
    }
  }
  return o;
}

}  // namespace

// BPS: bytes of a sample (the scratch and the rung are at the context's bits_out).
// SEMI: the destination is semi-planar (entry 1: the pairs)
template <int BPS, bool SEMI>
__global__ void __launch_bounds__(REPACK_THREADS) k_repack420(const RepackParams P) {
  // which entry (uniform), then the lane's column and rows
  int b = blockIdx.x, e = 0;
  if (b >= P.pl[0].nblk) {
    b -= P.pl[0].nblk, e = 1;
    if (b >= P.pl[1].nblk) b -= P.pl[1].nblk, e = 2;
  }
  const RepackPlane& L = P.pl[e];
  const int idx = b * REPACK_THREADS + (int)threadIdx.x;
  const int rg = idx / L.nch, ch = idx - rg * L.nch;
  const int y0 = rg * REPACK_ROWS;
  if (y0 >= L.rows) return;
  const long long f = blockIdx.y;
  const int valid = min(16, L.row_bytes - ch * 16);
  const bool vec = P.vec_out != 0;
  const int sh = P.sh;

  if (SEMI && L.np == 2) {
    const uint8_t* const sb = L.src[0] + f * L.sfp + (long long)y0 * L.sls + ch * 16;
    const uint8_t* const sr = L.src[1] + f * L.sfp + (long long)y0 * L.sls + ch * 16;
    uint8_t* const d = L.dst + f * L.dfp + (long long)y0 * L.dls + ch * 32;
    u32x4 cb[REPACK_ROWS], cr[REPACK_ROWS];
#pragma unroll
    for (int r = 0; r < REPACK_ROWS; r++) {
      if (y0 + r < L.rows) {
        cb[r] = *reinterpret_cast<const u32x4*>(sb + r * L.sls);
        cr[r] = *reinterpret_cast<const u32x4*>(sr + r * L.sls);
      }
    }
#pragma unroll
    for (int r = 0; r < REPACK_ROWS; r++) {
      if (y0 + r < L.rows) {
        store_chunk<BPS>(d + r * L.dls, pairs_of<BPS>(cb[r], cr[r], 0, sh), 2 * valid, vec);
        store_chunk<BPS>(d + r * L.dls + 16, pairs_of<BPS>(cb[r], cr[r], 1, sh), 2 * valid - 16, vec);
      }
    }
  } else {
    const uint8_t* const s = L.src[0] + f * L.sfp + (long long)y0 * L.sls + ch * 16;
    uint8_t* const d = L.dst + f * L.dfp + (long long)y0 * L.dls + ch * 16;
    u32x4 v[REPACK_ROWS];
#pragma unroll
    for (int r = 0; r < REPACK_ROWS; r++)
      if (y0 + r < L.rows) v[r] = *reinterpret_cast<const u32x4*>(s + r * L.sls);
#pragma unroll
    for (int r = 0; r < REPACK_ROWS; r++) {
      if (y0 + r < L.rows) {
        // (a code << sh stays inside its 16-bit word)
        if (SEMI && BPS == 2) v[r] = v[r] << sh;
        store_chunk<BPS>(d + r * L.dls, v[r], valid, vec);
      }
    }
  }
}

// it fills P's chunk and block counts
hipError_t launch_repack420(const RepackParams& P0, int bps, bool semi, int nframes, hipStream_t s) {
  if (nframes <= 0) return hipSuccess;
  RepackParams P = P0;
  long long nblk = 0;
  for (int e = 0; e < 3; e++) {
    RepackPlane& L = P.pl[e];
    if (e >= P.nplanes) {
      L.nch = 1, L.nblk = 0;
      continue;
    }
    if (L.row_bytes <= 0 || L.rows <= 0) return hipErrorInvalidValue;
    L.nch = (L.row_bytes + 15) / 16;
    const long long items = (long long)L.nch * ((L.rows + REPACK_ROWS - 1) / REPACK_ROWS);
    L.nblk = (int)((items + REPACK_THREADS - 1) / REPACK_THREADS);
    nblk += L.nblk;
  }
  const dim3 grid((unsigned)nblk, (unsigned)nframes), block(REPACK_THREADS);
  if (bps == 1 && !semi) hipLaunchKernelGGL((k_repack420<1, false>), grid, block, 0, s, P);
  else if (bps == 1) hipLaunchKernelGGL((k_repack420<1, true>), grid, block, 0, s, P);
  else if (!semi) hipLaunchKernelGGL((k_repack420<2, false>), grid, block, 0, s, P);
  else hipLaunchKernelGGL((k_repack420<2, true>), grid, block, 0, s, P);
  return hipGetLastError();
}

}  // namespace h2s
