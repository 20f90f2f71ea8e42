// h2s_math.h — the scalar helpers that the tile kernel, the generic kernel
// and the host arithmetic really share.
// What belongs here: functions of their arguments alone, with no parameter
// block behind them: the edge rule and block remap, the load / store bit
// moves, the hardware transcendentals, the ST 2084 / HLG constants with the
// double-precision ST 2084 forms every curve set-up uses (host and device),
// Hable's curve, the spline and black-point forms both kernels evaluate, and
// the two dither patterns.  What only the generic kernel's chain calls (the
// libm forms and everything over them) is h2s_chain.h's, and the tile
// kernel's own table forms are h2s_tile_tone.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace h2s {

// S1 chroma upsampler edge rule (enum h2s_chroma_edge; oracle edge()): the
// sample read at position i of an n-sample chroma row / column.  0 ZIMG: -1
// mirrors to 1, n folds to n-1; 1 REPLICATE: both sides repeat the last
// sample; 2 MIRROR: both sides mirror about it (n -> n-2)
__host__ __device__ __forceinline__ int chroma_edge_at(int i, int n, int mode) {
  if (i < 0) i = mode == 1 ? 0 : -i;
  if (i > n - 1) i = mode == 2 ? 2 * (n - 1) - i : n - 1;
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// XCD-aware block remap: hardware deals blocks round-robin over 8 XCDs;
// give XCD x the contiguous logical range [x*per(+rem), ...).  Bijective.
__device__ __forceinline__ long long xcd_remap(long long b, long long nb) {
  const long long xcd = b & 7, idx = b >> 3, per = nb >> 3, rem = nb & 7;
  return xcd < rem ? xcd * (per + 1) + idx : rem * (per + 1) + (xcd - rem) * per + idx;
}

// the 16-bit words of a 16-byte / 8-byte load, in memory order, and the
// store word(s) of N codes, 8 or 16 bits each (N = 8: uint2 / uint4, N = 4:
// unsigned / uint2).  Pure bit moves: code_of / expand_code are the caller's
__device__ __forceinline__ void unpack16(const uint4 q, unsigned (&w)[8]) {
  w[0] = q.x & 0xffff, w[1] = q.x >> 16, w[2] = q.y & 0xffff, w[3] = q.y >> 16;
  w[4] = q.z & 0xffff, w[5] = q.z >> 16, w[6] = q.w & 0xffff, w[7] = q.w >> 16;
}
__device__ __forceinline__ void unpack16(const uint2 q, unsigned (&w)[4]) {
  w[0] = q.x & 0xffff, w[1] = q.x >> 16, w[2] = q.y & 0xffff, w[3] = q.y >> 16;
}
template <bool OUT8, int N>
__device__ __forceinline__ auto pack_codes(const int (&c)[N]) {
  constexpr int PER = OUT8 ? 4 : 2, SH = OUT8 ? 8 : 16, NW = N / PER;
  unsigned w[NW];
#pragma unroll
  for (int i = 0; i < NW; i++) {
    w[i] = (unsigned)c[PER * i];
#pragma unroll
    for (int k = 1; k < PER; k++) w[i] |= (unsigned)c[PER * i + k] << (SH * k);
  }
  if constexpr (NW == 4) return make_uint4(w[0], w[1], w[2], w[3]);
  else if constexpr (NW == 2) return make_uint2(w[0], w[1]);
  else return w[0];
}

// ---- fast transcendentals (v_log_f32 / v_exp_f32 / v_rcp_f32) ----------
__device__ __forceinline__ float flog2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
// x^p for x >= 0 (x == 0 -> 0 for p > 0)
__device__ __forceinline__ float fpow(float x, float p) { return fexp2(p * flog2(x)); }
__device__ __forceinline__ float clamp01(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }

// ST 2084 constants, stated once: the specification's fractions, every one
// an exact binary value (as zimg defines them), so the float forms below and
// every double user (here, h2s_chain.h, h2s_lpx.h, h2s_resolve.hip) hold the
// same numbers
constexpr double PQ_M1_D = 2610.0 / 16384.0;  // 0.1593017578125
constexpr double PQ_M2_D = 2523.0 / 32.0;     // 78.84375
constexpr double PQ_C1_D = 3424.0 / 4096.0;   // 0.8359375
constexpr double PQ_C2_D = 2413.0 / 128.0;    // 18.8515625
constexpr double PQ_C3_D = 2392.0 / 128.0;    // 18.6875
#define PQ_M1 ((float)h2s::PQ_M1_D)
#define PQ_M2 ((float)h2s::PQ_M2_D)
#define PQ_C1 ((float)h2s::PQ_C1_D)
#define PQ_C2 ((float)h2s::PQ_C2_D)
#define PQ_C3 ((float)h2s::PQ_C3_D)
static_assert((double)PQ_M1 == PQ_M1_D && (double)PQ_M2 == PQ_M2_D && (double)PQ_C1 == PQ_C1_D &&
                  (double)PQ_C2 == PQ_C2_D && (double)PQ_C3 == PQ_C3_D,
              "the ST 2084 constants are exact in float");
#define HLG_A 0.17883277f
#define HLG_B 0.28466892f
#define HLG_C 0.55991073f

// ST 2084 in double (normalised: 1.0 = 10000 nits), host and device: the
// inverse EOTF and the EOTF of every curve set-up (h2s_peak.h, h2s_resolve.hip)
__host__ __device__ inline double hd_pq_encode(double y) {
  const double ym = pow(fmax(y, 0.0), PQ_M1_D);
  return pow((PQ_C1_D + PQ_C2_D * ym) / (1.0 + PQ_C3_D * ym), PQ_M2_D);
}
__host__ __device__ inline double hd_pq_eotf(double e) {
  if (!(e > 0.0)) return 0.0;
  const double xp = pow(e, 1.0 / PQ_M2_D);
  const double num = xp - PQ_C1_D > 0.0 ? xp - PQ_C1_D : 0.0;
  return pow(num / (PQ_C2_D - PQ_C3_D * xp), 1.0 / PQ_M1_D);
}

// vf_tonemap hable(), host and device (the curve set-ups' 1 / hable(peak))
__host__ __device__ __forceinline__ float hable(float in) {
  const float a = 0.15f, b = 0.50f, c = 0.10f, d = 0.20f, e = 0.02f, f = 0.30f;
  return (in * (in * a + b * c) + d * e) / (in * (in * a + b) + d * f) - e / f;
}

// libplacebo spline on a PQ-domain signal: quadratic toe below the knee,
// cubic shoulder above it (constants: spline_consts in h2s_peak.h)
// (the oracle's spline_pq_f expression: unfused where the translation unit
// does not contract, as h2s_kernels.hip)
template <class K>
__device__ __forceinline__ float spline_pq(const K& P, float e) {
  const float x = fminf(fmaxf(e, P.sp_srcmin), P.sp_srcmax) - P.sp_kin;
  const float y = x > 0.0f ? ((P.sp_qa * x + P.sp_qb) * x + P.sp_qc) * x : (P.sp_pa * x + P.sp_pb) * x;
  return fminf(fmaxf(y + P.sp_kout, P.sp_dmin), P.sp_dmax);
}

// libplacebo bt2390 black-point adaptation on the normalised curve output
// (x += minLum (1 - x)^bp, x = gain (x - minLum) + minLum, for x < 1): the
// tile kernel's form (HLG input), bp = 4 as two squarings
__device__ __forceinline__ float bt2390_black(float mn, float bp, float gain, float x) {
  if (!(mn > 0.0f) || !(x < 1.0f)) return x;
  const float om = 1.0f - x;
  const float pw = bp == 4.0f ? (om * om) * (om * om) : powf(om, bp);
  x += mn * pw;
  return gain * (x - mn) + mn;
}

// 16 x 16 Bayer matrix (M_2n = 4 M_n + M_1 per 2 x 2 block, M_1 = [0 2; 3 1])
// as a dither offset (M + 0.5) / 256 in (0, 1): the h2s_lp_dither ORDERED model
__host__ __device__ __forceinline__ float bayer16(int x, int y) {
  int m = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int bx = (x >> i) & 1, by = (y >> i) & 1;
    m += (2 * (bx ^ by) + by) << (2 * (3 - i));
  }
  return ((float)m + 0.5f) * (1.0f / 256.0f);
}

// swscale ff_dither_8x8_128 (1/128 LSB): the H2S_DITHER_ORDERED rounding
__device__ __forceinline__ float dither_off(int x, int y) {
  constexpr unsigned char T[8][8] = {
      {36, 68, 60, 92, 34, 66, 58, 90},   {100, 4, 124, 28, 98, 2, 122, 26},
      {52, 84, 44, 76, 50, 82, 42, 74},   {116, 20, 108, 12, 114, 18, 106, 10},
      {32, 64, 56, 88, 38, 70, 62, 94},   {96, 0, 120, 24, 102, 6, 126, 30},
      {48, 80, 40, 72, 54, 86, 46, 78},   {112, 16, 104, 8, 118, 22, 110, 14}};
  return (float)T[y & 7][x & 7] * (1.0f / 128.0f);
}

}  // namespace h2s
