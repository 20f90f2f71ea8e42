// h2s_rgb.hip — the RGB tensor output's last stage (h2s_process_rgb): the
// chain's quantised planar 4:2:0 codes in the scaled-output scratch to R'G'B'
// in the caller's tensor, [EXT].  The model is k_yuv8_rgb24's (h2s_preview.hip)
// at depth q, s = 2^(q - 8): pixel (x, y) takes chroma sample (x >> 1, y >> 1),
// and in float32
//   Y = 1.16438356 ((float)y - 16 s), U = (float)u - 128 s, V = (float)v - 128 s
//   cR = fmaf(1.79274107, V, Y), cG = fmaf(-0.53290933, V, fmaf(-0.21324861, U, Y)),
//   cB = fmaf(2.11240179, U, Y)
// U8: floor(c / s + 0.5) clamped to [0, 255] (1 / s is a power of two: exact);
// the float dtypes: v = min(max(c inv, 0), 1), inv = (float)(1 / (255 s)), then
// fmaf(scale[k], v, bias[k]), stored as float32 or rounded to nearest-even to
// half / bfloat16.  No display gamma.
//
// A pure streaming kernel: a lane owns RGB_RUN consecutive luma columns of one
// row pair, which shares one chroma row: two 16-byte luma loads and one chroma
// load a plane (1-byte scratch samples; 2-byte ones: four luma loads of 16
// bytes and a 16-byte chroma load a plane), no LDS, no barrier.  Its output is
// a contiguous run of each row in either layout (HWC: R, G, B interleaved in
// registers, 48 elements; CHW: three runs of 16), written with whole 16-byte
// non-temporal stores where the tensor's row starts are 16-byte aligned
// (P.vec) and the run is whole, element by element otherwise (an unaligned
// view, the ragged last run of a row).  Adjacent lanes own adjacent runs, so a
// wave's accesses coalesce; the frame is the grid's y.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/h2s.h"
#include "h2s_launch.h"
#include "h2s_rgb.h"

namespace h2s {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr int rgb_esize(int dt) { return dt == H2S_RGB_U8 ? 1 : (dt == H2S_RGB_F32 ? 4 : 2); }

// channel k's value as the bits of an element of DT
template <int DT>
__device__ __forceinline__ unsigned elem_bits(float c, const RgbParams& P, int k) {
  if constexpr (DT == H2S_RGB_U8) {
    return (unsigned)fminf(fmaxf(floorf(c * P.inv + 0.5f), 0.0f), 255.0f);
  } else {
    const float v = fminf(fmaxf(c * P.inv, 0.0f), 1.0f);
    const float o = fmaf(P.scale[k], v, P.bias[k]);
    if constexpr (DT == H2S_RGB_F32) {
      return __float_as_uint(o);
    } else if constexpr (DT == H2S_RGB_F16) {
      return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)o);   // (round to nearest even)
    } else {
      const unsigned b = __float_as_uint(o);   // (finite: scale and bias are)
      return (b + 0x7FFFu + ((b >> 16) & 1u)) >> 16;
    }
  }
}

template <int E>
__device__ __forceinline__ void store_elem(uint8_t* p, unsigned bits) {
  if constexpr (E == 1) *p = (uint8_t)bits;
  else if constexpr (E == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)bits;
  else *reinterpret_cast<uint32_t*>(p) = bits;
}

// `n` whole 16-byte pieces at p from the elements el(e), e ascending
template <int E, class F>
__device__ __forceinline__ void store_run16(uint8_t* p, int pieces, F el) {
  constexpr int PW = 4 / E;   // elements of a word
#pragma unroll
  for (int q = 0; q < pieces; q++) {
    u32x4 o;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      unsigned w = 0;
#pragma unroll
      for (int j = 0; j < PW; j++) w |= el((4 * q + t) * PW + j) << (8 * E * j);
      o[t] = w;
    }
    __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(p) + q);
  }
}

}  // namespace

// BPS: bytes of a scratch sample.  DT: enum h2s_rgb_dtype.  LAYOUT: enum h2s_rgb_layout
template <int BPS, int DT, int LAYOUT>
__global__ __launch_bounds__(RGB_THREADS) void k_rgb420(const RgbParams P) {
  constexpr int E = rgb_esize(DT);
  const int idx = blockIdx.x * RGB_THREADS + threadIdx.x;
  if (idx >= P.ngroups * P.npairs) return;
  const int r = idx / P.ngroups, g = idx - r * P.ngroups;
  const int x0 = g * RGB_RUN, n = min(RGB_RUN, P.w - x0);
  const long long f = blockIdx.y;
  const uint8_t* yp = P.y + f * P.sfp + (long long)(2 * r) * P.yls + x0 * BPS;
  const long long cat = f * P.sfp + (long long)r * P.cls + (x0 >> 1) * BPS;
  uint8_t* dst = P.dst + f * P.fp;

  // the run's 8 chroma samples of each plane
  float U[RGB_RUN / 2], V[RGB_RUN / 2];
  if constexpr (BPS == 1) {
    const u32x2 cu = *reinterpret_cast<const u32x2*>(P.u + cat), cv = *reinterpret_cast<const u32x2*>(P.v + cat);
#pragma unroll
    for (int j = 0; j < RGB_RUN / 2; j++) {
      U[j] = (float)(((cu[j >> 2] >> (8 * (j & 3))) & 0xFFu) >> P.shift) - P.coff;
      V[j] = (float)(((cv[j >> 2] >> (8 * (j & 3))) & 0xFFu) >> P.shift) - P.coff;
    }
  } else {
    const u32x4 cu = *reinterpret_cast<const u32x4*>(P.u + cat), cv = *reinterpret_cast<const u32x4*>(P.v + cat);
#pragma unroll
    for (int j = 0; j < RGB_RUN / 2; j++) {
      U[j] = (float)(((cu[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) >> P.shift) - P.coff;
      V[j] = (float)(((cv[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) >> P.shift) - P.coff;
    }
  }
  // both rows' luma, in flight together (2-byte samples: the run is two pieces,
  // and a ragged run of at most 8 columns has no second one inside the row)
  u32x4 L[2][BPS];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    L[j][0] = *reinterpret_cast<const u32x4*>(yp + j * P.yls);
    if constexpr (BPS == 2) {
      L[j][1] = u32x4{0, 0, 0, 0};
      if (n > RGB_RUN / 2) L[j][1] = *reinterpret_cast<const u32x4*>(yp + j * P.yls + 16);
    }
  }
  const bool whole = P.vec && n == RGB_RUN;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    unsigned b[3][RGB_RUN];
#pragma unroll
    for (int i = 0; i < RGB_RUN; i++) {
      unsigned code;
      if constexpr (BPS == 1) code = (L[j][0][i >> 2] >> (8 * (i & 3))) & 0xFFu;
      else code = (L[j][i >> 3][(i & 7) >> 1] >> (16 * (i & 1))) & 0xFFFFu;
      const float Y = 1.16438356f * ((float)(code >> P.shift) - P.yoff);
      const float u = U[i >> 1], v = V[i >> 1];
      b[0][i] = elem_bits<DT>(fmaf(1.79274107f, v, Y), P, 0);
      b[1][i] = elem_bits<DT>(fmaf(-0.53290933f, v, fmaf(-0.21324861f, u, Y)), P, 1);
      b[2][i] = elem_bits<DT>(fmaf(2.11240179f, u, Y), P, 2);
    }
    uint8_t* row = dst + (long long)(2 * r + j) * P.rp;
    if constexpr (LAYOUT == H2S_RGB_HWC) {
      uint8_t* p = row + (long long)x0 * 3 * E;
      if (whole) {
        store_run16<E>(p, 3 * E, [&](int e) { return b[e % 3][e / 3]; });
      } else {
#pragma unroll
        for (int i = 0; i < RGB_RUN; i++)
          if (i < n) {
#pragma unroll
            for (int k = 0; k < 3; k++) store_elem<E>(p + (3 * i + k) * E, b[k][i]);
          }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        uint8_t* p = row + k * P.pp + (long long)x0 * E;
        if (whole) {
          store_run16<E>(p, E, [&](int e) { return b[k][e]; });
        } else {
#pragma unroll
          for (int i = 0; i < RGB_RUN; i++)
            if (i < n) store_elem<E>(p + i * E, b[k][i]);
        }
      }
    }
  }
}

namespace {

template <int BPS>
hipError_t launch_bps(const RgbParams& P, int dtype, int layout, dim3 grid, hipStream_t s) {
  const dim3 block(RGB_THREADS);
#define H2S_RGB_CASE(DT)                                                                              \
  case DT:                                                                                            \
    if (layout == H2S_RGB_HWC) hipLaunchKernelGGL((k_rgb420<BPS, DT, H2S_RGB_HWC>), grid, block, 0, s, P); \
    else hipLaunchKernelGGL((k_rgb420<BPS, DT, H2S_RGB_CHW>), grid, block, 0, s, P);                  \
    break;
  switch (dtype) {
    H2S_RGB_CASE(H2S_RGB_U8)
    H2S_RGB_CASE(H2S_RGB_F16)
    H2S_RGB_CASE(H2S_RGB_BF16)
    H2S_RGB_CASE(H2S_RGB_F32)
    default:
      return hipErrorInvalidValue;
  }
#undef H2S_RGB_CASE
  return hipGetLastError();
}

}  // namespace

hipError_t launch_rgb420(const RgbParams& P0, int src_bps, int dtype, int layout, int nframes, hipStream_t s) {
  if (nframes <= 0) return hipSuccess;
  if (layout != H2S_RGB_HWC && layout != H2S_RGB_CHW) return hipErrorInvalidValue;
  RgbParams P = P0;
  P.ngroups = (P.w + RGB_RUN - 1) / RGB_RUN, P.npairs = P.h / 2;
  const long long pieces = (long long)P.ngroups * P.npairs;
  const dim3 grid((unsigned)((pieces + RGB_THREADS - 1) / RGB_THREADS), (unsigned)nframes);
  return src_bps == 1 ? launch_bps<1>(P, dtype, layout, grid, s) : launch_bps<2>(P, dtype, layout, grid, s);
}

}  // namespace h2s
