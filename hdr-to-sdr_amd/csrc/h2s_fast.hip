// h2s_fast.hip — launcher of the tile kernel (h2s_tile.h): the CPU chain's
// planar product instances, the key, predicate and dispatch over every
// instance set (h2s_tile_sets.h), and the Y'CbCr lattice build.
#include <hip/hip_runtime.h>

#include "h2s_tile_sets.h"

H2S_TILE_UNIT(fast)   // the CPU chain's product instances for planar frame sets

namespace h2s {

// YUV-premultiplied lattice (12-byte records, .cube order):
// ((16 + 219*Y)*s, 224*s*Cb/4, 224*s*Cr/4) with Y, Cb, Cr the BT.709
// values of the clamped RGB lattice point, in the oracle's S6 operation order.
__global__ void k_build_lut_yuv(const float4* rgb, float* yuv, int n3, const YuvLutConsts K) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n3) return;
  const float4 c = rgb[i];
  const float R = clamp01(c.x), G = clamp01(c.y), B = clamp01(c.z);
  const float Y = K.k709[0] * R + K.k709[1] * G + K.k709[2] * B;
  const float cb = K.kcb[0] * R + K.kcb[1] * G + K.kcb[2] * B;
  const float cr = K.kcr[0] * R + K.kcr[1] * G + K.kcr[2] * B;
  const float s = K.s;
  if (K.rgb) {  // plain R'G'B' (libplacebo branch): lut3d's own lattice values, unclamped
    yuv[3 * i] = c.x, yuv[3 * i + 1] = c.y, yuv[3 * i + 2] = c.z;
    return;
  }
  // the luma record's rounding offset: none (k_tile rounds to nearest instead, px_chain's EQM)
  constexpr float Y_ROUND = 0.0f;
  yuv[3 * i] = (16.0f + 219.0f * Y) * s + Y_ROUND;
  yuv[3 * i + 1] = 224.0f * s * 0.25f * cb;
  yuv[3 * i + 2] = 224.0f * s * 0.25f * cr;
}

// The key of the launch that converts k's frames: dbg, the chain's debug
// instance (which also writes the planes of F.dbg_stage); semi, a semi-planar
// set on either side.
// trc 2: Dolby Vision records (h2s_set_dovi), the k_tile<2, ...> instances.
// desat: 0 off, 1 weighted luma, 2 RGB-coefficient luma (vf_tonemap's;
// BT.2390, spline and the libplacebo branch's curves have none).
// sub: the input's chroma subsampling (1 = 4:2:2, 2 = 4:4:4), or 3 = 4:2:0
// sited top-left (h2s_set_input_tags); those sets are SEMI instances whatever
// the layouts are
TileKey tile_key(const KParams& k, bool semi, bool dbg) {
  TileKey t;
  t.trc = k.dovi ? 2 : k.transfer;
  t.tm = k.tonemap;
  t.lp = k.pipe == PIPE_LIBPLACEBO ? 1 : 0;
  t.desat = !k.desat_on ? 0 : (k.lr == 1.0f && k.lg == 1.0f && k.lb == 1.0f ? 2 : 1);
  if (t.tm == 7 || t.tm == 8 || t.lp) t.desat = 0;
  t.dbg = dbg ? 1 : 0;
  t.sub = k.vco ? 3 : k.sub;
  t.semi = semi || t.sub ? 1 : 0;
  return t;
}

namespace {

struct TileSet {
  int dbg, lp, semi, sub, family;
  hipError_t (*launch)(const FastParams&, const TileKey&, dim3, size_t, hipStream_t);
};
const TileSet SETS[] = {
#define S(UNIT, DBG, LP, SEMI, SUB, FAMILY) {DBG, LP, SEMI, SUB, FAMILY_##FAMILY, launch_set<SET_##UNIT>},
    H2S_TILE_SETS(S)
#undef S
};

// the set that holds k's instance; none: there is no such instance
const TileSet* set_of(const TileKey& k) {
  for (const TileSet& r : SETS)
    if (r.dbg == k.dbg && r.lp == k.lp && r.semi == k.semi && r.sub == k.sub && family_case(r.family, k)) return &r;
  return nullptr;
}

}  // namespace

bool tile_instance(const TileKey& k) { return set_of(k) != nullptr; }

// a key without an instance is an error, never another kernel
hipError_t launch_fast(const FastParams& F, const TileKey& k, hipStream_t s) {
  const long long nt = (long long)F.nbx * F.nby * F.nframes;
  if (nt == 0) return hipSuccess;
  const long long nb = (nt + F.tpb - 1) / F.tpb;
  dim3 grid((unsigned)nb);
  // (5 blocks per CU, the LDS bound; 4 and 3, forced by padding this
  // allocation, measured +4 % and +42 % on the bench content:
  // profiles/r03/ablations/blocks_per_cu.log)
  const size_t lds = ((size_t)F.eq_n * sizeof(uint16_t) + 15) & ~(size_t)15;
  const TileSet* set = set_of(k);
  return set ? set->launch(F, k, grid, lds, s) : hipErrorInvalidValue;
}

hipError_t build_lut_yuv(const float4* rgb, float* yuv, int n, const YuvLutConsts& K, hipStream_t st) {
  const int n3 = n * n * n;
  hipLaunchKernelGGL(k_build_lut_yuv, dim3((n3 + 255) / 256), dim3(256), 0, st, rgb, yuv, n3, K);
  return hipGetLastError();
}

}  // namespace h2s
