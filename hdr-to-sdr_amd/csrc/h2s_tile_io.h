// h2s_tile_io.h — the tile kernel's tile I/O (h2s_tile.h has the overview;
// DESIGN.md §4.1, "The tile I/O").  What belongs here: the tile geometry and
// the walk over tiles (TileGeo, tile_geo, tile_next), the launch's lane offsets
// (lane_ofs), the loads of a tile into registers (TileRegs, tile_load and the
// load rule), the commit of those registers to LDS (luma_at, stage_*), and the
// way out: quantise and pack (read_*), the store rule and the stores
// (tile_store, put_*).  Every frame format's addressing lives here; the
// per-pixel arithmetic between load and store is h2s_tile_px.h's.
#pragma once
#include "h2s_tile_px.h"

namespace h2s {

constexpr int CBW = 32, CBH = 16;  // chroma tile
// The 2x2 chroma sums in LDS (csum, one plane of CBH * CBW floats each for Cb
// and Cr): sample (cx, cy) of the chroma tile at float csum_at(cx, cy), laid
// out by macro-column (8 chroma columns = one 16-pixel macro-block column of
// k_tile's steps), then row, then column.  A step's offset from the wave's
// per-lane base (macro-column: 512 bytes, macro-row: 8 rows = 256 bytes) and
// the plane stride (2048 bytes) are then all multiples of 256 bytes, the unit
// of the offsets of the one ds_write2st64_b32 that stores both sums, so every
// step writes from the same base register.  The 4 rows x 4 columns a wave
// writes per step lie 8 floats apart per row: 16 distinct banks, no conflict.
// The store phase reads a row's 8-sample chunk (one macro-column) as 32
// contiguous bytes
constexpr int csum_at(int cx, int cy) { return (cx >> 3) * (CBH * 8) + cy * 8 + (cx & 7); }
static_assert(csum_at(8, 0) * 4 % 256 == 0 && csum_at(0, 8) * 4 % 256 == 0 && CBH * CBW * 4 % 256 == 0,
              "a step's and the plane's offsets are whole 256-byte units");
static_assert(csum_at(CBW - 1, CBH - 1) == CBH * CBW - 1, "csum_at fills the plane");
// LDS row stride (floats) of the horizontally upsampled chroma rows (and, until
// the luma tile became 16-bit codes at its own stride, luma_at, of the staged
// luma floats: the measurements below are of both).  72 on the CPU chain's instances: a step's 8 rows x 8
// columns then start 8 banks apart and cover all 64 banks (68 overlapped
// 2-way: 34 % -> 20 % of LDS-active cycles in bank conflicts, time unchanged;
// profiles/r04/ablations/lds_stride.txt).  68 on the libplacebo instances,
// whose PQ-encode table and native-depth eq table leave no room: +1.1 KB there
// drops them from 5 blocks per CU to 4 (C3 +9 %).  Round 5: their 8-segment
// PQ-encode table puts them at 4 blocks per CU anyway; 72 measured the same
// as 68 there (0.939 / 0.936 ms, profiles/r05/lp_variants.log), 68 kept for
// the LDS (the 12-bit output's 8 KB eq table)
constexpr int ROW_STRIDE = 72, ROW_STRIDE_LP = 68;
template <int LP>
constexpr int row_stride() { return LP ? ROW_STRIDE_LP : ROW_STRIDE; }
// buffer-op aux bits: non-temporal (streamed frame bytes).  Frame loads that
// bypass the L1 (sc1 nt, sc0 sc1 nt) or use workgroup scope (sc0 nt) time the
// same within 1 %: the streamed bytes do not evict the lattice lines the
// gathers wait on (profiles/r03/ablations/frame_load_cache_policy.log)
constexpr int AUX_NT = 2;
constexpr int NT = AUX_NT, NTS = AUX_NT;   // cache-policy bits of the frame loads / stores

__device__ __forceinline__ void unpack8(const uint4 a, float* o) {
  o[0] = (float)(a.x & 0xffff), o[1] = (float)(a.x >> 16), o[2] = (float)(a.y & 0xffff), o[3] = (float)(a.y >> 16);
  o[4] = (float)(a.z & 0xffff), o[5] = (float)(a.z >> 16), o[6] = (float)(a.w & 0xffff), o[7] = (float)(a.w >> 16);
}

// bytes: the plane's extent, clamped to 2^31-1 on the host (FastParams in/out_bytes)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const uint8_t* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, bytes, 0x00020000);
}

// one tile's global loads, held in registers between issue and the LDS commit
// (semi-planar input, F.in_semi: ua = four (Cb, Cr) pairs of the interleaved
// plane on threads t < 144, uh = the pair right of them; the same registers)
// (SUB 1, 4:2:2 input: the same registers, a chunk on every thread; SUB 2,
// 4:4:4: one chunk of each chroma plane per thread and no halo)
template <bool SEMI, int SUB = 0>
struct TileRegs {
  uint4 ya, ua;     // luma chunk; chroma chunk of plane pc (threads tc < 72)
  std::conditional_t<SEMI, unsigned, uint16_t> uh;   // the chroma chunk's right-halo sample (SEMI: or pair; planar input: the word that holds it, halo_half)
};
template <bool SEMI>
struct TileRegs<SEMI, 2> {
  uint4 ya, ua, va;   // luma chunk; the Cb and Cr chunks under it
};

struct TileGeo {
  int f, px0, py0, cx0, cy0;
};

__device__ __forceinline__ TileGeo tile_geo(const FastParams& F, unsigned tile) {
  const unsigned bx = tile % F.nbx, bt = tile / F.nbx;
  TileGeo g;
  g.f = (int)(bt / F.nby);
  const int by = (int)(bt % F.nby);
  g.px0 = (int)bx * TBW, g.py0 = by * TBH, g.cx0 = (int)bx * CBW, g.cy0 = by * CBH;
  return g;
}

// the tile after g in walk order (x, then y, then frame): block-uniform
// scalar arithmetic, no division
__device__ __forceinline__ void tile_next(const FastParams& F, TileGeo& g) {
  g.px0 += TBW, g.cx0 += CBW;
  if (g.px0 >= F.W) {
    g.px0 = 0, g.cx0 = 0, g.py0 += TBH, g.cy0 += CBH;
    if (g.py0 >= (int)F.nby * TBH) g.py0 = 0, g.cy0 = 0, g.f++;
  }
}

// per-lane byte offsets of a tile's loads and stores relative to the tile's
// origin, fixed for the whole launch (the strides do not change): interior
// tiles then address with one scalar origin (soffset) and no per-lane
// arithmetic
struct LaneOfs {
  int y, u;        // loads: luma row yr, chunk yc; chroma row clr, chunk ccx of plane pc
  int sy, sc;      // stores: luma row / 8-sample chunk; chroma row of plane pl
};

template <bool SEMI>
__device__ __forceinline__ LaneOfs lane_ofs(const FastParams& F, int t) {
  LaneOfs L;
  L.y = (t >> 3) * (int)F.in_ls[0] + 16 * (t & 7);
  const int pc = (t >> 7) & 1, tc = t & 127;
  L.u = (tc >> 2) * (int)F.in_ls[1 + pc] + 16 * (tc & 3);
  // semi-planar: chroma row t >> 3, 16-byte chunk t & 7 (four pairs) of the interleaved plane
  if (SEMI && F.in_semi) L.u = (t >> 3) * (int)F.in_ls[1] + 16 * (t & 7);
  const int sb = F.out8 ? 8 : 16;
  L.sy = (t >> 3) * (int)F.out_ls[0] + sb * (t & 7);
  const int pl = (t >> 6) & 1, rem = t & 63;
  L.sc = (rem >> 2) * (int)F.out_ls[1 + pl] + sb * (rem & 3);
  if (SEMI && F.out_semi) L.sc = (t >> 3) * (int)F.out_ls[1] + sb * (t & 7);
  return L;
}

// issue (do not wait for) the loads of one tile: luma 64 x 32 (one 16-byte
// load per thread) and chroma rows cy0-1 .. cy0+16 (18 rows x 4 chunks of 8
// samples + 1 right-halo sample): plane U on threads 0..71, plane V on threads
// 128..199, so waves 0-1 and 2-3 share the chroma work and the plane (hence the
// buffer resource) is wave-uniform.  Tiles whose rows (and chroma
// halo) lie inside the frame take the lane offsets of LaneOfs plus a scalar
// origin; border tiles clamp per lane.  The chroma registers of threads >= 72
// are left undefined (never committed).
// SUB (h2s_set_input_subsampling; 0 = 4:2:0, the text above): the chroma
// window of a 4:2:2 / 4:4:4 input has the tile's own 32 rows and no halo rows,
// so a bottom tile clamps its chroma rows as it clamps its luma rows.
//  1 (4:2:2): 32 rows x 4 chunks per plane, and the right-halo sample of each
//    row's last chunk: every thread loads one chunk, U on threads 0..127, V
//    on 128..255 (LaneOfs::u as it is; the scalar origin is row py0, not
//    cy0 - 1)
//  2 (4:4:4): 32 rows x 8 chunks per plane, the luma chunk's own geometry:
//    every thread loads the Cb and the Cr chunk under its luma chunk
template <bool SEMI, int SUB = 0>
__device__ __forceinline__ TileRegs<SEMI, SUB> tile_load(const FastParams& F, const TileGeo& g, int t, const LaneOfs& L) {
  // Every thread issues exactly one load of each kind whatever the tile: the
  // offsets are chosen per case and the loads follow the merge; threads
  // without a chroma chunk read out of range, which returns 0 and fetches
  // nothing
  const __amdgpu_buffer_rsrc_t iy = plane_rsrc(F.in[0] + g.f * F.in_fp[0], F.in_bytes[0]);
  const int yr = t >> 3, yc = t & 7;
  TileRegs<SEMI, SUB> r;
  int vy, sy;
  if (g.py0 + TBH <= F.H) {   // block-uniform
    vy = L.y, sy = g.py0 * (int)F.in_ls[0] + 2 * g.px0;
  } else {
    vy = (g.py0 + yr < F.H ? g.py0 + yr : F.H - 1) * (int)F.in_ls[0] + 2 * (g.px0 + 8 * yc), sy = 0;
  }
  r.ya = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(iy, vy, sy, NT));
  if constexpr (SUB == 2) {
    const __amdgpu_buffer_rsrc_t iu = plane_rsrc(F.in[1] + g.f * F.in_fp[1], F.in_bytes[1]);
    const __amdgpu_buffer_rsrc_t iv = plane_rsrc(F.in[2] + g.f * F.in_fp[2], F.in_bytes[2]);
    const int lu = (int)F.in_ls[1], lv = (int)F.in_ls[2];
    int vu, vv, su, sv;
    if (g.py0 + TBH <= F.H) {   // block-uniform
      vu = yr * lu + 16 * yc, vv = yr * lv + 16 * yc;
      su = g.py0 * lu + 2 * g.px0, sv = g.py0 * lv + 2 * g.px0;
    } else {
      const int row = g.py0 + yr < F.H ? g.py0 + yr : F.H - 1;
      vu = row * lu + 2 * (g.px0 + 8 * yc), vv = row * lv + 2 * (g.px0 + 8 * yc), su = sv = 0;
    }
    r.ua = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(iu, vu, su, NT));
    r.va = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(iv, vv, sv, NT));
    return r;
  } else if constexpr (SUB == 1) {
    const int pc = __builtin_amdgcn_readfirstlane(t >> 7), tc = t & 127;
    const __amdgpu_buffer_rsrc_t ic = plane_rsrc(F.in[1 + pc] + g.f * F.in_fp[1 + pc], F.in_bytes[1 + pc]);
    const int ls = (int)F.in_ls[1 + pc];
    int vc, vh, sc;
    if (g.py0 + TBH <= F.H && g.cx0 + CBW + 1 <= F.icw) {   // block-uniform
      vc = L.u, vh = L.u + 16, sc = g.py0 * ls + 2 * g.cx0;
    } else {
      const int clr = tc >> 2, ccx = tc & 3;
      const int row = g.py0 + clr < F.H ? g.py0 + clr : F.H - 1;
      vc = row * ls + 2 * (g.cx0 + 8 * ccx);
      vh = row * ls + 2 * chroma_edge_at(g.cx0 + 8 * ccx + 8, F.icw, F.chroma_edge);
      sc = 0;
    }
    // only a row's last chunk has a halo the tile does not hold already (the
    // others' is the next chunk's first sample): theirs is read out of range,
    // which returns 0 and fetches nothing
    if ((tc & 3) != 3) vh = 0x7FFFFFF0;
    r.ua = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ic, vc, sc, NT));
    r.uh = __builtin_amdgcn_raw_buffer_load_b16(ic, vh, sc, 0);
    return r;
  } else {
  // One chunk load and one halo load for both layouts of a SEMI instance (the
  // layouts differ in plane, offsets and the halo's width, not in the
  // instructions: two arms that each held their loads would leave the
  // compiler a path with neither and one with both, and its waits for the
  // second arm's registers would drain the previous tile's stores)
  const bool pair = SEMI && F.in_semi;   // block-uniform
  int pc, vc, vh, sc;
  if (pair) {
    // the interleaved plane: 18 rows x 8 chunks of four (Cb, Cr) pairs on
    // threads 0..143, each with the pair right of its chunk (4 bytes), so
    // every line of the plane is read once
    pc = 0;
    const int ls = (int)F.in_ls[1];
    if (g.cy0 >= 1 && g.cy0 + CBH + 1 <= F.ch && g.cx0 + CBW + 1 <= F.cw) {   // block-uniform
      vc = L.u, vh = L.u + 16, sc = (g.cy0 - 1) * ls + 4 * g.cx0;
    } else {
      const int clr = t >> 3, ccx = t & 7;
      const int row = chroma_edge_at(g.cy0 - 1 + clr, F.ch, F.chroma_edge);
      vc = row * ls + 4 * (g.cx0 + 4 * ccx);
      vh = row * ls + 4 * chroma_edge_at(g.cx0 + 4 * ccx + 4, F.cw, F.chroma_edge);
      sc = 0;
    }
    if (t >= 144) vc = vh = 0x7FFFFFF0;
  } else {
    pc = __builtin_amdgcn_readfirstlane(t >> 7);
    const int tc = t & 127;
    const int ls = (int)F.in_ls[1 + pc];
    if (g.cy0 >= 1 && g.cy0 + CBH + 1 <= F.ch && g.cx0 + CBW + 1 <= F.cw) {   // block-uniform
      vc = L.u, vh = L.u + 16, sc = (g.cy0 - 1) * ls + 2 * g.cx0;
    } else {
      const int clr = tc >> 2, ccx = tc & 3;
      const int row = chroma_edge_at(g.cy0 - 1 + clr, F.ch, F.chroma_edge);
      vc = row * ls + 2 * (g.cx0 + 8 * ccx);
      vh = row * ls + 2 * chroma_edge_at(g.cx0 + 8 * ccx + 8, F.cw, F.chroma_edge);
      sc = 0;
    }
    if (tc >= 72) vc = vh = 0x7FFFFFF0;
  }
  const __amdgpu_buffer_rsrc_t ic = plane_rsrc(F.in[1 + pc] + g.f * F.in_fp[1 + pc], F.in_bytes[1 + pc]);
  sc = __builtin_amdgcn_readfirstlane(sc);   // (block-uniform; said so, or the merged origin costs a lane loop per load)
  r.ua = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ic, vc, sc, NT));
  if constexpr (SEMI) {
    // the halo as the aligned word that holds it (rows and scalar origins are
    // 4-byte aligned, so the word lies inside the plane): the pair itself,
    // or the word with the planar sample, whose half halo_half takes at the
    // commit (not here: that would wait for the load)
    r.uh = __builtin_amdgcn_raw_buffer_load_b32(ic, vh & ~2, sc, 0);
  } else {
    r.uh = __builtin_amdgcn_raw_buffer_load_b16(ic, vh, sc, 0);
  }
  return r;
  }
}

// a SEMI instance's planar 4:2:0 halo sample from the word tile_load read for
// tile g: the low half, or on a border tile the half of the clamped column
__device__ __forceinline__ unsigned halo_half(const FastParams& F, const TileGeo& g, int t, unsigned hw) {
  int hs = 0;
  if (!(g.cy0 >= 1 && g.cy0 + CBH + 1 <= F.ch && g.cx0 + CBW + 1 <= F.cw))   // block-uniform, as tile_load
    hs = (chroma_edge_at(g.cx0 + 8 * (t & 3) + 8, F.cw, F.chroma_edge) & 1) << 4;
  return (hw >> hs) & 0xffffu;
}

// staging and store helpers of k_tile
// The luma tile in LDS: the 16-bit codes as loaded (after a semi-planar or
// truncating input's shift and mask), pixel (x, y) of the 64 x 32 tile at
// byte luma_at(x, y).  A step converts its sample (S0) and writes the output
// code over it (S7); the store phase moves a chunk's 16 bytes as they are.
// Row stride 144 bytes: the 8 rows of a step's 8 x 8 block start 36 dwords
// apart, i.e. on banks 0, 4, .., 28 of the 32 that 16-bit reads and every
// write use, and a row's 8 samples take 4 dwords (two lanes per dword, one
// address), so a step's 64 reads and 64 writes have no bank conflict
constexpr int YROW = 144;
constexpr int luma_at(int x, int y) { return y * YROW + 2 * x; }
static_assert(YROW % 16 == 0 && luma_at(8, 0) == 16, "a chunk of 8 samples is one aligned 16-byte slot");
static_assert(luma_at(0, 1) >= luma_at(TBW - 1, 0) + 2, "the rows' slots are disjoint");
static_assert((luma_at(0, 1) / 4) % 32 == 4 && luma_at(7, 0) / 4 == 3, "a step's 8 rows x 4 dwords cover the 32 banks once");
constexpr int YIN_BYTES = luma_at(0, TBH);
typedef unsigned short us2v __attribute__((ext_vector_type(2)));
// commit the thread's chunk (row, 8 col8); returns its largest code staged
// as the step stages it (fmaf is monotonic in the code: ysc > 0), for the
// tile's branch-free-body flag
__device__ __forceinline__ float stage_luma(unsigned char* yin, uint4 a, int row, int col8, float ysc, float yoff) {
  *reinterpret_cast<uint4*>(yin + luma_at(8 * col8, row)) = a;
  const us2v m = __builtin_elementwise_max(
      __builtin_elementwise_max(__builtin_bit_cast(us2v, a.x), __builtin_bit_cast(us2v, a.y)),
      __builtin_elementwise_max(__builtin_bit_cast(us2v, a.z), __builtin_bit_cast(us2v, a.w)));
  return fmaf((float)(m.x > m.y ? m.x : m.y), ysc, yoff);
}
// horizontal pass (left siting, x2 scale) on centred codes c = code - mid:
// h[2k] = 2 c[k], h[2k+1] = c[k] + c[k+1]; exact in float.  tt: chunk index
// (row tt >> 2, 8-sample chunk tt & 3) of the tile's 18 x 4 chroma chunks
// returns the largest |centred code|
template <int HST>
__device__ __forceinline__ float stage_chroma(float* plane, uint4 a, unsigned h, int tt, float cmid) {
  float v[9];
  unpack8(a, v);
  v[8] = (float)h;
#pragma unroll
  for (int k = 0; k < 9; k++) v[k] -= cmid;
  float m = fabsf(v[0]);
#pragma unroll
  for (int k = 1; k < 9; k++) m = __builtin_fmaxf(m, fabsf(v[k]));
  float* d = plane + (tt >> 2) * HST + 16 * (tt & 3);
#pragma unroll
  for (int k = 0; k < 4; k++)
    *reinterpret_cast<float4*>(d + 4 * k) =
        make_float4(v[2 * k] + v[2 * k], v[2 * k] + v[2 * k + 1], v[2 * k + 1] + v[2 * k + 1], v[2 * k + 1] + v[2 * k + 2]);
  return m;
}
// the same for a semi-planar chunk: a = four (Cb, Cr) pairs (Cb in the low
// half of each word), h = the pair right of them, codes already shifted down
// and masked; tt: row tt >> 3, 4-pair chunk tt & 7 of the tile's 18 x 8
// chunks.  Both planes' rows leave in one call, same arithmetic per sample
template <int HST>
__device__ __forceinline__ float stage_chroma_semi(float* plane_u, float* plane_v, uint4 a, unsigned h, int tt, float cmid) {
  const unsigned w[5] = {a.x, a.y, a.z, a.w, h};
  float u[5], v[5];
#pragma unroll
  for (int k = 0; k < 5; k++) u[k] = (float)(w[k] & 0xffff) - cmid, v[k] = (float)(w[k] >> 16) - cmid;
  float m = __builtin_fmaxf(fabsf(u[0]), fabsf(v[0]));
#pragma unroll
  for (int k = 1; k < 5; k++) m = __builtin_fmaxf(m, __builtin_fmaxf(fabsf(u[k]), fabsf(v[k])));
  const int o = (tt >> 3) * HST + 8 * (tt & 7);
#pragma unroll
  for (int k = 0; k < 2; k++) {
    *reinterpret_cast<float4*>(plane_u + o + 4 * k) =
        make_float4(u[2 * k] + u[2 * k], u[2 * k] + u[2 * k + 1], u[2 * k + 1] + u[2 * k + 1], u[2 * k + 1] + u[2 * k + 2]);
    *reinterpret_cast<float4*>(plane_v + o + 4 * k) =
        make_float4(v[2 * k] + v[2 * k], v[2 * k] + v[2 * k + 1], v[2 * k + 1] + v[2 * k + 1], v[2 * k + 1] + v[2 * k + 2]);
  }
  return m;
}
// 4:2:2 input (SUB 1): the chunk's centred codes as they are (x1: the
// horizontal pass runs in the step), row stride C422_ST floats; tt: row
// tt >> 2, chunk tt & 3 of the tile's 32 x 4 chunks; a row's last chunk also
// stores its right-halo sample h (column 32; the other chunks' h is not
// loaded).  Returns the largest |centred code| of what the chunk stages, so
// the tile's flag sees every staged sample
constexpr int C422_ST = 36;   // 33 samples; rows 16-byte aligned, 8 rows of a step on distinct bank groups
constexpr int C444_ST = 72;   // 4:4:4: 64 16-bit centred codes per row (+ pad: rows 36 banks apart)
__device__ __forceinline__ float stage_chroma422(float* plane, uint4 a, unsigned h, int tt, float cmid) {
  float v[9];
  unpack8(a, v);
  v[8] = (float)h;
#pragma unroll
  for (int k = 0; k < 9; k++) v[k] -= cmid;
  float m = fabsf(v[0]);
#pragma unroll
  for (int k = 1; k < 8; k++) m = __builtin_fmaxf(m, fabsf(v[k]));
  float* d = plane + (tt >> 2) * C422_ST + 8 * (tt & 3);
  *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
  if ((tt & 3) == 3) d[8] = v[8], m = __builtin_fmaxf(m, fabsf(v[8]));
  return m;
}
// 4:4:4 input (SUB 2): a chunk of each plane as 16-bit centred codes (exact:
// |code - mid| <= 2048), one 16-byte store per plane at (row, 8 col8)
__device__ __forceinline__ float stage_chroma444(float* plane_u, float* plane_v, uint4 a, uint4 b, int row, int col8,
                                                 int imid) {
  auto pack = [&](uint4 q, float* plane, float& m) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    unsigned o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int lo = (int)(w[k] & 0xffff) - imid, hi = (int)(w[k] >> 16) - imid;
      m = __builtin_fmaxf(m, __builtin_fmaxf(fabsf((float)lo), fabsf((float)hi)));
      o[k] = ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16);
    }
    *reinterpret_cast<uint4*>(reinterpret_cast<int16_t*>(plane) + row * C444_ST + 8 * col8) = make_uint4(o[0], o[1], o[2], o[3]);
  };
  float m = 0.0f;
  pack(a, plane_u, m);
  pack(b, plane_v, m);
  return m;
}
// luma codes of tile row r, chunk c (8 pixels) for the store: the 16 bytes as
// they lie in LDS, or (8-bit output) their low bytes in .xy by two permutes
__device__ __forceinline__ u4v read_luma(const FastParams& F, const unsigned char* yin, int r, int c) {
  const uint4 a = *reinterpret_cast<const uint4*>(yin + luma_at(8 * c, r));
  if (F.out8)
    return u4v{__builtin_amdgcn_perm(a.y, a.x, 0x06040200u), __builtin_amdgcn_perm(a.w, a.z, 0x06040200u), 0u, 0u};
  return u4v{a.x, a.y, a.z, a.w};
}
// Store rule (the loads' rule, tile_load): every thread issues exactly one
// luma and one chroma store per tile, the same 16-byte instruction on every
// path and under no branch, so the compiler counts them and its vmcnt waits
// for the next tile's loads leave them outstanding (k_tile's commit).  A
// branch around a store, even a block-uniform one between an 8-byte and a
// 16-byte arm, leaves a path without it in the compiler's count.  A thread
// with nothing to store (a row past the frame, no chroma role, the BICUBIC
// scratch path) stores at ST_DROP, an offset at or past every plane extent
// (those are clamped to 2^31 - 1, the offset is unsigned and the scalar
// origin takes no part in the range check): the hardware drops it.
// 8-bit output (v.xy = the thread's 8 bytes): threads t and t ^ 1 hold
// neighbouring chunks of one row, so the even one stores both (the odd
// thread's words by a DPP quad permute) and the odd one drops its store
constexpr int ST_DROP = (int)0x80000000u;
__device__ __forceinline__ void tile_store(const FastParams& F, u4v v, __amdgpu_buffer_rsrc_t rs, int vo, int so, int t) {
  if (F.out8) {   // block-uniform
    v.z = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v.x, 0xB1, 0xF, 0xF, false);
    v.w = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v.y, 0xB1, 0xF, 0xF, false);
    if (t & 1) vo = ST_DROP;
  }
  __builtin_amdgcn_raw_buffer_store_b128(v, rs, vo, so, NTS);
}
__device__ __forceinline__ void put_luma(const FastParams& F, const TileGeo& g, u4v v, int r, int vo, int t) {
  if (g.py0 + r >= F.H) vo = ST_DROP;
  const __amdgpu_buffer_rsrc_t oy_ = plane_rsrc(F.out[0] + g.f * F.out_fp[0], F.out_bytes[0]);
  tile_store(F, v, oy_, vo, g.py0 * (int)F.out_ls[0] + (F.out8 ? g.px0 : 2 * g.px0), t);
}
// chroma plane pl, row r, chunk c (8 samples): ((c0 + c1) + (c2 + c3)) + bias,
// quantised once per sample, packed as read_luma
__device__ __forceinline__ u4v read_chroma(const FastParams& F, const float* csum, int pl, int r, int c) {
  const float4* src = reinterpret_cast<const float4*>(csum + pl * (CBH * CBW) + csum_at(8 * c, r));
  const float4 v0 = src[0], v1 = src[1];
  const float vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  unsigned code[8];
  if (F.dither) {   // S6 ordered dither: sample (cx, cy) mod 8 = (k, r mod 8)
#pragma unroll
    for (int k = 0; k < 8; k++) code[k] = (unsigned)(int)(vv[k] + (F.c_bias - 0.5f + dither_off(k, r)));
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) code[k] = (unsigned)(int)(vv[k] + F.c_bias);
  }
  if (F.rep_rs == 31) {   // plain shift (block-uniform); else bit replication (h2s_expand)
#pragma unroll
    for (int k = 0; k < 8; k++) code[k] <<= F.shift_out;
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) code[k] = (code[k] << F.shift_out) | (code[k] >> F.rep_rs);
  }
  if (F.out8)
    return u4v{code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24),
               code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24), 0u, 0u};
  return u4v{code[0] | (code[1] << 16), code[2] | (code[3] << 16), code[4] | (code[5] << 16), code[6] | (code[7] << 16)};
}
// (vo: the lane's offset, or ST_DROP; semi: the interleaved plane, pl = 0, of
// a semi-planar output, two codes per chroma column.  One store for both
// layouts: see the store rule)
__device__ __forceinline__ void put_chroma(const FastParams& F, const TileGeo& g, u4v v, int pl, bool semi, int vo, int t) {
  const __amdgpu_buffer_rsrc_t oc_ = plane_rsrc(F.out[1 + pl] + g.f * F.out_fp[1 + pl], F.out_bytes[1 + pl]);
  tile_store(F, v, oc_, vo, g.cy0 * (int)F.out_ls[1 + pl] + ((F.out8 ? g.cx0 : 2 * g.cx0) << (semi ? 1 : 0)), t);
}

// semi-planar output: row r, chunk c (four (Cb, Cr) pairs) of the tile's 16 x
// 8 chunks, quantised as read_chroma, packed as pairs for one 16-byte store
// (u16: the code in the word's high bits, F.out_sh) or 8-byte store (nv12: .xy)
__device__ __forceinline__ u4v read_chroma_semi(const FastParams& F, const float* csum, int r, int c) {
  const float4 vu = *reinterpret_cast<const float4*>(csum + csum_at(4 * c, r));
  const float4 vv = *reinterpret_cast<const float4*>(csum + CBH * CBW + csum_at(4 * c, r));
  const float s[8] = {vu.x, vv.x, vu.y, vv.y, vu.z, vv.z, vu.w, vv.w};
  unsigned code[8];
  if (F.dither) {   // sample (cx, cy) mod 8 = (4 (c & 1) + k / 2, r mod 8)
#pragma unroll
    for (int k = 0; k < 8; k++) code[k] = (unsigned)(int)(s[k] + (F.c_bias - 0.5f + dither_off(4 * (c & 1) + (k >> 1), r)));
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) code[k] = (unsigned)(int)(s[k] + F.c_bias);
  }
  if (F.rep_rs == 31) {
#pragma unroll
    for (int k = 0; k < 8; k++) code[k] <<= F.shift_out;
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) code[k] = (code[k] << F.shift_out) | (code[k] >> F.rep_rs);
  }
  if (F.out8)
    return u4v{code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24),
               code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24), 0u, 0u};
  return u4v{(code[0] | (code[1] << 16)) << F.out_sh, (code[2] | (code[3] << 16)) << F.out_sh,
             (code[4] | (code[5] << 16)) << F.out_sh, (code[6] | (code[7] << 16)) << F.out_sh};
}

}  // namespace h2s
