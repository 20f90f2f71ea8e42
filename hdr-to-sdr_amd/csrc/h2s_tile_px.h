// h2s_tile_px.h — one pixel through the tile kernel's chain S1..S7 (px_chain;
// h2s_tile.h has the overview).  What belongs here: the composition of S1 and
// S2 (h2s_tile_tone.h) with the dark re-run (lin_tone), the Dolby Vision
// front-end (dovi_tile_front), the libplacebo branch's table read and Y'CbCr
// (lp_table_read, lp_ycbcr), the lattice blend and the eq lookup (px_chain),
// the step's VGPR constants (StepK, in_vgpr, in_vgpr64) and the quad
// reduction.  Nothing here knows where a pixel lies in a tile or a frame: that
// is h2s_tile_io.h's.
#pragma once
#include "h2s_tile_tone.h"

// Round-4 VALU trims of the step (the forms they replaced are
// kept as a patch, profiles/tile_split/ab_patches):
//  (TAG)         tetrahedron from axis-tagged fractions + a 3-entry LDS
//                offset table, one-key uniformity test (9 + 6 half-rate ops -> 6)
//  (EXPCLAMP)    lut3d's [0, N-1] clamp as v_exp_f32's output clamp
//  (EQM)         eq index by a 2^23 add and a 16-bit shift (full-rate ops)

namespace h2s {

typedef float f3 __attribute__((ext_vector_type(3)));

typedef unsigned u2v __attribute__((ext_vector_type(2)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

// a global pointer held in a VGPR pair (address space 1: the loads through it
// are global_load, counted in vmcnt only -- a flat load would also count in
// lgkmcnt, so every LDS wait would wait for it too)
typedef __attribute__((address_space(1))) const unsigned gu32;
__device__ __forceinline__ gu32* in_vgpr64(const unsigned* x) {
  gu32* y;
  asm volatile("v_mov_b64 %0, %1" : "=v"(y) : "s"((gu32*)x));
  return y;
}

// hot constants the kernels keep in VGPRs for their whole run (in_vgpr)
struct StepK {
  float a_rv, a_gv, a_gu, a_bu;   // chroma terms of E, x ESC
  float stride_g, stride_b;       // lattice byte strides (as floats)
  int og, ob, ocr, ocg, ocb;      // corner byte offsets
  float log2_nm1, x_max;
  float hable_kb;                 // F.hable_kb (Hable instances)
  int c111;                       // the far corner's byte offset
  float nm1;                      // N - 1
  const int* offtab;              // LDS: byte offset of the +1 corner along r, g, b at bytes 0, 4, 8
  float lp_k2, lp_hi, lp_cy;      // LP: the encode's clamp bounds lp_k2, 255 + lp_k2; lp_cy + ydq
  float lp_k1;                    // LP: the encode's exponent offset (a VGPR: it meets a literal)
};

// S1 + S2 of one pixel (px_chain, lp_front): staged luma ybs (Y*ys + y_off,
// +1 on PQ), x8-upsampled centred chroma U, V -> the tone-mapped linear
// R, G, B, with the dark re-run below.  dput: the debug planes' writer (DBG
// = 1: the planes of F.dbg_stage, a launch-uniform test at each site; DBG = 0
// compiles every site away)
// The Dolby Vision profile-5 front-end of the tile kernel (TRC 2; model:
// include/h2s.h, steps 1-3): the pixel's code fractions -> L'M'S' in the EOTF
// table's coordinate v PQ_SEG + 1.  R is the tile's frame record (block-
// uniform: its fields come through the scalar cache).  The shape the tile
// kernel takes (h2s_api_dovi.hip dovi_tile_shape; any other record runs on
// the generic kernel): luma polynomial pieces only, selected by a compare per
// pivot; each chroma component one piece, polynomial or MMR up to order 3
// (the record through the constant address space, so that a block-uniform
// address gives scalar loads, as curve_of's)
typedef __attribute__((address_space(4))) const DoviRec CDoviRec;
typedef __attribute__((address_space(4))) const DoviCurve CDoviCurve;
__device__ __forceinline__ void dovi_tile_front(CDoviRec& R, float s0, float s1, float s2, float& er, float& eg,
                                                float& eb) {
  CDoviCurve& Y = R.comp[0];
  const int last = Y.num_pivots - 2;
  float a0 = Y.poly[0][0], a1 = Y.poly[0][1], a2 = Y.poly[0][2];
#pragma unroll
  for (int i = 1; i < 8; i++) {
    if (i <= last) {   // (block-uniform)
      const bool hit = Y.pivots[i] <= s0;
      a0 = hit ? Y.poly[i][0] : a0, a1 = hit ? Y.poly[i][1] : a1, a2 = hit ? Y.poly[i][2] : a2;
    }
  }
  const float r0 = __builtin_amdgcn_fmed3f(fmaf(fmaf(a2, s0, a1), s0, a0), Y.pivots[0], Y.pivots[last + 1]);
  // a chroma component's one piece (piece 0: every load has a block-uniform address)
  const float t[7] = {s0, s1, s2, s0 * s1, s0 * s2, s1 * s2, s0 * s1 * s2};
  auto chroma = [&](CDoviCurve& C, float x) -> float {
    float r;
    if (C.method[0] == 0) {   // (block-uniform)
      r = fmaf(fmaf(C.poly[0][2], x, C.poly[0][1]), x, C.poly[0][0]);
    } else {
      r = C.mmr_const[0];
      float p[7];
#pragma unroll
      for (int j = 0; j < 7; j++) p[j] = t[j];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        if (i < C.mmr_order[0]) {   // (block-uniform)
#pragma unroll
          for (int j = 0; j < 7; j++) {
            r = fmaf(C.mmr[0][i][j], p[j], r);
            p[j] *= t[j];
          }
        }
      }
    }
    return __builtin_amdgcn_fmed3f(r, C.pivots[0], C.pivots[1]);
  };
  const float d0 = r0 - R.off[0];
  const float d1 = chroma(R.comp[1], s1) - R.off[1];
  const float d2 = chroma(R.comp[2], s2) - R.off[2];
  auto row = [&](int c) {
    const float v = clamp01(fmaf(R.nl[3 * c], d0, fmaf(R.nl[3 * c + 1], d1, R.nl[3 * c + 2] * d2)));
    return fmaf(v, (float)PQ_SEG, 1.0f);
  };
  er = row(0), eg = row(1), eb = row(2);
}

// dv (TRC 2): the tile's Dolby Vision record
template <int TRC, int TM, int DESAT, int LP, int DBG, bool NOEX, class DPut>
__device__ __forceinline__ void lin_tone(const FastParams& F, const CurveConsts& cv, const float4* pq_lds,
                                         const float4* pqi_lds, const StepK& K, float ybs, float U, float V,
                                         const DPut& dput, float& r, float& gg, float& bl,
                                         const CDoviRec* dv = nullptr) {
  if constexpr (TRC == 2) {
    // ybs is the luma fraction (staged unscaled); chroma back from x8 centred codes
    static_assert(TRC != 2 || LP == 1, "Dolby Vision: the libplacebo branch");
    H2S_MARK("S1a DoVi reshape, non-linear matrix");
    float er, eg, eb;
    dovi_tile_front(*dv, ybs, fmaf(U, F.dv_cs, F.dv_cm), fmaf(V, F.dv_cs, F.dv_cm), er, eg, eb);
    H2S_MARK("S1b EOTF, linear matrix");
    // L, M, S (units of npl) from the EOTF table, then the record's linear matrix
    auto s1 = [&](auto dark, float& o0, float& o1, float& o2) -> float {
      float l0, l1, l2;
      to_linear<0, PQ_SEG, true, decltype(dark)::value>(F, pq_lds, er, eg, eb, l0, l1, l2);
      o0 = fmaf(dv->lin[0], l0, fmaf(dv->lin[1], l1, dv->lin[2] * l2));
      o1 = fmaf(dv->lin[3], l0, fmaf(dv->lin[4], l1, dv->lin[5] * l2));
      o2 = fmaf(dv->lin[6], l0, fmaf(dv->lin[7], l1, dv->lin[8] * l2));
      return (l0 + l1) + l2;   // (a marked first-segment read shows here: L, M, S >= 0 do not cancel)
    };
    const float s1probe = s1(std::false_type{}, r, gg, bl);
    if (DBG && F.dbg_stage == 1) {
      float r1, g1, b1;
      s1(std::true_type{}, r1, g1, b1);
      dput(r1, g1, b1);
    }
    float luma = 0.0f;
    tone<0, TM, DESAT, LP, false, true>(F, cv, pq_lds, pqi_lds, r, gg, bl, false, 0.0f, K.hable_kb, luma);
    float probe = ((fabsf(r) + fabsf(gg)) + fabsf(bl)) + s1probe;
    if constexpr (TM >= 4 && TM <= 6) probe += luma;
    if (__builtin_amdgcn_ballot_w64(!(probe <= DARK_MARK))) {
      H2S_MARK("rare: dark re-run");
      s1(std::true_type{}, r, gg, bl);
      tone<0, TM, DESAT, LP, true, true>(F, cv, pq_lds, pqi_lds, r, gg, bl, false, 0.0f, K.hable_kb, luma);
    }
    return;
  }
  // E in table-segment units for the table forms: the PQ EOTF, and the HLG
  // inverse OETF on the CPU chain (the libplacebo branch keeps direct HLG)
  constexpr int ESC = TRC == 0 || !LP ? PQ_SEG : 1;
  H2S_MARK("S1a E");
  const float er = fmaf(V, K.a_rv, ybs);
  const float eg = fmaf(V, K.a_gv, fmaf(U, K.a_gu, ybs));
  const float eb = fmaf(U, K.a_bu, ybs);
  H2S_MARK("S1b EOTF");
  const bool safe = to_linear<TRC, ESC, NOEX>(F, pq_lds, er, eg, eb, r, gg, bl);
  H2S_MARKV("S2 tone", r, gg, bl);
  if (DBG && F.dbg_stage == 1) {   // the stage-1 planes with the first segment exact, as the dark re-run below gives them
    float r1, g1, b1;
    to_linear<TRC, ESC, NOEX, true>(F, pq_lds, er, eg, eb, r1, g1, b1);
    dput(r1, g1, b1);
  }
  const float emax_s = __builtin_fmaxf(__builtin_fmaxf(er, eg), eb);
  // S1's own marked channels are probed before the tone map wherever the
  // tone map can drop the mark: the libplacebo branch's IPT form caps its
  // input at 1e6 npl, and a max(R,G,B) gain without desaturation scales the
  // marked channel back to the curve's output (k = curve(sig) / sig)
  constexpr bool S1P = TRC == 0 && (LP || !(DESAT && TM <= 6));
  const float s1probe = S1P ? (r + gg) + bl : 0.0f;
  float luma = 0.0f;
  tone<TRC, TM, DESAT, LP>(F, cv, pq_lds, pqi_lds, r, gg, bl, safe, emax_s, K.hable_kb, luma);
  H2S_MARKV("S2z dark probe", r, gg, bl);
  // The EOTF table's first segment is marked wherever it is read (S1 on PQ
  // input; the libplacebo branch's IPT decode and curve reads): a value that
  // reached it is huge (> DARK_MARK) in S1's output or the tone map's.  The
  // CPU chain's desaturating instances see it in their luma for free, the
  // others sum the channels' magnitudes (and S1's, S1P); a wave that meets one re-runs S1 and S2
  // with that segment evaluated exactly (about 1 % of the bench content's
  // 8x8 steps)
  if constexpr (TRC == 0 || LP) {
    float probe;
    if constexpr (!LP && DESAT && TM <= 6) {
      probe = luma;
    } else {
      probe = (fabsf(r) + fabsf(gg)) + fabsf(bl);   // (the IPT rows mix signs: magnitudes do not cancel)
      if constexpr (S1P) probe += s1probe;
      if constexpr (LP && TM >= 4 && TM <= 6) probe += luma;   // the NORM curve's decoded intensity
    }
    if (__builtin_amdgcn_ballot_w64(!(probe <= DARK_MARK))) {   // (NaN / inf from a marked value too)
      H2S_MARK("rare: dark re-run");
      const bool safe2 = to_linear<TRC, ESC, NOEX, true>(F, pq_lds, er, eg, eb, r, gg, bl);
      tone<TRC, TM, DESAT, LP, true>(F, cv, pq_lds, pqi_lds, r, gg, bl, safe2, emax_s, K.hable_kb, luma);
    }
  }
}

// The libplacebo branch's rgba8 download and lut3d table read (S3, S4) of one
// pixel from its tone-mapped linear R, G, B: the BT.1886 encode against the
// target black, 255 x it rounded to the 8-bit rgba code (qoff: the range=tv
// and rounding / dither offsets, h2s_lp_range / _dither, less lp_k2 lp_qs_f:
// the encode's - lp_k2 is folded into the clamp's bounds K.lp_k2 / K.lp_hi;
// all offsets >= 0, so the conversion's truncation is the floor).
// Everything after the download -- lut3d's 8-bit coordinate (q / 255)
// (N-1), the tetrahedral blend in vf_lut3d's order, the truncation to 8 bits
// -- is a function of the three codes alone, so it is one read of the
// context's 2^24-entry table of lut3d's 8-bit outputs (k_build_lut8x: the
// generic kernel's own lut3d_8bit arithmetic, bit for bit), instead of a
// lattice cell, four gathers and the blend per pixel (round 6, VERDICT r05
// item 2).  Returns the table entry (R | G << 8 | B << 16) as loaded: the
// caller decides where to wait for it
__device__ __forceinline__ unsigned lp_table_read(const FastParams& F, const StepK& K, gu32* lut8v,
                                                  const unsigned* spread_lds, float r, float gg, float bl,
                                                  float qoff) {
  auto q8 = [&](float x) -> unsigned {
    const float e = fexp2(fmaf(flog2(__builtin_amdgcn_fmed3f(x, 0.0f, F.lp_xmax)), 1.0f / 2.4f, K.lp_k1));
    return (unsigned)fmaf(__builtin_amdgcn_fmed3f(e, K.lp_k2, K.lp_hi), F.lp_qs_f, qoff);
  };
  unsigned idx;
  const unsigned qr = q8(r), qg = q8(gg), qb = q8(bl);
  H2S_MARK("S4 lut3d table read");
  // the table's bit-interleaved (Morton) index: nearby colours share lines
  asm("v_lshl_or_b32 %0, %1, 1, %2" : "=v"(idx) : "v"(spread_lds[qb]), "v"(spread_lds[qg]));
  asm("v_lshl_or_b32 %0, %1, 1, %2" : "=v"(idx) : "v"(idx), "v"(spread_lds[qr]));
  // (a global load from a 64-bit VGPR base, one shift-add for the address:
  // the table's buffer descriptor took four SGPRs that the LP instances
  // spill, i.e. four lane reads per step)
  return lut8v[idx];
}

// BT.709 limited-range Y'CbCr at depth q straight from lut3d's 8-bit output
// codes (FastParams lp_ky / lp_kcb / lp_kcr: the rows x 1/255 x the depth
// scales, folded on the host): o = (luma code + 0.5, 56 q Cb, 56 q Cr)
__device__ __forceinline__ f3 lp_ycbcr(const FastParams& F, const StepK& K, float R8, float G8, float B8) {
  f3 o;
  o.x = fmaf(F.lp_ky[0], R8, fmaf(F.lp_ky[1], G8, fmaf(F.lp_ky[2], B8, K.lp_cy)));
  o.y = fmaf(F.lp_kcb[0], R8, fmaf(F.lp_kcb[1], G8, F.lp_kcb[2] * B8));
  o.z = fmaf(F.lp_kcr[0], R8, fmaf(F.lp_kcr[1], G8, F.lp_kcr[2] * B8));
  return o;
}

// One pixel through S1..S7 (both tile kernels): staged luma ybs (Y*ys +
// y_off, +1 on PQ), x8-upsampled centred chroma U, V -> the eq'd luma code at
// the output depth (returned) and the pixel's two chroma quantiser
// contributions (oyv, ozv) for the 2x2 sum.  di: this pixel's index in the
// debug planes (DBG > 0, frame 0), else -1.  (The libplacebo branch's
// product steps run lin_tone / lp_table_read / lp_ycbcr software-pipelined
// instead: k_tile's steps.)
template <int TRC, int TM, int DESAT, int LP, int DBG, bool NOEX = false>
__device__ __forceinline__ unsigned px_chain(const FastParams& F, const CurveConsts& cv, const float4* pq_lds,
                                             const float4* pqi_lds, const uint16_t* eq_lds, gu32* lut8v, const unsigned* spread_lds,
                                             __amdgpu_buffer_rsrc_t lut, const StepK K, float ybs, float U, float V,
                                             long long di, float& oyv, float& ozv, float qoff, float ydq,
                                             const CDoviRec* dv = nullptr) {
  constexpr bool EQM = !LP;   // see the eq lookup at the end
  const long long dpl = (long long)F.dbg_w * F.H;
  auto dput = [&](float a, float b_, float c) {
    if (di >= 0) F.dbg[di] = a, F.dbg[dpl + di] = b_, F.dbg[2 * dpl + di] = c;
  };
  float r, gg, bl;
  lin_tone<TRC, TM, DESAT, LP, DBG, NOEX>(F, cv, pq_lds, pqi_lds, K, ybs, U, V, dput, r, gg, bl, dv);
  H2S_MARKV("S3 encode", r, gg, bl);
  if (DBG && F.dbg_stage == 2) dput(r, gg, bl);
  f3 o;
  if (LP && F.lut_off) {
    // LUT off: libplacebo's BT.2020 -> BT.709 matrix on the linear
    // values, the BT.1886 encode clipped to [0, 1] (no rgba rounding: the
    // branch downloads nv12), then Y'CbCr at depth q as below
    // (255-scaled, into the same folded Y'CbCr rows as the 8-bit codes below)
    auto enc = [&](float x) -> float {
      const float e = fexp2(fmaf(flog2(__builtin_amdgcn_fmed3f(x, 0.0f, F.lp_xmax)), 1.0f / 2.4f, F.lp_k1)) - F.lp_k2;
      return __builtin_amdgcn_fmed3f(e, 0.0f, 255.0f);
    };
    const float R = enc(F.m709[0] * r + F.m709[1] * gg + F.m709[2] * bl);
    const float G = enc(F.m709[3] * r + F.m709[4] * gg + F.m709[5] * bl);
    const float B = enc(F.m709[6] * r + F.m709[7] * gg + F.m709[8] * bl);
    if (DBG && (F.dbg_stage == 3 || F.dbg_stage == 4)) dput(R * F.inv255, G * F.inv255, B * F.inv255);
    o.x = fmaf(F.lp_ky[0], R, fmaf(F.lp_ky[1], G, fmaf(F.lp_ky[2], B, K.lp_cy)));
    o.y = fmaf(F.lp_kcb[0], R, fmaf(F.lp_kcb[1], G, F.lp_kcb[2] * B));
    o.z = fmaf(F.lp_kcr[0], R, fmaf(F.lp_kcr[1], G, F.lp_kcr[2] * B));
  } else if constexpr (LP) {
    if (DBG && F.dbg_stage == 3) {
      auto ev = [&](float x) {
        const float e = fexp2(fmaf(flog2(__builtin_amdgcn_fmed3f(x, 0.0f, F.lp_xmax)), 1.0f / 2.4f, F.lp_k1)) - F.lp_k2;
        return __builtin_amdgcn_fmed3f(e, 0.0f, 255.0f) * F.inv255;
      };
      dput(ev(r), ev(gg), ev(bl));
    }
    const unsigned v = lp_table_read(F, K, lut8v, spread_lds, r, gg, bl, qoff);
    const float R8 = (float)(v & 255u), G8 = (float)((v >> 8) & 255u), B8 = (float)((v >> 16) & 255u);   // (v_cvt_f32_ubyte0..2)
    H2S_MARK("S5 Y'CbCr");
    if (DBG && F.dbg_stage == 4) dput(R8 * F.inv255, G8 * F.inv255, B8 * F.inv255);
    o = lp_ycbcr(F, K, R8, G8, B8);
  } else {
    // lattice cell origins (cr, cg, cb) and fractions (dr, dg, db) per channel
    float cr, cg, cb, dr, dg, db;
    {
      float sr, sg, sb;
      // S3+S4: s = (N-1) x^(1/2.4) with x clamped to [0, K.x_max] (NaN -> 0), so
      // s < N-1 and the lattice cell index never needs a clamp
      // lut3d's clamp to [0, N-1] (NaN -> 0) as the exp's output clamp:
      // x^(1/2.4) clamped to [0, 1] (v_exp_f32 ... clamp; a NaN from the log
      // of a negative or NaN x clamps to 0), then N - 1 times that.  s may
      // reach N-1 exactly: its corners past the lattice edge get weight 0
      // (zero fraction), and the lattice allocation is padded for them
      sr = __builtin_amdgcn_fmed3f(fexp2(flog2(r) * (1.0f / 2.4f)), 0.0f, 1.0f) * K.nm1;
      sg = __builtin_amdgcn_fmed3f(fexp2(flog2(gg) * (1.0f / 2.4f)), 0.0f, 1.0f) * K.nm1;
      sb = __builtin_amdgcn_fmed3f(fexp2(flog2(bl) * (1.0f / 2.4f)), 0.0f, 1.0f) * K.nm1;
      // s is a product when N-1 is not a power of two (N-1 times the clamped
      // power): without this barrier the compiler contracts the cell origin
      // s - fract(s) below into fma(N-1, x, -fract(s)), which carries the
      // product's rounding error, so the origin is no longer an integer and a
      // byte offset truncates to a misaligned record (N = 177: 45 of 3072
      // samples of a uniform frame)
      asm("" : "+v"(sr), "+v"(sg), "+v"(sb));
      H2S_MARKV("S4a cell, fractions", sr, sg, sb);
      dr = __builtin_amdgcn_fractf(sr), dg = __builtin_amdgcn_fractf(sg), db = __builtin_amdgcn_fractf(sb);
      cr = sr - dr, cg = sg - dg, cb = sb - db;
    }
    H2S_MARKV("S4b tetrahedron select", dr, dg, db);
    const int base = (int)fmaf(cb, K.stride_b, fmaf(cg, K.stride_g, cr * 12.0f));
    // TAG (the CPU chain): tetrahedron by sorting axis-tagged
    // fractions: the 4 low mantissa bits of each fraction carry its axis a
    // (bits 3:2 and 1:0 both = a; r 0, g 1, b 2; a change of <= 2^-19
    // relative in the weights), so max3 / min3 / med3 of the bit patterns
    // (non-negative floats order as integers) give the sorted fractions and
    // the axes of the largest and smallest; the corner offsets come from a
    // 3-entry LDS table (om = +1 along the max axis, ocn = the far corner less
    // the min axis), not from compares and selects (9 half-rate VALU ops ->
    // 3).  (Not for the libplacebo branch's 8-bit coordinates, whose exact
    // ties between fractions the tags would break: that branch reads its
    // table above.)
    int om, ocn;
    float dmax, dmin, dmid;
    unsigned umin = 0, amax = 0;
    {
      const unsigned ur = __builtin_bit_cast(unsigned, dr) & ~15u;
      const unsigned ug = (__builtin_bit_cast(unsigned, dg) & ~15u) | 5u;
      const unsigned ub = (__builtin_bit_cast(unsigned, db) & ~15u) | 10u;
      unsigned umax, umid;
      asm("v_max3_u32 %0, %1, %2, %3" : "=v"(umax) : "v"(ur), "v"(ug), "v"(ub));
      asm("v_min3_u32 %0, %1, %2, %3" : "=v"(umin) : "v"(ur), "v"(ug), "v"(ub));
      asm("v_med3_u32 %0, %1, %2, %3" : "=v"(umid) : "v"(ur), "v"(ug), "v"(ub));
      amax = umax & 12u;
      const unsigned amin = umin & 12u;
      om = *reinterpret_cast<const int*>(reinterpret_cast<const char*>(K.offtab) + amax);
      ocn = K.c111 - *reinterpret_cast<const int*>(reinterpret_cast<const char*>(K.offtab) + amin);
      dmax = __builtin_bit_cast(float, umax), dmin = __builtin_bit_cast(float, umin), dmid = __builtin_bit_cast(float, umid);
    }
    H2S_MARKV("S4c weights, uniformity, gathers, blend", dmax, dmid, dmin);
    const float w0 = 1.0f - dmax, w1 = dmax - dmid, w2 = dmid - dmin, w3 = dmin;
    auto blend = [&](const f3 c0, const f3 c1, const f3 c2, const f3 c3) {
      f3 r = w0 * c0 + w1 * c1 + w2 * c2 + w3 * c3;
      // the luma quantiser's ordered-dither offset (ydq = d - 0.5, 0 without
      // dither: the record's +0.5 rounds) as the blend's first term (FMA for MUL)
      r.x = fmaf(w3, c3.x, fmaf(w2, c2.x, fmaf(w1, c1.x, fmaf(w0, c0.x, ydq))));
      return r;
    };
    // when every lane of the step is in one cell and one tetrahedron, its
    // four records come through the scalar cache and the step issues no
    // vector-memory gather (bit-identical; C2 -1.8 % smooth, -5 % on the
    // website frame: profiles/r03/ablations/sgather_*.log)
    bool step_uniform;
    int b0, m0, n0;
    {
      // one key per lane: cell (base) and tetrahedron (the max and min axes)
      unsigned tkey, key;
      asm("v_and_or_b32 %0, %1, 3, %2" : "=v"(tkey) : "v"(umin), "v"(amax));
      asm("v_lshl_or_b32 %0, %1, 4, %2" : "=v"(key) : "v"(base), "v"(tkey));
      const unsigned key0 = __builtin_amdgcn_readfirstlane(key);
      step_uniform = __builtin_amdgcn_ballot_w64(key != key0) == 0;
      b0 = 0, m0 = 0, n0 = 0;
      if (step_uniform) {
        b0 = (int)(key0 >> 4);
        m0 = __builtin_amdgcn_readfirstlane(om), n0 = __builtin_amdgcn_readfirstlane(ocn);
      }
    }
    if (step_uniform) {
      typedef __attribute__((address_space(4))) const float cfl;
      cfl* L = (cfl*)F.lut_yuv;
      auto sl = [&](int off) {
        const int i = off >> 2;
        return f3{L[i], L[i + 1], L[i + 2]};
      };
      o = blend(sl(b0), sl(b0 + m0), sl(b0 + n0), sl(b0 + F.c111));
    } else {
      o = blend(__builtin_amdgcn_raw_buffer_load_b96(lut, base, 0, 0), __builtin_amdgcn_raw_buffer_load_b96(lut, base + om, 0, 0),
                __builtin_amdgcn_raw_buffer_load_b96(lut, base + ocn, 0, 0),
                __builtin_amdgcn_raw_buffer_load_b96(lut, base, F.c111, 0));
    }
    if (DBG && F.dbg_stage == 3) dput((cr + dr) * F.inv_nm1, (cg + dg) * F.inv_nm1, (cb + db) * F.inv_nm1);   // = s exactly
    if (DBG && F.dbg_stage == 4) {  // same cell / corners / weights on the RGB lattice (12-byte record -> float4 index)
      const float4 q0 = F.dbg_lut[base / 12], q1 = F.dbg_lut[(base + om) / 12], q2 = F.dbg_lut[(base + ocn) / 12],
                   q3 = F.dbg_lut[(base + F.c111) / 12];
      dput(w0 * q0.x + w1 * q1.x + w2 * q2.x + w3 * q3.x, w0 * q0.y + w1 * q1.y + w2 * q2.y + w3 * q3.y,
           w0 * q0.z + w1 * q1.z + w2 * q2.z + w3 * q3.z);
    }
  }
  H2S_MARKV("S7 eq", o.x, o.y, o.z);
  if (DBG && F.dbg_stage == 5) dput(o.x - (EQM ? 0.0f : 0.5f) - ydq, 4.0f * o.y, 4.0f * o.z);
  oyv = o.y, ozv = o.z;
  if constexpr (EQM) {
    // o.x = the luma quantiser input less 0.5 (the lattice records carry no
    // +0.5): adding 2^23 rounds it to the nearest integer in the mantissa's
    // low bits, and a 16-bit shift turns that into the table's byte offset
    // (two full-rate ops instead of a conversion and a 32-bit shift-add; an
    // exact .5 tie rounds to even instead of up: continuous blends of the
    // CPU chain, not the libplacebo branch's 8-bit-derived values)
    const unsigned qb = __builtin_bit_cast(unsigned, o.x + 8388608.0f);
    unsigned off;
    asm("v_lshlrev_b16 %0, 1, %1" : "=v"(off) : "v"(qb));
    return *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(eq_lds) + off);
  } else {
    return eq_lds[(int)o.x];
  }
}

__device__ __forceinline__ float quad_sum(float v) {
  // (v0 + v1) + (v2 + v3) over the 2x2 pixels of a quad, in all 4 lanes
  // (quad_perm [1,0,3,2] pairs horizontally, then [2,3,0,1] adds the rows):
  // the oracle's summation order, so the chroma sum is bit-identical.  (The
  // lane moves as ds_swizzle through the LDS crossbar with full-rate adds:
  // 2-3 % slower, the swizzle latency sits in every step's chain;
  // profiles/r03/ablations/quad_sum_swizzle_*.log)
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
}

// keep a wave-uniform constant in a VGPR (avoids per-use SGPR->VGPR moves
// forced by the one-scalar-operand limit of VOP3 on gfx950)
template <class T>
__device__ __forceinline__ T in_vgpr(T x) {
  T y;
  asm volatile("v_mov_b32 %0, %1" : "=v"(y) : "s"(x));
  return y;
}

}  // namespace h2s
