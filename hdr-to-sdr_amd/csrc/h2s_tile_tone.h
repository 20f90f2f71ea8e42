// h2s_tile_tone.h — S1 and S2 of the tile kernel's per-pixel chain: from the
// pixel's E' to its tone-mapped linear R, G, B (h2s_tile.h has the overview).
// What belongs here: the readers of the EOTF / inverse-OETF and PQ-encode
// tables in LDS (pq_z, pq_z_dark, pqi) with the exact forms beside them, the
// transfer to linear (to_linear), every tone curve and the desaturation
// (tone), and the H2S_MARK stage markers that the whole chain uses.  How they
// are put together for one pixel, and everything after S2, is h2s_tile_px.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "h2s_dovi.h"
#include "h2s_math.h"
#include "h2s_params.h"

// The PQ table's first segment (E' < 1/128, below ~0.0015 nits), where the
// EOTF ~ (E - E0)^6.28 and no cubic holds 1e-3 relative, is staged as the
// cubic FLT_MAX t: exactly 0 at E = 0 (black, common in real content), and
// above DARK_MARK for every E in (0, 1/128).  The pixel's luma sum (or an
// explicit probe) carries such a channel to one wave-wide test; the rare
// waves that meet it re-run S1 and S2 with those channels exact.  No
// per-channel range test in the common path.

// Stage markers for the per-stage slot table (scripts/isa_stages.py): in a
// marked build (-DH2S_ISA_MARKS, ISA listing only, never linked) each is an
// assembler comment ";@@name" that opens stage `name` in the listing, with a
// scheduling barrier so that no instruction crosses it; the product build
// defines them away
#ifdef H2S_ISA_MARKS
#define H2S_MARK(name)                  \
  do {                                  \
    __builtin_amdgcn_sched_barrier(0);  \
    asm volatile(";@@" name);           \
    __builtin_amdgcn_sched_barrier(0);  \
  } while (0)
// the same, with three values pinned to the marker (read and rewritten by
// it), so that the IR passes cannot sink their computation past it
#define H2S_MARKV(name, a, b, c)                                  \
  do {                                                            \
    __builtin_amdgcn_sched_barrier(0);                            \
    asm volatile(";@@" name : "+v"(a), "+v"(b), "+v"(c));         \
    __builtin_amdgcn_sched_barrier(0);                            \
  } while (0)
#else
#define H2S_MARK(name)
#define H2S_MARKV(name, a, b, c)
#endif

namespace h2s {

// exact zimg st_2084_eotf x 2^log2_scale (S1: 10000/npl for PQ input; used
// above the table's range and in its first segment)
__device__ __forceinline__ float pq_exact_s(float e, float log2_scale) {
  const float xp = fexp2(flog2(fmaxf(e, 0.0f)) * (1.0f / PQ_M2));
  const float num = fmaxf(xp - PQ_C1, 0.0f);
  const float den = fmaxf(PQ_C2 - PQ_C3 * xp, 1.17549435e-38f);  // zimg: max(.., FLT_MIN)
  return fexp2(flog2(num * frcp(den)) * (1.0f / PQ_M1) + log2_scale);
}
__device__ __forceinline__ float pq_exact(const FastParams& F, float e) { return pq_exact_s(e, F.log2_lin_scale); }


// Zero-segment form used by k_tile: the LDS table holds a zero segment at
// index 0 and segment i of pq_tab at i+1, and the caller passes
// u = E*PQ_SEG + 1 (the +1 is folded into the staged luma).  v_cvt_u32_f32
// saturates negatives to 0, so E < 0 reads the zero segment (EOTF = 0) with no
// clamp; at and past PQZ_LIM the value is garbage and the caller takes the
// exact path.  The byte offset is formed with a 16-bit shift (full rate; bits
// 31:16 are written as zero on gfx950, and the index fits 12 bits).
__device__ __forceinline__ float pq_z(const float4* tab, float u) {
  unsigned off;
  asm("v_cvt_u32_f32 %0, %1\n\tv_lshlrev_b16 %0, 4, %0" : "=v"(off) : "v"(u));
  const float4 c = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tab) + off);
  const float t = __builtin_amdgcn_fractf(u);
  return fmaf(fmaf(fmaf(c.x, t, c.y), t, c.z), t, c.w);
}
// staged E (table-segment units, +1) at and above which pq_z is invalid
constexpr float PQZ_LIM = PQ_EMAX * (float)PQ_SEG + 1.0f;

// legitimate table values stay below ~1e10 (E < 1.875); the marked first
// segment gives >= FLT_MAX 2^-23 = 4e31 for any E > 0
constexpr float DARK_MARK = 1e30f;

// the EOTF-table read with its first segment (staged u in (1, 2)) evaluated
// exactly instead: the dark re-run of a wave (px_chain).  Only the lanes in
// that segment take the exact form (a divergent branch inside the rare re-run)
__device__ __forceinline__ float pq_z_dark(const float4* tab, float u, float log2_scale) {
  float v = pq_z(tab, u);
  if (u > 1.0f && u < 2.0f) v = pq_exact_s((u - 1.0f) * (1.0f / (float)PQ_SEG), log2_scale);
  return v;
}

// ST 2084 inverse EOTF of y = luminance / 10000 >= 0 from the LDS table
// (build_pqi_table): the segment is the float's exponent and top three
// mantissa bits, t the remaining 20 mantissa bits as [0, 1/8); the bit
// pattern is clamped (as a signed integer) to the table's octaves 2^-64 ..
// 2^14, where one pattern below the first octave reads entry 0, the constant
// PQ(0) = c1^m2: y <= 0 (black, or an LMS row of a saturated colour) exactly
// as the oracle's max(y, 0), and y below 2^-64 (1e-15 nits, within 3e-7 of
// PQ(0)).  The IPT form caps its input at 1e6 npl, inside the top octave.
// The near-black octaves matter: an LMS row of a dark pixel on synthetic
// content reaches 1e-13, and clamping at 2^-40 (PQ 1.4e-5 instead of down to
// 7.3e-7) put 0.5 % errors on stage-2 values of 1e-5.  Eight segments per
// octave, not four (round 5): the LMS encode error the decode amplifies (x
// ~11-45 through the EOTF's slope) drops from ~1e-6 to the float32 floor
// (scripts/c3_table_flips.py: the rgba8 download flips this table alone
// causes drop 7x); the 10 KB table puts the libplacebo instances above 32 KB
// of LDS, i.e. at 4 blocks per CU.  Round 6: 8 VALU instructions (integer
// med3, bfe, shift-add, and-or, add, 3 FMA) instead of 13 -- the clamp on the
// pattern replaces the segment clamp and the y <= 0 select
__device__ __forceinline__ float pqi(const float4* tab, float y) {
  constexpr int S0 = (127 + PQI_OCT0) << 3;                  // absolute segment of 2^-64
  constexpr int LO = (S0 - 1) << 20;                         // reads entry 0
  constexpr int HI = ((S0 + PQI_NSEG) << 20) - 1;            // the top segment's last pattern
  const int bc = min(max(__builtin_bit_cast(int, y), LO), HI);   // (v_med3_i32)
  unsigned sa;
  asm("v_bfe_u32 %0, %1, 20, 11" : "=v"(sa) : "v"(bc));      // absolute segment (sign bit is 0)
  const float4 c = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tab) + ((sa - (unsigned)(S0 - 1)) << 4));
  const float t = __builtin_bit_cast(float, ((unsigned)bc & 0xFFFFFu) | 0x3F800000u) - 1.0f;
  return fmaf(fmaf(fmaf(c.x, t, c.y), t, c.z), t, c.w);
}

// S1 transfer to linear (units of npl), specialised
// returns true (wave-uniform) when some lane of the wave took the exact PQ
// path: linear values may then be huge or infinite, and the tone curve must
// use its overflow-safe form
// NOEX: the caller knows no E reaches the table's end (a tile of legal codes,
// see k_tile): no ballot, no exact path, so a step has no branch
// DARK: the table's first segment exactly (pq_z_dark) instead of the NaN
template <int TRC, int ESC = 1, bool NOEX = false, bool DARK = false>
__device__ __forceinline__ bool to_linear(const FastParams& F, const float4* pq_lds, float er, float eg, float eb,
                                          float& r, float& g, float& b) {
  if (TRC == 0) {
    // E arrives as E*PQ_SEG + 1 (pq_z)
    static_assert(TRC != 0 || ESC == PQ_SEG, "PQ staging is in table-segment units");
    if (DARK) {
      r = pq_z_dark(pq_lds, er, F.log2_lin_scale), g = pq_z_dark(pq_lds, eg, F.log2_lin_scale);
      b = pq_z_dark(pq_lds, eb, F.log2_lin_scale);
    } else {   // a channel in the table's first segment is marked here (px_chain's dark re-run)
      r = pq_z(pq_lds, er), g = pq_z(pq_lds, eg), b = pq_z(pq_lds, eb);
    }
    constexpr float EI = 1.0f / (float)PQ_SEG;
    // NOEX (the fast body): the tile's codes keep every E inside the table
    // (tflag): no exact path above it, no ballot for it
    if (NOEX) return false;
    const float emax = __builtin_fmaxf(__builtin_fmaxf(er, eg), eb);
    const bool high = __builtin_amdgcn_ballot_w64(emax >= PQZ_LIM) != 0;   // rare: extreme out-of-gamut codes
    if (high) {
      r = er >= PQZ_LIM ? pq_exact(F, (er - 1.0f) * EI) : r;
      g = eg >= PQZ_LIM ? pq_exact(F, (eg - 1.0f) * EI) : g;
      b = eb >= PQZ_LIM ? pq_exact(F, (eb - 1.0f) * EI) : b;
    }
    return high;
  } else {
    // zimg arib_b67_inverse_oetf, branch-free; then the OOTF (gamma 1.2)
    auto inv = [](float e) -> float {
      const float x = fmaxf(e, 0.0f);
      const float lo = (x * x) * (1.0f / 3.0f);
      const float hi = (fexp2((x - HLG_C) * (1.4426950408889634f / HLG_A)) + HLG_B) * (1.0f / 12.0f);
      return x <= 0.5f ? lo : hi;
    };
    if (ESC == PQ_SEG) {
      // the CPU chain's instances: the inverse OETF from the same LDS cubic
      // table layout as the PQ EOTF (build_hlg_table; E staged as
      // E*PQ_SEG + 1), the direct form past the table
      r = pq_z(pq_lds, er), g = pq_z(pq_lds, eg), b = pq_z(pq_lds, eb);
      const float emax = __builtin_fmaxf(__builtin_fmaxf(er, eg), eb);
      constexpr float EI = 1.0f / (float)PQ_SEG;
      if (!NOEX && __builtin_amdgcn_ballot_w64(emax >= PQZ_LIM)) {
        r = er >= PQZ_LIM ? inv((er - 1.0f) * EI) : r;
        g = eg >= PQZ_LIM ? inv((eg - 1.0f) * EI) : g;
        b = eb >= PQZ_LIM ? inv((eb - 1.0f) * EI) : b;
      }
    } else {
      r = inv(er), g = inv(eg), b = inv(eb);
    }
    const float ys = 0.2627f * r + 0.6780f * g + 0.0593f * b;
    const float w = fexp2(flog2(ys) * 0.2f + F.log2_lin_scale);  // ys == 0 -> 0
    r *= w, g *= w, b *= w;
    return false;  // HLG is bounded (E <= 2.2 -> a few 1e4)
  }
}

// S2 vf_tonemap, specialised.  DESAT: 0 off, 1 weighted luma (F.lr/lg/lb),
// 2 the RGB-coefficient luma r+g+b (vf_tonemap's table entry for the linear
// RGB frame zscale hands it; the default).
//
// Bounded form (every lane's linear values from the PQ table or HLG, so
// sig <= ~6e8 and den*sig cannot overflow): the desaturation and the gain
// fold into out = c*A + B with A = (1-ob)*k, B = L*ob*k, since
// max(c*(1-ob) + L*ob) = max(c)*(1-ob) + L*ob for 0 <= ob <= 1; the curve
// uses one reciprocal.  Safe form (the wave met the exact PQ path): the
// statement order of vf_tonemap, two reciprocals.
//
// BT.2390 on PQ input (TRC 0, bounded form): the EETF's first step encodes
// sig = max(R,G,B) back to PQ, and PQ(EOTF(max E)) = max E, so e1 is the
// input's own max code value (emax_s = max E * PQ_SEG + 1, clamped below at
// the code of sig = 1e-6); the final decode reads the EOTF table in LDS.
// libplacebo branch with h2s_lp_tone IPT (F.lp_ipt): the curve acts on the
// intensity of IPT-PQ instead (three LMS rows encoded through the PQ-encode
// table, L'M'S' += I' - I decoded through the EOTF table), as the oracle's
// tone_ipt.
// DARK: the dark re-run (px_chain): every EOTF-table read takes its first
// segment exactly (pq_z_dark) instead of the mark staged there.  luma: the
// desaturation's luma (DESAT instances), the CPU chain's free dark probe
// DV (the Dolby Vision instances, lin_tone TRC 2, which call this as TRC 0:
// their light comes from the PQ table too): with a linear matrix after the
// EOTF, PQ(max RGB) is not the largest E, so the max-RGB form of BT.2390 /
// spline encodes sig through the PQ-encode table instead of reading emax_s
template <int TRC, int TM, int DESAT, int LP, bool DARK = false, bool DV = false>
__device__ __forceinline__ void tone(const FastParams& F, const CurveConsts& C, const float4* pq_lds,
                                     const float4* pqi_lds, float& r, float& g, float& b, bool safe, float emax_s,
                                     float hable_kb, float& luma_out) {
  auto pz = [&](float u) { return DARK ? pq_z_dark(pq_lds, u, F.log2_pq_scale) : pq_z(pq_lds, u); };
  if (LP && TM >= 4 && TM <= 6) {
    // libplacebo's reinhard / hable / mobius (scaling PL_HDR_NORM: 1 = the
    // target white; oracle lp_norm_curve), on the IPT intensity or as the
    // max(R,G,B) gain; the frame's constants come from its curve record
    auto curve = [&](float x) -> float {
      x = __builtin_amdgcn_fmed3f(x, 0.0f, C.n_peak);
      if (TM == 4) return C.n_rein_scale * x / (x + C.n_rein_off);
      if (TM == 5) return hable(x) * C.n_hable_inv;
      return x <= C.n_mob_j ? x : C.n_mob_scale * (x + C.n_mob_a) / (x + C.n_mob_b);
    };
    const float R = fminf(r, 1e6f), G = fminf(g, 1e6f), B = fminf(b, 1e6f);
    if (F.lp_ipt) {
      const float q0 = pqi(pqi_lds, F.ipt_r2l[0] * R + F.ipt_r2l[1] * G + F.ipt_r2l[2] * B);
      const float q1 = pqi(pqi_lds, F.ipt_r2l[3] * R + F.ipt_r2l[4] * G + F.ipt_r2l[5] * B);
      const float q2 = pqi(pqi_lds, F.ipt_r2l[6] * R + F.ipt_r2l[7] * G + F.ipt_r2l[8] * B);
      const float I = 0.4f * q0 + 0.4f * q1 + 0.2f * q2;
      const float x = pz(fmaf(I, (float)PQ_SEG, 1.0f)) * F.tw_fold;     // NORM
      luma_out = x;   // (marked for a dark I: the curve's clamp below would drop it; px_chain probes it)
      const float I2 = pqi(pqi_lds, curve(x) * F.tw_1e4);
      const float du = fmaf(I2 - I, (float)PQ_SEG, 1.0f);
      auto lz = [&](float q) { return pz(__builtin_amdgcn_fmed3f(fmaf(q, (float)PQ_SEG, du), 1.0f, PQZ_LIM - 0.01f)); };
      const float l0 = lz(q0), l1 = lz(q1), l2 = lz(q2);
      r = F.ipt_l2r[0] * l0 + F.ipt_l2r[1] * l1 + F.ipt_l2r[2] * l2;
      g = F.ipt_l2r[3] * l0 + F.ipt_l2r[4] * l1 + F.ipt_l2r[5] * l2;
      b = F.ipt_l2r[6] * l0 + F.ipt_l2r[7] * l1 + F.ipt_l2r[8] * l2;
    } else {
      const float sig = fmaxf(__builtin_fmaxf(__builtin_fmaxf(R, G), B), 1e-6f);
      const float k = curve(sig * F.n_nw) / sig;
      r = R * k, g = G * k, b = B * k;
    }
    return;
  }
  if (TM == 7 || TM == 8) {  // BT.2390 / spline (PQ-domain curves, no desat)
    // PQ input: the curve straight into pq_z's table coordinate u = e4*PQ_SEG
    // + 1 (the output scale and offset are folded into the polynomial
    // coefficients on the host, resolve_fast)
    auto curve_u = [&](float e1) -> float {
      float u;
      if (TM == 7) {   // BT.2390 Hermite knee as one cubic in t, Horner form
        const float e1n = __builtin_amdgcn_fmed3f(fmaf(e1, C.b_e1a, C.b_e1b), 0.0f, 1.0f);
        const float t = fmaf(e1n, C.b_ta, C.b_tb);
        const float uk = fmaf(fmaf(fmaf(C.b_c3, t, C.b_c2), t, C.b_c1), t, C.b_c0);
        u = e1n > C.b_thr ? uk : fmaf(e1n, C.b_lr, C.b_lc);
        if (C.b_minlum > 0.0f) {   // libplacebo black-point adaptation (block-uniform branch)
          const float om = fmaf(u, C.b_bk_a, C.b_bk_b);          // 1 - e2
          float pw;
          if (C.b_bp == 4.0f) {
            const float o2 = om * om;
            pw = o2 * o2;
          } else {
            pw = fexp2(C.b_bp * flog2(fmaxf(om, 0.0f)));
          }
          const float ub = fmaf(pw, C.b_bk_c, fmaf(u, C.b_gain, C.b_bk_d));
          u = om > 0.0f ? ub : u;
        }
      } else {         // spline: cubic shoulder / quadratic toe around the knee
        const float x = __builtin_amdgcn_fmed3f(e1, C.sp_srcmin, C.sp_srcmax) - C.sp_kin;
        const float uq = fmaf(fmaf(fmaf(C.sp_qa_u, x, C.sp_qb_u), x, C.sp_qc_u), x, C.sp_k_u);
        const float up = fmaf(fmaf(C.sp_pa_u, x, C.sp_pb_u), x, C.sp_k_u);
        u = __builtin_amdgcn_fmed3f(x > 0.0f ? uq : up, C.sp_umin, C.sp_umax);
      }
      return u;
    };
    // HLG input: the curve's PQ output e4
    auto curve_e4 = [&](float e1) -> float {
      if (TM == 7) {
        const float e1n = fmaxf(fminf((e1 - C.b_srcmin) * C.b_inv_range, 1.0f), 0.0f);
        const float t = (e1n - C.b_ks) * C.b_inv_1mks;
        const float t2 = t * t, t3 = t2 * t;
        const float p = (2.0f * t3 - 3.0f * t2 + 1.0f) * C.b_ks + (t3 - 2.0f * t2 + t) * (1.0f - C.b_ks) +
                        (-2.0f * t3 + 3.0f * t2) * C.b_maxlum;
        const float e2 = bt2390_black(C.b_minlum, C.b_bp, C.b_gain, (C.b_ks < 1.0f && e1n > C.b_ks) ? p : e1n);
        return fmaxf(e2 * C.b_range + C.b_srcmin, 0.0f);   // <= source max <= 1
      }
      return spline_pq(C, e1);                              // within [PQ(0), PQ(npl)]
    };
    auto eotf_exact = [](float e) -> float {   // normalised (1 = 10000 nits), e in [0, ~1.1]
      const float xp = fexp2(flog2(fmaxf(e, 0.0f)) * (1.0f / PQ_M2));
      return fexp2(flog2(fmaxf(xp - PQ_C1, 0.0f) * frcp(PQ_C2 - PQ_C3 * xp)) * (1.0f / PQ_M1));
    };
    auto pq_enc = [](float y) -> float {       // y = luminance / 10000
      const float ym = fexp2(flog2(fmaxf(y, 0.0f)) * PQ_M1);
      return fexp2(flog2((PQ_C1 + PQ_C2 * ym) * frcp(1.0f + PQ_C3 * ym)) * PQ_M2);
    };
    if (LP && F.lp_ipt) {   // (LP instances only: they stage both tables)
      // libplacebo branch, h2s_lp_tone IPT (oracle tone_ipt): the curve on
      // the intensity of IPT-PQ with P and T kept, i.e. L'M'S' += I' - I;
      // encode and decode through the LDS tables (launch-uniform branch; the
      // EOTF table is staged for HLG input too)
      H2S_MARK("S2a RGB->LMS, PQ encode x3");
      const float R = fminf(r, 1e6f), G = fminf(g, 1e6f), B = fminf(b, 1e6f);
      const float q0 = pqi(pqi_lds, F.ipt_r2l[0] * R + F.ipt_r2l[1] * G + F.ipt_r2l[2] * B);
      const float q1 = pqi(pqi_lds, F.ipt_r2l[3] * R + F.ipt_r2l[4] * G + F.ipt_r2l[5] * B);
      const float q2 = pqi(pqi_lds, F.ipt_r2l[6] * R + F.ipt_r2l[7] * G + F.ipt_r2l[8] * B);
      H2S_MARK("S2b I, curve");
      const float I = 0.4f * q0 + 0.4f * q1 + 0.2f * q2;
      const float du = curve_u(I) - I * (float)PQ_SEG;   // (I' - I) PQ_SEG + 1
      H2S_MARK("S2c EOTF x3, LMS->RGB");
      auto lz = [&](float q) { return pz(__builtin_amdgcn_fmed3f(fmaf(q, (float)PQ_SEG, du), 1.0f, PQZ_LIM - 0.01f)); };
      const float l0 = lz(q0), l1 = lz(q1), l2 = lz(q2);
      r = F.ipt_l2r[0] * l0 + F.ipt_l2r[1] * l1 + F.ipt_l2r[2] * l2;
      g = F.ipt_l2r[3] * l0 + F.ipt_l2r[4] * l1 + F.ipt_l2r[5] * l2;
      b = F.ipt_l2r[6] * l0 + F.ipt_l2r[7] * l1 + F.ipt_l2r[8] * l2;
      return;
    }
    const float sig = fmaxf(__builtin_fmaxf(__builtin_fmaxf(r, g), b), 1e-6f);
    float e1;
    if (DV) {
      e1 = fmaxf(pqi(pqi_lds, sig * F.npl_1e4), F.b_e1min);
    } else if (TRC == 0 && !safe) {
      e1 = fmaxf(fmaf(emax_s, 1.0f / (float)PQ_SEG, -1.0f / (float)PQ_SEG), F.b_e1min);
    } else {  // exact PQ encode: HLG input, or the wave met the exact EOTF path
      e1 = pq_enc(sig * F.npl_1e4);
    }
    // EOTF(e4) * 10000/target white (TRC 0: the table is npl-scaled)
    const float s2 = TRC == 0 ? pz(curve_u(e1)) * F.tw_fold : eotf_exact(curve_e4(e1)) * F.e4_npl;
    const float k = safe ? s2 / sig : s2 * frcp(sig);   // IEEE division on the exact path (see below)
    r *= k, g *= k, b *= k;
    return;
  }
  if (safe) {
    // the wave met the exact PQ path: linear values up to ~1e38 or inf.
    // vf_tonemap's statement order with IEEE division, as the generic kernel
    // (tonemap_px): v_rcp_f32 flushes the (denormal) reciprocal of anything
    // above 8.5e37 to zero, which Hable's num/den reaches at sig ~ 2.7e19
    if (DESAT) {
      const float luma = DESAT == 2 ? (r + g) + b : F.lr * r + F.lg * g + F.lb * b;
      luma_out = luma;
      const float ob = fmaxf(luma - F.desat, 1e-6f) / fmaxf(luma, 1e-6f);
      r = r * (1.0f - ob) + luma * ob;
      g = g * (1.0f - ob) + luma * ob;
      b = b * (1.0f - ob) + luma * ob;
    }
    const float sig = fmaxf(__builtin_fmaxf(__builtin_fmaxf(r, g), b), 1e-6f);
    float t;
    if (TM == 4) {  // REINHARD
      t = sig / (sig + F.rein_p) * F.rein_k;
    } else if (TM == 5) {  // HABLE
      t = hable(sig) * F.hable_peak_inv;
    } else {  // MOBIUS: identity below j
      t = sig <= F.mob_j ? sig : F.mob_k * (sig + F.mob_a) / (sig + F.mob_b);
    }
    const float k = t / sig;
    r *= k, g *= k, b *= k;
    return;
  }
  float sig, A = 1.0f, B = 0.0f;
  if (DESAT) {
    const float luma = DESAT == 2 ? (r + g) + b : F.lr * r + F.lg * g + F.lb * b;
    luma_out = luma;
    const float ob = fmaxf(luma - F.desat, 1e-6f) * frcp(fmaxf(luma, 1e-6f));
    A = 1.0f - ob, B = luma * ob;
    sig = fmaxf(fmaf(__builtin_fmaxf(__builtin_fmaxf(r, g), b), A, B), 1e-6f);
  } else {
    sig = fmaxf(__builtin_fmaxf(__builtin_fmaxf(r, g), b), 1e-6f);
  }
  float k;
  if (TM == 4) {
    k = F.rein_k * frcp(sig + F.rein_p);
  } else if (TM == 5) {
    // hable(x) = N/D - e/f with 15 N - D = x (2.1 x + 0.25) (the constant
    // terms cancel: d*e*15 = d*f), so hable(x)/x = (0.14 x + 1/60) / D:
    // one reciprocal, no cancellation, and sig drops out of the gain
    const float den = fmaf(sig, fmaf(sig, 0.15f, 0.50f), 0.06f);
    k = fmaf(sig, F.hable_ka, hable_kb) * frcp(den);   // (kb in a VGPR: one scalar operand per VOP3)
  } else {
    const float m = F.mob_k * (sig + F.mob_a) * frcp((sig + F.mob_b) * sig);
    k = sig <= F.mob_j ? 1.0f : m;
  }
  if (DESAT) {
    A *= k, B *= k;
    r = fmaf(r, A, B), g = fmaf(g, A, B), b = fmaf(b, A, B);
  } else {
    r *= k, g *= k, b *= k;
  }
}

}  // namespace h2s
