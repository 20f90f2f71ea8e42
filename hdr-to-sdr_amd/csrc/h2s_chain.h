// h2s_chain.h — the generic kernel's per-pixel chain for gfx950 (device code):
// S1 .. S8 of h2s_params.h's stage list on one pixel, in the oracle's
// operation order.  The CPU statement each function must agree with is
// oracle/h2s_oracle.c.
// What belongs here: the glibc powf / expf forms over h2s_libm.h's tables
// (this header is that file's only includer), every transfer, tone curve,
// lattice and quantiser form written over them or over KParams, and
// chain_px, which puts them together.  Its users are h2s_kernels.hip
// (through h2s_lpx.h, the libplacebo branch's double-precision stages),
// h2s_peak.hip and h2s_testhooks.hip; the tile kernel and the host units never
// include it.  What the tile kernel shares with this chain is h2s_math.h's.
// No FMA contraction inside the libm forms: that rule is stated with them
// below and holds in whichever translation unit includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include "h2s_libm.h"
#include "h2s_math.h"
#include "h2s_params.h"

namespace h2s {

// a frame's curve record over the generic kernel's constants (dynamic peak)
__device__ __forceinline__ void apply_curve(KParams& P, const CurveConsts& C) {
  P.b_srcmin = C.b_srcmin, P.b_range = C.b_range, P.b_inv_range = C.b_inv_range, P.b_ks = C.b_ks;
  P.b_inv_1mks = C.b_inv_1mks, P.b_maxlum = C.b_maxlum, P.b_minlum = C.b_minlum, P.b_bp = C.b_bp, P.b_gain = C.b_gain;
  P.sp_srcmin = C.sp_srcmin, P.sp_srcmax = C.sp_srcmax, P.sp_kin = C.sp_kin, P.sp_kout = C.sp_kout;
  P.sp_pa = C.sp_pa, P.sp_pb = C.sp_pb, P.sp_qa = C.sp_qa, P.sp_qb = C.sp_qb, P.sp_qc = C.sp_qc;
  P.sp_dmin = C.sp_dmin, P.sp_dmax = C.sp_dmax;
  P.n_peak = C.n_peak, P.n_rein_off = C.n_rein_off, P.n_rein_scale = C.n_rein_scale, P.n_hable_inv = C.n_hable_inv;
  P.n_mob_j = C.n_mob_j, P.n_mob_a = C.n_mob_a, P.n_mob_b = C.n_mob_b, P.n_mob_scale = C.n_mob_scale;
  P.x_peak = C.x_peak, P.x_avg = C.x_avg;
}

// the generic chain's pow and exp: the oracle's own, glibc 2.35 powf / expf
// (the x86-64 FMA build: double-precision table + polynomial forms, one
// rounding to float), over the tables scripts/gen_libm_tables.py reads out of
// the libm the oracle links (h2s_libm.h; tests/test_libm_tables.py pins them).
// Their last rounding is not the correctly rounded one for a few inputs in
// 10^4, and the PQ EOTF amplifies a pow ulp ~500-fold (m2 = 78.84; the
// xp - c1 and c2 - c3 xp cancellations): enough to flip the libplacebo
// branch's 8-bit rgba rounding.  The generic kernel is the branch's exact
// path (H2S_OPT_LP_EXACT; h2s_kernels.hip is built without FMA contraction, in
// the oracle's operation order); the tile kernel keeps its own fast forms.
// (no FMA contraction inside: the forms round where glibc's do, whichever
// translation unit includes them; tests/test_libm_tables.py checks the device
// forms bit for bit against the libm through h2stest_libm)
__device__ __forceinline__ float libm_exp2_tail(double xd, double shift, const double* C) {
#pragma clang fp contract(off)
  double kd = xd + shift;
  const unsigned long long ki = (unsigned long long)__double_as_longlong(kd);
  kd -= shift;
  const double r = xd - kd;
  const unsigned long long t = libm::EXP2F_TAB[ki & 31] + (ki << 47);
  const double s = __longlong_as_double((long long)t);
  const double z = __builtin_fma(C[0], r, C[1]);
  const double r2 = r * r;
  double y = __builtin_fma(C[2], r, 1.0);
  y = __builtin_fma(z, r2, y);
  return (float)(y * s);
}
// powf for x >= 0 (the chain's uses); other bases take the double form
__device__ __forceinline__ float libm_powf(float x, float yf) {
#pragma clang fp contract(off)
  if (!(x > 0.0f) || !(x < __builtin_inff()) || yf == 0.0f || !(fabsf(yf) < __builtin_inff()))
    return (float)pow((double)x, (double)yf);
  unsigned ix = __float_as_uint(x);
  if (ix < 0x00800000u) ix = __float_as_uint(x * 0x1p23f) - (23u << 23);  // subnormal
  const unsigned tmp = ix - 0x3f330000u;
  const int i = (int)((tmp >> 19) & 15u);
  const unsigned top = tmp & 0xff800000u;
  const unsigned iz = ix - top;
  const int k = (int)top >> 23;
  const double invc = libm::POWF_LOG2_TAB[i][0], logc = libm::POWF_LOG2_TAB[i][1];
  const double z = (double)__uint_as_float(iz);
  const double* A = libm::POWF_LOG2_POLY;
  const double r = __builtin_fma(z, invc, -1.0);
  const double y0 = logc + (double)k;
  const double r2 = r * r;
  double y = __builtin_fma(A[0], r, A[1]);
  const double p = __builtin_fma(A[2], r, A[3]);
  const double r4 = r2 * r2;
  double q = __builtin_fma(A[4], r, y0);
  q = __builtin_fma(p, r2, q);
  y = __builtin_fma(y, r4, q);
  const double ylogx = (double)yf * y;
  if ((((unsigned long long)__double_as_longlong(ylogx) >> 47) & 0xffffu) >= (0x405f800000000000ull >> 47)) {
    if (ylogx > 0x1.fffffffd1d571p+6) return __builtin_inff();
    if (ylogx <= -150.0) return 0.0f;
  }
  return libm_exp2_tail(ylogx, libm::EXP2F_SHIFT_SCALED, libm::EXP2F_POLY);
}
__device__ __forceinline__ float libm_expf(float x) {
  if (x != x) return x;
  if (x > 0x1.62e42ep6f) return __builtin_inff();
  if (x < -0x1.9fe368p6f) return 0.0f;
  return libm_exp2_tail(libm::EXP2F_INVLN2_SCALED * (double)x, libm::EXP2F_SHIFT, libm::EXP2F_POLY_SCALED);
}
__device__ __forceinline__ float apow(float x, float p) { return libm_powf(x, p); }
__device__ __forceinline__ float aexp(float x) { return libm_expf(x); }
// S1 transfer: zimg st_2084_eotf (normalised, 1.0 = 10000 nits)
__device__ __forceinline__ float pq_eotf(float x) {
  if (!(x > 0.0f)) return 0.0f;
  float xpow = apow(x, 1.0f / PQ_M2);
  float num = fmaxf(xpow - PQ_C1, 0.0f);
  float den = fmaxf(PQ_C2 - PQ_C3 * xpow, 1.17549435e-38f);
  return apow(num / den, 1.0f / PQ_M1);
}

// ST 2084 inverse EOTF (BT.2390 works in the PQ domain)
__device__ __forceinline__ float pq_encode(float y) {
  float ym = apow(fmaxf(y, 0.0f), PQ_M1);
  return apow((PQ_C1 + PQ_C2 * ym) / (1.0f + PQ_C3 * ym), PQ_M2);
}

// zimg arib_b67_inverse_oetf
__device__ __forceinline__ float hlg_inv_oetf(float x) {
  x = fmaxf(x, 0.0f);
  if (x <= 0.5f) return (x * x) * (1.0f / 3.0f);
  return (aexp((x - HLG_C) / HLG_A) + HLG_B) * (1.0f / 12.0f);
}

// libplacebo bt2390 on a PQ-domain signal, in the oracle's operation order
// (oracle bt2390_pq: divisions by the range and by 1 - ks, powf for any bp)
__device__ __forceinline__ float bt2390_pq(const KParams& P, float e1) {
  float e1n = (e1 - P.b_srcmin) / P.b_range;
  e1n = fmaxf(fminf(e1n, 1.0f), 0.0f);  // clip to the source range (NaN -> 1)
  const float ks = P.b_ks, ml = P.b_maxlum;
  float e2 = e1n;
  if (ks < 1.0f && e1n > ks) {
    float t = (e1n - ks) / (1.0f - ks);
    float t2 = t * t, t3 = t2 * t;
    e2 = (2.0f * t3 - 3.0f * t2 + 1.0f) * ks + (t3 - 2.0f * t2 + t) * (1.0f - ks) + (-2.0f * t3 + 3.0f * t2) * ml;
  }
  if (P.b_minlum > 0.0f && e2 < 1.0f) {
    const float mn = P.b_minlum;
    e2 += mn * apow(1.0f - e2, P.b_bp);
    e2 = P.b_gain * (e2 - mn) + mn;
  }
  return e2 * P.b_range + P.b_srcmin;
}

// libplacebo branch, h2s_lp_tone IPT (oracle tone_ipt): the PQ-domain curve
// on the intensity of IPT-PQ, P and T kept, i.e. L'M'S' += I' - I.  In double
// around the float curve, as the oracle: the LMS -> RGB rows turn float32
// EOTF noise into large errors on channels they cancel to near zero
// (the encode is h2s_math.h's hd_pq_encode; the EOTF stays its own form:
// hd_pq_eotf takes its maximum as a select, this one as fmax)
__device__ __forceinline__ double pq_eotf_dd(double e) {
  if (!(e > 0.0)) return 0.0;
  const double xp = pow(e, 1.0 / (double)PQ_M2);
  return pow(fmax(xp - (double)PQ_C1, 0.0) / ((double)PQ_C2 - (double)PQ_C3 * xp), 1.0 / (double)PQ_M1);
}
// libplacebo's reinhard / hable / mobius in NORM units (oracle lp_norm_curve)
__device__ __forceinline__ float lp_norm_curve(const KParams& P, float x) {
  x = fminf(fmaxf(x, 0.0f), P.n_peak);
  if (P.tonemap == 4) return P.n_rein_scale * x / (x + P.n_rein_off);
  if (P.tonemap == 5) return hable(x) / hable(P.n_peak);   // (oracle: hable(x) / hable(pk))
  return x <= P.n_mob_j ? x : P.n_mob_scale * (x + P.n_mob_a) / (x + P.n_mob_b);
}

__device__ __forceinline__ void tone_ipt(const KParams& P, float& r, float& g, float& b) {
  const double s = P.ipt_npl;
  const double v0 = fmin((double)r, 1e6) * s, v1 = fmin((double)g, 1e6) * s, v2 = fmin((double)b, 1e6) * s;
  double q[3];
#pragma unroll
  for (int k = 0; k < 3; k++) q[k] = hd_pq_encode(P.ipt_r2l[3 * k] * v0 + P.ipt_r2l[3 * k + 1] * v1 + P.ipt_r2l[3 * k + 2] * v2);
  const double I = 0.4 * q[0] + 0.4 * q[1] + 0.2 * q[2];
  double I2;
  if (P.tonemap == 8) I2 = spline_pq(P, (float)I);
  else if (P.tonemap == 7) I2 = bt2390_pq(P, (float)I);
  else I2 = hd_pq_encode((double)lp_norm_curve(P, (float)(pq_eotf_dd(I) * P.ipt_os)) * P.ipt_tw);
  const double dI = I2 - I;
  double l[3];
#pragma unroll
  for (int k = 0; k < 3; k++) l[k] = pq_eotf_dd(q[k] + dI);
  const double os = P.ipt_os;
  r = (float)((P.ipt_l2r[0] * l[0] + P.ipt_l2r[1] * l[1] + P.ipt_l2r[2] * l[2]) * os);
  g = (float)((P.ipt_l2r[3] * l[0] + P.ipt_l2r[4] * l[1] + P.ipt_l2r[5] * l[2]) * os);
  b = (float)((P.ipt_l2r[6] * l[0] + P.ipt_l2r[7] * l[1] + P.ipt_l2r[8] * l[2]) * os);
}

// S2: vf_tonemap tonemap() on one linear RGB pixel (units of npl)
__device__ __forceinline__ void tonemap_px(const KParams& P, float& r, float& g, float& b) {
  float sig, sig_orig;
  if (P.lp_ipt) {   // set on the libplacebo branch only
    tone_ipt(P, r, g, b);
    return;
  }
  if (P.lp_norm) {  // libplacebo branch, max(R,G,B) gain (oracle tonemap_px)
    r = fminf(r, 1e6f), g = fminf(g, 1e6f), b = fminf(b, 1e6f);
    sig = fmaxf(fmaxf(fmaxf(r, g), b), 1e-6f);
    const float k = lp_norm_curve(P, sig * P.n_nw) / sig;
    r *= k, g *= k, b *= k;
    return;
  }
  if (P.tonemap == 8 /* SPLINE */) {
    sig = fmaxf(fmaxf(fmaxf(r, g), b), 1e-6f);
    const float s2 = pq_eotf(spline_pq(P, pq_encode(sig * P.npl_1e4))) * P.e4_npl;
    const float k = s2 / sig;
    r *= k, g *= k, b *= k;
    return;
  }
  if (P.tonemap == 7 /* BT2390 */) {
    sig = fmaxf(fmaxf(fmaxf(r, g), b), 1e-6f);
    float s2 = pq_eotf(bt2390_pq(P, pq_encode(sig * P.npl_1e4))) * P.e4_npl;
    float k = s2 / sig;
    r *= k, g *= k, b *= k;
    return;
  }
  if (P.desat_on) {
    float luma = P.lr * r + P.lg * g + P.lb * b;
    float ob = fmaxf(luma - P.desat, 1e-6f) / fmaxf(luma, 1e-6f);
    r = r * (1.0f - ob) + luma * ob;
    g = g * (1.0f - ob) + luma * ob;
    b = b * (1.0f - ob) + luma * ob;
  }
  sig = fmaxf(fmaxf(fmaxf(r, g), b), 1e-6f);
  sig_orig = sig;
  switch (P.tonemap) {
    case 1:  // LINEAR
      sig = sig * P.lin_k;
      break;
    case 2:  // GAMMA
      sig = sig > 0.05f ? apow(sig * P.gam_inv_peak, P.gam_inv_param) : sig * P.gam_low_k;
      break;
    case 3:  // CLIP
      sig = clamp01(sig * P.clip_k);
      break;
    case 4:  // REINHARD
      sig = sig / (sig + P.rein_p) * P.rein_k;
      break;
    case 5:  // HABLE
      sig = hable(sig) * P.hable_peak_inv;
      break;
    case 6:  // MOBIUS
      sig = sig <= P.mob_j ? sig : P.mob_k * (sig + P.mob_a) / (sig + P.mob_b);
      break;
    default:
      break;
  }
  float k = sig / sig_orig;
  r *= k, g *= k, b *= k;
}

// S3: zimg rec_1886_inverse_eotf
__device__ __forceinline__ float bt1886_inv(float x) {
  return x > 0.0f ? apow(x, 1.0f / 2.4f) : 0.0f;
}

// S4: vf_lut3d sanitizef + clip + interp_tetrahedral.  The lattice is in
// .cube order (red fastest): index(r,g,b) = r + g*N + b*N^2.  Case selection
// uses the same strict comparisons as interp_tetrahedral, expressed as
// selects instead of branches (no divergence); the weights and the term order
// are the reference's.
__device__ __forceinline__ float lut_coord(float x, float lut_max) {
  x = (x == x) ? x : 0.0f;  // NaN -> 0 (sanitizef); +-inf clip below
  return __builtin_amdgcn_fmed3f(x * lut_max, 0.0f, lut_max);
}

// tetrahedral blend at lattice coordinates s in [0, N-1] (lut3d interp_tetrahedral)
__device__ __forceinline__ void lut3d_tetra_at(const KParams& P, float sr, float sg, float sb, float& r, float& g,
                                               float& b) {
  const int pr = (int)sr, pg = (int)sg, pb = (int)sb;
  const int last = P.lut_n - 1;
  const int str = pr < last ? 1 : 0;
  const int stg = pg < last ? P.lut_sg : 0;
  const int stb = pb < last ? P.lut_sb : 0;
  const float dr = sr - (float)pr, dg = sg - (float)pg, db = sb - (float)pb;
  const bool rg = dr > dg, gb = dg > db, rb = dr > db, bg = db > dg, br = db > dr;
  float x1, x2, x3;
  int o1, o2;
  if (rg) {
    if (gb) { x1 = dr; x2 = dg; x3 = db; o1 = str; o2 = stg; }
    else if (rb) { x1 = dr; x2 = db; x3 = dg; o1 = str; o2 = stb; }
    else { x1 = db; x2 = dr; x3 = dg; o1 = stb; o2 = str; }
  } else {
    if (bg) { x1 = db; x2 = dg; x3 = dr; o1 = stb; o2 = stg; }
    else if (br) { x1 = dg; x2 = db; x3 = dr; o1 = stg; o2 = stb; }
    else { x1 = dg; x2 = dr; x3 = db; o1 = stg; o2 = str; }
  }
  const int base = pr + pg * P.lut_sg + pb * P.lut_sb;
  const float4 c000 = P.lut[base];
  const float4 c1 = P.lut[base + o1];
  const float4 c2 = P.lut[base + o1 + o2];
  const float4 c111 = P.lut[base + str + stg + stb];
  const float w0 = 1.0f - x1, w1 = x1 - x2, w2 = x2 - x3, w3 = x3;
  r = w0 * c000.x + w1 * c1.x + w2 * c2.x + w3 * c111.x;
  g = w0 * c000.y + w1 * c1.y + w2 * c2.y + w3 * c111.y;
  b = w0 * c000.z + w1 * c1.z + w2 * c2.z + w3 * c111.z;
}

__device__ __forceinline__ void lut3d_tetra(const KParams& P, float& r, float& g, float& b) {
  lut3d_tetra_at(P, lut_coord(r, P.lut_max), lut_coord(g, P.lut_max), lut_coord(b, P.lut_max), r, g, b);
}

// libplacebo branch: BT.1886 encode against the target black (oracle lp_encode)
__device__ __forceinline__ float lp_encode(const KParams& P, float x) {
  x = x > 0.0f ? x : 0.0f;
  return apow(x / P.enc_a, 1.0f / 2.4f) - P.enc_b;
}

// libplacebo branch: rgba8 download (round to nearest), then vf_lut3d's 8-bit
// path: coordinate clip((q / 255) (N-1)), tetrahedral, output truncated to
// 8 bits; returns the 8-bit values / 255
// qoff: lp_qoff (the range=tv offset and the rounding / dither offset)
__device__ __forceinline__ float rgba8_q(const KParams& P, float v, float qoff) {
  return floorf(clamp01(v) * P.lp_qs + qoff);   // (two roundings, as the oracle's rgba8_q)
}

// the rgba8 download's offset for pixel (x, y)
__device__ __forceinline__ float lp_qoff(const KParams& P, int x, int y) {
  return P.lp_qo + (P.lp_dith ? bayer16(x, y) : 0.5f);
}

__device__ __forceinline__ void lut3d_8bit(const KParams& P, float& r, float& g, float& b, float qoff) {
  const float sf = 1.0f / 255.0f;
  // lut3d_tetra multiplies by lut_max and clips; (q * 1/255) is its input
  r = rgba8_q(P, r, qoff) * sf, g = rgba8_q(P, g, qoff) * sf, b = rgba8_q(P, b, qoff) * sf;
  lut3d_tetra(P, r, g, b);
  const float R = fminf(fmaxf(truncf(r * 255.0f), 0.0f), 255.0f);
  const float G = fminf(fmaxf(truncf(g * 255.0f), 0.0f), 255.0f);
  const float B = fminf(fmaxf(truncf(b * 255.0f), 0.0f), 255.0f);
  r = R * sf, g = G * sf, b = B * sf;
}

// S3 -> S4 as 16-bit R'G'B' (h2s_lut_input RGB48; oracle rgb48_q /
// lut3d_16bit): round to 16 bits, lut3d's 16-bit coordinate, output truncated
__device__ __forceinline__ float rgb48_q(float v) { return floorf(clamp01(v) * 65535.0f + 0.5f); }
__device__ __forceinline__ void lut3d_16bit(const KParams& P, float& r, float& g, float& b) {
  const float scale = (1.0f / 65535.0f) * P.lut_max;
  const float sr = __builtin_amdgcn_fmed3f(rgb48_q(r) * scale, 0.0f, P.lut_max);
  const float sg = __builtin_amdgcn_fmed3f(rgb48_q(g) * scale, 0.0f, P.lut_max);
  const float sb = __builtin_amdgcn_fmed3f(rgb48_q(b) * scale, 0.0f, P.lut_max);
  float orr, og, ob;
  lut3d_tetra_at(P, sr, sg, sb, orr, og, ob);
  r = fminf(fmaxf(truncf(orr * 65535.0f), 0.0f), 65535.0f) / 65535.0f;
  g = fminf(fmaxf(truncf(og * 65535.0f), 0.0f), 65535.0f) / 65535.0f;
  b = fminf(fmaxf(truncf(ob * 65535.0f), 0.0f), 65535.0f) / 65535.0f;
}

// S1 (after upsampling) .. S4 on one pixel.  UPTO = last stage to apply.
template <int UPTO>
__device__ __forceinline__ void chain_px(const KParams& P, float y, float cb, float cr, float& r, float& g,
                                         float& b, float qoff = 0.5f) {
  float er = y + P.m_rcr * cr;
  float eg = y + P.m_gcb * cb + P.m_gcr * cr;
  float eb = y + P.m_bcb * cb;
  if (P.transfer == 1) {  // HLG: inverse OETF + OOTF (gamma 1.2 at 1000 nits)
    r = hlg_inv_oetf(er), g = hlg_inv_oetf(eg), b = hlg_inv_oetf(eb);
    float ys = 0.2627f * r + 0.6780f * g + 0.0593f * b;
    float w = ys > 0.0f ? P.lin_scale * apow(ys, 0.2f) : 0.0f;
    r *= w, g *= w, b *= w;
  } else {
    r = pq_eotf(er) * P.lin_scale;
    g = pq_eotf(eg) * P.lin_scale;
    b = pq_eotf(eb) * P.lin_scale;
  }
  if (UPTO == 1) return;
  tonemap_px(P, r, g, b);
  if (UPTO == 2) return;
  if (P.pipe == PIPE_LIBPLACEBO) {
    if (P.lut_enabled) {
      r = lp_encode(P, r), g = lp_encode(P, g), b = lp_encode(P, b);
      if (UPTO == 3) return;
      lut3d_8bit(P, r, g, b, qoff);
    } else {
      float mr = P.m709[0] * r + P.m709[1] * g + P.m709[2] * b;
      float mg = P.m709[3] * r + P.m709[4] * g + P.m709[5] * b;
      float mb = P.m709[6] * r + P.m709[7] * g + P.m709[8] * b;
      r = clamp01(lp_encode(P, mr)), g = clamp01(lp_encode(P, mg)), b = clamp01(lp_encode(P, mb));
    }
    return;
  }
  if (P.lut_enabled) {
    r = bt1886_inv(r), g = bt1886_inv(g), b = bt1886_inv(b);
    if (UPTO == 3) return;
    if (P.lut_in16) {
      lut3d_16bit(P, r, g, b);
      return;
    }
    lut3d_tetra(P, r, g, b);
  } else {
    float mr = P.m709[0] * r + P.m709[1] * g + P.m709[2] * b;
    float mg = P.m709[3] * r + P.m709[4] * g + P.m709[5] * b;
    float mb = P.m709[6] * r + P.m709[7] * g + P.m709[8] * b;
    r = clamp01(bt1886_inv(mr)), g = clamp01(bt1886_inv(mg)), b = clamp01(bt1886_inv(mb));
  }
}

__device__ __forceinline__ int quant(float v, int qmax) {
  int i = (int)floorf(v + 0.5f);
  return min(max(i, 0), qmax);
}

__device__ __forceinline__ int quant_o(float v, float off, int qmax) {
  int i = (int)floorf(v + off);
  return min(max(i, 0), qmax);
}

// S8 expansion of a quantised code to the output depth
__device__ __forceinline__ int expand_code(const KParams& P, int v) {
  // (out_sh: a semi-planar 16-bit word carries the code in its high bits)
  if (!P.shift_out) return v << P.out_sh;
  return (P.expand_rep ? (v << P.shift_out) | (v >> (8 - P.shift_out)) : v << P.shift_out) << P.out_sh;
}

}  // namespace h2s
