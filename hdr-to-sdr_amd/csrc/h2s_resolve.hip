// h2s_resolve.hip — the host arithmetic of the C-ABI: parameter validation
// and resolution (KParams, FastParams), the source constants, the cubic
// tables, the filter taps and the peak model.
//
// Rule of this unit: it makes no HIP API call.  Everything here is a function
// of its arguments (and of the context's plain members), so it can be read,
// and reasoned about, without a device; whatever allocates, copies, launches
// or waits lives in h2s_api*.hip.
#include "h2s_host.h"
#include "h2s_math.h"

using namespace h2s::host;
using h2s::FastParams;
using h2s::KParams;

namespace h2s {
namespace host {

// ---- parameter resolution (mirrors vf_tonemap init/filter_frame, zimg,
// vf_eq create_lut; the CPU statement is oracle/h2s_oracle.c resolve()) ----
int validate_params(h2s_ctx* c, const h2s_params* p) {
  if (p->transfer_in != H2S_TRC_PQ && p->transfer_in != H2S_TRC_HLG)
    return fail(c, H2S_E_INVALID_ARG, "transfer_in must be PQ or HLG");
  if (p->bits_in != 10 && p->bits_in != 12)
    return fail(c, H2S_E_UNSUPPORTED, "bits_in must be 10 or 12 (yuv420p10le / yuv420p12le)");
  if (p->bits_out != 8 && p->bits_out != 10 && p->bits_out != 12)
    return fail(c, H2S_E_UNSUPPORTED, "bits_out must be 8, 10 or 12");
  if (p->tonemap < H2S_TM_NONE || p->tonemap > H2S_TM_SPLINE)
    return fail(c, H2S_E_INVALID_ARG, "unknown tonemap operator");
  if (p->tonemap == H2S_TM_SPLINE && !isnan(p->tm_param) && !(p->tm_param >= 0.0 && p->tm_param <= 1.5))
    return fail(c, H2S_E_INVALID_ARG, "spline contrast (tm_param) must be in [0, 1.5]");
  if (p->mode != H2S_MODE_COMPAT8 && p->mode != H2S_MODE_NATIVE)
    return fail(c, H2S_E_INVALID_ARG, "mode must be COMPAT8 or NATIVE");
  if (p->desat_luma < 0 || p->desat_luma > 2) return fail(c, H2S_E_INVALID_ARG, "unknown desat_luma");
  if (!(p->gamma > 0) || !isfinite(p->gamma)) return fail(c, H2S_E_INVALID_ARG, "gamma must be > 0");
  if (!(p->npl > 0) || !isfinite(p->npl)) return fail(c, H2S_E_INVALID_ARG, "npl must be > 0");
  if (!(p->desat >= 0)) return fail(c, H2S_E_INVALID_ARG, "desat must be >= 0");
  if (p->chroma_filter != H2S_CHROMA_BOX && p->chroma_filter != H2S_CHROMA_BICUBIC)
    return fail(c, H2S_E_INVALID_ARG, "unknown chroma_filter");
  if (p->dither != H2S_DITHER_NONE && p->dither != H2S_DITHER_ORDERED)
    return fail(c, H2S_E_INVALID_ARG, "unknown dither");
  if (p->expand != H2S_EXPAND_SHIFT && p->expand != H2S_EXPAND_REPLICATE)
    return fail(c, H2S_E_INVALID_ARG, "unknown expand");
  if (p->chroma_edge < H2S_EDGE_ZIMG || p->chroma_edge > H2S_EDGE_MIRROR)
    return fail(c, H2S_E_INVALID_ARG, "unknown chroma_edge");
  if (p->lut_input != H2S_LUT_IN_FLOAT && p->lut_input != H2S_LUT_IN_RGB48)
    return fail(c, H2S_E_INVALID_ARG, "unknown lut_input");
  if (p->pipeline < H2S_PIPE_AUTO || p->pipeline > H2S_PIPE_LIBPLACEBO)
    return fail(c, H2S_E_INVALID_ARG, "unknown pipeline");
  if (p->lp_tone != H2S_LP_TONE_IPT && p->lp_tone != H2S_LP_TONE_MAX_RGB)
    return fail(c, H2S_E_INVALID_ARG, "unknown lp_tone");
  if (p->pipeline == H2S_PIPE_LIBPLACEBO && (p->tonemap < H2S_TM_REINHARD || p->tonemap > H2S_TM_SPLINE))
    return fail(c, H2S_E_UNSUPPORTED,
                "libplacebo pipeline: the reference's operators are reinhard, mobius, hable, bt.2390 and spline");
  if (!isnan(p->knee_offset) && !(p->knee_offset >= 0.5 && p->knee_offset <= 2.0))
    return fail(c, H2S_E_INVALID_ARG, "knee_offset must be in [0.5, 2] (libplacebo's range)");
  if (!isnan(p->target_white) && !(p->target_white > 0 && isfinite(p->target_white)))
    return fail(c, H2S_E_INVALID_ARG, "target_white must be > 0");
  if (!isnan(p->target_black) && !(p->target_black >= 0 && isfinite(p->target_black)))
    return fail(c, H2S_E_INVALID_ARG, "target_black must be >= 0");
  if (!isnan(p->target_black) && !isnan(p->target_white) && !(p->target_black < p->target_white))
    return fail(c, H2S_E_INVALID_ARG, "target_black must be below target_white");
  if (p->lp_range != H2S_LP_RANGE_FULL && p->lp_range != H2S_LP_RANGE_LIMITED)
    return fail(c, H2S_E_INVALID_ARG, "unknown lp_range");
  if (p->lp_dither != H2S_LP_DITHER_NONE && p->lp_dither != H2S_LP_DITHER_ORDERED)
    return fail(c, H2S_E_INVALID_ARG, "unknown lp_dither");
  if (p->lp_p010 != H2S_LP_P010_KEEP && p->lp_p010 != H2S_LP_P010_TRUNCATE)
    return fail(c, H2S_E_INVALID_ARG, "unknown lp_p010");
  // vf_libplacebo's option ranges (smoothing_period 0..1000, scene thresholds
  // -1..100 (negative: scene detection off), percentile 0..100, minimum_peak 0..100)
  if (!isnan(p->pd_smoothing) && !(p->pd_smoothing >= 0.0 && p->pd_smoothing <= 1000.0))
    return fail(c, H2S_E_INVALID_ARG, "pd_smoothing must be in [0, 1000] frames");
  if (!isnan(p->pd_scene_low) && !(p->pd_scene_low >= -1.0 && p->pd_scene_low <= 100.0))
    return fail(c, H2S_E_INVALID_ARG, "pd_scene_low must be in [-1, 100]");
  if (!isnan(p->pd_scene_high) && !(p->pd_scene_high >= -1.0 && p->pd_scene_high <= 100.0))
    return fail(c, H2S_E_INVALID_ARG, "pd_scene_high must be in [-1, 100]");
  if (!isnan(p->pd_percentile) && !(p->pd_percentile > 0.0 && p->pd_percentile <= 100.0))
    return fail(c, H2S_E_INVALID_ARG, "pd_percentile must be in (0, 100]");
  if (!isnan(p->pd_min_peak) && !(p->pd_min_peak >= 0.0 && p->pd_min_peak <= 100.0))
    return fail(c, H2S_E_INVALID_ARG, "pd_min_peak must be in [0, 100]");
  return 0;
}

// the per-frame curve constants (BT.2390, spline, libplacebo's NORM curves)
// and their folded fast-kernel form are h2s_peak.h's host/device functions

// IPT-PQ matrices (h2s_lp_tone IPT), in double: BT.2020 RGB -> XYZ from the
// primaries and D65 white, XYZ -> LMS by the Hunt-Pointer-Estevez matrix of
// IPT (D65-normalised: neutral L = M = S = Y), and the inverse.  Keeping P and
// T reduces to L'M'S' += I' - I (the inverse IPT matrix has an I column of 1)
static void inv3(const double m[3][3], double o[3][3]) {
  const double d = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                   m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      o[i][j] = (m[(j + 1) % 3][(i + 1) % 3] * m[(j + 2) % 3][(i + 2) % 3] -
                 m[(j + 1) % 3][(i + 2) % 3] * m[(j + 2) % 3][(i + 1) % 3]) / d;
}

static void ipt_matrices(double r2l[9], double l2r[9]) {
  const double prim[3][2] = {{0.708, 0.292}, {0.170, 0.797}, {0.131, 0.046}}, wx = 0.3127, wy = 0.3290;
  double xyz[3][3], xyzi[3][3];
  for (int k = 0; k < 3; k++) {
    xyz[0][k] = prim[k][0] / prim[k][1];
    xyz[1][k] = 1.0;
    xyz[2][k] = (1.0 - prim[k][0] - prim[k][1]) / prim[k][1];
  }
  inv3(xyz, xyzi);
  const double w[3] = {wx / wy, 1.0, (1.0 - wx - wy) / wy};
  for (int k = 0; k < 3; k++) {
    const double sk = xyzi[k][0] * w[0] + xyzi[k][1] * w[1] + xyzi[k][2] * w[2];
    for (int i = 0; i < 3; i++) xyz[i][k] *= sk;                       // RGB -> XYZ
  }
  const double hpe[3][3] = {{0.4002, 0.7076, -0.0808}, {-0.2263, 1.1653, 0.0457}, {0.0, 0.0, 0.9182}};
  double rl[3][3], lr[3][3];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) rl[i][k] = hpe[i][0] * xyz[0][k] + hpe[i][1] * xyz[1][k] + hpe[i][2] * xyz[2][k];
  inv3(rl, lr);
  for (int i = 0; i < 9; i++) r2l[i] = rl[i / 3][i % 3], l2r[i] = lr[i / 3][i % 3];
}

// ---- the source constants (S1) ----
// The one derivation of a source set's depth-conversion constants and matrix
// terms.  Limited range (zimg's depth conversion): Y' = (code - 16 s) / 219 s,
// Cb, Cr = (code - 128 s) / 224 s, s = 2^(bits - 8).  Full range (zimg's
// full-range integer to float conversion): Y' = code / (2^b - 1), Cb, Cr =
// (code - 2^(b-1)) / (2^b - 1).  Its users round each term to float where they
// need one: source_kparams (the generic kernels' KParams), resolve_fast (the
// tile kernel's folded form) and the source pane (SrcPreviewParams).  The exact
// path on the device (h2s_lpx.h) restates the limited-range terms for itself

// (Kr, Kb) of enum h2s_src_matrix; the conversion kernels read BT.2020-NCL
static const double kKrKb[3][2] = {{0.2627, 0.0593}, {0.2126, 0.0722}, {0.299, 0.114}};

SourceConsts source_consts(int bits, bool full, int matrix) {
  const int sh = bits - 8;
  const double yr = full ? (double)((1 << bits) - 1) : (double)(219 << sh);
  const double cr = full ? yr : (double)(224 << sh);
  SourceConsts s;
  s.y_black = full ? 0.0 : (double)(16 << sh);
  s.mid = (double)(128 << sh);
  s.y_scale = 1.0 / yr, s.y_off = full ? 0.0 : -s.y_black / yr;
  s.c_scale = 1.0 / cr, s.c_off = -s.mid / cr;
  const double kr = kKrKb[matrix][0], kb = kKrKb[matrix][1], kg = 1.0 - kr - kb;
  s.m_rcr = 2.0 * (1.0 - kr);
  s.m_gcb = -2.0 * kb * (1.0 - kb) / kg;
  s.m_gcr = -2.0 * kr * (1.0 - kr) / kg;
  s.m_bcb = 2.0 * (1.0 - kb);
  return s;
}

// the one writer of KParams' S1 constants: resolve() for the parameters' depth
// (limited range), fill_geometry for the range of the set a call binds
void source_kparams(KParams* k, int bits, bool full) {
  const SourceConsts s = source_consts(bits, full);
  k->y_scale = (float)s.y_scale, k->y_off = (float)s.y_off;
  k->c_scale = (float)s.c_scale, k->c_off = (float)s.c_off;
  k->m_rcr = (float)s.m_rcr, k->m_gcb = (float)s.m_gcb, k->m_gcr = (float)s.m_gcr, k->m_bcb = (float)s.m_bcb;
}

void resolve(const h2s_params* p, KParams* k, std::vector<uint16_t>* eq) {
  memset(k, 0, sizeof(*k));
  // S1 zimg: depth conversion (limited range), BT.2020-NCL matrix, scale
  source_kparams(k, p->bits_in, false);
  k->transfer = p->transfer_in;
  k->lin_scale = (float)((p->transfer_in == H2S_TRC_HLG ? 1000.0 : 10000.0) / p->npl);

  // S2 vf_tonemap init defaults
  double param = p->tm_param;
  switch (p->tonemap) {
    case H2S_TM_GAMMA:
      if (isnan(param)) param = 1.8;
      break;
    case H2S_TM_REINHARD:
      if (!isnan(param)) param = (1.0 - param) / param;
      break;
    case H2S_TM_MOBIUS:
      if (isnan(param)) param = 0.3;
      break;
  }
  if (isnan(param)) param = 1.0;
  // ff_determine_signal_peak; trc at tonemap's input is linear -> 10.0
  double peak = p->peak;
  if (!(peak > 0)) {
    peak = 0;
    if (p->maxcll > 0) peak = p->maxcll / 100.0;
    if (!(peak > 0) && p->mastering_max > 0) peak = p->mastering_max / 100.0;
    if (!(peak > 0)) peak = 10.0;
  }
  k->tonemap = p->tonemap;
  k->desat_on = p->desat > 0 ? 1 : 0;
  k->desat = (float)p->desat;
  switch (p->desat_luma) {
    case H2S_DESAT_LUMA_BT2020: k->lr = 0.2627f, k->lg = 0.6780f, k->lb = 0.0593f; break;
    case H2S_DESAT_LUMA_BT709: k->lr = 0.2126f, k->lg = 0.7152f, k->lb = 0.0722f; break;
    default: k->lr = 1.0f, k->lg = 1.0f, k->lb = 1.0f;
  }
  k->lin_k = (float)(param / peak);
  k->gam_inv_peak = (float)(1.0 / peak);
  k->gam_inv_param = (float)(1.0 / param);
  k->gam_low_k = (float)(pow(0.05 / peak, 1.0 / param) / 0.05);
  k->clip_k = (float)param;
  k->hable_peak_inv = 1.0f / h2s::hable((float)peak);
  k->rein_p = (float)param;
  k->rein_k = (float)((peak + param) / peak);
  {
    const float j = (float)param;
    const float a = (float)(-j * j * (peak - 1.0f) / (j * j - 2.0f * j + peak));
    const float b = (float)((j * j - 2.0f * j * peak + peak) / fmax(peak - 1.0f, 1e-6));
    k->mob_j = j, k->mob_a = a, k->mob_b = b;
    k->mob_k = (b * b + 2.0f * b * j + j * j) / (b - a);
  }
  k->peak = peak;
  k->x_peak = peak, k->x_avg = 0.0, k->x_npl = p->npl, k->x_tm_param = p->tm_param, k->x_sh = p->bits_in - 8;
  // pipeline and SDR target (oracle resolve: the CPU chain's curve output is
  // relative to npl with no black; libplacebo targets PL_COLOR_SDR_WHITE =
  // 203 nits at PL_COLOR_SDR_CONTRAST = 1000:1)
  k->pipe = p->pipeline != H2S_PIPE_AUTO ? p->pipeline
                                         : (p->tonemap == H2S_TM_BT2390 || p->tonemap == H2S_TM_SPLINE ? h2s::PIPE_LIBPLACEBO
                                                                                                      : h2s::PIPE_CPU);
  const bool lp = k->pipe == h2s::PIPE_LIBPLACEBO;
  k->rgba8 = lp && p->lut_enabled ? 1 : 0;
  k->lp_ipt = lp && p->lp_tone == H2S_LP_TONE_IPT ? 1 : 0;
  // libplacebo stage options (ABI v3): range=tv on the rgba output, the
  // download's dither, the 12-bit input through format=p010
  const bool lim = lp && p->lp_range == H2S_LP_RANGE_LIMITED;
  k->lp_qs = lim ? 219.0f : 255.0f;
  k->lp_qo = lim ? 16.0f : 0.0f;
  k->lp_dith = lp && p->lp_dither == H2S_LP_DITHER_ORDERED ? 1 : 0;
  k->in_mask = lp && p->lp_p010 == H2S_LP_P010_TRUNCATE && p->bits_in == 12 ? 0xFFFCu : 0xFFFFu;
  ipt_matrices(k->ipt_r2l, k->ipt_l2r);
  k->t_white = isnan(p->target_white) ? (lp ? 203.0 : p->npl) : p->target_white;
  k->t_black = isnan(p->target_black) ? (lp ? k->t_white / 1000.0 : 0.0) : p->target_black;
  // peak_detect=1: vf_libplacebo's option defaults (smoothing_period 100,
  // scene_threshold_low / high 5.5 / 10, percentile 99.995, minimum_peak 1
  // x the SDR white); PARITY UNPINNED
  k->pd_smoothing = isnan(p->pd_smoothing) ? 100.0 : p->pd_smoothing;
  k->pd_scene_low = isnan(p->pd_scene_low) ? 5.5 : p->pd_scene_low;
  k->pd_scene_high = isnan(p->pd_scene_high) ? 10.0 : p->pd_scene_high;
  k->pd_percentile = isnan(p->pd_percentile) ? 99.995 : p->pd_percentile;
  k->pd_min = (isnan(p->pd_min_peak) ? 1.0 : p->pd_min_peak) * k->t_white / 100.0;
  k->knee_off = isnan(p->knee_offset) ? 1.0 : p->knee_offset;
  {
    const double lb = pow(k->t_black / k->t_white, 1.0 / 2.4), a = pow(1.0 - lb, 2.4);
    k->enc_ainv = (float)(1.0 / a);
    k->enc_a = (float)a;
    k->enc_b = (float)(lb / (1.0 - lb));
  }
  h2s::bt2390_consts(peak, k->t_white, k->t_black, k->knee_off, k, h2s::pq_refs(k->t_white, k->t_black));
  k->sp_contrast = isnan(p->tm_param) ? 0.5f : (float)p->tm_param;
  h2s::spline_consts(peak, 0.0, (double)k->sp_contrast, k->t_white, k->t_black, k, h2s::pq_refs(k->t_white, k->t_black));
  k->npl_1e4 = (float)(p->npl / 10000.0);
  k->e4_npl = (float)(10000.0 / k->t_white);
  k->ipt_npl = p->npl / 10000.0, k->ipt_os = 10000.0 / k->t_white, k->ipt_tw = k->t_white / 10000.0;
  k->lp_norm = lp && p->tonemap >= H2S_TM_REINHARD && p->tonemap <= H2S_TM_MOBIUS ? 1 : 0;
  k->n_nw = (float)(p->npl / k->t_white);
  h2s::lp_norm_consts(peak, p->tm_param, k->t_white, k);
  // closed-form gamut step (lut_enabled = 0), tools/generate_lut.py:36-40
  const double m[9] = {1.6604910021, -0.5876411388, -0.0728498633, -0.1245504745, 1.1328998971,
                       -0.0083494226, -0.0181507634, -0.1005788980, 1.1187296614};
  for (int i = 0; i < 9; i++) k->m709[i] = (float)m[i];
  k->lut_enabled = p->lut_enabled ? 1 : 0;
  // S6 BT.709 limited-range Y'CbCr rows
  const double r709 = 0.2126, g709 = 0.7152, b709 = 0.0722;
  k->k709[0] = (float)r709, k->k709[1] = (float)g709, k->k709[2] = (float)b709;
  k->kcb[0] = (float)(-r709 / 1.8556), k->kcb[1] = (float)(-g709 / 1.8556), k->kcb[2] = (float)(0.9278 / 1.8556);
  k->kcr[0] = (float)(0.7874 / 1.5748), k->kcr[1] = (float)(-g709 / 1.5748), k->kcr[2] = (float)(-b709 / 1.5748);
  // quantisation depth (oracle resolve): eq's yuv420p (compat8) or bits_out
  // (native; the libplacebo rgba frame with gamma 1 has no eq to pass)
  const int q = p->mode == H2S_MODE_NATIVE || (k->rgba8 && p->gamma == 1.0) ? p->bits_out : 8;
  k->qmax = (1 << q) - 1;
  k->qscale = (float)(1 << (q - 8));
  k->shift_out = p->bits_out - q;
  k->dither = p->dither == H2S_DITHER_ORDERED && q == 8 ? 1 : 0;
  k->expand_rep = p->expand == H2S_EXPAND_REPLICATE ? 1 : 0;
  k->chroma_edge = p->chroma_edge;
  k->lut_in16 = p->lut_input == H2S_LUT_IN_RGB48 && !lp ? 1 : 0;  // the CPU chain's S3 -> S4
  // S7 vf_eq create_lut, generalised to 2^q entries
  const int qn = 1 << q;
  eq->assign(qn, 0);
  bool ident = true;
  const double g = 1.0 / p->gamma;
  for (int i = 0; i < qn; i++) {
    double v = i / (double)(qn - 1);
    uint16_t o;
    if (v <= 0.0) {
      o = 0;
    } else {
      v = pow(v, g);
      o = v >= 1.0 ? (uint16_t)(qn - 1) : (uint16_t)(int)((double)qn * v);
    }
    (*eq)[i] = o;
    if (o != i) ident = false;
  }
  k->eq_identity = ident ? 1 : 0;
}

// ---- the cubic tables ----
// the cubic c0 + c1 t + c2 t^2 + c3 t^3 through four points: the 4x4
// Vandermonde system A c = y by Gaussian elimination (every table's solve)
static void solve_cubic(const double t[4], const double y[4], double c[4]) {
  double A[4][5];
  for (int k = 0; k < 4; k++) {
    for (int j = 0; j < 4; j++) A[k][j] = pow(t[k], j);
    A[k][4] = y[k];
  }
  for (int col = 0; col < 4; col++) {
    int piv = col;
    for (int r = col + 1; r < 4; r++)
      if (fabs(A[r][col]) > fabs(A[piv][col])) piv = r;
    for (int j = 0; j < 5; j++) std::swap(A[col][j], A[piv][j]);
    for (int r = 0; r < 4; r++) {
      if (r == col) continue;
      const double fct = A[r][col] / A[col][col];
      for (int j = col; j < 5; j++) A[r][j] -= fct * A[col][j];
    }
  }
  for (int k = 0; k < 4; k++) c[k] = A[k][4] / A[k][k];
}

// ST 2084 inverse EOTF (y = luminance / 10000 -> E) as PQI_NSEG cubic
// segments for the tile kernel's IPT form (h2s_tile_tone.h pqi): segment s covers
// y = 2^e (1 + j/8 + t), e = PQI_OCT0 + s/8, j = s%8, t in [0, 1/8), read from
// the float's exponent and top three mantissa bits; the cubic in t through
// the exact (double) encode at the 4 Chebyshev nodes (relative error <=
// 1.5e-7 with float32 coefficients).  Entry 0 is the constant PQ(0), read for
// y <= 0 and for y below the first octave (2^-64, 1e-15 nits: PQ within 3e-7
// of PQ(0)); segment s is entry 1 + s (PQI_NTAB entries)
void build_pqi_table(std::vector<float4>* out) {
  constexpr int K = h2s::PQI_PER_OCT;
  out->resize(h2s::PQI_NTAB);
  (*out)[0] = make_float4(0.0f, 0.0f, 0.0f, (float)h2s::hd_pq_encode(0.0));
  double t[4];
  for (int k = 0; k < 4; k++) t[k] = (1.0 - cos((2 * k + 1) * M_PI / 8.0)) / 2.0 / K;
  for (int sg = 0; sg < h2s::PQI_NSEG; sg++) {
    const double base = ldexp(1.0, h2s::PQI_OCT0 + sg / K);
    double y[4], c[4];
    for (int k = 0; k < 4; k++) y[k] = h2s::hd_pq_encode(base * (1.0 + (double)(sg % K) / K + t[k]));
    solve_cubic(t, y, c);
    (*out)[1 + sg] = make_float4((float)c[3], (float)c[2], (float)c[1], (float)c[0]);
  }
}

// PQ EOTF x scale as PQ_NSEG cubic segments: per segment, the cubic through
// the exact (double) EOTF at the 4 Chebyshev nodes of the segment.  Measured
// max relative error 1.2e-7 for E > 0.05 (float32 evaluation).
// cubic segments of f over E in [i, i+1) / PQ_SEG, i < PQ_NSEG, interpolating
// f at the four Chebyshev nodes of each segment (k_tile's pq_z layout)
template <class Fn>
static void build_seg_table(const Fn& eotf, std::vector<float4>* out) {
  double t[4];
  for (int k = 0; k < 4; k++) t[k] = (1.0 - cos((2 * k + 1) * M_PI / 8.0)) / 2.0;
  out->resize(h2s::PQ_NSEG);
  for (int i = 0; i < h2s::PQ_NSEG; i++) {
    double y[4], c[4];
    for (int k = 0; k < 4; k++) y[k] = eotf((i + t[k]) / h2s::PQ_SEG);
    solve_cubic(t, y, c);
    if (i == 0) c[0] = 0.0;  // E = 0 maps to exactly 0, as zimg's x > 0 test
    (*out)[i] = make_float4((float)c[3], (float)c[2], (float)c[1], (float)c[0]);
  }
}

void build_pq_table(double scale, std::vector<float4>* out) {
  // (hd_pq_eotf's expression with the table's own guard: past the pole, den <= 0, +inf)
  const double m1 = h2s::PQ_M1_D, m2 = h2s::PQ_M2_D, c1 = h2s::PQ_C1_D, c2 = h2s::PQ_C2_D, c3 = h2s::PQ_C3_D;
  build_seg_table([&](double e) {
    if (!(e > 0)) return 0.0;
    const double xp = pow(e, 1.0 / m2);
    const double num = fmax(xp - c1, 0.0), den = c2 - c3 * xp;
    return den > 0 ? pow(num / den, 1.0 / m1) * scale : HUGE_VAL;
  }, out);
}

// zimg arib_b67_inverse_oetf (k_tile's HLG input on the CPU chain; the OOTF
// follows in the kernel): E^2 / 3 up to 1/2, (exp((E - c) / a) + b) / 12
// above; 1/2 is a segment boundary, so every segment interpolates one smooth
// branch (the quadratic one exactly)
void build_hlg_table(std::vector<float4>* out) {
  const double a = 0.17883277, b = 0.28466892, c = 0.55991073;
  build_seg_table([&](double e) {
    if (!(e > 0)) return 0.0;
    return e <= 0.5 ? e * e / 3.0 : (exp((e - c) / a) + b) / 12.0;
  }, out);
}

// FastParams from the resolved KParams (same constants, scales folded)
void resolve_fast(const h2s_ctx* c, const KParams& k, FastParams* F) {
  memset(F, 0, sizeof(*F));
  const h2s_params* p = &c->params;
  const int sh = p->bits_in - 8;
  // (the range of the set k binds, k.full: source_consts' terms in double)
  const SourceConsts sc = source_consts(p->bits_in, k.full != 0);
  const double ys = sc.y_scale, yo = sc.y_off, cs = sc.c_scale, co = sc.c_off;
  const double mrcr = sc.m_rcr, mgcb = sc.m_gcb, mgcr = sc.m_gcr, mbcb = sc.m_bcb;
  F->ys = (float)ys;
  F->k_r = (float)(yo + mrcr * co);
  F->k_g = (float)(yo + (mgcb + mgcr) * co);
  F->k_b = (float)(yo + mbcb * co);
  F->y_off_c = (float)yo;
  F->c_mid = (float)sc.mid;
  for (int odd = 0; odd < 2; odd++) {
    const double d = odd ? 8.0 : 4.0;
    F->a_rv[odd] = (float)(mrcr * cs / d);
    F->a_gu[odd] = (float)(mgcb * cs / d);
    F->a_gv[odd] = (float)(mgcr * cs / d);
    F->a_bu[odd] = (float)(mbcb * cs / d);
  }
  F->log2_lin_scale = (float)log2((p->transfer_in == H2S_TRC_HLG ? 1000.0 : 10000.0) / p->npl);
  F->log2_pq_scale = (float)log2(10000.0 / p->npl);
  {
    // k_tile takes a tile's steps without the exact-path ballot when every
    // pixel's E stays below the table's end: staged luma <= safe_y and
    // |centred chroma| <= safe_c (the legal half-range) give
    // E <= Y' + max_c sum |a| * safe_c < PQ_EMAX.  Table forms only (E staged
    // in segment units + 1); the direct HLG form has no exact path
    const bool table = p->transfer_in == H2S_TRC_PQ || k.pipe != h2s::PIPE_LIBPLACEBO;
    // Full range (k.full): every code is legal.  With safe_c at the whole
    // half-range (128 << sh) the luma bound would fall to Y' < 0.93 and every
    // bright tile would lose the branch-free body, so the split goes the other
    // way: the luma bound is set just above Y' = 1 (every luma code passes)
    // and safe_c is what that leaves, (EMAX - 1e-3 - ymax) / amax = 92.9 % of
    // the half-range (475 of 512 codes at 10 bits).  Only tiles with chroma
    // beyond it take the exact-capable body
    const double amax = std::max(std::max(fabs(mrcr), fabs(mgcb) + fabs(mgcr)), fabs(mbcb)) * cs;
    const double safe_c = k.full ? floor(((double)h2s::PQ_EMAX - 1e-3 - (1.0 + 1e-4)) / amax) : (double)(112 << sh);
    const double ymax = k.full ? 1.0 + 1e-4 : (double)h2s::PQ_EMAX - amax * safe_c - 1e-3;
    F->safe_c = table ? (float)safe_c : HUGE_VALF;
    F->safe_y = table ? (float)(ymax * h2s::PQ_SEG + 1.0) : HUGE_VALF;
  }
  F->lr = k.lr, F->lg = k.lg, F->lb = k.lb, F->desat = k.desat;
  F->rein_p = k.rein_p, F->rein_k = k.rein_k;
  F->hable_peak_inv = k.hable_peak_inv;
  F->hable_ka = (float)(2.1 / 15.0 * (double)k.hable_peak_inv);
  F->hable_kb = (float)(0.25 / 15.0 * (double)k.hable_peak_inv);
  F->mob_j = k.mob_j, F->mob_a = k.mob_a, F->mob_b = k.mob_b, F->mob_k = k.mob_k;
  F->npl_1e4 = k.npl_1e4, F->e4_npl = k.e4_npl;
  F->b_e1min = (float)h2s::hd_pq_encode(1e-6 * p->npl / 10000.0);
  F->tw_fold = (float)(p->npl / k.t_white);
  // libplacebo branch: 255 ((x ainv)^(1/2.4) - b) as exp2(log2(x)/2.4 + k1) - k2
  F->lp_k1 = (float)(log2((double)k.enc_ainv) / 2.4 + log2(255.0));
  F->lp_k2 = (float)(255.0 * (double)k.enc_b);
  F->lp_xmax = (float)(pow(1.0 + (double)k.enc_b, 2.4) / (double)k.enc_ainv * 1.001);
  F->nm1 = (float)(c->lut_n - 1);
  F->inv255 = 1.0f / 255.0f;
  F->qscale = k.qscale;
  F->c56 = 56.0f * k.qscale;
  for (int i = 0; i < 3; i++) F->k709[i] = k.k709[i], F->kcb[i] = k.kcb[i], F->kcr[i] = k.kcr[i];
  F->lp_ipt = k.lp_ipt;
  F->lp_qs_f = k.lp_qs / 255.0f;
  F->lp_qo = k.lp_qo;
  for (int i = 0; i < 3; i++) {
    F->lp_ky[i] = (float)((double)k.k709[i] / 255.0 * 219.0 * (double)k.qscale);
    F->lp_kcb[i] = (float)((double)k.kcb[i] / 255.0 * 56.0 * (double)k.qscale);
    F->lp_kcr[i] = (float)((double)k.kcr[i] / 255.0 * 56.0 * (double)k.qscale);
  }
  F->lp_cy = 16.0f * k.qscale + 0.5f;
  F->lp_dith = k.lp_dith;
  F->in_mask2 = k.in_mask | (k.in_mask << 16);
  for (int i = 0; i < 9; i++)
    F->ipt_r2l[i] = (float)(k.ipt_r2l[i] * k.ipt_npl), F->ipt_l2r[i] = (float)(k.ipt_l2r[i] * (p->npl / k.t_white));
  F->pqi_tab = c->d_pqi;
  F->lut_off = k.lut_enabled ? 0 : 1;
  F->n_nw = k.n_nw;
  F->tw_1e4 = (float)(k.t_white / 10000.0);
  for (int i = 0; i < 9; i++) F->m709[i] = k.m709[i];
  h2s::curve_fast(k, static_cast<h2s::CurveConsts*>(F));
  const int n = c->lut_n;
  F->log2_nm1 = (float)log2((double)(n - 1));
  F->s_max = nextafterf((float)(n - 1), 0.0f);
  F->x_max = 0.999999f;  // (N-1) * x_max^(1/2.4) stays > 3 ulp below N-1
  F->stride_g = (float)(12 * n);
  F->stride_b = (float)(12 * n * n);
  F->og = 12 * n;
  F->ob = 12 * n * n;
  F->c111 = 12 * (1 + n + n * n);
  F->cr = F->c111 - 12;
  F->cg = F->c111 - F->og;
  F->cb = F->c111 - F->ob;
  F->lut_yuv = c->d_lut_yuv;
  F->lut_bytes = 12 * n * n * n;
  F->lut8x = c->d_lut8x;
  F->eq_lut = c->d_eq;
  F->eq_n = k.qmax + 1;
  F->c_bias = 128.0f * k.qscale + 0.5f;
  F->shift_out = k.shift_out;
  F->rep_rs = k.expand_rep && k.shift_out ? 8 - k.shift_out : 31;
  F->dither = k.dither;
  F->out8 = p->bits_out == 8 ? 1 : 0;
  // the table k_tile stages for its input transfer: the PQ EOTF, or for HLG
  // input on the CPU chain the inverse OETF (the libplacebo branch keeps the
  // PQ table for its IPT form and evaluates the HLG curve directly)
  F->pq_tab = p->transfer_in == H2S_TRC_HLG && k.pipe != h2s::PIPE_LIBPLACEBO ? c->d_hlg : c->d_pq;
}

// ---- filter taps ----

// swscale SWS_BICUBIC with its default parameters B = 0, C = 0.6
static double bicubic(double x) {
  const double B = 0.0, C = 0.6;
  x = fabs(x);
  if (x < 1.0) return ((12 - 9 * B - 6 * C) * x * x * x + (-18 + 12 * B + 6 * C) * x * x + (6 - 2 * B)) / 6.0;
  if (x < 2.0) return ((-B - 6 * C) * x * x * x + (6 * B + 30 * C) * x * x + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) / 6.0;
  return 0.0;
}

// BICUBIC chroma taps (oracle_chroma_taps): horizontal 7 taps around the
// left-sited position, vertical 8 around the centre-sited one, normalised
void chroma_taps(float* wx7, float* wy8) {
  double tx[7], ty[8], sx = 0, sy = 0;
  for (int i = 0; i < 7; i++) sx += (tx[i] = bicubic((i - 3) / 2.0));
  for (int j = 0; j < 8; j++) sy += (ty[j] = bicubic((j - 3.5) / 2.0));
  for (int i = 0; i < 7; i++) wx7[i] = (float)(tx[i] / sx);
  for (int j = 0; j < 8; j++) wy8[j] = (float)(ty[j] / sy);
}

// the preview's resize, appended to w / start: per output index the first
// source tap and T normalised weights (centre-aligned sampling; the kernel
// widens by the ratio when downscaling).  Returns T
int resize_taps(int src, int dst, std::vector<float>* w, std::vector<int>* start) {
  const double scale = (double)src / dst, fw = scale > 1.0 ? scale : 1.0;
  const int T = (int)ceil(4.0 * fw) + 1;
  const size_t w0 = w->size(), s0_ = start->size();
  w->resize(w0 + (size_t)dst * T, 0.0f);
  start->resize(s0_ + dst, 0);
  for (int o = 0; o < dst; o++) {
    const double c = (o + 0.5) * scale - 0.5;
    const int s0 = (int)floor(c - 2.0 * fw) + 1;
    // (T <= 49 at the ratio limit of 12; a 4:4:4 source pane's chroma columns reach 24, T = 97)
    double sum = 0.0, tmp[128];
    for (int i = 0; i < T && i < 128; i++) sum += (tmp[i] = bicubic((s0 + i - c) / fw));
    for (int i = 0; i < T && i < 128; i++) (*w)[w0 + (size_t)o * T + i] = (float)(tmp[i] / sum);
    (*start)[s0_ + o] = s0;
  }
  return T;
}

// ---- the dynamic peak's model (h2s_api_peak.hip runs it) ----
PeakModel peak_model(const h2s_ctx* c, const KParams& k) {
  h2s::PeakModel m;
  m.t_white = k.t_white, m.t_black = k.t_black, m.knee_off = k.knee_off;
  m.contrast = k.sp_contrast, m.tm_param = c->params.tm_param, m.static_peak = k.peak;
  m.smoothing = k.pd_smoothing, m.scene_low = k.pd_scene_low, m.scene_high = k.pd_scene_high;
  m.percentile = k.pd_percentile, m.min_peak = k.pd_min;
  m.iir_a = k.pd_smoothing > 0.0 ? 1.0 - exp(-1.0 / k.pd_smoothing) : 1.0;
  m.npx = (double)k.W * k.H;
  m.nblocks = c->peak_blocks;
  m.pct = k.pd_percentile < 100.0 ? 1 : 0;
  m.family = k.tonemap;
  m.pq = h2s::pq_refs(k.t_white, k.t_black);
  return m;
}

}  // namespace host
}  // namespace h2s
