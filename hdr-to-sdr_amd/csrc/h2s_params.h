// h2s_params.h — the launch parameter blocks and the constants that the host
// units and every kernel share.
// What belongs here: the structs a launch passes by value or that the context
// keeps in device memory (DoviCurve / DoviRec, KParams, CurveConsts,
// FastParams, YuvLutConsts) and the compile-time constants both sides agree on
// (PIPE_*, the tile size TBW x TBH, the table layouts PQ_* / PQI_*).  No
// function bodies: the helpers both kernels share are h2s_math.h's, the
// generic kernel's per-pixel chain is h2s_chain.h's.  The layout of every
// struct is part of the kernels' listings: a new field goes last.
//
// Stage numbering follows the reference chain string (src/utils.py:38-42):
//   S1 zscale=t=linear:npl=100   S2 tonemap={tm}   S3 zscale=t=bt709
//   S4 lut3d=interp=tetrahedral  S6 (auto) scale->yuv420p  S7 eq=gamma
//   S8 (auto) scale->-pix_fmt (src/ffmpeg_command.py:355-360)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace h2s {

struct CurveConsts;

// A frame's Dolby Vision profile-5 record (h2s_set_dovi): the device's view of
// include/h2s.h's h2s_dovi_curve / h2s_dovi_rpu, field for field
// (h2s_api_dovi.hip asserts it), as the context keeps them in device memory
struct DoviCurve {
  int num_pivots;
  float pivots[9];
  int method[8];
  float poly[8][3];
  int mmr_order[8];
  float mmr_const[8];
  float mmr[8][3][7];
};
struct DoviRec {
  float off[3], nl[9], lin[9];   // row-major
  DoviCurve comp[3];
};

struct KParams {
  // geometry (luma W x H, output chroma cw x ch, ngx groups of QPT chroma columns)
  int W, H, cw, ch, ngx;
  int nframes;
  long long total;  // nframes * ch * ngx work items
  const uint8_t* in[3];
  long long in_ls[3], in_fp[3];
  uint8_t* out[3];
  long long out_ls[3], out_fp[3];
  // frame layout (h2s_set_frame_layout).  Semi-planar: plane 2 aliases plane
  // 1 one sample on (same linesize and pitch), samples of a chroma row lie
  // cstep samples apart, and 16-bit words carry the code in the high bits:
  // code = word >> in_sh (in_mask then drops the word's wrapped-down bits),
  // word = code << out_sh.  Planar: cstep 1, shifts 0
  int in_cstep, in_sh, out_cstep, out_sh;
  // S1: zimg depth conversion, BT.2020-NCL matrix, transfer
  float y_scale, y_off, c_scale, c_off;
  float m_rcr, m_gcb, m_gcr, m_bcb;
  float lin_scale;
  int transfer;  // h2s_transfer
  // S2: vf_tonemap
  int tonemap;  // h2s_tonemap
  int desat_on;
  float desat, lr, lg, lb;
  float lin_k;          // LINEAR: param/peak
  float gam_inv_peak, gam_inv_param, gam_low_k;  // GAMMA
  float clip_k;         // CLIP: param
  float hable_peak_inv; // HABLE: 1/hable(peak)
  float rein_p, rein_k; // REINHARD: param, (peak+param)/peak
  float mob_j, mob_a, mob_b, mob_k;  // MOBIUS
  float b_srcmin, b_range, b_inv_range, b_ks, b_inv_1mks, b_maxlum;  // BT2390
  float npl_1e4, e4_npl;  // npl/10000, 10000/npl
  // SPLINE (libplacebo, PQ domain): clip range, knee, toe P, shoulder Q, output range
  float sp_srcmin, sp_srcmax, sp_kin, sp_kout, sp_pa, sp_pb, sp_qa, sp_qb, sp_qc, sp_dmin, sp_dmax;
  float sp_contrast;
  double peak;            // resolved static source peak (units of 100 nits; host side)
  // libplacebo bt2390 black-point adaptation (min_lum = 0: off)
  float b_minlum, b_bp, b_gain;
  double t_black, t_white, knee_off;  // SDR target (nits) and BT.2390 knee offset (host side)
  // pipeline (h2s_pipeline, resolved to CPU_CHAIN or LIBPLACEBO)
  int pipe, rgba8;
  float enc_ainv, enc_b;  // libplacebo BT.1886 encode: (x * ainv)^(1/2.4) - b
  float enc_a;            // (the generic kernel divides by a, as the oracle)
  int lp_ipt;             // libplacebo branch: the curve on IPT-PQ intensity (h2s_lp_tone IPT)
  // libplacebo branch options (include/h2s.h ABI v3): rgba8 code =
  // floor(clamp01(v) lp_qs + lp_qo + (lp_dith ? bayer16(x, y) : 0.5));
  // in_mask: input code mask (0xFFFC: a 12-bit input through format=p010
  // with the two low bits dropped, h2s_lp_p010 TRUNCATE)
  float lp_qs, lp_qo;
  int lp_dith;
  unsigned in_mask;
  // peak_detect (host side): IIR period (frames), scene thresholds (% PQ),
  // percentile, minimum peak (units of 100 nits)
  double pd_smoothing, pd_scene_low, pd_scene_high, pd_percentile, pd_min;
  double ipt_r2l[9], ipt_l2r[9];  // BT.2020 RGB -> LMS (HPE), inverse (row-major)
  double ipt_npl, ipt_os, ipt_tw; // npl / 10000, 10000 / target white, target white / 10000 (double)
  // libplacebo reinhard / hable / mobius (scaling PL_HDR_NORM: 1 = target white)
  int lp_norm;                    // the libplacebo branch with one of them
  float n_peak, n_nw;             // source peak / white; npl / white (npl units -> NORM)
  float n_rein_off, n_rein_scale, n_hable_inv, n_mob_j, n_mob_a, n_mob_b, n_mob_scale;
  // S3/S4
  int lut_enabled, lut_n, lut_sg, lut_sb;
  float lut_max;
  const float4* lut;
  float m709[9];
  // S6..S8
  int qmax, shift_out;
  float qscale;
  int eq_identity;
  const uint16_t* eq_lut;
  int chroma_edge;        // S1 upsampler edge rule (chroma_edge_at)
  int lut_in16;           // S3 -> S4 as 16-bit R'G'B' (h2s_lut_input RGB48)
  int dither;             // ordered 8x8 dither at the 8-bit quantiser
  int expand_rep;         // S8 bit replication instead of a shift
  // Y'CbCr 709 rows
  float k709[3], kcb[3], kcr[3];
  int gx0;  // first column group this launch covers (tail launches)
  float2* chr444;         // BICUBIC: per-pixel (Cb, Cr) of one frame (two-pass path)
  // dynamic peak detection (one frame per launch): the frame's curve record,
  // written on the device by k_peak_curves; null: the constants above
  const CurveConsts* cv;
  // the libplacebo branch's exact path (h2s_lpx.h): source peak (units of 100
  // nits) and average PQ level (0: the default spline knee) its double
  // constants derive from, npl, tm_param (NaN: default), bits_in - 8
  double x_peak, x_avg, x_npl, x_tm_param;
  int x_sh;
  // the input's chroma subsampling (h2s_set_input_subsampling: 0 = 4:2:0, 1 =
  // 4:2:2, 2 = 4:4:4) and its chroma plane icw x ich (W/2 x H/2, W/2 x H, W x
  // H).  cw, ch, ngx and total above are the output side's, always W/2 x H/2
  int sub, icw, ich;
  // the input's tags (h2s_set_input_tags).  full: full-range codes, y_scale ..
  // c_off above are then 1 / (2^b - 1), 0, 1 / (2^b - 1), -2^(b-1) / (2^b - 1)
  // (the exact path's double forms read the flag).  vco: 4:2:0 chroma rows
  // co-sited with the even luma rows (top-left): vertical taps (0, 1) on even
  // rows, (1/2, 1/2) with row cy + 1 on odd ones; 0 whenever sub != 0
  int full, vco;
  // Dolby Vision profile 5 (h2s_set_dovi; null: off): the context's records,
  // read by the k_process<..., DOVI> / k_debug<..., DOVI> / k_peak_stats<2, ...>
  // instances only (last, so that no other field moves).  Frame f of the
  // launch takes record dovi_n == 1 ? 0 : dovi_f0 + f (dovi_f0: the launch's
  // first frame within its call)
  const DoviRec* dovi;
  int dovi_n, dovi_f0;
};

constexpr int PIPE_CPU = 1, PIPE_LIBPLACEBO = 2;

// Constants of the PQ-domain curves (BT.2390 / spline) in the tile kernel's
// folded form.  They are the only parameters that change from frame to frame
// under dynamic peak detection, so a launch can take one record per frame.
struct CurveConsts {
  float b_srcmin, b_range, b_inv_range, b_ks, b_inv_1mks, b_maxlum;  // BT.2390, HLG input
  float b_minlum, b_bp, b_gain;  // black-point adaptation (b_minlum = 0: off)
  // PQ-input forms that land directly on pq_z's table coordinate u = e*PQ_SEG + 1:
  // BT.2390: e1n = med3(e1*e1a + e1b), t = e1n*ta + tb, u = c3..c0 Horner (knee) or e1n*lr + lc
  float b_e1a, b_e1b, b_ta, b_tb, b_c3, b_c2, b_c1, b_c0, b_lr, b_lc, b_thr;
  float sp_srcmin, sp_srcmax, sp_kin, sp_kout, sp_pa, sp_pb, sp_qa, sp_qb, sp_qc, sp_dmin, sp_dmax;  // SPLINE
  // spline: u = Horner(x) with the coefficients and kout scaled by PQ_SEG, clamped to [umin, umax]
  float sp_qa_u, sp_qb_u, sp_qc_u, sp_pa_u, sp_pb_u, sp_k_u, sp_umin, sp_umax;
  // BT.2390 black-point adaptation on the table coordinate u = e2*R + C:
  // 1 - e2 = u*bk_a + bk_b; u' = gain*u + bk_c*(1 - e2)^bp + bk_d for e2 < 1
  float b_bk_a, b_bk_b, b_bk_c, b_bk_d;
  // libplacebo reinhard / hable / mobius in NORM units (1 = target white)
  float n_peak, n_rein_off, n_rein_scale, n_hable_inv, n_mob_j, n_mob_a, n_mob_b, n_mob_scale;
  // the frame's source peak (units of 100 nits) and smoothed average PQ level,
  // from which the generic kernel's exact libplacebo path (h2s_lpx.h) derives
  // its double constants
  double x_peak, x_avg;
};

// Parameters of the tile kernel (k_tile, h2s_tile.h): the same chain with
// every scale folded into constants.
struct FastParams : CurveConsts {
  int W, H, cw, ch;                // luma / chroma geometry (W % 64 == 0)
  int chroma_edge;                 // S1 upsampler edge rule (chroma_edge_at)
  unsigned nbx, nby, nframes;      // 64 x 32 tiles per row / column, frames
  int tpb;                         // tiles walked by one block (k_tile prefetches tile i+1 during tile i)
  const uint8_t* in[3];
  long long in_ls[3], in_fp[3];
  uint8_t* out[3];
  long long out_ls[3], out_fp[3];
  int in_bytes[3], out_bytes[3];   // plane extents for buffer resources (clamped to 2^31-1)
  // S1: R'G'B' = k + ys*Y + a*{U,V}; index [0] even columns (x4), [1] odd (x8)
  float ys, k_r, k_g, k_b;
  float a_rv[2], a_gv[2], a_gu[2], a_bu[2];
  float log2_lin_scale;
  float log2_pq_scale;             // log2(10000 / npl): the PQ EOTF table's scale (the IPT decode reads it for HLG input too)
  float y_off_c, c_mid;            // k_tile staging: Y' = Y*ys + y_off_c, chroma centred on c_mid
  // S2
  float lr, lg, lb, desat;
  float rein_p, rein_k;
  float hable_peak_inv;
  float hable_ka, hable_kb;        // 0.14 / hable(peak), (1/60) / hable(peak): hable(x)/x = (0.14 x + 1/60) / D(x)
  float mob_j, mob_a, mob_b, mob_k;
  float npl_1e4, e4_npl;
  float tw_fold;                   // BT.2390 / spline on PQ input: npl / target white (the EOTF table is npl-scaled)
  float b_e1min;                   // PQ code of sig = 1e-6 (BT.2390 / spline e1 lower bound)
  // libplacebo branch (k_tile<..., LP = 1>): 255 (x ainv)^(1/2.4) - 255 b =
  // exp2(log2(x)/2.4 + lp_k1) - lp_k2, x clamped to [0, lp_xmax] (v >= 1 above);
  // lut3d's 8-bit coordinate (q * inv255) * nm1; BT.709 rows at depth q
  float lp_k1, lp_k2, lp_xmax, nm1, inv255, qscale, c56;
  float k709[3], kcb[3], kcr[3];
  // lp_tone = IPT: RGB (npl units) -> LMS / 10000 (npl/10000 folded in); LMS
  // -> RGB; the PQ encode as PQI_NSEG cubic segments (pqi)
  int lp_ipt;
  // rgba8 download (the LP instances): code = floor(e lp_qs_f + qoff), e the
  // 255-scaled encode, qoff = lp_qo + (lp_dith ? bayer16 : 0.5) per pixel;
  // in_mask2: the input code mask on a packed pair of samples
  float lp_qs_f, lp_qo;
  int lp_dith;
  unsigned in_mask2;
  // the Y'CbCr rows applied to lut3d's 8-bit output codes directly (tile
  // kernel): o = (sum lp_ky[c] code_c + lp_cy, sum lp_kcb[c] code_c,
  // sum lp_kcr[c] code_c), i.e. k709 / kcb / kcr x inv255 x (219 qscale | 56
  // qscale) folded on the host; lp_cy = 16 qscale + 0.5
  float lp_ky[3], lp_kcb[3], lp_kcr[3], lp_cy;
  float ipt_r2l[9], ipt_l2r[9];
  const float4* pqi_tab;
  // libplacebo branch with the LUT off (k_tile<..., LP = 1>): libplacebo's own
  // BT.2020 -> BT.709 conversion (linear matrix, clip) and the nv12 download
  int lut_off;
  float m709[9];
  float n_nw, tw_1e4;              // npl / target white (npl units -> NORM); target white / 10000
  const CurveConsts* cv_frames;    // dynamic peak: one curve per frame of the launch (else null:
                                   // the base CurveConsts is the batch's curve)
  // S3/S4: lattice coordinates and byte offsets (float4 records)
  float log2_nm1, s_max, stride_g, stride_b;  // byte strides 12N, 12N^2 (as floats)
  float x_max;                                 // largest x with (N-1) x^(1/2.4) < N-1 (margin)
  int og, ob, cr, cg, cb, c111;                // corner byte offsets
  const float* lut_yuv;                        // 12-byte records (Y', Cb', Cr')
  int lut_bytes;
  const unsigned* lut8x;                       // libplacebo branch: lut3d's 8-bit output per rgba code triple
                                               // (bit-interleaved index; R | G << 8 | B << 16), k_build_lut8x
  // S6..S8
  const uint16_t* eq_lut;
  int eq_n;
  float c_bias;
  int shift_out, out8;
  int rep_rs;                      // S8: 8 - shift_out (bit replication) or 31 (shift)
  int dither;                      // S6 ordered dither at the 8-bit quantiser
  // BICUBIC chroma (two-pass, one frame per launch): per-pixel (Cb, Cr) into
  // chr444 (row pitch chr_w) instead of the 2x2 sums; inv_c56 = 1 / (56 q)
  float2* chr444;
  int chr_w;
  float inv_c56;
  // k_tile's branch-free tiles: every staged luma <= safe_y and every centred
  // chroma code <= safe_c bound E below the EOTF table's end (resolve_fast)
  float safe_y, safe_c;
  // S1 PQ EOTF (x 10000/npl) as a piecewise cubic: segment i covers
  // E in [i, i+1)/PQ_SEG, coefficients (c3, c2, c1, c0) of t = E*PQ_SEG - i
  const float4* pq_tab;
  // debug instances (k_tile<..., DBG = 1>): stage planes of frame 0, row pitch
  // dbg_w floats; the float4 RGB lattice for stage 4; 1 / (N-1); the stage
  // whose planes are written is dbg_stage (the struct's last member)
  float* dbg;
  int dbg_w;
  const float4* dbg_lut;
  float inv_nm1;
  // semi-planar surfaces (h2s_set_frame_layout), read by the k_tile<..., SEMI>
  // instances only (block-uniform branches there; the planar instances never
  // touch these, and they sit last so that no other field moves): plane 1
  // holds (Cb, Cr) pairs and plane 2 is unused; 16-bit words carry the code
  // in the high bits.  Input words are shifted down by in_sh and masked with
  // in_mask2 (which then also clears the bits that cross the halves of a word
  // pair); output codes are shifted up by out_sh
  int in_semi, in_sh, out_semi, out_sh;
  // 4:2:2 / 4:4:4 input (h2s_set_input_subsampling), read by the k_tile<...,
  // SUB> instances only (last again, so that no other field moves): the
  // input's chroma plane is icw x ich samples (W/2 x H, or W x H); cw and ch
  // above stay the output's W/2 x H/2
  int icw, ich;
  // the h2s_stage (1..5) whose planes a debug instance writes to dbg, read by
  // the k_tile<..., DBG = 1> instances only (launch-uniform branches there;
  // last again, so that no other field moves)
  int dbg_stage;
  // Dolby Vision profile 5 (h2s_set_dovi), read by the k_tile<TRC = 2, ...>
  // instances only (last again): the context's records; a tile of frame f of
  // the launch takes record dovi_n == 1 ? 0 : dovi_f0 + f (block-uniform per
  // tile, read through the scalar cache).  Those instances stage luma as the
  // code fraction y / (2^b - 1) (ys, y_off_c folded so on the host) and chroma
  // centred on c_mid; dv_cs = 1 / (8 (2^b - 1)) and dv_cm = c_mid / (2^b - 1)
  // turn the x8 upsampled centred chroma back into its fraction
  const DoviRec* dovi;
  int dovi_n, dovi_f0;
  float dv_cs, dv_cm;
};

constexpr int TBW = 64, TBH = 32;   // k_tile: luma tile of one block
constexpr int PQ_SEG = 128;          // segments per unit of E
constexpr int PQ_NSEG = 240;         // table covers E in [0, 1.875)
constexpr float PQ_EMAX = 1.875f;    // above: exact transcendental path
constexpr int PQI_OCT0 = -64;        // PQ encode table: first octave 2^-64 (x 10000 nits)
constexpr int PQI_PER_OCT = 8;       // segments per octave (exponent + top 3 mantissa bits)
constexpr int PQI_NSEG = 78 * PQI_PER_OCT;   // octaves 2^-64 .. 2^14
// the table holds PQI_NSEG + 1 entries: [0] = PQ(0) as a constant (y <= 0,
// and y below the first octave), [1 + s] = segment s
constexpr int PQI_NTAB = PQI_NSEG + 1;

struct YuvLutConsts {
  float s, k709[3], kcb[3], kcr[3];
  int rgb;  // 1: plain R'G'B' records (the libplacebo branch truncates lut3d's output before Y'CbCr)
};

}  // namespace h2s
