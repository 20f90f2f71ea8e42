// h2s_kernels.hip — the chain's exact restatement for gfx950: k_process,
// k_debug, k_chroma_bicubic, k_build_lut8x and their launchers, built without
// FMA contraction so that the float arithmetic rounds where the oracle's does.
//
// k_process: the whole per-frame chain of src/utils.py:38-42 fused into one
// pass over HBM: read packed 10/12-bit planar 4:2:0, upsample chroma, S1..S4
// per pixel, RGB->Y'CbCr, 2x2 chroma reduction, quantise, eq, write 4:2:0.
// One work item = QPT horizontally adjacent 2x2 luma quads (one output chroma
// sample each) of one chroma row of one frame; the flattened item index runs
// columns fastest, so a wavefront reads contiguous row segments (16-B Y loads,
// 8-B chroma loads per lane).  Blocks are remapped so that each XCD walks a
// contiguous range of rows (chroma halo rows and LUT lines stay in its L2;
// xcd_remap, h2s_math.h).
#include <hip/hip_runtime.h>

#include "h2s_launch.h"
#include "h2s_lpx.h"
#include "h2s_math.h"
#include "h2s_params.h"

namespace h2s {

// the upsampler's edge rule (params.chroma_edge; oracle/h2s_oracle.c edge())
__device__ __forceinline__ int edge(const KParams& P, int i, int n) { return chroma_edge_at(i, n, P.chroma_edge); }

__device__ __forceinline__ int ld16(const uint8_t* row, int x) {
  return *reinterpret_cast<const uint16_t*>(row + 2 * x);
}
// the input code of a 16-bit word (semi-planar: in its high bits), masked
// (h2s_lp_p010 TRUNCATE; the mask also bounds a semi-planar code)
__device__ __forceinline__ int code_of(const KParams& P, unsigned w16) { return (int)((w16 >> P.in_sh) & P.in_mask); }
// luma sample x / chroma sample x (P.in_cstep words apart) of a row
__device__ __forceinline__ int ldy(const KParams& P, const uint8_t* row, int x) { return code_of(P, (unsigned)ld16(row, x)); }
__device__ __forceinline__ int ldc(const KParams& P, const uint8_t* row, int x) {
  return code_of(P, (unsigned)ld16(row, x * P.in_cstep));
}

// C444: BICUBIC chroma (two-pass path): store every pixel's (Cb, Cr) into
// P.chr444 (frame 0 of the launch, W x H) instead of the 2x2 mean; the
// chroma planes are then written by k_chroma_bicubic
// LPX: the libplacebo branch, stages 1-3 in exact arithmetic (h2s_lpx.h)
// from the integer codes (cc*: the chroma codes kept for it)
// SUB: the input's chroma subsampling (P.sub; CPU chain, static peak): 1 =
// 4:2:2, chroma rows 2cy and 2cy+1 of a W/2 x H plane through the horizontal
// pass alone; 2 = 4:4:4, the pixel's own sample of a W x H plane.  The output
// side (the work item, the 2x2 reduction, the stores) is 4:2:0 whatever SUB
// P.vco (launch-uniform; h2s_set_input_tags, 4:2:0 input sited top-left): the
// vertical taps are (0, 1) on the even luma row and (1/2, 1/2) with row cy + 1
// on the odd one, in every form (DYN and LPX included); a field (read as four
// tap weights, no branch in the pixel loop), not a template value, so that no
// instance is added
// DOVI (h2s_set_dovi; LPX only): stage 1 is the Dolby Vision profile-5
// front-end on the frame's record (dovi_record), in double like the rest of
// the exact path; own instances, so that the others are what they were
template <int QPT, bool VEC, bool OUT8, bool C444 = false, bool DYN = false, bool LPX = false, int SUB = 0,
          bool DOVI = false>
__global__ __launch_bounds__(256) void k_process(const KParams P0) {
  static_assert(SUB == 0 || (!DYN && !LPX), "4:2:2 / 4:4:4 input: CPU chain, static peak");
  static_assert(!DOVI || (LPX && SUB == 0), "Dolby Vision: the libplacebo branch, 4:2:0 input");
  LpX X;
  auto body = [&](const KParams& P, const int f, const int cy, const int cx0) {
  const int cw = P.cw, ch = P.ch;
  const DoviRec* const rec = DOVI ? dovi_record(P, f) : nullptr;

  // ---- chroma: rows cy-1, cy, cy+1; columns cx0 .. cx0+QPT (halo) ----
  // (SUB 1: rows 2cy, 2cy+1 of the 4:2:2 plane, the same columns; SUB 2 below)
  constexpr int NR = SUB ? 2 : 3;
  float cu[3][QPT + 1], cv[3][QPT + 1];
  int ccu[3][QPT + 1], ccv[3][QPT + 1];
  const int crow[3] = {SUB ? 2 * cy : edge(P, cy - 1, ch), SUB ? 2 * cy + 1 : cy, edge(P, cy + 1, ch)};
  const bool full = cx0 + QPT <= cw;
#pragma unroll
  for (int i = 0; i < (SUB == 2 ? 0 : NR); i++) {
    const uint8_t* ru = P.in[1] + f * P.in_fp[1] + crow[i] * P.in_ls[1];
    const uint8_t* rv = P.in[2] + f * P.in_fp[2] + crow[i] * P.in_ls[2];
    if (VEC && full && QPT == 4) {
      const int hx = edge(P, cx0 + 4, cw);
      if (P.in_cstep == 2) {   // semi-planar: four (Cb, Cr) pairs in one 16-byte load
        // (the three 16-byte unpacks of this kernel are spelt out: through unpack16 the exact-path
        // instances compile to other code, profiles/peak_unit/build.md)
        const uint4 q = *reinterpret_cast<const uint4*>(ru + 4 * cx0);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++) ccu[i][k] = code_of(P, w[k] & 0xffff), ccv[i][k] = code_of(P, w[k] >> 16);
      } else {
        // (code_of: h2s_lp_p010 TRUNCATE drops the two low bits)
        unsigned su[4], sv[4];
        unpack16(*reinterpret_cast<const uint2*>(ru + 2 * cx0), su);
        unpack16(*reinterpret_cast<const uint2*>(rv + 2 * cx0), sv);
#pragma unroll
        for (int k = 0; k < 4; k++) ccu[i][k] = code_of(P, su[k]), ccv[i][k] = code_of(P, sv[k]);
      }
      ccu[i][4] = ldc(P, ru, hx), ccv[i][4] = ldc(P, rv, hx);
    } else {
#pragma unroll
      for (int k = 0; k <= QPT; k++) {
        const int x = edge(P, cx0 + k, cw);
        ccu[i][k] = ldc(P, ru, x);
        ccv[i][k] = ldc(P, rv, x);
      }
    }
#pragma unroll
    for (int k = 0; k <= QPT; k++) {
      cu[i][k] = (float)ccu[i][k] * P.c_scale + P.c_off;
      cv[i][k] = (float)ccv[i][k] * P.c_scale + P.c_off;
    }
  }
  // horizontal pass (left siting): h[2k] = c[k], h[2k+1] = (c[k] + c[k+1]) / 2
  float hu[3][2 * QPT], hv[3][2 * QPT];
#pragma unroll
  for (int i = 0; i < (SUB == 2 ? 0 : NR); i++)
#pragma unroll
    for (int k = 0; k < QPT; k++) {
      hu[i][2 * k] = cu[i][k];
      hu[i][2 * k + 1] = 0.5f * cu[i][k] + 0.5f * cu[i][k + 1];
      hv[i][2 * k] = cv[i][k];
      hv[i][2 * k + 1] = 0.5f * cv[i][k] + 0.5f * cv[i][k + 1];
    }

  // ---- luma: rows 2cy, 2cy+1; columns 2cx0 .. 2cx0+2QPT-1 ----
  const int x0 = 2 * cx0;
  if constexpr (SUB == 2) {   // 4:4:4: chroma rows 2cy, 2cy+1, the luma columns; no resampling
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const uint8_t* ru = P.in[1] + f * P.in_fp[1] + (2 * cy + j) * P.in_ls[1];
      const uint8_t* rv = P.in[2] + f * P.in_fp[2] + (2 * cy + j) * P.in_ls[2];
      int cu4[2 * QPT], cv4[2 * QPT];
      if (VEC && full && QPT == 4) {
        // (spelt out, not unpack16: see the semi-planar chroma load above)
        const uint4 a = *reinterpret_cast<const uint4*>(ru + 2 * x0), b = *reinterpret_cast<const uint4*>(rv + 2 * x0);
        const unsigned wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
          cu4[2 * k] = code_of(P, wa[k] & 0xffff), cu4[2 * k + 1] = code_of(P, wa[k] >> 16);
          cv4[2 * k] = code_of(P, wb[k] & 0xffff), cv4[2 * k + 1] = code_of(P, wb[k] >> 16);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 2 * QPT; k++) {
          const int x = x0 + k < P.W ? x0 + k : P.W - 1;
          cu4[k] = ldy(P, ru, x), cv4[k] = ldy(P, rv, x);
        }
      }
#pragma unroll
      for (int k = 0; k < 2 * QPT; k++) {
        hu[j][k] = (float)cu4[k] * P.c_scale + P.c_off;
        hv[j][k] = (float)cv4[k] * P.c_scale + P.c_off;
      }
    }
  }
  int ys[2][2 * QPT];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const uint8_t* ry = P.in[0] + f * P.in_fp[0] + (2 * cy + j) * P.in_ls[0];
    if (VEC && full && QPT == 4) {
      // (spelt out, not unpack16: see the semi-planar chroma load above)
      const uint4 a = *reinterpret_cast<const uint4*>(ry + 2 * x0);
      const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        ys[j][2 * k] = code_of(P, w[k] & 0xffff);
        ys[j][2 * k + 1] = code_of(P, w[k] >> 16);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 2 * QPT; k++) {
        const int x = x0 + k < P.W ? x0 + k : P.W - 1;
        ys[j][k] = ldy(P, ry, x);
      }
    }
  }

  // ---- per pixel chain, Y'CbCr, quantise ----
  int yo[2][2 * QPT], uo[QPT], vo[QPT];
  const float vw[4] = {P.vco ? 0.0f : 0.25f, P.vco ? 1.0f : 0.75f, P.vco ? 0.5f : 0.75f, P.vco ? 0.5f : 0.25f};
#pragma unroll
  for (int k = 0; k < QPT; k++) {
    float cbs[4], crs[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int j = p >> 1, x = 2 * k + (p & 1);
      // (SUB: no vertical pass; row j of the loaded pair is the pixel's own)
      // (the taps as launch-uniform weights, vw: centre siting 1/4, 3/4 | 3/4, 1/4; top-left 0, 1 | 1/2, 1/2,
      // where 0 x + 1 y is y exactly)
      const float cb = SUB ? hu[j][x] : j == 0 ? vw[0] * hu[0][x] + vw[1] * hu[1][x] : vw[2] * hu[1][x] + vw[3] * hu[2][x];
      const float cr = SUB ? hv[j][x] : j == 0 ? vw[0] * hv[0][x] + vw[1] * hv[1][x] : vw[2] * hv[1][x] + vw[3] * hv[2][x];
      const float yv = (float)ys[j][x] * P.y_scale + P.y_off;
      float r, g, b;
      const int px = 2 * (cx0 + k) + (p & 1), py = 2 * cy + j;
      if (LPX) {
        // the oracle's upsample_d: horizontal (left siting) then vertical, in double
        auto hx = [&](const int (&c)[3][QPT + 1], int i) -> double {
          const double a = lpx_chroma_of<DOVI>(P, c[i][x >> 1]);
          return (x & 1) ? 0.5 * (a + lpx_chroma_of<DOVI>(P, c[i][(x >> 1) + 1])) : a;
        };
        const double wd[4] = {vw[0], vw[1], vw[2], vw[3]};   // (exact in float)
        const double cbd = j == 0 ? wd[0] * hx(ccu, 0) + wd[1] * hx(ccu, 1) : wd[2] * hx(ccu, 1) + wd[3] * hx(ccu, 2);
        const double crd = j == 0 ? wd[0] * hx(ccv, 0) + wd[1] * hx(ccv, 1) : wd[2] * hx(ccv, 1) + wd[3] * hx(ccv, 2);
        lpx_chain<4, DOVI>(P, X, lpx_luma_of<DOVI>(P, ys[j][x]), cbd, crd, px, py, r, g, b, rec);
      } else {
        chain_px<4>(P, yv, cb, cr, r, g, b, lp_qoff(P, px, py));
      }
      r = clamp01(r), g = clamp01(g), b = clamp01(b);
      const float Y = P.k709[0] * r + P.k709[1] * g + P.k709[2] * b;
      cbs[p] = P.kcb[0] * r + P.kcb[1] * g + P.kcb[2] * b;
      crs[p] = P.kcr[0] * r + P.kcr[1] * g + P.kcr[2] * b;
      int yq = quant_o((16.0f + 219.0f * Y) * P.qscale, P.dither ? dither_off(px, py) : 0.5f, P.qmax);
      if (!P.eq_identity) yq = P.eq_lut[yq];
      yo[j][x] = expand_code(P, yq);
      if (C444 && px < P.W) P.chr444[(long long)py * P.W + px] = make_float2(cbs[p], crs[p]);
    }
    if (C444) continue;
    const float cb = ((cbs[0] + cbs[1]) + (cbs[2] + cbs[3])) * 0.25f;
    const float cr = ((crs[0] + crs[1]) + (crs[2] + crs[3])) * 0.25f;
    const float co = P.dither ? dither_off(cx0 + k, cy) : 0.5f;
    uo[k] = expand_code(P, quant_o((128.0f + 224.0f * cb) * P.qscale, co, P.qmax));
    vo[k] = expand_code(P, quant_o((128.0f + 224.0f * cr) * P.qscale, co, P.qmax));
  }

  // ---- stores ----
#pragma unroll
  for (int j = 0; j < 2; j++) {
    uint8_t* ry = P.out[0] + f * P.out_fp[0] + (2 * cy + j) * P.out_ls[0];
    if (VEC && full && QPT == 4) {
      if (OUT8) *reinterpret_cast<uint2*>(ry + x0) = pack_codes<true>(yo[j]);
      else *reinterpret_cast<uint4*>(ry + 2 * x0) = pack_codes<false>(yo[j]);
    } else {
#pragma unroll
      for (int k = 0; k < 2 * QPT; k++) {
        if (x0 + k < P.W) {
          if (OUT8) ry[x0 + k] = (uint8_t)yo[j][k];
          else reinterpret_cast<uint16_t*>(ry)[x0 + k] = (uint16_t)yo[j][k];
        }
      }
    }
  }
  if (C444) return;
  uint8_t* ru = P.out[1] + f * P.out_fp[1] + cy * P.out_ls[1];
  uint8_t* rv = P.out[2] + f * P.out_fp[2] + cy * P.out_ls[2];
  if (VEC && full && QPT == 4 && P.out_cstep == 2) {   // semi-planar: the four (Cb, Cr) pairs in one store
    const int uv[8] = {uo[0], vo[0], uo[1], vo[1], uo[2], vo[2], uo[3], vo[3]};
    if (OUT8) *reinterpret_cast<uint2*>(ru + 2 * cx0) = pack_codes<true>(uv);
    else *reinterpret_cast<uint4*>(ru + 4 * cx0) = pack_codes<false>(uv);
  } else if (VEC && full && QPT == 4) {
    if (OUT8) {
      *reinterpret_cast<unsigned*>(ru + cx0) = pack_codes<true>(uo);
      *reinterpret_cast<unsigned*>(rv + cx0) = pack_codes<true>(vo);
    } else {
      *reinterpret_cast<uint2*>(ru + 2 * cx0) = pack_codes<false>(uo);
      *reinterpret_cast<uint2*>(rv + 2 * cx0) = pack_codes<false>(vo);
    }
  } else {
#pragma unroll
    for (int k = 0; k < QPT; k++) {
      if (cx0 + k < cw) {
        const int xo = (cx0 + k) * P.out_cstep;
        if (OUT8) {
          ru[xo] = (uint8_t)uo[k];
          rv[xo] = (uint8_t)vo[k];
        } else {
          reinterpret_cast<uint16_t*>(ru)[xo] = (uint16_t)uo[k];
          reinterpret_cast<uint16_t*>(rv)[xo] = (uint16_t)vo[k];
        }
      }
    }
  }
  };
  // DYN (dynamic peak detection, one frame per launch): the frame's curve
  // constants come from the record the peak launches wrote on the device
  // (P0.cv), not from the launch parameters
  KParams P = P0;
  if (DYN) apply_curve(P, *P0.cv);
  if (LPX) X = lpx_consts(P, P.x_peak, P.x_avg);
  const long long lb = xcd_remap(blockIdx.x, gridDim.x);
  const long long item = lb * 256 + threadIdx.x;
  if (item >= P.total) return;
  const int gx = (int)(item % P.ngx);
  const long long t = item / P.ngx;
  body(P, (int)(t / P.ch), (int)(t % P.ch), (gx + P.gx0) * QPT);
}


// Debug/parity kernel: float RGB of frame 0 after stage STAGE, one thread per
// pixel, generic (unvectorised) sample access.
// DOVI: frame 0's Dolby Vision record (the libplacebo pipeline; own instances)
template <int STAGE, bool DOVI = false>
__global__ __launch_bounds__(256) void k_debug(const KParams P, float* out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long npx = (long long)P.W * P.H;
  if (i >= npx) return;
  const int x = (int)(i % P.W), y = (int)(i / P.W);
  const int cw = P.icw, ch = P.ich;   // (the input's chroma plane: 4:2:0 W/2 x H/2)
  auto hpass = [&](int plane, int cyy) -> float {
    const uint8_t* row = P.in[plane] + edge(P, cyy, ch) * P.in_ls[plane];
    if (P.sub == 2) return (float)ldc(P, row, x) * P.c_scale + P.c_off;   // 4:4:4: the pixel's own sample
    const int k = x >> 1;
    const float a = (float)ldc(P, row, edge(P, k, cw)) * P.c_scale + P.c_off;
    if (!(x & 1)) return a;
    const float b = (float)ldc(P, row, edge(P, k + 1, cw)) * P.c_scale + P.c_off;
    return 0.5f * a + 0.5f * b;
  };
  auto up = [&](int plane) -> float {
    if (P.sub) return hpass(plane, y);   // 4:2:2 / 4:4:4: chroma row y, no vertical pass
    const int m = y >> 1;
    if (P.vco) return !(y & 1) ? hpass(plane, m) : 0.5f * hpass(plane, m) + 0.5f * hpass(plane, m + 1);   // top-left
    if (!(y & 1)) return 0.25f * hpass(plane, m - 1) + 0.75f * hpass(plane, m);
    return 0.75f * hpass(plane, m) + 0.25f * hpass(plane, m + 1);
  };
  const float cb = up(1), cr = up(2);
  const int ycode = ldy(P, P.in[0] + y * P.in_ls[0], x);
  const float yv = (float)ycode * P.y_scale + P.y_off;
  float r, g, b;
  if (P.pipe == PIPE_LIBPLACEBO) {   // the exact path (h2s_lpx.h), as k_process<..., LPX>
    auto hpd = [&](int plane, int cyy) -> double {
      const uint8_t* row = P.in[plane] + edge(P, cyy, ch) * P.in_ls[plane];
      const int k = x >> 1;
      const double a = lpx_chroma_of<DOVI>(P, ldc(P, row, edge(P, k, cw)));
      if (!(x & 1)) return a;
      return 0.5 * (a + lpx_chroma_of<DOVI>(P, ldc(P, row, edge(P, k + 1, cw))));
    };
    auto upd = [&](int plane) -> double {
      const int m = y >> 1;
      if (P.vco) return !(y & 1) ? hpd(plane, m) : 0.5 * hpd(plane, m) + 0.5 * hpd(plane, m + 1);
      if (!(y & 1)) return 0.25 * hpd(plane, m - 1) + 0.75 * hpd(plane, m);
      return 0.75 * hpd(plane, m) + 0.25 * hpd(plane, m + 1);
    };
    const LpX X = lpx_consts(P, P.x_peak, P.x_avg);
    lpx_chain<STAGE < 5 ? STAGE : 4, DOVI>(P, X, lpx_luma_of<DOVI>(P, ycode), upd(1), upd(2), x, y, r, g, b,
                                           DOVI ? dovi_record(P, 0) : nullptr);
  } else {
    chain_px<STAGE < 5 ? STAGE : 4>(P, yv, cb, cr, r, g, b, lp_qoff(P, x, y));
  }
  if (STAGE == 5) {  // S6 quantiser inputs (oracle px_yuv)
    r = clamp01(r), g = clamp01(g), b = clamp01(b);
    const float Y = P.k709[0] * r + P.k709[1] * g + P.k709[2] * b;
    const float cbp = P.kcb[0] * r + P.kcb[1] * g + P.kcb[2] * b;
    const float crp = P.kcr[0] * r + P.kcr[1] * g + P.kcr[2] * b;
    r = (16.0f + 219.0f * Y) * P.qscale, g = 224.0f * P.qscale * cbp, b = 224.0f * P.qscale * crp;
  }
  out[i] = r;
  out[npx + i] = g;
  out[2 * npx + i] = b;
}

// BICUBIC chroma decimation (second pass): one thread per output chroma
// sample of one frame; separable taps (oracle process_frame_bicubic order:
// horizontal 7-tap sums per luma row, then the vertical 8-tap sum)
struct ChromaTaps {
  float wx[7], wy[8];
};

template <bool OUT8>
__global__ __launch_bounds__(256) void k_chroma_bicubic(const KParams P, const ChromaTaps T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P.cw * P.ch) return;
  const int k = i % P.cw, m = i / P.cw;
  float su = 0.0f, sv = 0.0f;
  for (int j = 0; j < 8; j++) {
    const int y = min(max(2 * m - 3 + j, 0), P.H - 1);
    const float2* row = P.chr444 + (long long)y * P.W;
    float hu = 0.0f, hv = 0.0f;
#pragma unroll
    for (int t = 0; t < 7; t++) {
      const float2 c = row[min(max(2 * k - 3 + t, 0), P.W - 1)];
      hu += T.wx[t] * c.x;
      hv += T.wx[t] * c.y;
    }
    su += T.wy[j] * hu;
    sv += T.wy[j] * hv;
  }
  const float co = P.dither ? dither_off(k, m) : 0.5f;
  const int u = expand_code(P, quant_o((128.0f + 224.0f * su) * P.qscale, co, P.qmax));
  const int v = expand_code(P, quant_o((128.0f + 224.0f * sv) * P.qscale, co, P.qmax));
  uint8_t* ru = P.out[1] + m * P.out_ls[1];
  uint8_t* rv = P.out[2] + m * P.out_ls[2];
  const int xo = k * P.out_cstep;   // (semi-planar: plane 2 aliases plane 1 one sample on)
  if (OUT8) {
    ru[xo] = (uint8_t)u, rv[xo] = (uint8_t)v;
  } else {
    reinterpret_cast<uint16_t*>(ru)[xo] = (uint16_t)u;
    reinterpret_cast<uint16_t*>(rv)[xo] = (uint16_t)v;
  }
}

// ---- host-side launchers (declared in h2s_launch.h) ---------------------

// k_process's instance for the launch, one runtime flag per step into the
// template arguments (VEC, OUT8, C444, DYN, LPX)
// (SUB first: the input's chroma subsampling, launch_process)
template <int SUB, bool VEC, bool OUT8, bool C444, bool DYN, bool LPX, bool DOVI>
static void launch_k(const KParams& P, dim3 grid, hipStream_t s) {
  // no such instances: launch_process clears VEC for them, and refuses SUB with DYN / LPX
  // and Dolby Vision records off the libplacebo branch or with SUB
  if constexpr (!(VEC && (C444 || DYN)) && !(SUB && (DYN || LPX)) && !(DOVI && (!LPX || SUB)))
    hipLaunchKernelGGL((k_process<4, VEC, OUT8, C444, DYN, LPX, SUB, DOVI>), grid, dim3(256), 0, s, P);
}
template <int SUB, bool... B, class... Flags>
static void launch_k(const KParams& P, dim3 grid, hipStream_t s, bool flag, Flags... rest) {
  flag ? launch_k<SUB, B..., true>(P, grid, s, rest...) : launch_k<SUB, B..., false>(P, grid, s, rest...);
}

// the generic kernel over the launch's column groups (P.gx0, P.ngx).  form
// (enum ProcessForm, h2s_launch.h): PF_VEC the rows allow vector accesses,
// PF_OUT8 8-bit output, PF_C444 BICUBIC chroma pass 1 (luma + per-pixel chroma
// into P.chr444).  P.cv: dynamic peak, the frame's curve record on the device;
// the libplacebo branch runs its exact path (h2s_lpx.h).  Dynamic-peak and
// C444 launches are never VEC
hipError_t launch_process(const KParams& P, unsigned form, hipStream_t s) {
  const long long nb = (P.total + 255) / 256;
  if (nb == 0) return hipSuccess;
  const bool c444 = form & PF_C444, dyn = P.cv != nullptr, lpx = P.pipe == PIPE_LIBPLACEBO;
  const bool vec = (form & PF_VEC) && !c444 && !dyn, out8 = (form & PF_OUT8) != 0;
  // 4:2:2 / 4:4:4 input: CPU chain, static peak (h2s_api.hip check_subsampling refuses the rest)
  if (P.sub && (dyn || lpx || P.sub > 2 || P.in_cstep != 1)) return hipErrorInvalidValue;
  // Dolby Vision records: the libplacebo branch, 4:2:0 input (h2s_api.hip check_dovi refuses the rest)
  const bool dovi = P.dovi != nullptr;
  if (dovi && (!lpx || P.sub || P.vco)) return hipErrorInvalidValue;
  if (P.sub == 1) launch_k<1>(P, dim3((unsigned)nb), s, vec, out8, c444, dyn, lpx, false);
  else if (P.sub == 2) launch_k<2>(P, dim3((unsigned)nb), s, vec, out8, c444, dyn, lpx, false);
  else launch_k<0>(P, dim3((unsigned)nb), s, vec, out8, c444, dyn, lpx, dovi);
  return hipGetLastError();
}

template <bool DOVI>
static hipError_t launch_debug_stage(const KParams& P, int stage, float* out, hipStream_t s) {
  const long long npx = (long long)P.W * P.H;
  dim3 grid((unsigned)((npx + 255) / 256)), block(256);
  switch (stage) {
    case 1: hipLaunchKernelGGL((k_debug<1, DOVI>), grid, block, 0, s, P, out); break;
    case 2: hipLaunchKernelGGL((k_debug<2, DOVI>), grid, block, 0, s, P, out); break;
    case 3: hipLaunchKernelGGL((k_debug<3, DOVI>), grid, block, 0, s, P, out); break;
    case 4: hipLaunchKernelGGL((k_debug<4, DOVI>), grid, block, 0, s, P, out); break;
    default: hipLaunchKernelGGL((k_debug<5, DOVI>), grid, block, 0, s, P, out); break;
  }
  return hipGetLastError();
}

hipError_t launch_debug(const KParams& P, int stage, float* out, hipStream_t s) {
  // frame 0's Dolby Vision record (libplacebo pipeline only: check_dovi)
  if (P.dovi && (P.pipe != PIPE_LIBPLACEBO || P.sub || P.vco)) return hipErrorInvalidValue;
  return P.dovi ? launch_debug_stage<true>(P, stage, out, s) : launch_debug_stage<false>(P, stage, out, s);
}

// BICUBIC chroma, pass 2: the decimation of one frame's chr444
hipError_t launch_chroma_bicubic(const KParams& P, const float* wx7, const float* wy8, bool out8, hipStream_t s) {
  ChromaTaps T;
  for (int i = 0; i < 7; i++) T.wx[i] = wx7[i];
  for (int j = 0; j < 8; j++) T.wy[j] = wy8[j];
  const unsigned nc = (unsigned)(((long long)P.cw * P.ch + 255) / 256);
  if (out8) hipLaunchKernelGGL((k_chroma_bicubic<true>), dim3(nc), dim3(256), 0, s, P, T);
  else hipLaunchKernelGGL((k_chroma_bicubic<false>), dim3(nc), dim3(256), 0, s, P, T);
  return hipGetLastError();
}

// The libplacebo branch's lut3d 8-bit table for the tile kernel: for every
// rgba8 code triple (r, g, b), lut3d's 8-bit output -- coordinate (q / 255)
// (N-1), tetrahedral blend, truncation -- in this translation unit's
// arithmetic (no FMA contraction: the oracle's lut3d_8bit order, as
// chain_px / lpx_chain), packed R | G << 8 | B << 16.  2^24 entries, 64 MiB;
// built once per lattice (h2s_api.hip ensure_lut8x)
// The entries are in bit-interleaved (Morton) order -- index bit 3k = r bit
// k, 3k+1 = g bit k, 3k+2 = b bit k -- so that a 128-byte line holds a 4 x 4
// x 2 block of codes (the order r | g << 8 | b << 16 measured up to 42 %
// slower on smooth content: profiles/r06/lp_table/, patch in
// profiles/r06/ab_patches/lp_tab_linear.patch)
__global__ __launch_bounds__(256) void k_build_lut8x(const KParams P, unsigned* out) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  unsigned cr = 0, cg = 0, cb = 0;
  for (int k = 0; k < 8; k++) {
    cr |= ((i >> (3 * k)) & 1u) << k;
    cg |= ((i >> (3 * k + 1)) & 1u) << k;
    cb |= ((i >> (3 * k + 2)) & 1u) << k;
  }
  const float sf = 1.0f / 255.0f;
  float r = (float)cr * sf, g = (float)cg * sf, b = (float)cb * sf;
  lut3d_tetra(P, r, g, b);
  const unsigned R = (unsigned)fminf(fmaxf(truncf(r * 255.0f), 0.0f), 255.0f);
  const unsigned G = (unsigned)fminf(fmaxf(truncf(g * 255.0f), 0.0f), 255.0f);
  const unsigned B = (unsigned)fminf(fmaxf(truncf(b * 255.0f), 0.0f), 255.0f);
  out[i] = R | (G << 8) | (B << 16);
}

hipError_t build_lut8x(const float4* lut, int n, unsigned* out, hipStream_t s) {
  KParams P{};
  P.lut = lut, P.lut_n = n, P.lut_sg = n, P.lut_sb = n * n, P.lut_max = (float)(n - 1);
  hipLaunchKernelGGL(k_build_lut8x, dim3((1u << 24) / 256), dim3(256), 0, s, P, out);
  return hipGetLastError();
}
}  // namespace h2s
