// h2s_peak.hip — the dynamic peak's device side (params.peak_detect; types:
// h2s_peak.h, host side: h2s_api_peak.hip), built without FMA contraction.
// Per frame, the maximum and the sum of the PQ-encoded max(R,G,B) of every
// pixel (libplacebo peak detection, src/utils.py:448; PARITY UNPINNED: no
// libplacebo here, model in DESIGN.md).  PQ sources: PQ(max(EOTF(E))) ==
// clamp(max(E), 0, 1) exactly, so no transcendental is needed.  Chroma is taken nearest.
// grid = (M.nblocks, frames); partial[f * M.nblocks + b] = (max, sum) over block b's rows / chunks
#include "h2s_chain.h"
#include "h2s_dovi.h"
#include "h2s_launch.h"
#include "h2s_peak.h"

namespace h2s {

// one pixel's PQ-domain max(R,G,B) from its integer codes (nearest chroma)
// TRC 2: a Dolby Vision profile-5 frame (R: its record, h2s_set_dovi): the
// front-end's linear BT.2020 light (h2s_dovi.h, float32; 1 = 10000 nits),
// PQ-encoded; no shortcut, since max(Lm lms) is not the largest L'M'S'
// DoviStat: what a block's pixels share (hoisted out of the row loop by
// k_peak_stats: block-uniform): 1 / (2^b - 1) and the record's linear matrix
struct DoviStat {
  float inv, lin[9];
};
template <int TRC>
__device__ __forceinline__ float peak_px(const KParams& P, unsigned yc, unsigned uc, unsigned vc,
                                         const DoviRec* R = nullptr, const DoviStat* S = nullptr) {
  yc = (yc >> P.in_sh) & P.in_mask, uc = (uc >> P.in_sh) & P.in_mask, vc = (vc >> P.in_sh) & P.in_mask;   // code_of
  if constexpr (TRC == 2) {
    // (model step 1's clamp to [0, 1] is no operation here: in_mask bounds every code by 2^b - 1)
    const float sv[3] = {(float)yc * S->inv, (float)uc * S->inv, (float)vc * S->inv};
    float v[3];
    dovi_lms_pq<float>(*R, sv, v);
    const float l[3] = {pq_eotf(v[0]), pq_eotf(v[1]), pq_eotf(v[2])};
    const float r = S->lin[0] * l[0] + S->lin[1] * l[1] + S->lin[2] * l[2];
    const float g = S->lin[3] * l[0] + S->lin[4] * l[1] + S->lin[5] * l[2];
    const float bl = S->lin[6] * l[0] + S->lin[7] * l[1] + S->lin[8] * l[2];
    // the linear matrix may leave every channel negative: such a pixel counts as black (PQ(0), as
    // pq_encode's own max(y, 0) would give; stated here rather than left to it)
    return clamp01(pq_encode(fmaxf(fmaxf(fmaxf(r, g), bl), 0.0f)));
  }
  const float Y = (float)yc * P.y_scale + P.y_off;
  const float cb = (float)uc * P.c_scale + P.c_off, cr = (float)vc * P.c_scale + P.c_off;
  const float er = Y + P.m_rcr * cr, eg = Y + P.m_gcb * cb + P.m_gcr * cr, eb = Y + P.m_bcb * cb;
  if (TRC == 0) return clamp01(fmaxf(fmaxf(er, eg), eb));
  const float r = hlg_inv_oetf(er), g = hlg_inv_oetf(eg), bl = hlg_inv_oetf(eb);
  const float ys = 0.2627f * r + 0.6780f * g + 0.0593f * bl;
  const float w = ys > 0.0f ? P.lin_scale * apow(ys, 0.2f) : 0.0f;
  return clamp01(pq_encode(fmaxf(fmaxf(r, g), bl) * w * P.npl_1e4));
}

// percentile model (pd_percentile < 100; PARITY UNPINNED): a PEAK_BINS-bin histogram of the
// per-pixel PQ(max R,G,B) per frame; the percentile is interpolated inside its bin by peak_frame_fold
// a thread's run of equal bins, added to the LDS histogram once per run: on
// smooth content neighbouring pixels share a bin, and one LDS atomic per pixel
// had all 64 lanes of a wave serialise on one address
struct HistRun {
  int bin = -1;
  unsigned n = 0;
  __device__ __forceinline__ void add(unsigned* lh, float m) {
    const int b = min((int)(m * (float)PEAK_BINS), PEAK_BINS - 1);
    if (b != bin) {
      if (n) atomicAdd(&lh[bin], n);
      bin = b, n = 0;
    }
    n++;
  }
  // n values of bin b (a whole quad-form unit in one step)
  __device__ __forceinline__ void add_n(unsigned* lh, int b, unsigned k) {
    if (b != bin) {
      if (n) atomicAdd(&lh[bin], n);
      bin = b, n = 0;
    }
    n += k;
  }
  __device__ __forceinline__ void flush(unsigned* lh) {
    if (n) atomicAdd(&lh[bin], n);
    n = 0;
  }
};
__device__ __forceinline__ void hist_flush(const unsigned* lh, unsigned* hist) {
  __syncthreads();
  for (int i = threadIdx.x; i < PEAK_BINS; i += 256)
    if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

// block (max, sum) reduction; thread 0 writes the record
__device__ __forceinline__ void peak_reduce(float mx, float sm, float2* out) {
  __shared__ float smx[256], ssm[256];
  smx[threadIdx.x] = mx, ssm[threadIdx.x] = sm;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
      ssm[threadIdx.x] += ssm[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = make_float2(smx[0], ssm[0]);
}

// ---- per-frame statistic and curve records on the device ----
// One frame's (PQ peak measurement, average PQ) from its nblocks partial
// (max, sum) records and, for pd_percentile < 100, the percentile from the
// frame's histogram: the first bin whose cumulative count reaches pct % of
// the pixels, interpolated linearly inside it, capped at the frame maximum
// (oracle_peak_stats).  Wave-level reductions and scans: the records fold in a
// fixed pairwise order in double (so sharded and sequential statistics stay
// bit-identical), the counts are integers (a u32 scan equals a serial
// accumulation).  The histogram is left zeroed for the next call.  256 threads.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ void peak_frame_fold(const float2* partial, unsigned* hist, const PeakModel& M, double2* fstat, int f) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  __shared__ double s_sum[4];
  __shared__ float s_mx[4];
  __shared__ unsigned s_wtot[4];
  __shared__ int s_bin;
  static_assert(PEAK_BLOCKS_MAX <= 256, "one partial record per thread");
  const float2 rec = t < M.nblocks ? partial[(size_t)f * M.nblocks + t] : make_float2(0.0f, 0.0f);
  const double ws = wave_sum_d((double)rec.y);
  const float wm = wave_max_f(rec.x);
  if (lane == 0) s_sum[w] = ws, s_mx[w] = wm;
  if (t == 0) s_bin = PEAK_BINS;
  unsigned cnt[4] = {0u, 0u, 0u, 0u}, incl = 0u;
  if (M.pct) {
    static_assert(PEAK_BINS == 4 * 256, "four bins per thread");
    uint4* h = reinterpret_cast<uint4*>(hist + (size_t)f * PEAK_BINS);
    const uint4 c = h[t];
    h[t] = make_uint4(0u, 0u, 0u, 0u);
    cnt[0] = c.x, cnt[1] = c.y, cnt[2] = c.z, cnt[3] = c.w;
    incl = c.x + c.y + c.z + c.w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {   // inclusive scan within the wave
      const unsigned v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) s_wtot[w] = incl;
  }
  __syncthreads();
  const double sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
  const double mx = (double)fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
  if (M.pct) {
    unsigned before = 0u, n = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      before += k < w ? s_wtot[k] : 0u;
      n += s_wtot[k];
    }
    const double target = M.percentile / 100.0 * (double)n;
    double cum = (double)(before + incl - (cnt[0] + cnt[1] + cnt[2] + cnt[3]));
    int mine = PEAK_BINS;
    double cum_at = 0.0;
    for (int k = 0; k < 4; k++) {
      if (mine == PEAK_BINS && cnt[k] && cum + cnt[k] >= target) mine = 4 * t + k, cum_at = cum;
      cum += cnt[k];
    }
    if (mine < PEAK_BINS) atomicMin(&s_bin, mine);
    __syncthreads();
    if (mine < PEAK_BINS && mine == s_bin) {   // the owner of the first bin
      const double v = (mine + (target - cum_at) / cnt[mine & 3]) / PEAK_BINS;
      fstat[f] = make_double2(v < mx ? v : mx, sum / M.npx);
    } else if (t == 0 && s_bin == PEAK_BINS) {
      fstat[f] = make_double2(mx, sum / M.npx);
    }
  } else if (t == 0) {
    fstat[f] = make_double2(mx, sum / M.npx);
  }
}

// The IIR over n frames in order (thread 0, from the state the previous calls
// left in *st), then each frame's peak and curve record in parallel.
// out = null: the state only.  Every thread of the block calls it.  The
// frames' statistics are staged through LDS, PEAK_IIR_CHUNK at a time, so
// the serial recurrence makes no global round trip per frame
constexpr int PEAK_IIR_CHUNK = 1024;
__device__ void peak_curves_body(double2* fstat, int n, const PeakModel& M, PeakState* st, CurveConsts* out) {
  const int t = threadIdx.x;
  __shared__ double2 s_f[PEAK_IIR_CHUNK];
  __shared__ PeakState s_st;
  if (t == 0) s_st = *st;
  for (int c0 = 0; c0 < n; c0 += PEAK_IIR_CHUNK) {
    const int cn = n - c0 < PEAK_IIR_CHUNK ? n - c0 : PEAK_IIR_CHUNK;
    __syncthreads();
    for (int f = t; f < cn; f += blockDim.x) s_f[f] = fstat[c0 + f];
    __syncthreads();
    if (t == 0) {
      PeakState s = s_st;
      for (int f = 0; f < cn; f++) {
        peak_iir_step(&s, M, s_f[f].x, s_f[f].y);
        s_f[f] = make_double2(s.max, s.avg);   // the smoothed values frame f's curve uses
      }
      s_st = s;
    }
    __syncthreads();
    for (int f = t; f < cn; f += blockDim.x) {
      fstat[c0 + f] = s_f[f];
      const double pk = peak_of(M, s_f[f].x);
      if (c0 + f == n - 1) s_st.peak = pk;    // the state's peak: the last frame's (its smoothed max)
      if (out) curve_for_peak(M, pk, s_f[f].y, &out[c0 + f]);
    }
  }
  __syncthreads();
  if (t == 0) *st = s_st;
}

// k_peak_finish: one block per frame folds that frame's records (and clears
// its histogram for the next call); the last frame to finish (a device-scope
// counter after a release fence: one per frame, so the fences stay few) runs
// the IIR and the curve records for all of the launch's frames.  PeakTail
// names the buffers; the counter is zeroed by the statistics launch queued
// before every finish launch (an aborted launch cannot leave it stale) and left zero.
__global__ __launch_bounds__(256) void k_peak_finish(const float2* partial, const PeakTail T) {
  const int f = blockIdx.x;
  __shared__ int s_last;
  peak_frame_fold(partial, T.hist, T.M, T.fstat, f);
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();   // fstat[f] and the cleared histogram, device-wide
    s_last = atomicAdd(T.done, 1u) == (unsigned)T.nframes - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  if (threadIdx.x == 0) *T.done = 0u;
  if (T.st) peak_curves_body(T.fstat, T.nframes, T.M, T.st, T.out);
}

// ---- the statistics kernels: three forms of one pass.  Each first zeroes
// k_peak_finish's counter (stream-ordered) and, HIST, its LDS histogram.  The
// streaming forms issue PEAK_INFLIGHT (quad: 2) units' loads before folding the
// first, unit by unit ("sharded = sequential, bit for bit" rests on that order);
// shared helpers for more than hist_clear compiled to other code (profiles/peak_unit/build.md)
constexpr int PEAK_INFLIGHT = 4;   // (against 2 and 8: profiles/r05/peak_inflight.log)
template <bool HIST>
__device__ __forceinline__ void hist_clear(unsigned* lh) {
  if (HIST)
    for (int i = threadIdx.x; i < PEAK_BINS; i += 256) lh[i] = 0;
  if (HIST) __syncthreads();
}

// row form: any width / alignment, 2-byte loads
template <int TRC, bool HIST>
__global__ __launch_bounds__(256) void k_peak_stats(const KParams P, float2* partial, const PeakTail T) {
  __shared__ unsigned lh[HIST ? PEAK_BINS : 1];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *T.done = 0u;
  hist_clear<HIST>(lh);
  const int f = blockIdx.y, b = blockIdx.x;
  const DoviRec* const rec = TRC == 2 ? dovi_record(P, f) : nullptr;   // (block-uniform: one frame per block)
  DoviStat ds;
  if constexpr (TRC == 2) {
    ds.inv = 1.0f / (float)((256 << P.x_sh) - 1);
    for (int i = 0; i < 9; i++) ds.lin[i] = rec->lin[i];
  }
  float mx = 0.0f, sm = 0.0f;
  HistRun run;
  for (int y = b; y < P.H; y += gridDim.x) {
    const uint16_t* yr = reinterpret_cast<const uint16_t*>(P.in[0] + f * P.in_fp[0] + y * P.in_ls[0]);
    const uint16_t* ur = reinterpret_cast<const uint16_t*>(P.in[1] + f * P.in_fp[1] + (y >> 1) * P.in_ls[1]);
    const uint16_t* vr = reinterpret_cast<const uint16_t*>(P.in[2] + f * P.in_fp[2] + (y >> 1) * P.in_ls[2]);
    float rs = 0.0f;
    for (int x = threadIdx.x; x < P.W; x += blockDim.x) {
      const int xc = (x >> 1) * P.in_cstep;   // (semi-planar: vr = ur + 1, pairs two words apart)
      const float m = peak_px<TRC>(P, yr[x], ur[xc], vr[xc], rec, &ds);
      mx = fmaxf(mx, m);
      rs += m;
      if (HIST) run.add(lh, m);
    }
    sm += rs;
  }
  if (HIST) run.flush(lh);
  if (HIST) hist_flush(lh, T.hist + (size_t)f * PEAK_BINS);
  peak_reduce(mx, sm, &partial[f * gridDim.x + b]);
}

// row-chunk form (W % 8 == 0, 16-byte luma / 8-byte chroma alignment): each
// thread takes 8-pixel row chunks (one 16-byte luma load, one 8-byte load per
// chroma plane), four chunks' loads in flight.  The form for HLG input, and
// for PQ input whose rows the quad form below cannot take
template <int TRC, bool HIST>
__global__ __launch_bounds__(256) void k_peak_stats_v(const KParams P, float2* partial, const PeakTail T) {
  __shared__ unsigned lh[HIST ? PEAK_BINS : 1];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *T.done = 0u;
  hist_clear<HIST>(lh);
  const int f = blockIdx.y;
  const int cpr = P.W >> 3;                       // chunks per row
  const int nch = P.H * cpr, stride = gridDim.x * 256;
  const uint8_t* y0 = P.in[0] + f * P.in_fp[0];
  const uint8_t* u0 = P.in[1] + f * P.in_fp[1];
  const uint8_t* v0 = P.in[2] + f * P.in_fp[2];
  float mx = 0.0f, sm = 0.0f;
  HistRun run;
  struct Chunk {
    uint4 ya;
    uint2 ua, va;
  };
  auto load = [&](int i, Chunk& c) {
    const int r = i / cpr, cx = i - r * cpr;
    c.ya = reinterpret_cast<const uint4*>(y0 + r * P.in_ls[0])[cx];
    if (P.in_cstep == 2) {   // semi-planar: the chunk's four (Cb, Cr) pairs, 16 bytes of plane 1
      const uint2* q = reinterpret_cast<const uint2*>(u0 + (r >> 1) * P.in_ls[1]) + 2 * cx;
      c.ua = q[0], c.va = q[1];
    } else {
      c.ua = reinterpret_cast<const uint2*>(u0 + (r >> 1) * P.in_ls[1])[cx];
      c.va = reinterpret_cast<const uint2*>(v0 + (r >> 1) * P.in_ls[2])[cx];
    }
  };
  auto fold = [&](const Chunk& c) {
    unsigned uu[4], vv[4], yy[8];
    unpack16(c.ua, uu), unpack16(c.va, vv), unpack16(c.ya, yy);
    if (P.in_cstep == 2) {   // pairs: word k = (Cb k, Cr k)
      const unsigned p[8] = {uu[0], uu[1], uu[2], uu[3], vv[0], vv[1], vv[2], vv[3]};
#pragma unroll
      for (int k = 0; k < 4; k++) uu[k] = p[2 * k], vv[k] = p[2 * k + 1];
    }
    float rs = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const float m = peak_px<TRC>(P, yy[k], uu[k >> 1], vv[k >> 1]);
      mx = fmaxf(mx, m);
      rs += m;
      if (HIST) run.add(lh, m);
    }
    sm += rs;
  };
  int i = blockIdx.x * 256 + threadIdx.x;
  for (; i + (PEAK_INFLIGHT - 1) * stride < nch; i += PEAK_INFLIGHT * stride) {
    Chunk c[PEAK_INFLIGHT];
#pragma unroll
    for (int k = 0; k < PEAK_INFLIGHT; k++) load(i + k * stride, c[k]);
#pragma unroll
    for (int k = 0; k < PEAK_INFLIGHT; k++) fold(c[k]);
  }
  for (; i < nch; i += stride) {
    Chunk c;
    load(i, c);
    fold(c);
  }
  if (HIST) run.flush(lh);
  if (HIST) hist_flush(lh, T.hist + (size_t)f * PEAK_BINS);
  peak_reduce(mx, sm, &partial[f * gridDim.x + blockIdx.x]);
}

// quad form, the default for PQ input (W % 16 == 0, 16-byte rows; VERDICT
// r05 item 4): a thread's unit is 32 pixels -- 16 columns of a luma row pair
// and their 8 chroma samples -- read as six 16-byte loads (no chroma row read
// twice), two units' loads in flight.  PQ(max EOTF(R'G'B')) = clamp(max E):
// the chroma terms are maximised once per chroma sample (with Y's offset:
// d = y_off + max(a_rv v, a_gu u + a_gv v, a_bu u)) and each pixel is one FMA
// clamped to [0, 1] (E = code ys + d).  The histogram (pd_percentile < 100)
// takes a whole unit in one run step when the unit's smallest and largest
// values share a bin (bin() is monotonic); a unit that spans bins (most do on
// the bench content) adds each value with its own LDS atomic,
// the bin index floor(1024 m) unclamped into a 1025th entry (m = 1 exactly)
// folded into the last bin before the flush.  Every sum runs in a fixed
// order within the frame (unit by unit, 32 pixels row by row), so sharded
// and sequential statistics stay bit-identical.
template <bool HIST>
__global__ __launch_bounds__(256) void k_peak_stats_q(const KParams P, float2* partial, const PeakTail T) {
  __shared__ unsigned lh[HIST ? PEAK_BINS + 1 : 1];   // + the bin of m = 1 exactly, folded into the last at the end
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *T.done = 0u;
  if (HIST)
    for (int i = threadIdx.x; i <= PEAK_BINS; i += 256) lh[i] = 0;
  if (HIST) __syncthreads();
  const int f = blockIdx.y;
  const int cpr = P.W >> 4, nch = (P.H >> 1) * cpr, stride = gridDim.x * 256;
  const uint8_t* y0 = P.in[0] + f * P.in_fp[0];
  const uint8_t* u0 = P.in[1] + f * P.in_fp[1];
  const uint8_t* v0 = P.in[2] + f * P.in_fp[2];
  const unsigned m2 = P.in_mask | (P.in_mask << 16);
  const int sh = P.in_sh;   // semi-planar: codes in the words' high bits (m2 clears what crosses the halves)
  const float ys = P.y_scale, yo = P.y_off, cs = P.c_scale, co = P.c_off;
  float mx = 0.0f, sm = 0.0f;
  HistRun run;
  struct Unit {
    uint4 u, v, y0a, y0b, y1a, y1b;
  };
  auto load = [&](int i, Unit& q) {
    const int r = i / cpr, cx = i - r * cpr;
    if (P.in_cstep == 2) {   // semi-planar: the unit's eight (Cb, Cr) pairs, 32 bytes of plane 1
      q.u = *reinterpret_cast<const uint4*>(u0 + r * P.in_ls[1] + 32 * cx);
      q.v = *reinterpret_cast<const uint4*>(u0 + r * P.in_ls[1] + 32 * cx + 16);
    } else {
      q.u = *reinterpret_cast<const uint4*>(u0 + r * P.in_ls[1] + 16 * cx);
      q.v = *reinterpret_cast<const uint4*>(v0 + r * P.in_ls[2] + 16 * cx);
    }
    const uint4* ya = reinterpret_cast<const uint4*>(y0 + 2 * r * P.in_ls[0] + 32 * cx);
    const uint4* yb = reinterpret_cast<const uint4*>(y0 + (2 * r + 1) * P.in_ls[0] + 32 * cx);
    q.y0a = ya[0], q.y0b = ya[1], q.y1a = yb[0], q.y1b = yb[1];
  };
  // the 32 values of a unit, in order, to fn(m)
  auto each = [&](const Unit& q, const float (&d)[8], auto&& fn) {
    const uint4 rows[4] = {q.y0a, q.y0b, q.y1a, q.y1b};
#pragma unroll
    for (int h = 0; h < 4; h++) {
      const unsigned w[4] = {(rows[h].x >> sh) & m2, (rows[h].y >> sh) & m2, (rows[h].z >> sh) & m2, (rows[h].w >> sh) & m2};
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const unsigned code = (k & 1) ? w[k >> 1] >> 16 : w[k >> 1] & 0xffffu;
        fn(__builtin_amdgcn_fmed3f(fmaf((float)code, ys, d[4 * (h & 1) + (k >> 1)]), 0.0f, 1.0f));
      }
    }
  };
  auto fold = [&](const Unit& q) {
    unsigned ua[4] = {(q.u.x >> sh) & m2, (q.u.y >> sh) & m2, (q.u.z >> sh) & m2, (q.u.w >> sh) & m2};
    unsigned va[4] = {(q.v.x >> sh) & m2, (q.v.y >> sh) & m2, (q.v.z >> sh) & m2, (q.v.w >> sh) & m2};
    if (P.in_cstep == 2) {   // pairs (word k = Cb k | Cr k << 16) -> the planar words (block-uniform)
      const unsigned p[8] = {ua[0], ua[1], ua[2], ua[3], va[0], va[1], va[2], va[3]};
#pragma unroll
      for (int i = 0; i < 4; i++) {
        ua[i] = (p[2 * i] & 0xffffu) | (p[2 * i + 1] << 16);
        va[i] = (p[2 * i] >> 16) | (p[2 * i + 1] & 0xffff0000u);
      }
    }
    float d[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float cb = fmaf((float)((j & 1) ? ua[j >> 1] >> 16 : ua[j >> 1] & 0xffffu), cs, co);
      const float cr = fmaf((float)((j & 1) ? va[j >> 1] >> 16 : va[j >> 1] & 0xffffu), cs, co);
      d[j] = yo + fmaxf(fmaxf(P.m_rcr * cr, fmaf(P.m_gcb, cb, P.m_gcr * cr)), P.m_bcb * cb);
    }
    float rs = 0.0f, umx = 0.0f, umn = 1.0f;
    each(q, d, [&](float m) {
      umx = fmaxf(umx, m);
      umn = fminf(umn, m);
      rs += m;
    });
    mx = fmaxf(mx, umx);
    sm += rs;
    if (HIST) {
      const int b0 = min((int)(umn * (float)PEAK_BINS), PEAK_BINS - 1);
      const int b1 = min((int)(umx * (float)PEAK_BINS), PEAK_BINS - 1);
      if (b0 == b1) {
        run.add_n(lh, b0, 32u);
      } else {
        each(q, d, [&](float m) { atomicAdd(&lh[(unsigned)(m * (float)PEAK_BINS)], 1u); });
      }
    }
  };
  int i = blockIdx.x * 256 + threadIdx.x;
  for (; i + (2 - 1) * stride < nch; i += 2 * stride) {
    Unit q[2];
#pragma unroll
    for (int k = 0; k < 2; k++) load(i + k * stride, q[k]);
#pragma unroll
    for (int k = 0; k < 2; k++) fold(q[k]);
  }
  for (; i < nch; i += stride) {
    Unit q;
    load(i, q);
    fold(q);
  }
  if (HIST) {
    run.flush(lh);
    __syncthreads();
    if (threadIdx.x == 0) lh[PEAK_BINS - 1] += lh[PEAK_BINS];
    hist_flush(lh, T.hist + (size_t)f * PEAK_BINS);
  }
  peak_reduce(mx, sm, &partial[f * gridDim.x + blockIdx.x]);
}

// the statistics kernel of a launch (a Dolby Vision set: the row form, whatever the rows allow)
template <bool HIST>
static auto peak_stats_kernel(bool dovi, bool quad, bool vec, int transfer) -> void (*)(const KParams, float2*, const PeakTail) {
  if (dovi) return k_peak_stats<2, HIST>;
  if (quad) return k_peak_stats_q<HIST>;
  if (vec) return transfer == 1 ? k_peak_stats_v<1, HIST> : k_peak_stats_v<0, HIST>;
  return transfer == 1 ? k_peak_stats<1, HIST> : k_peak_stats<0, HIST>;
}

// the statistics of P's frames, then (k_peak_finish) their (measurement, average)
// in T.fstat and, T.st set, the smoothed state and curve records: two launches
hipError_t launch_peak_stats(const KParams& P, float2* partial, const PeakTail& T, hipStream_t s) {
  if (P.nframes <= 0) return hipSuccess;
  const dim3 grid(T.M.nblocks, P.nframes);
  auto al = [](long long v, int a) { return (v & (a - 1)) == 0; };
  // (semi-planar: plane 2 is plane 1 one sample on, and is not loaded from)
  auto planes_al = [&](int ya, int ca) {
    return al((long long)(uintptr_t)P.in[0], ya) && al(P.in_ls[0], ya) && al(P.in_fp[0], ya) &&
           al((long long)(uintptr_t)P.in[1], ca) && al(P.in_ls[1], ca) && al(P.in_fp[1], ca) &&
           (P.in_cstep == 2 ||
            (al((long long)(uintptr_t)P.in[2], ca) && al(P.in_ls[2], ca) && al(P.in_fp[2], ca)));
  };
  const bool vec = P.W % 8 == 0 && planes_al(16, 8);
  const bool quad = P.W % 16 == 0 && P.transfer == 0 && planes_al(16, 16);
  const bool dovi = P.dovi != nullptr;
  hipLaunchKernelGGL(T.M.pct ? peak_stats_kernel<true>(dovi, quad, vec, P.transfer)
                             : peak_stats_kernel<false>(dovi, quad, vec, P.transfer),
                     grid, dim3(256), 0, s, P, partial, T);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_peak_finish, dim3(P.nframes), dim3(256), 0, s, partial, T);
  return hipGetLastError();
}

// h2s_peak_feed: the IIR over caller-supplied statistics.  One block
void __global__ __launch_bounds__(64) k_peak_curves(double2* fstat, int n, const PeakModel M, PeakState* st,
                                                    CurveConsts* out) {
  peak_curves_body(fstat, n, M, st, out);
}

hipError_t launch_peak_curves(double2* fstat, int n, const PeakModel& M, PeakState* st, CurveConsts* out,
                              hipStream_t s) {
  hipLaunchKernelGGL(k_peak_curves, dim3(1), dim3(64), 0, s, fstat, n, M, st, out);
  return hipGetLastError();
}

}  // namespace h2s
