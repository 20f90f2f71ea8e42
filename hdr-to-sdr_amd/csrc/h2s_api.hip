// h2s_api.hip — the C-ABI (include/h2s.h): contexts, parameter resolution,
// LUT upload, frame validation, host staging and kernel timing.  Which kernels
// a call launches is decided once (Route) and carried out by launch_route over
// three primitives: launch_tiles, launch_columns and launch_two_pass.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#define H2S_PRIVATE_TEST_HOOKS
#include "../../include/h2s.h"
#include "h2s_device.h"
#include "h2s_peak.h"
#include "h2s_srcprev.h"

namespace h2s {
enum ProcessForm : unsigned { PF_VEC = 1, PF_OUT8 = 2, PF_C444 = 4 };   // as h2s_kernels.hip defines it
hipError_t launch_process(const KParams& P, unsigned form, hipStream_t s);
hipError_t launch_debug(const KParams& P, int stage, float* out, hipStream_t s);
bool fast_supported(int tonemap);
hipError_t launch_fast(const FastParams& F, int trc, int tm, int desat, int lp, hipStream_t s, int sub = 0);
hipError_t launch_chroma_bicubic(const KParams& P, const float* wx7, const float* wy8, bool out8, hipStream_t s);
hipError_t build_lut_yuv(const float4* rgb, float* yuv, int n, const YuvLutConsts& K, hipStream_t st);
hipError_t build_lut8x(const float4* lut, int n, unsigned* out, hipStream_t s);
hipError_t launch_resize_u8(const uint8_t* src, int sw, int sh, long long sls, long long sfp, uint8_t* dst, int ow,
                            int oh, long long dls, long long dfp, const float* wx, const int* sx, const float* wy,
                            const int* sy, int T, int nframes, hipStream_t s);
hipError_t launch_yuv8_rgb24(const uint8_t* yp, long long yls, const uint8_t* up, const uint8_t* vp, long long cls,
                             long long yuv_fp, int w, int h, uint8_t* rgb, long long rls, long long rgb_fp,
                             const uint8_t* glut, int nframes, hipStream_t s);
hipError_t launch_peak_stats(const KParams& P, float2* partial, const PeakTail& T, hipStream_t s);
hipError_t launch_peak_curves(double2* fstat, int n, const PeakModel& M, PeakState* st, CurveConsts* out,
                              hipStream_t s);
}  // namespace h2s

using h2s::FastParams;
using h2s::KParams;

struct h2s_ctx;

namespace {
thread_local std::string g_err;  // errors with no context
constexpr int kEvRing = 256;
constexpr int kMaxChunks = 8;  // host-frame pipeline depth (chunks per call)

int fail(h2s_ctx* c, int code, const std::string& msg);
int hip_fail(h2s_ctx* c, hipError_t e, const char* what);

// The form of a frame set: its layout (enum h2s_layout; semi-planar: plane 1
// holds (Cb, Cr) pairs, a row of it is as long as a luma row, plane 2 is
// unused) and its chroma subsampling (enum h2s_subsampling: chroma planes of
// width >> cxs samples x height >> cys rows; a semi-planar set and every
// output set is 4:2:0).  Whatever reads an h2s_frames takes its Format, never
// defaulted; the planes' sizes are written here and nowhere else.  An input
// set also carries its source tags (h2s_set_input_tags): the colour range of
// its codes (enum h2s_range) and its 4:2:0 chroma location (enum
// h2s_chroma_loc); the kernels' S1 constants and vertical taps follow from
// them in fill_geometry.  An output set is always limited range
struct Format {
  int layout, sub;
  int range = H2S_RANGE_LIMITED, loc = H2S_CHROMA_LEFT;
  bool full() const { return range == H2S_RANGE_FULL; }
  // chroma rows co-sited with the even luma rows: 4:2:0 only (a 4:2:2 / 4:4:4
  // set has no vertical pass, the tag has no effect there)
  bool vco() const { return loc == H2S_CHROMA_TOPLEFT && sub == H2S_SUB_420; }
  bool semi() const { return layout == H2S_LAYOUT_SEMI; }
  int cxs() const { return sub == H2S_SUB_444 ? 0 : 1; }
  int cys() const { return sub == H2S_SUB_420 ? 1 : 0; }
  int planes() const { return semi() ? 2 : 3; }
  struct Plane {
    long long row_bytes, rows;
  };
  Plane plane(const h2s_frames* f, int p) const {
    const long long bps = f->bits == 8 ? 1 : 2;
    if (p == 0) return {f->width * bps, f->height};
    // (semi-planar: pairs, so a 4:2:0 row is as long as a luma row)
    return {(f->width >> cxs()) * bps * (semi() ? 2 : 1), f->height >> cys()};
  }
};
constexpr Format PLANAR_420{H2S_LAYOUT_PLANAR, H2S_SUB_420};

// ---- owners of the context's device resources ----

// device buffer of at least `cap` bytes (grown, never shrunk); a grown
// buffer is freed only after the launches that read the old one (hipFree
// synchronises).  pool set (the lattices): a stream-ordered allocation of
// that stream instead (hipMallocAsync / hipFreeAsync), which must still
// exist at release
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipStream_t pool = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), pool(o.pool) { o.p = nullptr, o.cap = 0; }
  ~DevBuf() { release(); }
  void release() {
    if (p) pool ? hipFreeAsync(p, pool) : hipFree(p);
    p = nullptr, cap = 0;
  }
  int reserve(h2s_ctx* c, size_t bytes, const char* what, bool* grew = nullptr) {
    if (bytes <= cap) return 0;
    release();
    if ((pool ? hipMallocAsync(&p, bytes, pool) : hipMalloc(&p, bytes)) != hipSuccess) {
      p = nullptr;
      return fail(c, H2S_E_OOM, std::string(what) + " allocation failed");
    }
    cap = bytes;
    if (grew) *grew = true;
    return 0;
  }
};

template <class T>
struct Dev : DevBuf {
  operator T*() const { return static_cast<T*>(p); }
};

// created on first use: non-blocking streams, and events without timing
// (the timing ring asks for hipEventDefault)
struct Stream {
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) hipStreamDestroy(s);
  }
  int get(h2s_ctx* c, const char* what) {
    if (s) return 0;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) return 0;
    s = nullptr;
    return hip_fail(c, e, what);
  }
};

struct Event {
  hipEvent_t ev = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
  Event& operator=(Event&& o) noexcept {
    std::swap(ev, o.ev);
    return *this;
  }
  ~Event() {
    if (ev) hipEventDestroy(ev);
  }
  int get(h2s_ctx* c, const char* what, unsigned flags = hipEventDisableTiming) {
    if (ev) return 0;
    hipError_t e = hipEventCreateWithFlags(&ev, flags);
    if (e == hipSuccess) return 0;
    ev = nullptr;
    return hip_fail(c, e, what);
  }
};

// One scratch of the context that calls on different streams share (the
// BICUBIC plane, the peak buffers and state, a derived lattice while it is
// built): the call that uses it marks its stream afterwards, and the next
// call waits on its own stream for that mark before it touches the scratch.
// The rule for the steady state: once the marked work is seen complete
// (hipEventQuery in wait) pending is cleared, and from then on the guard
// makes no HIP call until the next mark
struct Ordered {
  Event ev;
  bool pending = false;
  int wait(h2s_ctx* c, hipStream_t s, const char* what) {
    if (!pending) return 0;
    if (hipEventQuery(ev.ev) == hipSuccess) {
      pending = false;
      return 0;
    }
    hipError_t e = hipStreamWaitEvent(s, ev.ev, 0);
    return e == hipSuccess ? 0 : hip_fail(c, e, what);
  }
  int mark(h2s_ctx* c, hipStream_t s, const char* what) {
    if (int rc = ev.get(c, what)) return rc;
    hipError_t e = hipEventRecord(ev.ev, s);
    if (e != hipSuccess) return hip_fail(c, e, what);
    pending = true;
    return 0;
  }
  int sync_host(h2s_ctx* c, const char* what) {
    if (!pending) return 0;
    hipError_t e = hipEventSynchronize(ev.ev);
    if (e != hipSuccess) return hip_fail(c, e, what);
    pending = false;
    return 0;
  }
};
}  // namespace

// (hidden: its implicit destructor is no part of the library's symbol set)
struct __attribute__((visibility("hidden"))) h2s_ctx {
  int device = 0;
  h2s_params params{};
  bool params_set = false;
  KParams k{};  // resolved constants (pointers filled per call)
  // set_params / set_lut copy and (re)allocate on this non-blocking stream
  // (stream-ordered hipMallocAsync / hipFreeAsync for the lattices): no
  // null-stream copy or hipFree, which would wait for the whole device.
  // h2s_destroy releases the lattices and waits for the stream before the
  // members go; declared before them, it would outlive them in any case
  Stream aux;
  Dev<float4> d_lut;
  int lut_n = 0;
  Dev<float> d_lut_yuv;  // lattice pre-multiplied into output code space (3 floats/point)
  float lut_yuv_scale = -1.0f;  // quantiser scale it was built for (-1 = stale)
  int lut_yuv_rgb = 0;          // 1: it holds plain R'G'B' records (libplacebo rgba8 form)
  Dev<unsigned> d_lut8x;  // libplacebo branch: lut3d's 8-bit output per rgba code triple (2^24, 64 MiB)
  bool lut8x_ok = false;        // built for the current lattice
  Ordered lut_built;      // after the last build of d_lut_yuv / d_lut8x (queued on the caller's stream)
  bool fast_enabled = true;
  bool lp_exact = false;  // H2S_OPT_LP_EXACT
  // how later calls read `in` and write `out`: h2s_set_frame_layout sets both
  // layouts, h2s_set_input_subsampling in_fmt.sub (the output is always 4:2:0),
  // h2s_set_input_tags in_fmt.range and in_fmt.loc
  Format in_fmt = PLANAR_420, out_fmt = PLANAR_420;
  int peak_blocks = h2s::PEAK_BLOCKS;   // H2S_OPT_TEST_PEAK_BLOCKS (private A/B hook)
  int peak_form = 0;      // H2S_OPT_TEST_PEAK_FORM (private A/B hook)
  bool serial_host = false;  // H2S_HOST_SERIAL=1: one H2D, kernel, D2H per call (no chunk pipeline)
  int tiles_per_block = 8;  // k_tile: tiles one block walks (H2S_TILES_PER_BLOCK overrides, 1..64)
  Dev<uint16_t> d_eq;
  Dev<float4> d_pq;   // PQ EOTF cubic segments (fast path)
  Dev<float4> d_hlg;  // HLG inverse-OETF cubic segments (fast path, CPU chain)
  Dev<float4> d_pqi;  // PQ inverse EOTF cubic segments (fast path, lp_tone IPT)
  Dev<uint8_t> d_stage;
  Dev<uint8_t> d_prev;  // preview scratch
  // dynamic peak (params.peak_detect), all on the device: statistics ->
  // per-frame (max, avg) -> IIR + curve records -> conversion, queued on the
  // caller's stream with no host round trip (h2s_peak.h)
  Dev<float2> d_stats;           // per-block partials, then (percentile model) histograms
  int stats_nf = 0;   // frames d_stats is laid out for (frame_stats)
  Dev<double2> d_fstat;          // per frame: the statistic, then the smoothed (max, avg) its curve uses
  Dev<h2s::CurveConsts> d_curve; // one curve record per frame of a dynamic-peak launch
  Dev<h2s::PeakState> d_pk;      // [0] the smoothing state; [1] a preview's saved copy of it
  Ordered peak_use;              // after the last launch that used the buffers above
  // pipelined schedule (run_dynamic_peak_chunked; private A/B hook
  // H2S_OPT_TEST_PEAK_CHUNK, off: measured slower): frames per
  // chunk (0 = one statistics launch, then one conversion launch, all on the
  // caller's stream), the statistics stream and a second conversion stream,
  // events: start | end | per-chunk statistics
  int peak_chunk = 0;
  Stream pk_s[2];
  std::vector<Event> pk_ev;
  std::string err;
  bool fail_after_launch = false;  // H2S_OPT_TEST_FAIL_AFTER_LAUNCH (private test hook, one call)
  bool timing = false;
  Event ev0[kEvRing], ev1[kEvRing];
  long long ev_count = 0;  // launches recorded since reset
  // host-frame pipeline: H2D, compute and D2H of consecutive chunks on
  // their own streams (two DMA directions overlap the kernel and each other)
  Stream ps[3];
  Event pev[2 * kMaxChunks + 2];
  // events recorded after this context's own asynchronous launches, on the
  // streams they went to: set_params / set_lut wait for exactly these (no
  // device-wide synchronisation), then recycle them
  std::vector<Event> pend, ev_free;
  Dev<float2> d_chr;             // BICUBIC chroma: one frame's per-pixel (Cb, Cr)
  Ordered chr_use;               // after the last BICUBIC two-pass launch (d_chr in use)
};

namespace {

int fail(h2s_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  else g_err = msg;
  return code;
}

int hip_fail(h2s_ctx* c, hipError_t e, const char* what) {
  return fail(c, H2S_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) hipSetDevice(prev);
  }
};

// ---- parameter resolution (mirrors vf_tonemap init/filter_frame, zimg,
// vf_eq create_lut; the CPU statement is oracle/h2s_oracle.c resolve()) ----
float hable_h(float in) { return h2s::hd_hable(in); }

double pq_encode_d(double y) { return h2s::hd_pq_encode(y); }

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

void resolve(const h2s_params* p, KParams* k, std::vector<uint16_t>* eq) {
  memset(k, 0, sizeof(*k));
  // S1 zimg: depth conversion (limited range), BT.2020-NCL matrix, scale
  const int sh = p->bits_in - 8;
  k->y_scale = (float)(1.0 / (219 << sh));
  k->y_off = (float)(-(double)(16 << sh) / (219 << sh));
  k->c_scale = (float)(1.0 / (224 << sh));
  k->c_off = (float)(-(double)(128 << sh) / (224 << sh));
  const double kr = 0.2627, kb = 0.0593, kg = 1.0 - kr - kb;
  k->m_rcr = (float)(2.0 * (1.0 - kr));
  k->m_gcb = (float)(-2.0 * kb * (1.0 - kb) / kg);
  k->m_gcr = (float)(-2.0 * kr * (1.0 - kr) / kg);
  k->m_bcb = (float)(2.0 * (1.0 - kb));
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
  k->hable_peak_inv = 1.0f / hable_h((float)peak);
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

// ST 2084 inverse EOTF (y = luminance / 10000 -> E) as PQI_NSEG cubic
// segments for the tile kernel's IPT form (h2s_tile.h pqi): segment s covers
// y = 2^e (1 + j/8 + t), e = PQI_OCT0 + s/8, j = s%8, t in [0, 1/8), read from
// the float's exponent and top three mantissa bits; the cubic in t through
// the exact (double) encode at the 4 Chebyshev nodes (relative error <=
// 1.5e-7 with float32 coefficients).  Entry 0 is the constant PQ(0), read for
// y <= 0 and for y below the first octave (2^-64, 1e-15 nits: PQ within 3e-7
// of PQ(0)); segment s is entry 1 + s (PQI_NTAB entries)
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

void build_pqi_table(std::vector<float4>* out) {
  constexpr int K = h2s::PQI_PER_OCT;
  out->resize(h2s::PQI_NTAB);
  (*out)[0] = make_float4(0.0f, 0.0f, 0.0f, (float)pq_encode_d(0.0));
  double t[4];
  for (int k = 0; k < 4; k++) t[k] = (1.0 - cos((2 * k + 1) * M_PI / 8.0)) / 2.0 / K;
  for (int sg = 0; sg < h2s::PQI_NSEG; sg++) {
    const double base = ldexp(1.0, h2s::PQI_OCT0 + sg / K);
    double y[4], c[4];
    for (int k = 0; k < 4; k++) y[k] = pq_encode_d(base * (1.0 + (double)(sg % K) / K + t[k]));
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
    // solve the 4x4 Vandermonde system A c = y (c = c0..c3) by Gaussian elimination
    double A[4][5];
    for (int k = 0; k < 4; k++) {
      for (int j = 0; j < 4; j++) A[k][j] = pow(t[k], j);
      A[k][4] = eotf((i + t[k]) / h2s::PQ_SEG);
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
    double c[4];
    for (int k = 0; k < 4; k++) c[k] = A[k][4] / A[k][k];
    if (i == 0) c[0] = 0.0;  // E = 0 maps to exactly 0, as zimg's x > 0 test
    (*out)[i] = make_float4((float)c[3], (float)c[2], (float)c[1], (float)c[0]);
  }
}

void build_pq_table(double scale, std::vector<float4>* out) {
  const double m1 = 2610.0 / 16384, m2 = 2523.0 / 32, c1 = 3424.0 / 4096, c2 = 2413.0 / 128, c3 = 2392.0 / 128;
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

bool aligned(const void* p, long long a) { return ((uintptr_t)p % (uintptr_t)a) == 0; }

int check_frames(h2s_ctx* c, const h2s_frames* f, int bits, const char* which, Format fmt) {
  if (!f) return fail(c, H2S_E_INVALID_ARG, std::string(which) + " frames is NULL");
  if (f->width <= 0 || f->height <= 0) return fail(c, H2S_E_INVALID_ARG, std::string(which) + ": empty frame");
  if ((f->width & 1) || (f->height & 1))
    return fail(c, H2S_E_UNSUPPORTED, std::string(which) + (fmt.sub ? ": the 4:2:0 output needs even width and height"
                                                                     : ": 4:2:0 frames need even width and height"));
  if (f->bits != bits)
    return fail(c, H2S_E_INVALID_ARG,
                std::string(which) + ": bits " + std::to_string(f->bits) + " != params " + std::to_string(bits));
  if (f->location != H2S_LOC_DEVICE && f->location != H2S_LOC_HOST)
    return fail(c, H2S_E_INVALID_ARG, std::string(which) + ": bad location");
  const int bps = bits == 8 ? 1 : 2;
  for (int p = 0; p < fmt.planes(); p++) {
    if (!f->data[p]) return fail(c, H2S_E_INVALID_ARG, std::string(which) + ": NULL plane");
    if (f->linesize[p] < fmt.plane(f, p).row_bytes)
      return fail(c, H2S_E_INVALID_ARG, std::string(which) + ": linesize smaller than a row");
    if (bps == 2 && ((f->linesize[p] & 1) || !aligned(f->data[p], 2)))
      return fail(c, H2S_E_INVALID_ARG, std::string(which) + ": 16-bit planes must be 2-byte aligned");
    if (fmt.semi() && bps == 2 && (f->frame_pitch[p] & 1))
      return fail(c, H2S_E_INVALID_ARG, std::string(which) + ": 16-bit planes need an even frame pitch");
  }
  return 0;
}

// every plane fmt has: its base, its rows and its frames a bytes apart
bool planes_aligned(const h2s_frames* f, Format fmt, long long ay, long long ac) {
  for (int p = 0; p < fmt.planes(); p++) {
    const long long a = p ? ac : ay;
    if (!aligned(f->data[p], a) || f->linesize[p] % a || f->frame_pitch[p] % a) return false;
  }
  return true;
}

// vector path needs 16-B luma / 8-B chroma alignment of every row start
// (semi-planar: four pairs of the interleaved plane are one luma-sized access)
// (4:4:4 input: a chroma row is read like a luma row)
bool vec_ok(const h2s_frames* f, bool out8, Format fmt) {
  const long long ay = out8 ? 8 : 16;
  return planes_aligned(f, fmt, ay, fmt.semi() || fmt.sub == H2S_SUB_444 ? ay : ay / 2);
}

// tile kernel: at least one 64-pixel tile, every row start 16-B aligned (8-B
// for 8-bit output), of the planes each set has
bool tile_ok(const h2s_frames* in, const h2s_frames* out, bool out8, int tw, Format in_fmt, Format out_fmt) {
  if (in->width < tw) return false;  // width % tw columns go to k_process (launch_columns)
  const long long a = out8 ? 8 : 16;
  return planes_aligned(in, in_fmt, 16, 16) && planes_aligned(out, out_fmt, a, a);
}

size_t frame_bytes(const h2s_frames* f, Format fmt) {
  size_t n = 0;
  for (int p = 0; p < fmt.planes(); p++) n += (size_t)(fmt.plane(f, p).row_bytes * fmt.plane(f, p).rows);
  return n;
}

// tight device copy descriptor laid out in `base`: the planes fmt has back to
// back, rows packed, frames frame_bytes apart (a semi-planar frame's bytes
// are the planar one's); a plane it has not is zero
h2s_frames tight(const h2s_frames* f, void* base, Format fmt) {
  h2s_frames t = *f;
  const long long fb = (long long)frame_bytes(f, fmt);
  long long off = 0;
  for (int p = 0; p < 3; p++) {
    const bool has = p < fmt.planes();
    t.data[p] = has ? (uint8_t*)base + off : nullptr;
    t.linesize[p] = has ? fmt.plane(f, p).row_bytes : 0;
    t.frame_pitch[p] = has ? fb : 0;
    if (has) off += fmt.plane(f, p).row_bytes * fmt.plane(f, p).rows;
  }
  t.location = H2S_LOC_DEVICE;
  return t;
}

// the set the kernels bind: a device set itself, a host set's tight copy staged in `base`
h2s_frames device_view(const h2s_frames* f, void* base, Format fmt) {
  return f->location == H2S_LOC_HOST ? tight(f, base, fmt) : *f;
}

// the whole batch is one contiguous span laid out as tight() describes
bool is_tight(const h2s_frames* f, Format fmt) {
  const h2s_frames t = tight(f, f->data[0], fmt);
  for (int p = 0; p < fmt.planes(); p++)
    if (f->data[p] != t.data[p] || f->linesize[p] != t.linesize[p] || f->frame_pitch[p] != t.frame_pitch[p])
      return false;
  return true;
}

hipError_t copy_frames(const h2s_frames* dst, const h2s_frames* src, int nframes, hipStream_t s, Format fmt) {
  if (is_tight(src, fmt) && is_tight(dst, fmt))  // one DMA for the whole batch
    return hipMemcpyAsync(dst->data[0], src->data[0], (size_t)src->frame_pitch[0] * nframes, hipMemcpyDefault, s);
  for (int fr = 0; fr < nframes; fr++)
    for (int p = 0; p < fmt.planes(); p++) {
      const Format::Plane pl = fmt.plane(src, p);
      hipError_t e = hipMemcpy2DAsync((uint8_t*)dst->data[p] + fr * dst->frame_pitch[p], dst->linesize[p],
                                      (const uint8_t*)src->data[p] + fr * src->frame_pitch[p], src->linesize[p],
                                      pl.row_bytes, pl.rows, hipMemcpyDefault, s);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

// A semi-planar set (h2s_set_frame_layout) is bound with plane 2 as plane 1 one sample on, samples two apart, so
// the kernels address both layouts alike; 16-bit words carry the code in
// their high bits
// The input's chroma plane (h2s_set_input_subsampling) is icw x ich; cw, ch,
// ngx and total stay the output's
// The input's tags (h2s_set_input_tags): a full-range set replaces the S1
// depth-conversion constants resolve() wrote (zimg's full-range integer to
// float conversion: Y' = code / (2^b - 1), Cb, Cr = (code - 2^(b-1)) /
// (2^b - 1)); resolve_fast folds the same from k.full
void fill_geometry(KParams* k, const h2s_frames* in, const h2s_frames* out, int nframes, Format in_fmt,
                   Format out_fmt) {
  k->W = in->width;
  k->H = in->height;
  k->cw = in->width / 2;
  k->ch = in->height / 2;
  k->sub = in_fmt.sub, k->icw = in->width >> in_fmt.cxs(), k->ich = in->height >> in_fmt.cys();
  k->full = in_fmt.full() ? 1 : 0, k->vco = in_fmt.vco() ? 1 : 0;
  if (k->full) {
    const double top = (double)((1 << in->bits) - 1);
    k->y_scale = (float)(1.0 / top), k->y_off = 0.0f;
    k->c_scale = (float)(1.0 / top), k->c_off = (float)(-(double)(1 << (in->bits - 1)) / top);
  }
  k->ngx = (k->cw + 3) / 4;
  k->nframes = nframes;
  k->total = (long long)nframes * k->ch * k->ngx;
  for (int p = 0; p < 3; p++) {
    k->in[p] = (const uint8_t*)in->data[p];
    k->in_ls[p] = in->linesize[p];
    k->in_fp[p] = in->frame_pitch[p];
    if (out) {
      k->out[p] = (uint8_t*)out->data[p];
      k->out_ls[p] = out->linesize[p];
      k->out_fp[p] = out->frame_pitch[p];
    }
  }
  k->in_cstep = k->out_cstep = 1, k->in_sh = k->out_sh = 0;
  if (in_fmt.semi()) {
    k->in[2] = k->in[1] + 2, k->in_ls[2] = k->in_ls[1], k->in_fp[2] = k->in_fp[1];
    k->in_cstep = 2, k->in_sh = 16 - in->bits;
    k->in_mask &= 0xFFFFu >> k->in_sh;
  }
  if (out && out_fmt.semi()) {
    const int bps = out->bits == 8 ? 1 : 2;
    k->out[2] = k->out[1] + bps, k->out_ls[2] = k->out_ls[1], k->out_fp[2] = k->out_fp[1];
    k->out_cstep = 2, k->out_sh = bps == 2 ? 16 - out->bits : 0;
  }
}

}  // namespace

extern "C" {

int h2s_abi_version(void) { return H2S_ABI_VERSION; }

int h2s_abi_minor(void) { return H2S_ABI_MINOR; }

const char* h2s_last_error(const h2s_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

void h2s_params_default(h2s_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  // FFMPEG_CONVERT_FILTER defaults (src/utils.py:38-42) with the settings
  // defaults (src/settings.py:10-26: gamma 1.0, tonemapper Mobius) and the
  // GUI's 10-bit output for <=10-bit sources (src/gui.py:1009-1021).
  p->transfer_in = H2S_TRC_PQ;
  p->bits_in = 10;
  p->bits_out = 10;
  p->tonemap = H2S_TM_MOBIUS;
  p->tm_param = NAN;
  p->desat = 2.0;
  p->peak = 0.0;
  p->npl = 100.0;
  p->gamma = 1.0;
  p->lut_enabled = 1;
  p->mode = H2S_MODE_COMPAT8;
  p->desat_luma = H2S_DESAT_LUMA_RGB;
  // [EXT] switches: the round-1 models; pipeline AUTO; libplacebo targets from the branch
  p->chroma_filter = H2S_CHROMA_BOX;
  p->dither = H2S_DITHER_NONE;
  p->expand = H2S_EXPAND_SHIFT;
  p->pipeline = H2S_PIPE_AUTO;
  p->knee_offset = NAN;
  p->target_black = NAN;
  p->target_white = NAN;
  p->chroma_edge = H2S_EDGE_ZIMG;
  p->lut_input = H2S_LUT_IN_FLOAT;
  p->lp_tone = H2S_LP_TONE_IPT;   // libplacebo >= 6 tone-maps in IPT (h2s.h enum h2s_lp_tone)
  p->lp_range = H2S_LP_RANGE_FULL;
  p->lp_dither = H2S_LP_DITHER_NONE;
  p->lp_p010 = H2S_LP_P010_TRUNCATE;   // format=p010,hwupload (src/utils.py:431)
  p->pd_smoothing = p->pd_scene_low = p->pd_scene_high = p->pd_percentile = p->pd_min_peak = NAN;
}

int h2s_create(int device, h2s_ctx** out) {
  if (!out) return fail(nullptr, H2S_E_INVALID_ARG, "out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return fail(nullptr, H2S_E_HIP, "no HIP device available");
  if (device < 0 || device >= n) return fail(nullptr, H2S_E_INVALID_ARG, "device ordinal out of range");
  h2s_ctx* c = new (std::nothrow) h2s_ctx();
  if (!c) return fail(nullptr, H2S_E_OOM, "context allocation failed");
  c->device = device;
  h2s_params_default(&c->params);
  if (const char* v = getenv("H2S_HOST_SERIAL")) c->serial_host = atoi(v) != 0;
  if (const char* v = getenv("H2S_TILES_PER_BLOCK")) {
    const int tpb = atoi(v);
    if (tpb >= 1 && tpb <= 64) c->tiles_per_block = tpb;
  }
  *out = c;
  return 0;
}

void h2s_destroy(h2s_ctx* c) {
  if (!c) return;
  DeviceGuard g(c->device);
  hipDeviceSynchronize();
  if (c->aux.s) {  // the lattices are stream-ordered allocations of the context stream
    c->d_lut.release();
    c->d_lut_yuv.release();
    c->d_lut8x.release();
    hipStreamSynchronize(c->aux.s);
  }
  delete c;  // the members' destructors free the rest, on this device (g is still in scope)
}

// set_params / set_lut rewrite device tables that this context's queued
// kernels may still read: wait for the events recorded after its own
// launches (include/h2s.h), not for the device
static int drain_launches(h2s_ctx* c) {
  hipError_t e = hipSuccess;
  for (Event& ev : c->pend) {
    const hipError_t r = hipEventSynchronize(ev.ev);
    if (e == hipSuccess) e = r;
    c->ev_free.push_back(std::move(ev));
  }
  c->pend.clear();
  if (e != hipSuccess) return hip_fail(c, e, "draining queued launches");
  return 0;
}

// the context stream, which is also the lattices' allocation pool
static int aux_stream(h2s_ctx* c, hipStream_t* out) {
  if (int rc = c->aux.get(c, "table stream")) return rc;
  *out = c->d_lut.pool = c->d_lut_yuv.pool = c->d_lut8x.pool = c->aux.s;
  return 0;
}

// host -> device table copy on the context's own stream, waited for there
static hipError_t table_copy(h2s_ctx* c, void* dst, const void* src, size_t bytes) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->aux.s);
  return e == hipSuccess ? hipStreamSynchronize(c->aux.s) : e;
}

// a table of the context's: (first use) allocate, then upload
static int upload_table(h2s_ctx* c, DevBuf& buf, const void* src, size_t bytes, const char* what) {
  if (int rc = buf.reserve(c, bytes, what)) return rc;
  hipError_t e = table_copy(c, buf.p, src, bytes);
  return e == hipSuccess ? 0 : hip_fail(c, e, (std::string(what) + " upload").c_str());
}

static int note_launch(h2s_ctx* c, hipStream_t s);

// an error exit of h2s_process after work was queued on s: record the launch
// event anyway, so that a later set_params / set_lut still waits for that work
// before rewriting the tables it reads (include/h2s.h); if even the event
// cannot be recorded, wait for the stream.  The caller's error stays the one
// reported.
static int queued_exit(h2s_ctx* c, hipStream_t s, int rc) {
  const std::string msg = c->err;
  if (note_launch(c, s) != 0) (void)hipStreamSynchronize(s);
  c->err = msg;
  return rc;
}

// record that this context queued work on stream s (after the launches)
static int note_launch(h2s_ctx* c, hipStream_t s) {
  if (c->pend.size() >= 32) {   // recycle the events that have completed
    size_t j = 0;
    for (size_t i = 0; i < c->pend.size(); i++) {
      if (hipEventQuery(c->pend[i].ev) == hipSuccess) c->ev_free.push_back(std::move(c->pend[i]));
      else c->pend[j++] = std::move(c->pend[i]);
    }
    c->pend.resize(j);
  }
  Event ev;
  if (!c->ev_free.empty()) {
    ev = std::move(c->ev_free.back());
    c->ev_free.pop_back();
  }
  if (int rc = ev.get(c, "launch event")) return rc;
  hipError_t e = hipEventRecord(ev.ev, s);
  if (e != hipSuccess) {
    c->ev_free.push_back(std::move(ev));
    return hip_fail(c, e, "launch event");
  }
  c->pend.push_back(std::move(ev));
  return 0;
}

int h2s_set_lut(h2s_ctx* c, const float* rgb, int n) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (!rgb || n < 2 || n > 256) return fail(c, H2S_E_INVALID_ARG, "LUT size must be in [2, 256]");
  DeviceGuard g(c->device);
  if (int rc = drain_launches(c)) return rc;
  const size_t cnt = (size_t)n * n * n;
  std::vector<float4> host(cnt);
  for (size_t i = 0; i < cnt; i++) host[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f);
  hipStream_t aux;
  if (int rc = aux_stream(c, &aux)) return rc;
  // a size change reallocates stream-ordered on the context's stream: a plain
  // hipFree would wait for every stream on the device
  if (c->lut_n != n) {
    c->d_lut.release();
    c->d_lut_yuv.release();
  }
  c->lut_yuv_scale = -1.0f;
  c->lut8x_ok = false;
  if (int rc = c->d_lut.reserve(c, cnt * sizeof(float4), "LUT device")) return rc;
  hipError_t e = table_copy(c, c->d_lut, host.data(), cnt * sizeof(float4));
  if (e != hipSuccess) return hip_fail(c, e, "LUT upload");
  c->lut_n = n;
  return 0;
}

int h2s_set_params(h2s_ctx* c, const h2s_params* p) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (!p) return fail(c, H2S_E_INVALID_ARG, "params is NULL");
  int rc = validate_params(c, p);
  if (rc) return rc;
  DeviceGuard g(c->device);
  if ((rc = drain_launches(c))) return rc;
  hipStream_t aux;
  if ((rc = aux_stream(c, &aux))) return rc;
  std::vector<uint16_t> eq;
  KParams k;
  resolve(p, &k, &eq);
  // the eq table is allocated for the deepest quantiser (12 bits)
  if ((rc = c->d_eq.reserve(c, 4096 * sizeof(uint16_t), "eq table")) ||
      (rc = upload_table(c, c->d_eq, eq.data(), eq.size() * sizeof(uint16_t), "eq table")))
    return rc;
  {
    std::vector<float4> tab;
    // (x 10000/npl for either input transfer: the libplacebo branch's IPT form
    // decodes PQ L'M'S' through it for HLG input too)
    build_pq_table(10000.0 / p->npl, &tab);
    if ((rc = upload_table(c, c->d_pq, tab.data(), tab.size() * sizeof(float4), "PQ table"))) return rc;
    if (!c->d_pqi) {
      build_pqi_table(&tab);
      if ((rc = upload_table(c, c->d_pqi, tab.data(), tab.size() * sizeof(float4), "PQ encode table"))) return rc;
    }
    if (!c->d_hlg && p->transfer_in == H2S_TRC_HLG) {   // parameter-independent: built once
      build_hlg_table(&tab);
      if ((rc = upload_table(c, c->d_hlg, tab.data(), tab.size() * sizeof(float4), "HLG table"))) return rc;
    }
  }
  c->params = *p;
  c->k = k;
  c->params_set = true;
  h2s_peak_reset(c);  // a new parameter set starts a new sequence
  return 0;
}

// FastParams from the resolved KParams (same constants, scales folded)
static void resolve_fast(const h2s_ctx* c, const KParams& k, FastParams* F) {
  memset(F, 0, sizeof(*F));
  const h2s_params* p = &c->params;
  const int sh = p->bits_in - 8;
  // (a full-range input set, k.full: fill_geometry's constants in double)
  const double top = (double)((256 << sh) - 1);
  const double ys = k.full ? 1.0 / top : 1.0 / (219 << sh), yo = k.full ? 0.0 : -(double)(16 << sh) / (219 << sh);
  const double cs = k.full ? 1.0 / top : 1.0 / (224 << sh);
  const double co = k.full ? -(double)(128 << sh) / top : -(double)(128 << sh) / (224 << sh);
  const double kr = 0.2627, kb = 0.0593, kg = 1.0 - kr - kb;
  const double mrcr = 2.0 * (1.0 - kr), mgcb = -2.0 * kb * (1.0 - kb) / kg, mgcr = -2.0 * kr * (1.0 - kr) / kg,
               mbcb = 2.0 * (1.0 - kb);
  F->ys = (float)ys;
  F->k_r = (float)(yo + mrcr * co);
  F->k_g = (float)(yo + (mgcb + mgcr) * co);
  F->k_b = (float)(yo + mbcb * co);
  F->y_off_c = (float)yo;
  F->c_mid = (float)(128 << sh);
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
  F->b_e1min = (float)pq_encode_d(1e-6 * p->npl / 10000.0);
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

// the libplacebo branch's lut3d 8-bit table (k_build_lut8x): allocated on
// the context stream once, rebuilt on s after every h2s_set_lut
static int ensure_lut8x(h2s_ctx* c, hipStream_t s) {
  if (c->d_lut8x && c->lut8x_ok) return 0;
  hipStream_t aux;
  bool grew = false;
  int rc;
  if ((rc = aux_stream(c, &aux)) || (rc = c->d_lut8x.reserve(c, sizeof(unsigned) << 24, "lut3d 8-bit table", &grew)))
    return rc;
  if (grew && hipStreamSynchronize(aux) != hipSuccess) {
    c->d_lut8x.release();
    return fail(c, H2S_E_OOM, "lut3d 8-bit table allocation failed");
  }
  hipError_t e = h2s::build_lut8x(c->d_lut, c->lut_n, c->d_lut8x, s);
  if (e != hipSuccess) return hip_fail(c, e, "lut3d 8-bit table build");
  if ((rc = c->lut_built.mark(c, s, "lut3d 8-bit table build"))) return rc;
  c->lut8x_ok = true;
  return 0;
}

// the tile kernel's derived lattice is current, and its build (queued on the
// stream of the call that found it stale) is ordered before this call's use
static int ensure_lut_yuv(h2s_ctx* c, const KParams& k, hipStream_t s) {
  int rc;
  if ((rc = c->lut_built.wait(c, s, "lattice build ordering"))) return rc;
  if (k.rgba8) return ensure_lut8x(c, s);   // the libplacebo branch reads only its 8-bit table
  if (c->d_lut_yuv && c->lut_yuv_scale == k.qscale && c->lut_yuv_rgb == k.rgba8) return 0;
  const size_t cnt = (size_t)c->lut_n * c->lut_n * c->lut_n;
  // beside d_lut: stream-ordered on the context stream, complete before s uses it.
  // zero-filled tail: a coordinate clamped to exactly N-1 (k_tile's
  // H2S_EXPCLAMP form) names cell N-1, whose corners past the lattice edge
  // carry weight 0 but are still read; the scalar-record steps read them
  // without the buffer resource's bounds check, so they must be mapped
  const size_t pad = 12 * (1 + (size_t)c->lut_n + (size_t)c->lut_n * c->lut_n) + 16;
  hipStream_t aux;
  bool grew = false;
  if ((rc = aux_stream(c, &aux)) || (rc = c->d_lut_yuv.reserve(c, cnt * 3 * sizeof(float) + pad, "YUV lattice", &grew)))
    return rc;
  if (grew) {
    hipError_t e = hipMemsetAsync(c->d_lut_yuv + cnt * 3, 0, pad, aux);
    if (e == hipSuccess) e = hipStreamSynchronize(aux);
    if (e != hipSuccess) {
      c->d_lut_yuv.release();
      return fail(c, H2S_E_OOM, "YUV lattice allocation failed");
    }
  }
  h2s::YuvLutConsts K;
  K.s = k.qscale;
  K.rgb = k.rgba8;
  for (int i = 0; i < 3; i++) K.k709[i] = k.k709[i], K.kcb[i] = k.kcb[i], K.kcr[i] = k.kcr[i];
  hipError_t e = h2s::build_lut_yuv(c->d_lut, c->d_lut_yuv, c->lut_n, K, s);
  if (e != hipSuccess) return hip_fail(c, e, "YUV lattice build");
  if ((rc = c->lut_built.mark(c, s, "YUV lattice build"))) return rc;
  c->lut_yuv_scale = k.qscale;
  c->lut_yuv_rgb = k.rgba8;
  return 0;
}

static int prepare(h2s_ctx* c, KParams* k, bool need_lut = true) {
  if (!c->params_set) return fail(c, H2S_E_INVALID_ARG, "h2s_set_params was not called");
  if (need_lut && c->params.lut_enabled && !c->d_lut)
    return fail(c, H2S_E_LUT_MISSING, "lut_enabled but no LUT loaded (h2s_set_lut)");
  *k = c->k;
  k->lut = c->d_lut;
  k->lut_n = c->lut_n;
  k->lut_sg = c->lut_n;
  k->lut_sb = c->lut_n * c->lut_n;
  k->lut_max = (float)(c->lut_n - 1);
  k->eq_lut = c->d_eq;
  return 0;
}

// BICUBIC chroma taps (oracle_chroma_taps): horizontal 7 taps around the
// left-sited position, vertical 8 around the centre-sited one, normalised
static void chroma_taps(float* wx7, float* wy8) {
  auto bic = [](double x) {
    const double B = 0.0, C = 0.6;
    x = fabs(x);
    if (x < 1.0) return ((12 - 9 * B - 6 * C) * x * x * x + (-18 + 12 * B + 6 * C) * x * x + (6 - 2 * B)) / 6.0;
    if (x < 2.0) return ((-B - 6 * C) * x * x * x + (6 * B + 30 * C) * x * x + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) / 6.0;
    return 0.0;
  };
  double tx[7], ty[8], sx = 0, sy = 0;
  for (int i = 0; i < 7; i++) sx += (tx[i] = bic((i - 3) / 2.0));
  for (int j = 0; j < 8; j++) sy += (ty[j] = bic((j - 3.5) / 2.0));
  for (int i = 0; i < 7; i++) wx7[i] = (float)(tx[i] / sx);
  for (int j = 0; j < 8; j++) wy8[j] = (float)(ty[j] / sy);
}

// How one call launches, decided once per call (process_frames,
// h2s_debug_float): the kernels (choose_path), what the rows' alignment and
// the output depth allow, the two sets' layouts and the stream.  A caller that
// spreads the call over its own streams copies it with another stream (on)
struct Route {
  int path;                    // H2S_PATH_*
  bool vec, out8;
  Format in_fmt, out_fmt;      // the two sets' forms
  hipStream_t s;
  bool tile() const { return path == H2S_PATH_TILE || path == H2S_PATH_TILE_TAIL; }
  Route on(hipStream_t other) const {
    Route r = *this;
    r.s = other;
    return r;
  }
};

// k restricted to frames [f0, f0 + n)
static KParams frame_range(const KParams& k, int f0, int n) {
  KParams kf = k;
  for (int p = 0; p < 3; p++) {
    kf.in[p] += (long long)f0 * kf.in_fp[p];
    kf.out[p] += (long long)f0 * kf.out_fp[p];
  }
  kf.nframes = n;
  kf.total = (long long)n * kf.ch * kf.ngx;
  return kf;
}

// the width the tile kernel covers: the whole 64-pixel tiles
static int tiled_width(const KParams& k) { return k.W & ~(h2s::TBW - 1); }

// what a tile launch does beside the plain conversion
struct TileOpts {
  const h2s::CurveConsts* cv_frames = nullptr;   // dynamic peak: one curve record per frame of the launch
  int dbg = 0;                 // > 0: the debug instance, which writes that stage's
  float* dbg_out = nullptr;    //      float planes of frame 0 here
  float2* chr444 = nullptr;    // BICUBIC pass 1: every pixel's (Cb, Cr) here, no chroma planes
};

// the tile kernel over the whole 64-pixel tiles of k's frames
static hipError_t launch_tiles(const h2s_ctx* c, const KParams& k, const Route& r, const TileOpts& o = {}) {
  FastParams F;
  resolve_fast(c, k, &F);
  for (int p = 0; p < 3; p++) {
    F.in[p] = k.in[p], F.in_ls[p] = k.in_ls[p], F.in_fp[p] = k.in_fp[p];
    F.out[p] = k.out[p], F.out_ls[p] = k.out_ls[p], F.out_fp[p] = k.out_fp[p];
  }
  // the chroma right halo of the last tile reads the real column (F.cw stays
  // the frame's), so the split from the ragged columns is exact
  F.W = tiled_width(k), F.H = k.H, F.cw = k.cw, F.ch = k.ch;
  F.icw = k.icw, F.ich = k.ich;
  F.chroma_edge = k.chroma_edge;
  F.in_semi = k.in_cstep == 2, F.in_sh = k.in_sh, F.out_semi = k.out_cstep == 2, F.out_sh = k.out_sh;
  for (int p = 0; p < 3; p++) {
    const long long ib = (long long)(p ? k.ich : k.H) * k.in_ls[p], ob = (long long)(p ? k.ch : k.H) * k.out_ls[p];
    F.in_bytes[p] = (int)(ib < 0x7fffffff ? ib : 0x7fffffff);
    F.out_bytes[p] = (int)(ob < 0x7fffffff ? ob : 0x7fffffff);
  }
  F.nbx = (unsigned)(F.W / h2s::TBW);
  F.nby = (unsigned)((k.H + h2s::TBH - 1) / h2s::TBH);
  F.nframes = (unsigned)k.nframes;
  F.tpb = c->tiles_per_block;
  F.cv_frames = o.cv_frames;
  F.dbg = o.dbg_out;
  F.dbg_stage = o.dbg;
  F.dbg_w = k.W;
  F.dbg_lut = c->d_lut;
  F.inv_nm1 = 1.0f / (float)(c->lut_n - 1);
  F.chr444 = o.chr444;
  F.chr_w = k.W;
  F.inv_c56 = 1.0f / F.c56;
  const int desat = !k.desat_on ? 0 : (k.lr == 1.0f && k.lg == 1.0f && k.lb == 1.0f ? 2 : 1);
  // (top-left 4:2:0: the SUB 3 instances, h2s_fast_tl.hip / h2s_fast_lp_tl.hip)
  return h2s::launch_fast(F, k.transfer, k.tonemap, desat, k.pipe == h2s::PIPE_LIBPLACEBO ? 1 : 0, r.s,
                          k.vco ? 3 : k.sub);
}

// the generic kernel over a column range of k's frames: every column, or the
// ragged ones right of the last whole tile (left-sited chroma needs no left
// neighbour, so the seam is exact; none: no launch).  k.chr444 set: BICUBIC
// pass 1 (luma, and every pixel's chroma into k.chr444)
enum Columns { COLUMNS_ALL, COLUMNS_RAGGED };

static hipError_t launch_columns(const KParams& k, const Route& r, Columns cols) {
  KParams kc = k;
  if (cols == COLUMNS_RAGGED) {
    const int w64 = tiled_width(k);
    kc.gx0 = w64 / 8;
    kc.ngx = (k.cw - w64 / 2 + 3) / 4;
    kc.total = (long long)k.nframes * k.ch * kc.ngx;
  }
  const unsigned form = (r.vec ? h2s::PF_VEC : 0) | (r.out8 ? h2s::PF_OUT8 : 0) | (k.chr444 ? h2s::PF_C444 : 0);
  return h2s::launch_process(kc, form, r.s);
}

// BICUBIC chroma, frame by frame: pass 1 writes luma and every pixel's
// (Cb, Cr) into the context scratch (the tile kernel, with the generic kernel
// over the ragged columns, or the generic kernel over every column), then the
// decimation pass writes the chroma planes
static hipError_t launch_two_pass(const h2s_ctx* c, const KParams& k, const Route& r) {
  float wx[7], wy[8];
  chroma_taps(wx, wy);
  TileOpts pass1;
  pass1.chr444 = c->d_chr;
  for (int f = 0; f < k.nframes; f++) {
    KParams kf = frame_range(k, f, 1);
    kf.chr444 = c->d_chr;
    hipError_t e = r.tile() ? launch_tiles(c, kf, r, pass1) : hipSuccess;
    if (e == hipSuccess) e = launch_columns(kf, r, r.tile() ? COLUMNS_RAGGED : COLUMNS_ALL);
    if (e == hipSuccess) e = h2s::launch_chroma_bicubic(kf, wx, wy, r.out8, r.s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// one conversion of k's frames as the route says (static peak; the dynamic
// peak's launches are run_dynamic_peak's)
static hipError_t launch_route(const h2s_ctx* c, const KParams& k, const Route& r) {
  if (c->params.chroma_filter == H2S_CHROMA_BICUBIC) return launch_two_pass(c, k, r);
  if (!r.tile()) return launch_columns(k, r, COLUMNS_ALL);
  const hipError_t e = launch_tiles(c, k, r);
  return e == hipSuccess ? launch_columns(k, r, COLUMNS_RAGGED) : e;
}

// the tile kernel serves: both of the reference's chains (the CPU chain, and
// the libplacebo branch with the LUT on: k_tile<..., LP = 1>), the LUT on at
// N <= 177 (its lattice byte offsets are formed in float32, exact for
// multiples of 4 below 2^26 = 12 * 177^3 + margin), the default [EXT]
// switches, 10/12-bit input and BASELINE's operators; frames with a 64-wide
// tile and 16-byte aligned rows
static bool fast_params_ok(const h2s_ctx* c, const KParams& k) {
  const h2s_params& p = c->params;
  if (!c->fast_enabled || !h2s::fast_supported(k.tonemap)) return false;
  if (c->lp_exact && k.pipe == h2s::PIPE_LIBPLACEBO) return false;
  // the LUT off runs on the tile kernel for the libplacebo branch only (the
  // CPU chain's legacy closed form stays on the generic kernel)
  if (!k.lut_enabled && k.pipe != h2s::PIPE_LIBPLACEBO) return false;
  // the CPU chain forms lattice byte offsets in float32 (exact to N = 177);
  // the libplacebo branch reads its 8-bit table, any N
  if (k.lut_enabled && c->lut_n > 177 && !k.rgba8) return false;
  if (k.lut_in16) return false;
  // BICUBIC: the tile kernel runs pass 1 frame by frame (not under dynamic peak detection)
  if (p.chroma_filter == H2S_CHROMA_BICUBIC && p.peak_detect) return false;
  return true;
}

static int choose_path(const h2s_ctx* c, const KParams& k, const h2s_frames* din, const h2s_frames* dout,
                       bool out8, Format in_fmt, Format out_fmt) {
  const int tw = h2s::TBW;
  if (fast_params_ok(c, k) && tile_ok(din, dout, out8, tw, in_fmt, out_fmt))
    return (din->width & (tw - 1)) ? H2S_PATH_TILE_TAIL : H2S_PATH_TILE;
  return c->params.chroma_filter == H2S_CHROMA_BICUBIC ? H2S_PATH_TWO_PASS : H2S_PATH_GENERIC;
}

// what a 4:2:2 / 4:4:4 input set (h2s_set_input_subsampling) does not run
// with: each is refused, none is routed to something else.  k: resolved
static int check_subsampling(h2s_ctx* c, const KParams& k, Format in_fmt) {
  if (in_fmt.sub == H2S_SUB_420) return 0;
  if (in_fmt.semi())
    return fail(c, H2S_E_UNSUPPORTED, "4:2:2 / 4:4:4 input is planar only (semi-planar p210 / p410 input is not supported)");
  if (k.pipe == h2s::PIPE_LIBPLACEBO)
    return fail(c, H2S_E_UNSUPPORTED,
                "4:2:2 / 4:4:4 input runs on the CPU chain only: the libplacebo pipeline (and its peak detection) "
                "uploads 4:2:0 (format=p010)");
  if (c->params.peak_detect && (k.tonemap == H2S_TM_BT2390 || k.tonemap == H2S_TM_SPLINE))
    return fail(c, H2S_E_UNSUPPORTED, "4:2:2 / 4:4:4 input: peak detection reads 4:2:0 input only");
  return 0;
}

static int ensure_chr(h2s_ctx* c, const KParams& k) {
  // whole 32-row tiles: k_tile writes the rows of its bottom tile past H
  const size_t need = (size_t)k.W * (size_t)((k.H + h2s::TBH - 1) / h2s::TBH * h2s::TBH);
  return c->d_chr.reserve(c, need * sizeof(float2), "bicubic chroma scratch");
}

// libplacebo-style detected peak (PARITY UNPINNED; model in DESIGN.md §4.6),
// all on the device (h2s_peak.h): k_peak_stats* (per-block partials and the
// percentile histograms) -> k_peak_frame (per-frame statistic) ->
// k_peak_curves (the IIR in frame order from the context's device state, and
// one curve record per frame) -> the conversion, which reads the records.
// h2s_process queues all of it on the caller's stream and returns; the state
// comes back to the host only on demand (h2s_peak_state).
static h2s::PeakModel peak_model(const h2s_ctx* c, const KParams& k) {
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

static int ensure_peak_state(h2s_ctx* c) {
  bool grew = false;
  int rc = c->d_pk.reserve(c, 2 * sizeof(h2s::PeakState), "peak state", &grew);
  if (rc || !grew) return rc;
  hipStream_t aux;
  if ((rc = aux_stream(c, &aux))) return rc;
  hipError_t e = hipMemsetAsync(c->d_pk, 0, 2 * sizeof(h2s::PeakState), aux);
  if (e == hipSuccess) e = hipStreamSynchronize(aux);
  return e == hipSuccess ? 0 : hip_fail(c, e, "peak state reset");
}

// the statistics, the curves and the state are one context's scratch
// (c->peak_use): a call on another stream waits (on the device) for the
// previous call's use of them, so consecutive calls see the state in call order
static int peak_order(h2s_ctx* c, hipStream_t s) { return c->peak_use.wait(c, s, "peak ordering"); }

static int peak_done(h2s_ctx* c, hipStream_t s) { return c->peak_use.mark(c, s, "peak event"); }

// per-frame statistic (PQ peak measurement, average PQ) of the batch k binds
// into c->d_fstat, queued on s as two launches (k_peak_stats*, then
// k_peak_finish: one block per frame folds its records; the last one, st set,
// runs the IIR from *st and writes the curve records to out).  d_stats holds,
// for stats_nf frames: partial records | histograms | the finish counter; the
// histograms and the counter are zero between launches (cleared at
// allocation, left zero by the kernels)
static int frame_stats(h2s_ctx* c, const KParams& k, hipStream_t s, h2s::PeakState* st, h2s::CurveConsts* out,
                       int f0 = 0) {
  const h2s::PeakModel m = peak_model(c, k);
  const int nframes = k.nframes;
  if (nframes > c->stats_nf) {
    const size_t nf = (size_t)nframes;
    const size_t part = nf * h2s::PEAK_BLOCKS_MAX * sizeof(float2), zero = (nf * h2s::PEAK_BINS + 1) * sizeof(unsigned);
    c->stats_nf = 0;
    if (int rc = c->d_stats.reserve(c, part + zero, "peak statistics")) return rc;
    hipError_t e = hipMemsetAsync(c->d_stats + nf * h2s::PEAK_BLOCKS_MAX, 0, zero, s);
    if (e != hipSuccess) return hip_fail(c, e, "peak statistics clear");
    c->stats_nf = nframes;
  }
  if (int rc = c->d_fstat.reserve(c, (size_t)(f0 + nframes) * sizeof(double2), "peak statistics")) return rc;
  const size_t nf = (size_t)c->stats_nf;
  float2* d_part = c->d_stats;
  h2s::PeakTail T;
  T.M = m;
  T.fstat = c->d_fstat + f0;
  T.hist = reinterpret_cast<unsigned*>(d_part + nf * h2s::PEAK_BLOCKS_MAX);
  T.done = T.hist + nf * h2s::PEAK_BINS;
  T.st = st;
  T.out = out;
  T.nframes = nframes;
  T.form = c->peak_form;
  hipError_t e = h2s::launch_peak_stats(k, d_part, T, s);
  return e == hipSuccess ? 0 : hip_fail(c, e, "peak statistics");
}

static int peak_streams(h2s_ctx* c, int nev) {
  for (Stream& ps : c->pk_s)
    if (int rc = ps.get(c, "peak stream")) return rc;
  if ((int)c->pk_ev.size() < nev) c->pk_ev.resize(nev);
  for (Event& ev : c->pk_ev)
    if (int rc = ev.get(c, "peak event")) return rc;
  return 0;
}

// The pipelined schedule (tile kernel, whole tiles): the statistics of chunk
// j + 1 run on their own stream while chunk j converts, and consecutive
// chunks convert on alternating streams, so that neither a chunk boundary
// nor the statistics leave the chip idle.  The state still advances frame by
// frame in order (the statistics stream is serial), exactly as one launch.
static int run_dynamic_peak_chunked(h2s_ctx* c, const KParams& k, const Route& r) {
  const int nframes = k.nframes, C = c->peak_chunk, nch = (nframes + C - 1) / C;
  hipStream_t s = r.s;
  int rc;
  // every allocation before the first launch (hipFree of a grown buffer
  // would wait for the device)
  if ((rc = peak_streams(c, nch + 2)) || (rc = c->d_fstat.reserve(c, (size_t)nframes * sizeof(double2), "peak statistics")))
    return rc;
  hipStream_t ss = c->pk_s[0].s, st[2] = {s, c->pk_s[1].s};
  hipEvent_t ev_start = c->pk_ev[0].ev, ev_end = c->pk_ev[1].ev;
  hipError_t e = hipEventRecord(ev_start, s);
  if (e == hipSuccess) e = hipStreamWaitEvent(ss, ev_start, 0);
  if (e == hipSuccess) e = hipStreamWaitEvent(st[1], ev_start, 0);
  if (e != hipSuccess) return hip_fail(c, e, "peak schedule");
  // an error exit still joins what was queued on the two internal streams
  // into s (best effort), so the caller's stream (and queued_exit's launch
  // event) covers all of it
  auto fail_joined = [&](int code) {
    if (hipEventRecord(ev_end, st[1]) == hipSuccess) (void)hipStreamWaitEvent(s, ev_end, 0);
    if (hipEventRecord(ev_start, ss) == hipSuccess) (void)hipStreamWaitEvent(s, ev_start, 0);
    return code;
  };
  for (int j = 0; j < nch; j++) {
    const int f0 = j * C, n = std::min(C, nframes - f0);
    const KParams kj = frame_range(k, f0, n);
    if ((rc = frame_stats(c, kj, ss, c->d_pk, c->d_curve + f0, f0))) return fail_joined(rc);
    hipEvent_t ev = c->pk_ev[2 + j].ev;
    if ((e = hipEventRecord(ev, ss)) != hipSuccess || (e = hipStreamWaitEvent(st[j & 1], ev, 0)) != hipSuccess)
      return fail_joined(hip_fail(c, e, "peak schedule"));
    TileOpts curves;
    curves.cv_frames = c->d_curve + f0;
    if ((e = launch_tiles(c, kj, r.on(st[j & 1]), curves)) != hipSuccess)
      return fail_joined(hip_fail(c, e, "kernel launch"));
  }
  // s joins the statistics stream (the state) and the second conversion stream
  if ((e = hipEventRecord(ev_end, st[1])) != hipSuccess || (e = hipStreamWaitEvent(s, ev_end, 0)) != hipSuccess ||
      (e = hipStreamWaitEvent(s, c->pk_ev[2 + nch - 1].ev, 0)) != hipSuccess)
    return fail_joined(hip_fail(c, e, "peak schedule"));
  return peak_done(c, s);
}

// statistics, then the frames in order, each with the BT.2390 / spline
// constants of its smoothed peak.  The fast kernel takes every frame's curve
// in one launch (a record per frame, selected by the tile's frame index), so
// the chip stays full; the generic kernel and the ragged tail columns go frame
// by frame, each launch reading its frame's record.
static int run_dynamic_peak(h2s_ctx* c, const KParams& k, const Route& r) {
  const int nframes = k.nframes;
  hipStream_t s = r.s;
  int rc;
  if ((rc = ensure_peak_state(c)) || (rc = peak_order(c, s))) return rc;
  if ((rc = c->d_curve.reserve(c, (size_t)nframes * sizeof(h2s::CurveConsts), "curve records"))) return rc;
  if (r.path == H2S_PATH_TILE && c->peak_chunk > 0 && nframes > c->peak_chunk) return run_dynamic_peak_chunked(c, k, r);
  if ((rc = frame_stats(c, k, s, c->d_pk, c->d_curve))) return rc;
  hipError_t e;
  if (r.tile()) {
    TileOpts curves;
    curves.cv_frames = c->d_curve;
    if ((e = launch_tiles(c, k, r, curves)) != hipSuccess) return hip_fail(c, e, "kernel launch");
  }
  if (r.path != H2S_PATH_TILE) {
    for (int f = 0; f < nframes; f++) {
      KParams kf = frame_range(k, f, 1);
      kf.cv = c->d_curve + f;
      e = r.tile() ? launch_columns(kf, r, COLUMNS_RAGGED) : launch_route(c, kf, r);
      if (e != hipSuccess) return hip_fail(c, e, "kernel launch");
    }
  }
  return peak_done(c, s);
}

// the host-side peak calls act on the state as the context's queued work
// leaves it: they wait for that work first (its launch events and the last
// peak launch), then run on the context stream and wait for it
static int peak_sync(h2s_ctx* c, hipStream_t* aux) {
  int rc;
  if ((rc = drain_launches(c)) || (rc = ensure_peak_state(c)) || (rc = aux_stream(c, aux))) return rc;
  return c->peak_use.sync_host(c, "peak launches");
}

int h2s_peak_reset(h2s_ctx* c) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  DeviceGuard g(c->device);
  hipStream_t aux;
  if (int rc = peak_sync(c, &aux)) return rc;
  hipError_t e = hipMemsetAsync(c->d_pk, 0, sizeof(h2s::PeakState), aux);
  if (e == hipSuccess) e = hipStreamSynchronize(aux);
  return e == hipSuccess ? 0 : hip_fail(c, e, "peak state reset");
}

int h2s_peak_feed(h2s_ctx* c, const double* fmax, const double* favg, int n) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (n < 0 || (n > 0 && (!fmax || !favg))) return fail(c, H2S_E_INVALID_ARG, "bad statistics arrays");
  KParams k;
  int rc = prepare(c, &k, false);  // the statistics need no LUT
  if (rc) return rc;
  if (n == 0) return 0;
  DeviceGuard g(c->device);
  hipStream_t aux;
  if ((rc = peak_sync(c, &aux))) return rc;
  if ((rc = c->d_fstat.reserve(c, (size_t)n * sizeof(double2), "peak statistics"))) return rc;
  std::vector<double2> st(n);
  for (int i = 0; i < n; i++) st[i] = make_double2(fmax[i], favg[i]);
  // the same device IIR as h2s_process (bit-identical state either way)
  hipError_t e = hipMemcpyAsync(c->d_fstat, st.data(), n * sizeof(double2), hipMemcpyHostToDevice, aux);
  if (e == hipSuccess) e = h2s::launch_peak_curves(c->d_fstat, n, peak_model(c, k), c->d_pk, nullptr, aux);
  if (e == hipSuccess) e = hipStreamSynchronize(aux);
  return e == hipSuccess ? 0 : hip_fail(c, e, "peak feed");
}

int h2s_peak_state(const h2s_ctx* cc, double* max_pq, double* avg_pq, double* peak, int64_t* frames) {
  if (!cc) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  // logically const: waits for the context's queued work, copies the state back
  h2s_ctx* c = const_cast<h2s_ctx*>(cc);
  DeviceGuard g(c->device);
  hipStream_t aux;
  if (int rc = peak_sync(c, &aux)) return rc;
  h2s::PeakState st;
  hipError_t e = hipMemcpyAsync(&st, c->d_pk, sizeof(st), hipMemcpyDeviceToHost, aux);
  if (e == hipSuccess) e = hipStreamSynchronize(aux);
  if (e != hipSuccess) return hip_fail(c, e, "peak state read-back");
  if (max_pq) *max_pq = st.max;
  if (avg_pq) *avg_pq = st.avg;
  if (peak) *peak = st.peak;
  if (frames) *frames = st.frames;
  return 0;
}

int h2s_peak_stats(h2s_ctx* c, const h2s_frames* in, int nframes, double* fmax, double* favg, void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (nframes < 0 || (nframes > 0 && (!fmax || !favg))) return fail(c, H2S_E_INVALID_ARG, "bad statistics arrays");
  KParams k;
  int rc = prepare(c, &k, false);  // the statistics need no LUT
  if (rc) return rc;
  if (c->in_fmt.sub != H2S_SUB_420)
    return fail(c, H2S_E_UNSUPPORTED, "h2s_peak_stats reads 4:2:0 input only (h2s_set_input_subsampling is 4:2:2 / 4:4:4)");
  if ((rc = check_frames(c, in, c->params.bits_in, "input", c->in_fmt))) return rc;
  if (in->location != H2S_LOC_DEVICE) return fail(c, H2S_E_INVALID_ARG, "h2s_peak_stats takes device frames");
  if (nframes == 0) return 0;
  DeviceGuard g(c->device);
  hipStream_t s = (hipStream_t)hip_stream;
  h2s_frames out = *in;                       // geometry only: the statistics read the input planes
  fill_geometry(&k, in, &out, nframes, c->in_fmt, PLANAR_420);
  if ((rc = peak_order(c, s)) || (rc = frame_stats(c, k, s, nullptr, nullptr))) return rc;
  std::vector<double2> st(nframes);
  hipError_t e = hipMemcpyAsync(st.data(), c->d_fstat, nframes * sizeof(double2), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(c, e, "peak statistics read-back");
  for (int f = 0; f < nframes; f++) fmax[f] = st[f].x, favg[f] = st[f].y;
  return 0;
}

// frames [start, ...) of a batch
static h2s_frames frames_at(const h2s_frames* f, int start) {
  h2s_frames t = *f;
  for (int p = 0; p < 3; p++) t.data[p] = (uint8_t*)f->data[p] + (long long)start * f->frame_pitch[p];
  return t;
}

// kernel timing (h2s_set_timing): one pair of the event ring around a call's
// launches on s, read back by h2s_kernel_ms
static void timing_begin(h2s_ctx* c, hipStream_t s) {
  if (!c->timing) return;
  Event &e0 = c->ev0[c->ev_count % kEvRing], &e1 = c->ev1[c->ev_count % kEvRing];
  (void)e0.get(c, "timing event", hipEventDefault);
  (void)e1.get(c, "timing event", hipEventDefault);
  hipEventRecord(e0.ev, s);
}

static void timing_end(h2s_ctx* c, hipStream_t s) {
  if (!c->timing) return;
  hipEventRecord(c->ev1[c->ev_count % kEvRing].ev, s);
  c->ev_count++;
}

// Host frames in and/or out: the batch is cut into up to kMaxChunks chunks of
// whole frames; chunk i's H2D copy, kernel and D2H copy run on three streams
// so that copies of neighbouring chunks overlap the kernel and each other.
// Staging holds the whole batch (no buffer reuse, so no WAR hazards); all
// three streams start after the work already queued on `s`, and `s` waits
// for them before the call returns. din/dout: staged (or caller's device)
// descriptors for frame 0; k binds the whole batch (k.nframes frames of them).
static int process_pipelined(h2s_ctx* c, KParams k, const h2s_frames* in, const h2s_frames* out,
                             const h2s_frames& din, const h2s_frames& dout, const Route& r, bool dyn_peak) {
  const int nframes = k.nframes;
  hipStream_t s = r.s;
  const bool host_in = in->location == H2S_LOC_HOST, host_out = out->location == H2S_LOC_HOST;
  for (Stream& ps : c->ps)
    if (int rc = ps.get(c, "pipeline stream")) return rc;
  for (Event& ev : c->pev)
    if (int rc = ev.get(c, "pipeline event")) return rc;
  hipStream_t s_in = c->ps[0].s, s_cmp = c->ps[1].s, s_out = c->ps[2].s;
  auto sync_all = [&] {
    for (Stream& ps : c->ps) hipStreamSynchronize(ps.s);
  };
  const int per = (nframes + kMaxChunks - 1) / kMaxChunks, nch = (nframes + per - 1) / per;
  hipEvent_t ev_start = c->pev[2 * kMaxChunks].ev, ev_done = c->pev[2 * kMaxChunks + 1].ev;
  hipError_t e = hipEventRecord(ev_start, s);
  for (Stream& ps : c->ps)
    if (e == hipSuccess) e = hipStreamWaitEvent(ps.s, ev_start, 0);
  if (e != hipSuccess) return hip_fail(c, e, "pipeline ordering");
  const char* what = nullptr;
  for (int i = 0; i < nch && !what; i++) {
    const int f0 = i * per, nf = nframes - f0 < per ? nframes - f0 : per;
    const h2s_frames ci = frames_at(&din, f0), co = frames_at(&dout, f0);
    if (host_in) {
      const h2s_frames hi = frames_at(in, f0);
      if ((e = copy_frames(&ci, &hi, nf, s_in, r.in_fmt)) != hipSuccess) what = "host->device copy";
      else if ((e = hipEventRecord(c->pev[i].ev, s_in)) != hipSuccess) what = "pipeline event";
      else if ((e = hipStreamWaitEvent(s_cmp, c->pev[i].ev, 0)) != hipSuccess) what = "pipeline ordering";
      if (what) break;
    }
    if (i == 0) timing_begin(c, s_cmp);
    fill_geometry(&k, &ci, &co, nf, r.in_fmt, r.out_fmt);
    if (dyn_peak) {
      if (int rc = run_dynamic_peak(c, k, r.on(s_cmp))) {
        sync_all();
        return rc;
      }
    } else if ((e = launch_route(c, k, r.on(s_cmp))) != hipSuccess) {
      what = "kernel launch";
    }
    if (!what && host_out) {
      const h2s_frames ho = frames_at(out, f0);
      if ((e = hipEventRecord(c->pev[kMaxChunks + i].ev, s_cmp)) != hipSuccess) what = "pipeline event";
      else if ((e = hipStreamWaitEvent(s_out, c->pev[kMaxChunks + i].ev, 0)) != hipSuccess) what = "pipeline ordering";
      else if ((e = copy_frames(&ho, &co, nf, s_out, r.out_fmt)) != hipSuccess) what = "device->host copy";
    }
  }
  if (what) {  // drain whatever was queued before returning the caller's buffers
    sync_all();
    return hip_fail(c, e, what);
  }
  timing_end(c, s_cmp);
  // s waits for the last stream of the chain (D2H if any, else compute)
  if ((e = hipEventRecord(ev_done, host_out ? s_out : s_cmp)) == hipSuccess) e = hipStreamWaitEvent(s, ev_done, 0);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    sync_all();
    return hip_fail(c, e, "stream synchronize");
  }
  return 0;
}

// h2s_process for the two layouts given (the context's own for its callers'
// sets; a preview's chain output is planar whatever the context's is).
// Nothing it calls reads c->in_fmt / c->out_fmt
static int process_frames(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, int nframes, hipStream_t s,
                          Format in_fmt, Format out_fmt) {
  if (nframes < 0) return fail(c, H2S_E_INVALID_ARG, "nframes < 0");
  KParams k;
  int rc = prepare(c, &k);
  if (rc) return rc;
  if ((rc = check_subsampling(c, k, in_fmt))) return rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", in_fmt))) return rc;
  if ((rc = check_frames(c, out, c->params.bits_out, "output", out_fmt))) return rc;
  if (in->width != out->width || in->height != out->height)
    return fail(c, H2S_E_INVALID_ARG, "input and output frame sizes differ");
  if (nframes == 0) return 0;
  DeviceGuard g(c->device);
  const bool out8 = c->params.bits_out == 8;

  // host sets are staged: input, then (256-byte aligned) output
  const bool host_in = in->location == H2S_LOC_HOST, host_out = out->location == H2S_LOC_HOST;
  const size_t ib = host_in ? (frame_bytes(in, in_fmt) * nframes + 255) / 256 * 256 : 0;
  const size_t ob = host_out ? frame_bytes(out, out_fmt) * nframes : 0;
  if ((host_in || host_out) && (rc = c->d_stage.reserve(c, ib + ob, "staging"))) return rc;
  const h2s_frames din = device_view(in, c->d_stage, in_fmt), dout = device_view(out, c->d_stage + ib, out_fmt);
  fill_geometry(&k, &din, &dout, nframes, in_fmt, out_fmt);
  // fast path: the tile kernel over whole 64 x 32 tiles; the generic kernel
  // covers the rest (choose_path / fast_params_ok) and the ragged columns
  const Route r{choose_path(c, k, &din, &dout, out8, in_fmt, out_fmt),
                vec_ok(&din, false, in_fmt) && vec_ok(&dout, out8, out_fmt), out8, in_fmt, out_fmt, s};
  if (r.tile() && k.lut_enabled && (rc = ensure_lut_yuv(c, k, s))) return rc;
  // BICUBIC chroma (generic two-pass, or k_tile pass 1) uses the context scratch
  const bool two_pass = c->params.chroma_filter == H2S_CHROMA_BICUBIC;
  if (two_pass) {
    if ((rc = ensure_chr(c, k))) return rc;
    // one context scratch (d_chr) for every two-pass launch: a launch on
    // another stream waits until the previous one has finished with it
    if ((rc = c->chr_use.wait(c, s, "two-pass ordering"))) return rc;
  }
  const bool dyn_peak = c->params.peak_detect &&
                        (k.tonemap == H2S_TM_BT2390 || k.tonemap == H2S_TM_SPLINE || k.pipe == h2s::PIPE_LIBPLACEBO);
  // host frames: the chunk pipeline, with the dynamic peak too (its
  // statistics, IIR and curve records run on the device, stream-ordered per
  // chunk on the compute stream, so the state still advances frame by frame)
  if ((host_in || host_out) && nframes > 1 && !c->serial_host)
    return process_pipelined(c, k, in, out, din, dout, r, dyn_peak);
  if (host_in) {
    hipError_t e = copy_frames(&din, in, nframes, s, in_fmt);
    if (e != hipSuccess) return queued_exit(c, s, hip_fail(c, e, "host->device copy"));
  }
  timing_begin(c, s);
  hipError_t e;
  if (dyn_peak) {
    if ((rc = run_dynamic_peak(c, k, r))) return queued_exit(c, s, rc);
    e = hipSuccess;
  } else {
    e = launch_route(c, k, r);
  }
  if (e == hipSuccess && c->fail_after_launch) {
    c->fail_after_launch = false;
    return queued_exit(c, s, fail(c, H2S_E_HIP, "injected failure after the launch (H2S_OPT_TEST_FAIL_AFTER_LAUNCH)"));
  }
  if (e != hipSuccess) return queued_exit(c, s, hip_fail(c, e, "kernel launch"));
  timing_end(c, s);
  if (host_out) {
    e = copy_frames(out, &dout, nframes, s, out_fmt);
    if (e != hipSuccess) return queued_exit(c, s, hip_fail(c, e, "device->host copy"));
  }
  if (two_pass && (rc = c->chr_use.mark(c, s, "two-pass event"))) return queued_exit(c, s, rc);
  if (host_in || host_out) {
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return queued_exit(c, s, hip_fail(c, e, "stream synchronize"));
    return 0;
  }
  return note_launch(c, s);
}

int h2s_process(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, int nframes, void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  return process_frames(c, in, out, nframes, (hipStream_t)hip_stream, c->in_fmt, c->out_fmt);
}

int h2s_debug_float(h2s_ctx* c, const h2s_frames* in, int stage, float* out_rgb, int out_location,
                    void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (stage < H2S_STAGE_LINEAR || stage > H2S_STAGE_YUV) return fail(c, H2S_E_INVALID_ARG, "bad stage");
  if (!out_rgb) return fail(c, H2S_E_INVALID_ARG, "out_rgb is NULL");
  KParams k;
  int rc = prepare(c, &k);
  if (rc) return rc;
  if ((rc = check_subsampling(c, k, c->in_fmt))) return rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", c->in_fmt))) return rc;
  DeviceGuard g(c->device);
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t npx = (size_t)in->width * in->height, ob = npx * 3 * sizeof(float);
  // scratch: a tight device copy of the input (host input), the float planes
  // (host output) and one output frame for the tile kernel's own stores
  h2s_frames fo{};
  fo.width = in->width, fo.height = in->height, fo.bits = c->params.bits_out, fo.location = H2S_LOC_DEVICE;
  const size_t ib = in->location == H2S_LOC_HOST ? (frame_bytes(in, c->in_fmt) + 255) / 256 * 256 : 0;
  const size_t fb = (frame_bytes(&fo, PLANAR_420) + 255) / 256 * 256, pb = out_location == H2S_LOC_HOST ? ob : 0;
  Dev<uint8_t> scratch;  // freed on every exit, after s has been waited for
  if ((rc = scratch.reserve(c, ib + fb + pb + 256, "debug"))) return rc;
  uint8_t* base = scratch;
  const h2s_frames din = device_view(in, base, c->in_fmt);
  hipError_t e;
  if (in->location == H2S_LOC_HOST && (e = copy_frames(&din, in, 1, s, c->in_fmt)) != hipSuccess)
    return hip_fail(c, e, "debug copy");
  fo = tight(&fo, base + ib, PLANAR_420);   // (the call's own planar scratch frame)
  float* dout = out_location == H2S_LOC_HOST ? (float*)(base + ib + fb) : out_rgb;
  fill_geometry(&k, &din, &fo, 1, c->in_fmt, PLANAR_420);
  const bool out8 = c->params.bits_out == 8;
  const Route r{choose_path(c, k, &din, &fo, out8, c->in_fmt, PLANAR_420), false, out8, c->in_fmt, PLANAR_420, s};
  // the generic debug kernel covers every pixel; on the tile path the tile
  // kernel's debug instance then rewrites the tile columns with its own values
  // (4:2:0 input: there are no debug instances of the tile kernel for 4:2:2 /
  // 4:4:4 input or for a top-left set, whose planes are the generic kernel's
  // whatever the path; a full-range set changes constants only)
  e = h2s::launch_debug(k, stage, dout, s);
  if (e == hipSuccess && r.tile() && c->in_fmt.sub == H2S_SUB_420 && !c->in_fmt.vco()) {
    if (k.lut_enabled && (rc = ensure_lut_yuv(c, k, s))) {
      hipStreamSynchronize(s);
      return rc;
    }
    TileOpts debug;
    debug.dbg = stage, debug.dbg_out = dout;
    e = launch_tiles(c, k, r, debug);
  }
  if (e == hipSuccess && out_location == H2S_LOC_HOST) e = hipMemcpyAsync(out_rgb, dout, ob, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(c, e, "debug kernel");
  return 0;
}

int h2s_set_option(h2s_ctx* c, int key, int64_t value) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  switch (key) {
    case H2S_OPT_FAST_PATH:
      c->fast_enabled = value != 0;
      return 0;
    case H2S_OPT_TILES_PER_BLOCK:
      if (value < 1 || value > 64) return fail(c, H2S_E_INVALID_ARG, "tiles per block must be in [1, 64]");
      c->tiles_per_block = (int)value;
      return 0;
    case H2S_OPT_HOST_SERIAL:
      c->serial_host = value != 0;
      return 0;
    case H2S_OPT_LP_EXACT:
      c->lp_exact = value != 0;
      return 0;
    case 4:   // reserved: H2S_OPT_LP_EXACT's key in ABI 3.3
      return fail(c, H2S_E_INVALID_ARG, "option 4 is reserved (H2S_OPT_LP_EXACT is option 5 since ABI 3.4)");
    case H2S_OPT_TEST_FAIL_AFTER_LAUNCH:
      c->fail_after_launch = value != 0;
      return 0;
    case H2S_OPT_TEST_PEAK_FORM:
      c->peak_form = (int)value;
      return 0;
    case H2S_OPT_TEST_PEAK_BLOCKS:
      if (value < 1 || value > h2s::PEAK_BLOCKS_MAX) return fail(c, H2S_E_INVALID_ARG, "peak blocks must be in [1, 256]");
      c->peak_blocks = (int)value;
      return 0;
    case H2S_OPT_TEST_PEAK_CHUNK:
      if (value < 0 || value > 4096) return fail(c, H2S_E_INVALID_ARG, "peak chunk must be in [0, 4096]");
      c->peak_chunk = (int)value;
      return 0;
    default:
      return fail(c, H2S_E_INVALID_ARG, "unknown option");
  }
}

int h2s_set_frame_layout(h2s_ctx* c, int in_layout, int out_layout) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  auto known = [](int l) { return l == H2S_LAYOUT_PLANAR || l == H2S_LAYOUT_SEMI; };
  if (!known(in_layout) || !known(out_layout)) return fail(c, H2S_E_INVALID_ARG, "unknown frame layout");
  // (only the arguments of later launches change: nothing queued reads these)
  c->in_fmt.layout = in_layout, c->out_fmt.layout = out_layout;
  return 0;
}

int h2s_set_input_subsampling(h2s_ctx* c, int subsampling) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (subsampling != H2S_SUB_420 && subsampling != H2S_SUB_422 && subsampling != H2S_SUB_444)
    return fail(c, H2S_E_INVALID_ARG, "unknown chroma subsampling");
  // (only the arguments of later launches change: nothing queued reads this)
  c->in_fmt.sub = subsampling;
  return 0;
}

int h2s_set_input_tags(h2s_ctx* c, int range, int chroma_location) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (range != H2S_RANGE_LIMITED && range != H2S_RANGE_FULL) return fail(c, H2S_E_INVALID_ARG, "unknown colour range");
  if (chroma_location != H2S_CHROMA_LEFT && chroma_location != H2S_CHROMA_TOPLEFT)
    return fail(c, H2S_E_INVALID_ARG, "unknown chroma location (left and topleft are modelled)");
  // (only the arguments of later launches change: nothing queued reads these)
  c->in_fmt.range = range, c->in_fmt.loc = chroma_location;
  return 0;
}

int h2s_query_path(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  KParams k;
  int rc = prepare(c, &k);
  if (rc) return rc;
  if ((rc = check_subsampling(c, k, c->in_fmt))) return rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", c->in_fmt))) return rc;
  if ((rc = check_frames(c, out, c->params.bits_out, "output", c->out_fmt))) return rc;
  // host sets are staged into tight device copies, whose alignment decides
  uint8_t* fake = (uint8_t*)(uintptr_t)4096;
  const h2s_frames din = device_view(in, fake, c->in_fmt), dout = device_view(out, fake, c->out_fmt);
  fill_geometry(&k, &din, &dout, 1, c->in_fmt, c->out_fmt);
  return choose_path(c, k, &din, &dout, c->params.bits_out == 8, c->in_fmt, c->out_fmt);
}

// ---- preview ---------------------------------------------------------------

int h2s_preview_size(int in_w, int in_h, int box_w, int box_h, int* out_w, int* out_h) {
  if (in_w <= 0 || in_h <= 0 || box_w <= 0 || box_h <= 0 || !out_w || !out_h)
    return fail(nullptr, H2S_E_INVALID_ARG, "preview sizes must be positive");
  // libavfilter scale_eval: av_rescale (round half away from zero) of the
  // box by the input aspect, then min with the box (decrease)
  auto rescale = [](long long a, long long b, long long c) { return (a * b + c / 2) / c; };
  const long long tw = rescale(box_h, in_w, in_h), th = rescale(box_w, in_h, in_w);
  *out_w = (int)(tw < box_w ? tw : box_w);
  *out_h = (int)(th < box_h ? th : box_h);
  if (*out_w < 1) *out_w = 1;
  if (*out_h < 1) *out_h = 1;
  return 0;
}

namespace {
// swscale SWS_BICUBIC with its default parameters B = 0, C = 0.6
double bicubic(double x) {
  const double B = 0.0, C = 0.6;
  x = fabs(x);
  if (x < 1.0) return ((12 - 9 * B - 6 * C) * x * x * x + (-18 + 12 * B + 6 * C) * x * x + (6 - 2 * B)) / 6.0;
  if (x < 2.0) return ((-B - 6 * C) * x * x * x + (6 * B + 30 * C) * x * x + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) / 6.0;
  return 0.0;
}

// per output index: first source tap and T normalised weights (centre-aligned
// sampling; the kernel widens by the ratio when downscaling)
int resize_taps(int src, int dst, std::vector<float>* w, std::vector<int>* start) {
  const double scale = (double)src / dst, fw = scale > 1.0 ? scale : 1.0;
  const int T = (int)ceil(4.0 * fw) + 1;
  w->assign((size_t)dst * T, 0.0f);
  start->assign(dst, 0);
  for (int o = 0; o < dst; o++) {
    const double c = (o + 0.5) * scale - 0.5;
    const int s0 = (int)floor(c - 2.0 * fw) + 1;
    // (T <= 49 at the ratio limit of 12; a 4:4:4 source pane's chroma columns reach 24, T = 97)
    double sum = 0.0, tmp[128];
    for (int i = 0; i < T && i < 128; i++) sum += (tmp[i] = bicubic((s0 + i - c) / fw));
    for (int i = 0; i < T && i < 128; i++) (*w)[(size_t)o * T + i] = (float)(tmp[i] / sum);
    (*start)[o] = s0;
  }
  return T;
}
}  // namespace

int h2s_preview_rgb24_batch(h2s_ctx* c, const h2s_frames* in, int nframes, uint8_t* rgb, int64_t rgb_linesize,
                            int64_t rgb_frame_pitch, int out_w, int out_h, double display_gamma, int rgb_location,
                            void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (nframes < 1) return fail(c, H2S_E_INVALID_ARG, "nframes must be >= 1");
  if (!rgb || out_w <= 0 || out_h <= 0 || rgb_linesize < 3LL * out_w ||
      (nframes > 1 && rgb_frame_pitch < rgb_linesize * out_h))
    return fail(c, H2S_E_INVALID_ARG, "bad RGB output geometry");
  if (!(display_gamma > 0.0)) return fail(c, H2S_E_INVALID_ARG, "display gamma must be > 0");
  if (!c->params_set) return fail(c, H2S_E_INVALID_ARG, "h2s_set_params was not called");
  if (c->params.bits_out != 8)
    return fail(c, H2S_E_INVALID_ARG, "preview needs params.bits_out == 8 (the chain's yuv420p)");
  int rc = check_frames(c, in, c->params.bits_in, "input", c->in_fmt);
  if (rc) return rc;
  const int W = in->width, H = in->height;
  const bool scale = out_w != W || out_h != H;
  if (scale && (out_w > 4 * 8192 || out_h > 4 * 8192 || (double)W / out_w > 12.0 || (double)H / out_h > 12.0))
    return fail(c, H2S_E_UNSUPPORTED, "preview resize ratio out of range");
  DeviceGuard g(c->device);
  hipStream_t s = (hipStream_t)hip_stream;
  // scratch: chain output (yuv420p), resized planes, tap tables, RGB, gamma LUT
  const int ow2 = (out_w + 1) / 2, oh2 = (out_h + 1) / 2;
  std::vector<float> wx, wy, wcx, wcy;
  std::vector<int> sx, sy, scx, scy;
  int T = 0, Tc = 0;
  if (scale) {
    T = resize_taps(W, out_w, &wx, &sx);
    const int Ty = resize_taps(H, out_h, &wy, &sy);
    Tc = resize_taps(W / 2, ow2, &wcx, &scx);
    const int Tcy = resize_taps(H / 2, oh2, &wcy, &scy);
    if (Ty != T || Tcy != Tc) {  // one T per plane: recompute on the wider support
      const int Tm = T > Ty ? T : Ty, Tcm = Tc > Tcy ? Tc : Tcy;
      auto widen = [](std::vector<float>* w, int n, int t, int tn) {
        std::vector<float> o((size_t)n * tn, 0.0f);
        for (int i = 0; i < n; i++)
          for (int k = 0; k < t; k++) o[(size_t)i * tn + k] = (*w)[(size_t)i * t + k];
        *w = o;
      };
      if (T < Tm) widen(&wx, out_w, T, Tm);
      if (Ty < Tm) widen(&wy, out_h, Ty, Tm);
      if (Tc < Tcm) widen(&wcx, ow2, Tc, Tcm);
      if (Tcy < Tcm) widen(&wcy, oh2, Tcy, Tcm);
      T = Tm, Tc = Tcm;
    }
  }
  uint8_t glut[256];
  for (int i = 0; i < 256; i++) {
    // PIL point() with round() of pow(i/255, 1/gamma)*255 (round half to even)
    const double v = display_gamma == 1.0 ? (double)i : pow(i / 255.0, 1.0 / display_gamma) * 255.0;
    const double r = nearbyint(v);
    glut[i] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
  }
  auto al = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t n = (size_t)nframes;
  const size_t yfp = (size_t)W * H * 3 / 2;                             // tight yuv420p frame
  const size_t sfp = (size_t)out_w * out_h + 2 * (size_t)ow2 * oh2;    // one resized frame
  const size_t yuv_b = al(yfp * n), syuv_b = scale ? al(sfp * n) : 0;
  const size_t tab_b = scale ? al((wx.size() + wy.size() + wcx.size() + wcy.size()) * 4) +
                                   al((sx.size() + sy.size() + scx.size() + scy.size()) * 4)
                             : 0;
  const size_t rgb_b = rgb_location == H2S_LOC_HOST ? al((size_t)out_w * 3 * out_h * n) : 0;
  const size_t need = yuv_b + syuv_b + tab_b + rgb_b + 256;
  if (need > c->d_prev.cap && c->d_prev) {
    // a previous preview's kernels may still read the old scratch
    drain_launches(c);
    hipStreamSynchronize(s);
  }
  if ((rc = c->d_prev.reserve(c, need, "preview scratch"))) return rc;
  uint8_t* base = c->d_prev;
  // the chain's output here is the call's own yuv420p scratch: planar, whatever
  // layout the context writes its callers' frames in
  h2s_frames y8{};
  y8.width = W, y8.height = H, y8.bits = 8, y8.location = H2S_LOC_DEVICE;
  y8 = tight(&y8, base, PLANAR_420);
  if (c->params.peak_detect) {
    // libplacebo branch: the reference converts each preview frame in its own
    // ffmpeg run (extract_frames_with_gpu_conversion_batch loops
    // extract_frame_with_gpu_conversion, src/utils.py:803-824), so peak
    // detection starts afresh on every frame: one launch per frame, state
    // reset in between.  The context's own state (a conversion sequence the
    // caller may be in the middle of) is saved first and restored afterwards,
    // all stream-ordered on s
    if ((rc = ensure_peak_state(c)) || (rc = peak_order(c, s))) return rc;
    const size_t pb = sizeof(h2s::PeakState);
    hipError_t e = hipMemcpyAsync(c->d_pk + 1, c->d_pk, pb, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return hip_fail(c, e, "peak state save");
    // every exit after the save queues the restore first (best effort)
    auto restored = [&](int code) {
      (void)hipMemcpyAsync(c->d_pk, c->d_pk + 1, pb, hipMemcpyDeviceToDevice, s);
      (void)peak_done(c, s);
      return code;
    };
    for (int f = 0; f < nframes; f++) {
      h2s_frames fi = *in, fo = y8;
      for (int k = 0; k < 3; k++) {
        if (in->data[k]) fi.data[k] = (uint8_t*)in->data[k] + (long long)f * in->frame_pitch[k];
        fo.data[k] = (uint8_t*)y8.data[k] + (long long)f * y8.frame_pitch[k];
      }
      if ((e = hipMemsetAsync(c->d_pk, 0, pb, s)) != hipSuccess)
        return restored(queued_exit(c, s, hip_fail(c, e, "peak state reset")));
      if ((rc = process_frames(c, &fi, &fo, 1, s, c->in_fmt, PLANAR_420))) return restored(rc);
    }
    if ((e = hipMemcpyAsync(c->d_pk, c->d_pk + 1, pb, hipMemcpyDeviceToDevice, s)) != hipSuccess)
      return queued_exit(c, s, hip_fail(c, e, "peak state restore"));
    if ((rc = peak_done(c, s))) return queued_exit(c, s, rc);
  } else if ((rc = process_frames(c, in, &y8, nframes, s, c->in_fmt, PLANAR_420))) {  // one launch for the batch
    return rc;
  }
  hipError_t e = hipSuccess;
  const uint8_t *yp = (const uint8_t*)y8.data[0], *up = (const uint8_t*)y8.data[1], *vp = (const uint8_t*)y8.data[2];
  long long yls = W, cls = W / 2, fp = (long long)yfp;
  uint8_t* p = base + yuv_b;
  if (scale) {
    uint8_t* sy_ = p;
    uint8_t* su_ = p + (size_t)out_w * out_h;
    uint8_t* sv_ = su_ + (size_t)ow2 * oh2;
    uint8_t* t = p + syuv_b;
    float* dwx = (float*)t;
    float* dwy = dwx + wx.size();
    float* dwcx = dwy + wy.size();
    float* dwcy = dwcx + wcx.size();
    int* dsx = (int*)(t + al((wx.size() + wy.size() + wcx.size() + wcy.size()) * 4));
    int* dsy = dsx + sx.size();
    int* dscx = dsy + sy.size();
    int* dscy = dscx + scx.size();
    struct {
      void* d;
      const void* h;
      size_t b;
    } up_[8] = {{dwx, wx.data(), wx.size() * 4},   {dwy, wy.data(), wy.size() * 4},   {dwcx, wcx.data(), wcx.size() * 4},
                {dwcy, wcy.data(), wcy.size() * 4}, {dsx, sx.data(), sx.size() * 4},   {dsy, sy.data(), sy.size() * 4},
                {dscx, scx.data(), scx.size() * 4}, {dscy, scy.data(), scy.size() * 4}};
    for (auto& u : up_)
      if (e == hipSuccess) e = hipMemcpyAsync(u.d, u.h, u.b, hipMemcpyHostToDevice, s);
    const long long sp = (long long)sfp;
    if (e == hipSuccess)
      e = h2s::launch_resize_u8(yp, W, H, W, fp, sy_, out_w, out_h, out_w, sp, dwx, dsx, dwy, dsy, T, nframes, s);
    if (e == hipSuccess)
      e = h2s::launch_resize_u8(up, W / 2, H / 2, W / 2, fp, su_, ow2, oh2, ow2, sp, dwcx, dscx, dwcy, dscy, Tc,
                                nframes, s);
    if (e == hipSuccess)
      e = h2s::launch_resize_u8(vp, W / 2, H / 2, W / 2, fp, sv_, ow2, oh2, ow2, sp, dwcx, dscx, dwcy, dscy, Tc,
                                nframes, s);
    yp = sy_, up = su_, vp = sv_, yls = out_w, cls = ow2, fp = sp;
  }
  uint8_t* dglut = base + need - 256;
  const bool host = rgb_location == H2S_LOC_HOST;
  uint8_t* drgb = host ? base + yuv_b + syuv_b + tab_b : rgb;
  const long long drls = host ? 3LL * out_w : rgb_linesize;
  const long long drfp = host ? 3LL * out_w * out_h : rgb_frame_pitch;
  if (e == hipSuccess) e = hipMemcpyAsync(dglut, glut, 256, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = h2s::launch_yuv8_rgb24(yp, yls, up, vp, cls, fp, out_w, out_h, drgb, drls, drfp, dglut, nframes, s);
  for (int f = 0; host && f < nframes && e == hipSuccess; f++)
    e = hipMemcpy2DAsync(rgb + (long long)f * rgb_frame_pitch, rgb_linesize, drgb + f * drfp, drls, 3 * (size_t)out_w,
                         out_h, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(c, e, "preview");
  return 0;
}

int h2s_preview_rgb24(h2s_ctx* c, const h2s_frames* in, uint8_t* rgb, int64_t rgb_linesize, int out_w, int out_h,
                      double display_gamma, int rgb_location, void* hip_stream) {
  return h2s_preview_rgb24_batch(c, in, 1, rgb, rgb_linesize, rgb_linesize * (int64_t)out_h, out_w, out_h,
                                 display_gamma, rgb_location, hip_stream);
}

// The source pane (extract_frame / extract_frames_batch, src/utils.py:827-859,
// :629-665): the frames as decoded, resized and matrixed by k_source_rgb24 in
// one launch.  Of the context it reads the input Format alone: no params, LUT,
// option or peak state, and it leaves all of them as they are
int h2s_preview_source_rgb24_batch(h2s_ctx* c, const h2s_frames* in, int nframes, uint8_t* rgb, int64_t rgb_linesize,
                                   int64_t rgb_frame_pitch, int out_w, int out_h, int matrix, int rgb_model,
                                   int rgb_location, void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (nframes < 1) return fail(c, H2S_E_INVALID_ARG, "nframes must be >= 1");
  if (!rgb || out_w <= 0 || out_h <= 0 || rgb_linesize < 3LL * out_w ||
      (nframes > 1 && rgb_frame_pitch < rgb_linesize * out_h))
    return fail(c, H2S_E_INVALID_ARG, "bad RGB output geometry");
  // (Kr, Kb) of enum h2s_src_matrix
  static const double kKrKb[3][2] = {{0.2627, 0.0593}, {0.2126, 0.0722}, {0.299, 0.114}};
  if (matrix < H2S_SRC_MATRIX_BT2020NC || matrix > H2S_SRC_MATRIX_BT601)
    return fail(c, H2S_E_INVALID_ARG, "unknown source matrix");
  if (rgb_model != H2S_SRC_RGB_TRUNC16 && rgb_model != H2S_SRC_RGB_ROUND8)
    return fail(c, H2S_E_INVALID_ARG, "unknown source rgb model");
  if (!in) return fail(c, H2S_E_INVALID_ARG, "input frames is NULL");
  if (in->bits != 10 && in->bits != 12)
    return fail(c, H2S_E_INVALID_ARG, "the source pane reads 10- or 12-bit frames");
  const Format fmt = c->in_fmt;
  if (fmt.sub != H2S_SUB_420 && fmt.semi())
    return fail(c, H2S_E_UNSUPPORTED, "4:2:2 / 4:4:4 input is planar only (semi-planar p210 / p410 input is not supported)");
  int rc = check_frames(c, in, in->bits, "input", fmt);
  if (rc) return rc;
  const int W = in->width, H = in->height, bits = in->bits;
  const bool scale = out_w != W || out_h != H;
  if (scale && (out_w > 4 * 8192 || out_h > 4 * 8192 || (double)W / out_w > 12.0 || (double)H / out_h > 12.0))
    return fail(c, H2S_E_UNSUPPORTED, "preview resize ratio out of range");
  DeviceGuard g(c->device);
  hipStream_t s = (hipStream_t)hip_stream;
  const int cw = W >> fmt.cxs(), ch = H >> fmt.cys(), ow2 = (out_w + 1) / 2;
  // tap tables, one upload each: weights wx | wy | wcx | wcy, first taps sx | sy | scx | scy
  std::vector<float> wt[4];
  std::vector<int> st[4];
  int T[4] = {0, 0, 0, 0};
  if (scale) {
    T[0] = resize_taps(W, out_w, &wt[0], &st[0]);
    T[1] = resize_taps(H, out_h, &wt[1], &st[1]);
  }
  T[2] = resize_taps(cw, ow2, &wt[2], &st[2]);
  T[3] = resize_taps(ch, out_h, &wt[3], &st[3]);
  std::vector<float> wall;
  std::vector<int> sall;
  size_t woff[4], soff[4];
  for (int i = 0; i < 4; i++) {
    woff[i] = wall.size(), soff[i] = sall.size();
    wall.insert(wall.end(), wt[i].begin(), wt[i].end());
    sall.insert(sall.end(), st[i].begin(), st[i].end());
  }
  // scratch: a host set's tight device copy, the tap tables, the RGB staging of a host output
  auto al = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t n = (size_t)nframes;
  const bool host_in = in->location == H2S_LOC_HOST, host_out = rgb_location == H2S_LOC_HOST;
  const size_t in_b = host_in ? al(frame_bytes(in, fmt) * n) : 0;
  const size_t w_b = al(wall.size() * 4), s_b = al(sall.size() * 4);
  const size_t rgb_b = host_out ? al((size_t)out_w * 3 * out_h * n) : 0;
  const size_t need = in_b + w_b + s_b + rgb_b;
  if (need > c->d_prev.cap && c->d_prev) {
    // a previous preview's kernels may still read the old scratch
    drain_launches(c);
    hipStreamSynchronize(s);
  }
  if ((rc = c->d_prev.reserve(c, need, "preview scratch"))) return rc;
  uint8_t* base = c->d_prev;
  float* dw = (float*)(base + in_b);
  int* ds = (int*)(base + in_b + w_b);
  const h2s_frames din = device_view(in, base, fmt);
  KParams k{};  // the source set as the conversion kernels bind it
  fill_geometry(&k, &din, nullptr, nframes, fmt, PLANAR_420);
  h2s::SrcPreviewParams P{};
  for (int p = 0; p < 3; p++) P.in[p] = k.in[p], P.ls[p] = k.in_ls[p], P.fp[p] = k.in_fp[p];
  P.cstep = k.in_cstep, P.sh = k.in_sh, P.mask = (1 << bits) - 1;
  P.W = W, P.H = H, P.cw = k.icw, P.ch = k.ich;
  P.ow = out_w, P.oh = out_h, P.ow2 = ow2;
  P.rgb = host_out ? base + in_b + w_b + s_b : rgb;
  P.rls = host_out ? 3LL * out_w : rgb_linesize;
  P.rfp = host_out ? 3LL * out_w * out_h : rgb_frame_pitch;
  P.identity = scale ? 0 : 1;
  P.Tx = T[0], P.Ty = T[1], P.Tcx = T[2], P.Tcy = T[3];
  P.wx = dw + woff[0], P.wy = dw + woff[1], P.wcx = dw + woff[2], P.wcy = dw + woff[3];
  P.sx = ds + soff[0], P.sy = ds + soff[1], P.scx = ds + soff[2], P.scy = ds + soff[3];
  const double sc = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
  P.y_off = fmt.full() ? 0 : 16 << (bits - 8), P.mid = 1 << (bits - 1);
  P.y_inv = (float)(1.0 / (fmt.full() ? top : 219.0 * sc));
  P.c_inv = (float)(1.0 / (fmt.full() ? top : 224.0 * sc));
  const double kr = kKrKb[matrix][0], kb = kKrKb[matrix][1], kg = 1.0 - kr - kb;
  P.m_rcr = (float)(2.0 * (1.0 - kr)), P.m_bcb = (float)(2.0 * (1.0 - kb));
  P.m_gcr = (float)(-2.0 * kr * (1.0 - kr) / kg), P.m_gcb = (float)(-2.0 * kb * (1.0 - kb) / kg);
  P.round8 = rgb_model == H2S_SRC_RGB_ROUND8;
  hipError_t e = hipMemcpyAsync(dw, wall.data(), wall.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(ds, sall.data(), sall.size() * 4, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && host_in) e = copy_frames(&din, in, nframes, s, fmt);
  if (e == hipSuccess) {
    timing_begin(c, s);  // (h2s_set_timing: the kernel alone, without the copies around it)
    e = h2s::launch_source_rgb24(P, nframes, s);
    timing_end(c, s);
  }
  for (int f = 0; host_out && f < nframes && e == hipSuccess; f++)
    e = hipMemcpy2DAsync(rgb + (long long)f * rgb_frame_pitch, rgb_linesize, P.rgb + f * P.rfp, P.rls,
                         3 * (size_t)out_w, out_h, hipMemcpyDeviceToHost, s);
  // synchronous: the tables above are this call's own, and the scratch is free on return
  const hipError_t es = hipStreamSynchronize(s);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return hip_fail(c, e, "source preview");
  return 0;
}

int h2s_preview_source_rgb24(h2s_ctx* c, const h2s_frames* in, uint8_t* rgb, int64_t rgb_linesize, int out_w,
                             int out_h, int matrix, int rgb_model, int rgb_location, void* hip_stream) {
  return h2s_preview_source_rgb24_batch(c, in, 1, rgb, rgb_linesize, rgb_linesize * (int64_t)out_h, out_w, out_h,
                                        matrix, rgb_model, rgb_location, hip_stream);
}

int h2s_set_timing(h2s_ctx* c, int enabled) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  c->timing = enabled != 0;
  c->ev_count = 0;
  return 0;
}

double h2s_kernel_ms(h2s_ctx* c, int count) {
  if (!c) return -1.0;
  if (count <= 0) {
    c->ev_count = 0;
    return 0.0;
  }
  DeviceGuard g(c->device);
  const long long avail = c->ev_count < kEvRing ? c->ev_count : kEvRing;
  if (count > avail) count = (int)avail;
  if (count == 0) return 0.0;
  double sum = 0.0;
  for (int i = 0; i < count; i++) {
    const int slot = (int)((c->ev_count - 1 - i) % kEvRing);
    if (hipEventSynchronize(c->ev1[slot].ev) != hipSuccess) return -1.0;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->ev0[slot].ev, c->ev1[slot].ev) != hipSuccess) return -1.0;
    sum += ms;
  }
  return sum / count;
}

}  // extern "C"
