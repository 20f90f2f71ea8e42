// h2s_host.h — what the host units of the C-ABI share (private to the
// library): the frame Format, the owners of the context's device resources,
// the context itself, and the helpers that cross the units
//
//   h2s_resolve.hip      host arithmetic only, no HIP API call
//   h2s_api.hip          contexts, tables, frame staging, routing, h2s_process
//   h2s_api_peak.hip     the dynamic peak's host side
//   h2s_api_preview.hip  the two preview panes
//   h2s_api_dovi.hip     Dolby Vision profile 5: the records' validation and upload
//   h2s_api_scale.hip    the scaled 4:2:0 output (h2s_process_scaled)
//   h2s_api_decimate.hip the 4:2:0 front-end of a 4:2:2 / 4:4:4 set (h2s_set_input_decimation)
//   h2s_api_rgb.hip      the RGB tensor output (h2s_process_rgb)
//   h2s_api_ladder.hip   a rendition ladder from one conversion (h2s_process_ladder)
//
// Everything declared here has hidden visibility: the library's dynamic
// symbols are the h2s_* calls of include/h2s.h and nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#define H2S_PRIVATE_TEST_HOOKS
#include "../../include/h2s.h"
#include "h2s_launch.h"
#include "h2s_params.h"
#include "h2s_peak.h"
#include "h2s_srcprev.h"

#pragma GCC visibility push(hidden)

namespace h2s {
namespace host {

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

// the tap tables of the scaled output (resize_taps), cached for one
// (W, H) -> (ow, oh): four axes (luma x, y; chroma x, y), the weights in one
// device array and the first taps in another, uploaded once.  The host copies
// stay: the launch's rows per block are picked from the first taps
struct ScaleTaps {
  enum Axis { X, Y, CX, CY };
  int W = 0, H = 0, ow = 0, oh = 0;   // the key (0: none yet)
  int T[4] = {0, 0, 0, 0};
  size_t woff[4] = {0, 0, 0, 0}, soff[4] = {0, 0, 0, 0};
  std::vector<float> w;
  std::vector<int> s;
  Dev<float> d_w;
  Dev<int> d_s;
  long long uploads = 0;   // (H2S_OPT_TEST_SCALE_UPLOADS)
  const float* wt(int a) const { return d_w + woff[a]; }
  const int* st(int a) const { return d_s + soff[a]; }
};

}  // namespace host
}  // namespace h2s

// (hidden: its implicit destructor is no part of the library's symbol set)
struct h2s_ctx {
  int device = 0;
  h2s_params params{};
  bool params_set = false;
  h2s::KParams k{};  // resolved constants (pointers filled per call)
  // set_params / set_lut copy and (re)allocate on this non-blocking stream
  // (stream-ordered hipMallocAsync / hipFreeAsync for the lattices): no
  // null-stream copy or hipFree, which would wait for the whole device.
  // h2s_destroy releases the lattices and waits for the stream before the
  // members go; declared before them, it would outlive them in any case
  h2s::host::Stream aux;
  h2s::host::Dev<float4> d_lut;
  int lut_n = 0;
  bool lut_unit = false;  // every lattice value is finite and in [0, 1] (what d_lut_yuv's clamped build assumes)
  h2s::host::Dev<float> d_lut_yuv;  // lattice pre-multiplied into output code space (3 floats/point)
  float lut_yuv_scale = -1.0f;  // quantiser scale it was built for (-1 = stale)
  int lut_yuv_rgb = 0;          // 1: it holds plain R'G'B' records (libplacebo rgba8 form)
  h2s::host::Dev<unsigned> d_lut8x;  // libplacebo branch: lut3d's 8-bit output per rgba code triple (2^24, 64 MiB)
  bool lut8x_ok = false;        // built for the current lattice
  h2s::host::Ordered lut_built;  // after the last build of d_lut_yuv / d_lut8x (queued on the caller's stream)
  bool fast_enabled = true;
  bool lp_exact = false;  // H2S_OPT_LP_EXACT
  // how later calls read `in` and write `out`: h2s_set_frame_layout sets both
  // layouts, h2s_set_input_subsampling in_fmt.sub (the output is always 4:2:0),
  // h2s_set_input_tags in_fmt.range and in_fmt.loc
  h2s::host::Format in_fmt = h2s::host::PLANAR_420, out_fmt = h2s::host::PLANAR_420;
  // Dolby Vision profile 5 (h2s_set_dovi, h2s_api_dovi.hip): the context's copy
  // of the caller's records; dovi_n 0: off, 1: one record for every frame,
  // n > 1: record f for frame f of a call
  h2s::host::Dev<h2s::DoviRec> d_dovi;
  int dovi_n = 0;
  bool dovi_tile = false;   // every record has the shape the tile kernel takes (dovi_tile_shape)
  int peak_blocks = h2s::PEAK_BLOCKS;   // H2S_OPT_TEST_PEAK_BLOCKS (private A/B hook)
  bool serial_host = false;  // H2S_HOST_SERIAL=1: one H2D, kernel, D2H per call (no chunk pipeline)
  int tiles_per_block = 8;  // k_tile: tiles one block walks (H2S_TILES_PER_BLOCK overrides, 1..64)
  h2s::host::Dev<uint16_t> d_eq;
  h2s::host::Dev<float4> d_pq;   // PQ EOTF cubic segments (fast path)
  h2s::host::Dev<float4> d_hlg;  // HLG inverse-OETF cubic segments (fast path, CPU chain)
  h2s::host::Dev<float4> d_pqi;  // PQ inverse EOTF cubic segments (fast path, lp_tone IPT)
  h2s::host::Dev<uint8_t> d_stage;
  h2s::host::Dev<uint8_t> d_prev;  // preview scratch
  // dynamic peak (params.peak_detect), all on the device: statistics ->
  // per-frame (max, avg) -> IIR + curve records -> conversion, queued on the
  // caller's stream with no host round trip (h2s_peak.h)
  h2s::host::Dev<float2> d_stats;           // per-block partials, then (percentile model) histograms
  int stats_nf = 0;   // frames d_stats is laid out for (frame_stats)
  h2s::host::Dev<double2> d_fstat;          // per frame: the statistic, then the smoothed (max, avg) its curve uses
  h2s::host::Dev<h2s::CurveConsts> d_curve; // one curve record per frame of a dynamic-peak launch
  h2s::host::Dev<h2s::PeakState> d_pk;      // [0] the smoothing state; [1] a preview's saved copy of it
  h2s::host::Ordered peak_use;              // after the last launch that used the buffers above
  // pipelined schedule (run_dynamic_peak_chunked; private A/B hook
  // H2S_OPT_TEST_PEAK_CHUNK, off: measured slower): frames per
  // chunk (0 = one statistics launch, then one conversion launch, all on the
  // caller's stream), the statistics stream and a second conversion stream,
  // events: start | end | per-chunk statistics
  int peak_chunk = 0;
  h2s::host::Stream pk_s[2];
  std::vector<h2s::host::Event> pk_ev;
  std::string err;
  bool fail_after_launch = false;  // H2S_OPT_TEST_FAIL_AFTER_LAUNCH (private test hook, one call)
  bool timing = false;
  h2s::host::Event ev0[h2s::host::kEvRing], ev1[h2s::host::kEvRing];
  long long ev_count = 0;  // launches recorded since reset
  // host-frame pipeline: H2D, compute and D2H of consecutive chunks on
  // their own streams (two DMA directions overlap the kernel and each other)
  h2s::host::Stream ps[3];
  h2s::host::Event pev[2 * h2s::host::kMaxChunks + 2];
  // events recorded after this context's own asynchronous launches, on the
  // streams they went to: set_params / set_lut wait for exactly these (no
  // device-wide synchronisation), then recycle them
  std::vector<h2s::host::Event> pend, ev_free;
  h2s::host::Dev<float2> d_chr;             // BICUBIC chroma: one frame's per-pixel (Cb, Cr)
  h2s::host::Ordered chr_use;               // after the last BICUBIC two-pass launch (d_chr in use)
  // scaled output (h2s_process_scaled): the chain's full-size planar frames of
  // one chunk, then a host output's staging; the cached tap tables
  h2s::host::Dev<uint8_t> d_scale;
  h2s::host::ScaleTaps scale_taps;
  h2s::host::Ordered scale_use;             // after the last scaled call (d_scale and the tables in use)
  // a rendition ladder (h2s_process_ladder): its own tap tables, one entry per
  // (W, H, ow, oh) of a scaled rung; scale_taps and its upload count stay
  // h2s_process_scaled's.  d_scale and scale_use serve the ladder too
  h2s::host::ScaleTaps ladder_taps[H2S_LADDER_MAX];
  long long ladder_uploads = 0;             // (H2S_OPT_TEST_LADDER_UPLOADS)
  unsigned ladder_evict = 0;                // the entry a new size replaces next when every one holds a size
  // the 4:2:0 front-end (h2s_set_input_decimation): a host chunk's staged
  // source frames, then the decimated chroma of one chunk
  int decimate = H2S_DECIMATE_OFF;
  h2s::host::Dev<uint8_t> d_dec;
  h2s::host::Ordered dec_use;               // after the last call that used d_dec
};

namespace h2s {
namespace host {

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

// what a tile launch does beside the plain conversion
struct TileOpts {
  const CurveConsts* cv_frames = nullptr;   // dynamic peak: one curve record per frame of the launch
  int dbg = 0;                 // > 0: the debug instance, which writes that stage's
  float* dbg_out = nullptr;    //      float planes of frame 0 here
  float2* chr444 = nullptr;    // BICUBIC pass 1: every pixel's (Cb, Cr) here, no chroma planes
};

// the generic kernel over a column range of k's frames: every column, or the
// ragged ones right of the last whole tile (left-sited chroma needs no left
// neighbour, so the seam is exact; none: no launch).  k.chr444 set: BICUBIC
// pass 1 (luma, and every pixel's chroma into k.chr444)
enum Columns { COLUMNS_ALL, COLUMNS_RAGGED };

// ---- h2s_resolve.hip (no HIP API call) ----

// The S1 constants of a source set, in double: Y' = code * y_scale + y_off
// (y_black: the code of Y' = 0), Cb, Cr = code * c_scale + c_off (mid: the
// code of 0), and the Y'CbCr -> R'G'B' terms of its matrix
struct SourceConsts {
  double y_scale, y_off, y_black;
  double c_scale, c_off, mid;
  double m_rcr, m_gcb, m_gcr, m_bcb;   // 2(1-Kr), -2Kb(1-Kb)/Kg, -2Kr(1-Kr)/Kg, 2(1-Kb)
};
SourceConsts source_consts(int bits, bool full, int matrix = H2S_SRC_MATRIX_BT2020NC);
void source_kparams(KParams* k, int bits, bool full);

int validate_params(h2s_ctx* c, const h2s_params* p);
void resolve(const h2s_params* p, KParams* k, std::vector<uint16_t>* eq);
void resolve_fast(const h2s_ctx* c, const KParams& k, FastParams* F);
void build_pqi_table(std::vector<float4>* out);
void build_pq_table(double scale, std::vector<float4>* out);
void build_hlg_table(std::vector<float4>* out);
void chroma_taps(float* wx7, float* wy8);
int resize_taps(int src, int dst, std::vector<float>* w, std::vector<int>* start);
PeakModel peak_model(const h2s_ctx* c, const KParams& k);

// ---- h2s_api.hip ----

int check_frames(h2s_ctx* c, const h2s_frames* f, int bits, const char* which, Format fmt);
size_t frame_bytes(const h2s_frames* f, Format fmt);
h2s_frames tight(const h2s_frames* f, void* base, Format fmt);
h2s_frames device_view(const h2s_frames* f, void* base, Format fmt);
hipError_t copy_frames(const h2s_frames* dst, const h2s_frames* src, int nframes, hipStream_t s, Format fmt);
void fill_geometry(KParams* k, const h2s_frames* in, const h2s_frames* out, int nframes, Format in_fmt,
                   Format out_fmt);
h2s_frames frames_at(const h2s_frames* f, int start);
int drain_launches(h2s_ctx* c);
int aux_stream(h2s_ctx* c, hipStream_t* out);
int queued_exit(h2s_ctx* c, hipStream_t s, int rc);
int prepare(h2s_ctx* c, KParams* k, bool need_lut = true);
KParams frame_range(const KParams& k, int f0, int n);
hipError_t launch_tiles(const h2s_ctx* c, const KParams& k, const Route& r, const TileOpts& o = {});
hipError_t launch_columns(const KParams& k, const Route& r, Columns cols);
hipError_t launch_route(const h2s_ctx* c, const KParams& k, const Route& r);
void timing_begin(h2s_ctx* c, hipStream_t s);
void timing_end(h2s_ctx* c, hipStream_t s);
int process_frames(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, int nframes, hipStream_t s,
                   Format in_fmt, Format out_fmt, int dovi_f0 = 0);
int upload_table(h2s_ctx* c, DevBuf& buf, const void* src, size_t bytes, const char* what);
int note_launch(h2s_ctx* c, hipStream_t s);

int debug_float(h2s_ctx* c, const h2s_frames* in, Format in_fmt, int stage, float* out_rgb, int out_location,
                hipStream_t s);
int query_path(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, Format in_fmt);

// ---- h2s_api_decimate.hip ----

// A call's use of the front-end: begin (the checks, the scratch, its ordering
// on s), then chunk by chunk (at most d.per frames: stage a host chunk, launch
// k_decimate420, and *view is the 4:2:0 set of Format d.fmt that the chain
// reads: the chunk's luma in place, the chroma in the scratch), then end
struct Decimated {
  Format src_fmt, fmt;
  int per = 0;               // frames of a chunk at the most
  uint8_t *stage = nullptr, *chroma = nullptr;   // in c->d_dec
};
bool decimating(const h2s_ctx* c, Format in_fmt);
h2s_frames decimated_view(const h2s_frames* in, Format in_fmt, const uint8_t* stage, const uint8_t* chroma);
int decimate_begin(h2s_ctx* c, const h2s_frames* in, int nframes, hipStream_t s, Format in_fmt, Decimated* d);
int decimate_chunk(h2s_ctx* c, const Decimated& d, const h2s_frames* in, int nf, hipStream_t s, h2s_frames* view,
                   int run = 0);
int decimate_end(h2s_ctx* c, hipStream_t s);
int process_decimated(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, int nframes, hipStream_t s,
                      Format in_fmt, Format out_fmt, int dovi_f0);

// ---- h2s_api_scale.hip (shared with h2s_api_rgb.hip and h2s_api_ladder.hip) ----

constexpr int kChunk = 16;   // frames of the scaled output's scratch at the most
h2s_frames scratch_frames(int W, int H, int bits, uint8_t* base);
bool rows_aligned16(const h2s_frames* f, Format fmt);
// the tables of one cache entry: t is c->scale_taps (ensure_taps) or one of c->ladder_taps
int fill_taps(h2s_ctx* c, ScaleTaps& t, int W, int H, int ow, int oh, hipStream_t s);
int ensure_taps(h2s_ctx* c, int W, int H, int ow, int oh, hipStream_t s);
// the resize of one chunk, mid -> dout with t's tables: the launch record
// (every choice of the host's, no HIP call), then its launch over nf frames
// whose destination starts dst_f0 frames into dout
int scale_record(h2s_ctx* c, const ScaleTaps& t, const h2s_frames* mid, const h2s_frames* dout, Format out_fmt,
                 ScaleParams* P);
int launch_scale(h2s_ctx* c, const ScaleParams& P, int src_bps, int dst_f0, int nf, hipStream_t s);
int launch_chunk(h2s_ctx* c, const h2s_frames* mid, const h2s_frames* dout, int nf, Format out_fmt, hipStream_t s);

// ---- h2s_api_dovi.hip ----

int check_dovi(h2s_ctx* c, const KParams& k, Format in_fmt, int f0, int nframes);

// ---- h2s_api_peak.hip ----

int ensure_peak_state(h2s_ctx* c);
int peak_order(h2s_ctx* c, hipStream_t s);
int peak_done(h2s_ctx* c, hipStream_t s);
int run_dynamic_peak(h2s_ctx* c, const KParams& k, const Route& r);

}  // namespace host
}  // namespace h2s

#pragma GCC visibility pop
