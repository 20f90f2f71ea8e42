// h2s_api_peak.hip — the dynamic peak's host side (params.peak_detect): the
// statistics launch, the schedules that feed the conversion its per-frame
// curve records, and the h2s_peak_* calls on the context's smoothing state.
//
// libplacebo-style detected peak (PARITY UNPINNED; model in DESIGN.md §4.6),
// all on the device (h2s_peak.h): k_peak_stats* (per-block partials and the
// percentile histograms) -> k_peak_frame (per-frame statistic) ->
// k_peak_curves (the IIR in frame order from the context's device state, and
// one curve record per frame) -> the conversion, which reads the records.
// h2s_process queues all of it on the caller's stream and returns; the state
// comes back to the host only on demand (h2s_peak_state).  The model's
// constants are peak_model's (h2s_resolve.hip).
#include "h2s_host.h"

using namespace h2s::host;
using h2s::KParams;

namespace h2s {
namespace host {

int ensure_peak_state(h2s_ctx* c) {
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
int peak_order(h2s_ctx* c, hipStream_t s) { return c->peak_use.wait(c, s, "peak ordering"); }

int peak_done(h2s_ctx* c, hipStream_t s) { return c->peak_use.mark(c, s, "peak event"); }

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
int run_dynamic_peak(h2s_ctx* c, const KParams& k, const Route& r) {
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

}  // namespace host
}  // namespace h2s

extern "C" {

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
  const bool dec = decimating(c, c->in_fmt);   // (h2s_set_input_decimation: the statistics of the 4:2:0 set)
  if (c->in_fmt.sub != H2S_SUB_420 && !dec)
    return fail(c, H2S_E_UNSUPPORTED, "h2s_peak_stats reads 4:2:0 input only (h2s_set_input_subsampling is 4:2:2 / 4:4:4)");
  // (behind the front-end the records are judged for the 4:2:0 set it makes: left-sited, whatever the tag)
  Format dv_fmt = c->in_fmt;
  if (dec) dv_fmt.sub = H2S_SUB_420, dv_fmt.loc = H2S_CHROMA_LEFT;
  if ((rc = check_dovi(c, k, dv_fmt, 0, nframes))) return rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", c->in_fmt))) return rc;
  if (in->location != H2S_LOC_DEVICE) return fail(c, H2S_E_INVALID_ARG, "h2s_peak_stats takes device frames");
  if (nframes == 0) return 0;
  DeviceGuard g(c->device);
  hipStream_t s = (hipStream_t)hip_stream;
  if ((rc = peak_order(c, s))) return rc;
  if (!dec) {
    h2s_frames out = *in;                       // geometry only: the statistics read the input planes
    fill_geometry(&k, in, &out, nframes, c->in_fmt, PLANAR_420);
    if ((rc = frame_stats(c, k, s, nullptr, nullptr))) return rc;
  } else {
    // chunk by chunk behind the front-end; d_fstat takes the whole call's frames first (a grown buffer is a new one)
    Decimated d;
    if ((rc = decimate_begin(c, in, nframes, s, c->in_fmt, &d)) ||
        (rc = c->d_fstat.reserve(c, (size_t)nframes * sizeof(double2), "peak statistics")))
      return rc;
    for (int f0 = 0; f0 < nframes; f0 += d.per) {
      const int nf = std::min(d.per, nframes - f0);
      const h2s_frames ci = frames_at(in, f0);
      h2s_frames view;
      if ((rc = decimate_chunk(c, d, &ci, nf, s, &view))) return queued_exit(c, s, rc);
      fill_geometry(&k, &view, &view, nf, d.fmt, PLANAR_420);
      k.dovi_f0 = f0;   // (a chunk's Dolby Vision records count frames of the call)
      if ((rc = frame_stats(c, k, s, nullptr, nullptr, f0))) return queued_exit(c, s, rc);
    }
    if ((rc = decimate_end(c, s))) return queued_exit(c, s, rc);
  }
  std::vector<double2> st(nframes);
  hipError_t e = hipMemcpyAsync(st.data(), c->d_fstat, nframes * sizeof(double2), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(c, e, "peak statistics read-back");
  for (int f = 0; f < nframes; f++) fmax[f] = st[f].x, favg[f] = st[f].y;
  return 0;
}

}  // extern "C"
