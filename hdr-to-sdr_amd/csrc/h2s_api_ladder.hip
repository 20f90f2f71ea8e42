// h2s_api_ladder.hip — a rendition ladder from one conversion
// (h2s_process_ladder, include/h2s.h): h2s_process_scaled's pipeline with
// several outputs.  Chunk by chunk on the caller's stream the chain runs once
// into the scaled output's planar scratch at full size, and every rung is made
// from that scratch: a scaled rung by k_scale420 (h2s_scale.hip) with the
// rung's tap tables, a rung of the source's size by k_repack420
// (h2s_repack.hip).  The scratch and its guard are h2s_process_scaled's; the
// tap tables are the ladder's own, one cache entry per size.
#include "h2s_host.h"
#include "h2s_repack.h"
#include "h2s_scale.h"

using namespace h2s::host;
using h2s::RepackParams;
using h2s::RepackPlane;
using h2s::ScaleParams;

namespace {

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Rung {
  bool same;            // the source's size: a repack, no resize
  int taps = -1;        // its entry of c->ladder_taps
  h2s_frames dout;      // what the kernels write: the device rung itself (frame 0), or a host rung's staging
  ScaleParams rec;      // the resize's launch record for dout's frame 0
};

// the cache entry of every scaled rung: the one that holds its size, else a
// free one, else one that no rung of this call reads (fill_taps waits for the
// launches that read the old tables first).  n <= H2S_LADDER_MAX entries are
// in use at the most, so there is always one
int ladder_taps(h2s_ctx* c, int W, int H, const h2s_frames* outs, Rung* rungs, int n, hipStream_t s) {
  bool used[H2S_LADDER_MAX] = {};
  auto find = [&](const h2s_frames& o) {
    for (int j = 0; j < H2S_LADDER_MAX; j++) {
      const ScaleTaps& t = c->ladder_taps[j];
      if (t.W == W && t.H == H && t.ow == o.width && t.oh == o.height) return j;
    }
    return -1;
  };
  for (int i = 0; i < n; i++)
    if (!rungs[i].same && (rungs[i].taps = find(outs[i])) >= 0) used[rungs[i].taps] = true;
  for (int i = 0; i < n; i++) {
    if (rungs[i].same || rungs[i].taps >= 0) continue;
    int j = find(outs[i]);   // (an earlier rung of this loop may have brought the size in)
    if (j < 0) {
      for (int k = 0; k < H2S_LADDER_MAX && j < 0; k++)
        if (!used[k] && c->ladder_taps[k].W == 0) j = k;
      while (j < 0) {
        const int k = (int)(c->ladder_evict++ % H2S_LADDER_MAX);
        if (!used[k]) j = k;
      }
      ScaleTaps& t = c->ladder_taps[j];
      const long long before = t.uploads;
      if (int rc = fill_taps(c, t, W, H, outs[i].width, outs[i].height, s)) return rc;
      c->ladder_uploads += t.uploads - before;
    }
    rungs[i].taps = j, used[j] = true;
  }
  return 0;
}

// k_repack420 over nf frames of the scratch set `mid` into frames dst_f0.. of dout
int launch_repack(h2s_ctx* c, const h2s_frames* mid, const h2s_frames* dout, int dst_f0, int nf, Format out_fmt,
                  hipStream_t s) {
  const int bps = mid->bits == 8 ? 1 : 2;
  RepackParams P{};
  P.nplanes = out_fmt.planes();
  for (int e = 0; e < P.nplanes; e++) {
    RepackPlane& L = P.pl[e];
    const Format::Plane pl = PLANAR_420.plane(mid, e);
    L.np = e && out_fmt.semi() ? 2 : 1;
    L.src[0] = (const uint8_t*)mid->data[e], L.src[1] = (const uint8_t*)mid->data[L.np == 2 ? 2 : e];
    L.sls = mid->linesize[e], L.sfp = mid->frame_pitch[e];
    L.dst = (uint8_t*)dout->data[e] + (long long)dst_f0 * dout->frame_pitch[e];
    L.dls = dout->linesize[e], L.dfp = dout->frame_pitch[e];
    L.row_bytes = (int)pl.row_bytes, L.rows = (int)pl.rows;
  }
  P.sh = out_fmt.semi() && bps == 2 ? 16 - mid->bits : 0;
  P.vec_out = rows_aligned16(dout, out_fmt) ? 1 : 0;
  timing_begin(c, s);
  const hipError_t e = h2s::launch_repack420(P, bps, out_fmt.semi(), nf, s);
  timing_end(c, s);
  return e == hipSuccess ? 0 : hip_fail(c, e, "repack kernel launch");
}

}  // namespace

extern "C" {

int h2s_process_ladder(h2s_ctx* c, const h2s_frames* in, const h2s_frames* outs, int n_outs, int nframes,
                       void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (!outs) return fail(c, H2S_E_INVALID_ARG, "ladder outputs is NULL");
  if (n_outs < 1 || n_outs > H2S_LADDER_MAX)
    return fail(c, H2S_E_INVALID_ARG, "a ladder has 1 to " + std::to_string(H2S_LADDER_MAX) + " rungs");
  // one rung: h2s_process_scaled and nothing else
  if (n_outs == 1) return h2s_process_scaled(c, in, &outs[0], nframes, hip_stream);
  hipStream_t s = (hipStream_t)hip_stream;
  const Format in_fmt = c->in_fmt, out_fmt = c->out_fmt;
  if (nframes < 0) return fail(c, H2S_E_INVALID_ARG, "nframes < 0");
  if (!c->params_set) return fail(c, H2S_E_INVALID_ARG, "h2s_set_params was not called");
  int rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", in_fmt))) return rc;
  const int W = in->width, H = in->height;
  // every rung is checked before anything is queued or any state moves
  Rung rungs[H2S_LADDER_MAX];
  for (int i = 0; i < n_outs; i++) {
    const h2s_frames& o = outs[i];
    const std::string which = "rung " + std::to_string(i);
    if (o.width <= 0 || o.height <= 0 || (o.width & 1) || (o.height & 1))
      return fail(c, H2S_E_INVALID_ARG, which + ": the target needs positive, even width and height");
    if ((rc = check_frames(c, &o, c->params.bits_out, which.c_str(), out_fmt))) return rc;
    if (o.location != outs[0].location)
      return fail(c, H2S_E_INVALID_ARG, which + ": every rung must have rung 0's location");
    // (h2s_process_scaled's limits)
    if (o.width > 4 * 8192 || o.height > 4 * 8192 || (double)W / o.width > 12.0 || (double)H / o.height > 12.0)
      return fail(c, H2S_E_UNSUPPORTED, which + ": resize ratio out of range");
    rungs[i].same = o.width == W && o.height == H;
  }
  if (nframes == 0) return 0;
  DeviceGuard g(c->device);

  // the scratch: one chunk of the chain's frames, then the host rungs' staging, one after the other
  const int per = std::min(nframes, kChunk);
  const bool host_out = outs[0].location == H2S_LOC_HOST;
  const int bits = c->params.bits_out;
  const size_t mid_bytes = (size_t)scratch_frames(W, H, bits, nullptr).frame_pitch[0] * per;
  size_t stage[H2S_LADDER_MAX], need = mid_bytes;
  for (int i = 0; i < n_outs; i++) {
    stage[i] = need;
    if (host_out) need += round_up(frame_bytes(&outs[i], out_fmt) * (size_t)per, 256);
  }
  if ((rc = c->scale_use.wait(c, s, "ladder ordering"))) return rc;
  if (need > c->d_scale.cap && c->d_scale) {
    // an earlier call's kernels may still use the old scratch
    drain_launches(c);
    hipStreamSynchronize(s);
  }
  if ((rc = c->d_scale.reserve(c, need, "ladder scratch"))) return rc;
  if ((rc = ladder_taps(c, W, H, outs, rungs, n_outs, s))) return queued_exit(c, s, rc);
  const h2s_frames mid = scratch_frames(W, H, bits, c->d_scale);
  for (int i = 0; i < n_outs; i++) {
    Rung& r = rungs[i];
    r.dout = device_view(&outs[i], c->d_scale + stage[i], out_fmt);
    if (!r.same && (rc = scale_record(c, c->ladder_taps[r.taps], &mid, &r.dout, out_fmt, &r.rec)))
      return queued_exit(c, s, fail(c, rc, "rung " + std::to_string(i) + ": " + c->err));
  }

  // chunks in order on s: the dynamic peak's state sees every frame once and in
  // order, and chunk i + 1's conversion overwrites the scratch after chunk i's last rung
  const int src_bps = bits == 8 ? 1 : 2;
  for (int f0 = 0; f0 < nframes; f0 += per) {
    const int nf = std::min(per, nframes - f0);
    const h2s_frames ci = frames_at(in, f0);
    if ((rc = process_frames(c, &ci, &mid, nf, s, in_fmt, PLANAR_420, f0))) return queued_exit(c, s, rc);
    for (int i = 0; i < n_outs; i++) {
      const Rung& r = rungs[i];
      const int dst_f0 = host_out ? 0 : f0;
      rc = r.same ? launch_repack(c, &mid, &r.dout, dst_f0, nf, out_fmt, s)
                  : launch_scale(c, r.rec, src_bps, dst_f0, nf, s);
      if (rc) return queued_exit(c, s, rc);
    }
    if (host_out) {
      for (int i = 0; i < n_outs; i++) {
        const h2s_frames ho = frames_at(&outs[i], f0);
        const hipError_t e = copy_frames(&ho, &rungs[i].dout, nf, s, out_fmt);
        if (e != hipSuccess) return queued_exit(c, s, hip_fail(c, e, "device->host copy"));
      }
    }
  }
  if ((rc = c->scale_use.mark(c, s, "ladder event"))) return queued_exit(c, s, rc);
  if (host_out) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return queued_exit(c, s, hip_fail(c, e, "stream synchronize"));
    return 0;
  }
  return note_launch(c, s);
}

}  // extern "C"
