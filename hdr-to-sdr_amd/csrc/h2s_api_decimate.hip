// h2s_api_decimate.hip — the 4:2:0 front-end of a 4:2:2 / 4:4:4 input set
// (h2s_set_input_decimation, include/h2s.h): k_decimate420 (h2s_decimate.hip)
// writes the decimated chroma of a chunk of frames into a context-owned
// scratch, and the conversion behind it runs unchanged on an ordinary 4:2:0
// set of the context's input layout whose luma is the caller's plane and whose
// chroma lies in the scratch.  A host-resident set is staged into the same
// scratch first, chunk by chunk, on the caller's stream.
#include "h2s_decimate.h"
#include "h2s_host.h"

using namespace h2s::host;
using h2s::DecimateParams;
using h2s::KParams;

namespace {

constexpr int kChunk = 16;   // frames of scratch at the most

long long round_up(long long v, long long a) { return (v + a - 1) / a * a; }

// the decimated chroma of one frame in the scratch: rows of `onw` 16-bit words,
// 16-byte aligned and padded to 16 bytes (k_decimate420 stores whole chunks),
// the planar set's two planes back to back, frames a multiple of 256 bytes apart
struct ChromaLayout {
  long long onw, ls, plane, fp;
};
ChromaLayout chroma_layout(const h2s_frames* in, Format in_fmt) {
  ChromaLayout l;
  l.onw = (long long)(in->width / 2) * (in_fmt.semi() ? 2 : 1);
  l.ls = round_up(l.onw * 2, 16);
  l.plane = l.ls * (in->height / 2);
  l.fp = round_up(l.plane * (in_fmt.semi() ? 1 : 2), 256);
  return l;
}

size_t stage_bytes(const h2s_frames* in, Format in_fmt, int per) {
  return in->location == H2S_LOC_HOST ? (size_t)round_up((long long)frame_bytes(in, in_fmt) * per, 256) : 0;
}

}  // namespace

namespace h2s {
namespace host {

bool decimating(const h2s_ctx* c, Format in_fmt) {
  return c->decimate != H2S_DECIMATE_OFF && in_fmt.sub != H2S_SUB_420;
}

// the 4:2:0 set the chain reads for `in` (frame 0 of a chunk): the luma plane
// of `in` (a host set: of its tight copy at `stage`) and the chroma at `chroma`
h2s_frames decimated_view(const h2s_frames* in, Format in_fmt, const uint8_t* stage, const uint8_t* chroma) {
  h2s_frames v = device_view(in, const_cast<uint8_t*>(stage), in_fmt);
  const ChromaLayout l = chroma_layout(in, in_fmt);
  v.data[1] = const_cast<uint8_t*>(chroma);
  v.data[2] = in_fmt.semi() ? nullptr : const_cast<uint8_t*>(chroma) + l.plane;
  for (int p = 1; p < 3; p++) {
    const bool has = p < in_fmt.planes();
    v.linesize[p] = has ? l.ls : 0, v.frame_pitch[p] = has ? l.fp : 0;
  }
  v.location = H2S_LOC_DEVICE;
  return v;
}

// the checks every caller makes of `in`, the scratch for chunks of up to 16
// frames (grown: the context's queued launches and s are waited for first, as
// for d_scale) and its ordering after an earlier call's use on another stream
int decimate_begin(h2s_ctx* c, const h2s_frames* in, int nframes, hipStream_t s, Format in_fmt, Decimated* d) {
  if (nframes < 0) return fail(c, H2S_E_INVALID_ARG, "nframes < 0");
  if (!c->params_set) return fail(c, H2S_E_INVALID_ARG, "h2s_set_params was not called");
  int rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", in_fmt))) return rc;
  d->src_fmt = d->fmt = in_fmt;
  d->fmt.sub = H2S_SUB_420, d->fmt.loc = H2S_CHROMA_LEFT;
  d->per = std::max(1, std::min(nframes, kChunk));
  const size_t sb = stage_bytes(in, in_fmt, d->per);
  const size_t need = sb + (size_t)chroma_layout(in, in_fmt).fp * d->per;
  DeviceGuard g(c->device);
  if ((rc = c->dec_use.wait(c, s, "decimation ordering"))) return rc;
  if (need > c->d_dec.cap && c->d_dec) {
    // an earlier call's kernels may still use the old scratch
    drain_launches(c);
    hipStreamSynchronize(s);
  }
  if ((rc = c->d_dec.reserve(c, need, "decimation scratch"))) return rc;
  d->stage = c->d_dec, d->chroma = c->d_dec + sb;
  return 0;
}

// one chunk (nf <= d.per frames from `in`'s frame 0), queued on s
int decimate_chunk(h2s_ctx* c, const Decimated& d, const h2s_frames* in, int nf, hipStream_t s, h2s_frames* view,
                   int run) {
  const Format f = d.src_fmt;
  *view = decimated_view(in, f, d.stage, d.chroma);
  const h2s_frames src = device_view(in, d.stage, f);
  if (in->location == H2S_LOC_HOST) {
    const hipError_t e = copy_frames(&src, in, nf, s, f);
    if (e != hipSuccess) return hip_fail(c, e, "host->device copy");
  }
  const ChromaLayout l = chroma_layout(in, f);
  DecimateParams P{};
  P.nplanes = f.semi() ? 1 : 2;
  P.src[0] = (const uint8_t*)src.data[1], P.src[1] = (const uint8_t*)src.data[f.semi() ? 1 : 2];
  P.dst[0] = (uint8_t*)view->data[1], P.dst[1] = (uint8_t*)view->data[f.semi() ? 1 : 2];
  P.sls = src.linesize[1], P.sfp = src.frame_pitch[1];
  P.dls = l.ls, P.dfp = l.fp;
  P.nw = (int)(f.plane(in, 1).row_bytes / 2), P.onw = (int)l.onw, P.rows = in->height;
  P.sh = f.semi() ? 16 - in->bits : 0, P.vmax = (1 << in->bits) - 1;
  P.vec = 1;
  for (int p = 1; p < f.planes(); p++)
    if ((uintptr_t)src.data[p] % 16 || src.linesize[p] % 16 || src.frame_pitch[p] % 16) P.vec = 0;
  // (the kernel reads both planar planes with plane 1's pitches)
  if (!f.semi() && (src.linesize[2] != src.linesize[1] || src.frame_pitch[2] != src.frame_pitch[1]))
    return fail(c, H2S_E_UNSUPPORTED, "input decimation: the two chroma planes need equal pitches");
  chroma_taps(P.wx, P.wy);
  timing_begin(c, s);
  const hipError_t e = h2s::launch_decimate420(P, f.sub, f.semi(), nf, run, s);
  timing_end(c, s);
  return e == hipSuccess ? 0 : hip_fail(c, e, "decimation kernel launch");
}

int decimate_end(h2s_ctx* c, hipStream_t s) { return c->dec_use.mark(c, s, "decimation event"); }

// process_frames for a 4:2:2 / 4:4:4 set with the front-end on: chunks in
// order on s, so the dynamic peak's state sees the frames in order and chunk
// i + 1's front-end overwrites the scratch after chunk i's conversion
int process_decimated(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, int nframes, hipStream_t s,
                      Format in_fmt, Format out_fmt, int dovi_f0) {
  Decimated d;
  int rc;
  if ((rc = decimate_begin(c, in, nframes, s, in_fmt, &d))) return rc;
  // (what process_frames would refuse is refused before anything is queued)
  KParams k;
  if ((rc = prepare(c, &k))) return rc;
  k.dovi_f0 = dovi_f0;
  if ((rc = check_dovi(c, k, d.fmt, dovi_f0, nframes))) return rc;
  if ((rc = check_frames(c, out, c->params.bits_out, "output", out_fmt))) return rc;
  if (in->width != out->width || in->height != out->height)
    return fail(c, H2S_E_INVALID_ARG, "input and output frame sizes differ");
  if (nframes == 0) return 0;
  DeviceGuard g(c->device);
  for (int f0 = 0; f0 < nframes; f0 += d.per) {
    const int nf = std::min(d.per, nframes - f0);
    const h2s_frames ci = frames_at(in, f0), co = frames_at(out, f0);
    h2s_frames view;
    if ((rc = decimate_chunk(c, d, &ci, nf, s, &view))) return queued_exit(c, s, rc);
    if ((rc = process_frames(c, &view, &co, nf, s, d.fmt, out_fmt, dovi_f0 + f0))) return queued_exit(c, s, rc);
  }
  if ((rc = decimate_end(c, s))) return queued_exit(c, s, rc);
  return 0;
}

}  // namespace host
}  // namespace h2s

extern "C" {

int h2s_set_input_decimation(h2s_ctx* c, int mode) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (mode != H2S_DECIMATE_OFF && mode != H2S_DECIMATE_BICUBIC)
    return fail(c, H2S_E_INVALID_ARG, "unknown input decimation");
  // (only the arguments of later launches change: nothing queued reads this)
  c->decimate = mode;
  return 0;
}

}  // extern "C"
