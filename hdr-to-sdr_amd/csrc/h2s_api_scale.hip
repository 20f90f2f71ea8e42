// h2s_api_scale.hip — convert and downscale in one call (h2s_process_scaled,
// include/h2s.h): the chain runs unchanged into a context-owned planar scratch
// at full size, chunk by chunk, and k_scale420 (h2s_scale.hip) resizes each
// chunk's planes into the caller's frames.  The tap tables are cached in the
// context and uploaded once per (W, H, ow, oh).
#include "h2s_host.h"
#include "h2s_scale.h"

using namespace h2s::host;
using h2s::KParams;
using h2s::ScaleParams;
using h2s::ScalePlane;

namespace {

long long round_up(long long v, long long a) { return (v + a - 1) / a * a; }

}  // namespace

// (library-private, h2s_host.h: h2s_process_rgb runs the same scratch, tables and resize launch)
namespace h2s {
namespace host {

// the chain's output of one chunk: planar 4:2:0 at `bits`, every row start
// 16-byte aligned (k_scale420 reads it in 16-byte pieces; the tile kernel
// takes it), frames a multiple of 256 bytes apart
h2s_frames scratch_frames(int W, int H, int bits, uint8_t* base) {
  const long long bps = bits == 8 ? 1 : 2;
  h2s_frames f{};
  f.width = W, f.height = H, f.bits = bits, f.location = H2S_LOC_DEVICE;
  const long long yls = round_up(W * bps, 16), cls = round_up(W / 2 * bps, 16);
  const long long fp = round_up(yls * H + 2 * cls * (H / 2), 256);
  f.data[0] = base, f.data[1] = base + yls * H, f.data[2] = base + yls * H + cls * (H / 2);
  f.linesize[0] = yls, f.linesize[1] = f.linesize[2] = cls;
  f.frame_pitch[0] = f.frame_pitch[1] = f.frame_pitch[2] = fp;
  return f;
}

// the tables for W x H -> ow x oh are the context's and on the device.  A new
// key rewrites them: the launches that read the old ones are waited for first
// (Scratch::reserve's rule, h2s_api_preview.hip)
int ensure_taps(h2s_ctx* c, int W, int H, int ow, int oh, hipStream_t s) {
  return fill_taps(c, c->scale_taps, W, H, ow, oh, s);
}

int fill_taps(h2s_ctx* c, ScaleTaps& t, int W, int H, int ow, int oh, hipStream_t s) {
  if (t.W == W && t.H == H && t.ow == ow && t.oh == oh) return 0;
  if (t.d_w) {
    drain_launches(c);
    hipStreamSynchronize(s);
  }
  t.W = 0;   // (no key while the tables are in pieces)
  t.w.clear(), t.s.clear();
  const int src[4] = {W, H, W / 2, H / 2}, dst[4] = {ow, oh, ow / 2, oh / 2};
  for (int a = 0; a < 4; a++) {
    t.woff[a] = t.w.size(), t.soff[a] = t.s.size();
    t.T[a] = resize_taps(src[a], dst[a], &t.w, &t.s);
  }
  int rc;
  if ((rc = t.d_w.reserve(c, t.w.size() * sizeof(float), "scale weights")) ||
      (rc = t.d_s.reserve(c, t.s.size() * sizeof(int), "scale taps")))
    return rc;
  // (the host arrays are the cache's own and outlive the copies)
  hipError_t e = hipMemcpyAsync(t.d_w, t.w.data(), t.w.size() * sizeof(float), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(t.d_s, t.s.data(), t.s.size() * sizeof(int), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_fail(c, e, "scale tap upload");
  t.uploads++;
  t.W = W, t.H = H, t.ow = ow, t.oh = oh;
  return 0;
}

}  // namespace host
}  // namespace h2s

namespace {

// One entry of the launch.  The rows a block owns: the most (up to
// SCALE_MAX_ROWS) whose source rows, with the entry's other pieces, fit the LDS
// budget: the smaller one while that leaves SCALE_ROWS_SMALL rows, else the
// whole; at the ratio limit (49 taps on both axes) that is one row
int fill_plane(h2s_ctx* c, ScalePlane* L, const ScaleTaps& t, int ax, int ay, int sw, int sh, int ow, int oh, int np,
               int src_bps, int out_bps) {
  L->sw = sw, L->sh = sh, L->ow = ow, L->oh = oh, L->np = np;
  L->wx = t.wt(ax), L->sx = t.st(ax), L->Tx = t.T[ax];
  L->wy = t.wt(ay), L->sy = t.st(ay), L->Ty = t.T[ay];
  const int* sx = t.s.data() + t.soff[ax];
  const int* sy = t.s.data() + t.soff[ay];
  auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
  // (what the kernel stages of a row: from the 16-byte boundary below the first column)
  const int V = 16 / src_bps;
  for (int x0 = 0; x0 < ow; x0 += h2s::SCALE_COLS) {
    const int x1 = std::min(x0 + h2s::SCALE_COLS, ow) - 1;
    const int lo = clampi(sx[x0], 0, sw - 1), hi = clampi(sx[x1] + L->Tx, lo + 1, sw);
    if ((hi - (lo & ~(V - 1)) + V - 1) / V * V > h2s::SCALE_SEG)
      return fail(c, H2S_E_UNSUPPORTED, "scaled output: a strip's source columns exceed the kernel's row segment");
  }
  for (int budget : {h2s::SCALE_LDS_SMALL, h2s::SCALE_LDS}) {
    for (int R = std::min(h2s::SCALE_MAX_ROWS, oh); R >= 1; R--) {
      int span = 0;
      for (int y0 = 0; y0 < oh; y0 += R) {
        const int ye = std::min(y0 + R, oh);
        const int r0 = clampi(sy[y0], 0, sh - 1), r1 = clampi(sy[ye - 1] + L->Ty - 1, r0, sh - 1);
        span = std::max(span, r1 - r0 + 1);
      }
      if (h2s::scale_lds(src_bps, L->Tx, R, np, out_bps, span).total > budget) continue;
      if (budget != h2s::SCALE_LDS && R < std::min(h2s::SCALE_ROWS_SMALL, oh)) break;   // too few rows: the larger budget
      L->rows = R, L->hrows = span;
      L->nsx = (ow + h2s::SCALE_COLS - 1) / h2s::SCALE_COLS;
      L->nblk = L->nsx * ((oh + R - 1) / R);
      return 0;
    }
  }
  return fail(c, H2S_E_UNSUPPORTED, "scaled output: one output row's taps exceed the kernel's LDS budget");
}

}  // namespace

namespace h2s {
namespace host {

bool rows_aligned16(const h2s_frames* f, Format fmt) {
  for (int p = 0; p < fmt.planes(); p++)
    if ((uintptr_t)f->data[p] % 16 || f->linesize[p] % 16 || f->frame_pitch[p] % 16) return false;
  return true;
}

// the launch record of one chunk: mid (the chain's frames) -> dout
int scale_record(h2s_ctx* c, const ScaleTaps& t, const h2s_frames* mid, const h2s_frames* dout, Format out_fmt,
                 ScaleParams* Pout) {
  KParams g{};   // the two sets as the conversion kernels bind them (semi-planar: plane 2 aliases plane 1)
  fill_geometry(&g, mid, dout, 1, PLANAR_420, out_fmt);
  const int src_bps = mid->bits == 8 ? 1 : 2, out_bps = dout->bits == 8 ? 1 : 2;
  const int W = mid->width, H = mid->height, ow = dout->width, oh = dout->height;
  ScaleParams& P = *Pout;
  P = ScaleParams{};
  P.nplanes = out_fmt.planes();
  int rc;
  if ((rc = fill_plane(c, &P.pl[0], t, ScaleTaps::X, ScaleTaps::Y, W, H, ow, oh, 1, src_bps, out_bps))) return rc;
  for (int e = 1; e < P.nplanes; e++)
    if ((rc = fill_plane(c, &P.pl[e], t, ScaleTaps::CX, ScaleTaps::CY, W / 2, H / 2, ow / 2, oh / 2,
                         out_fmt.semi() ? 2 : 1, src_bps, out_bps)))
      return rc;
  for (int e = 0; e < P.nplanes; e++) {
    ScalePlane& L = P.pl[e];
    L.src[0] = g.in[e], L.src[1] = g.in[e == 1 ? 2 : e];
    L.sls = g.in_ls[e], L.sfp = g.in_fp[e];
    L.dst = g.out[e], L.dls = g.out_ls[e], L.dfp = g.out_fp[e];
  }
  P.src_shift = c->k.shift_out, P.qmax = c->k.qmax;
  P.shift_out = c->k.shift_out, P.rep_rs = c->k.expand_rep && c->k.shift_out ? 8 - c->k.shift_out : 31;
  P.out_sh = g.out_sh, P.out_bps = out_bps;
  P.vec_out = rows_aligned16(dout, out_fmt) ? 1 : 0;
  return 0;
}

int launch_scale(h2s_ctx* c, const ScaleParams& P0, int src_bps, int dst_f0, int nf, hipStream_t s) {
  ScaleParams P = P0;
  for (int e = 0; e < P.nplanes; e++) P.pl[e].dst += (long long)dst_f0 * P.pl[e].dfp;
  timing_begin(c, s);
  const hipError_t e = h2s::launch_scale420(P, src_bps, nf, s);
  timing_end(c, s);
  return e == hipSuccess ? 0 : hip_fail(c, e, "scale kernel launch");
}

int launch_chunk(h2s_ctx* c, const h2s_frames* mid, const h2s_frames* dout, int nf, Format out_fmt, hipStream_t s) {
  ScaleParams P;
  if (int rc = scale_record(c, c->scale_taps, mid, dout, out_fmt, &P)) return rc;
  return launch_scale(c, P, mid->bits == 8 ? 1 : 2, 0, nf, s);
}

}  // namespace host
}  // namespace h2s

extern "C" {

int h2s_scaled_size(int in_w, int in_h, int box_w, int box_h, int* out_w, int* out_h) {
  if (int rc = h2s_preview_size(in_w, in_h, box_w, box_h, out_w, out_h)) return rc;   // the aspect fit
  // force_divisible_by=2: each dimension down to even, and not below 2
  *out_w = std::max(*out_w & ~1, 2);
  *out_h = std::max(*out_h & ~1, 2);
  return 0;
}

int h2s_process_scaled(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, int nframes, void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  hipStream_t s = (hipStream_t)hip_stream;
  const Format in_fmt = c->in_fmt, out_fmt = c->out_fmt;
  // equal size: h2s_process and nothing else
  if (in && out && in->width == out->width && in->height == out->height)
    return process_frames(c, in, out, nframes, s, in_fmt, out_fmt);
  if (nframes < 0) return fail(c, H2S_E_INVALID_ARG, "nframes < 0");
  if (!c->params_set) return fail(c, H2S_E_INVALID_ARG, "h2s_set_params was not called");
  int rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", in_fmt))) return rc;
  if (!out) return fail(c, H2S_E_INVALID_ARG, "output frames is NULL");
  if (out->width <= 0 || out->height <= 0 || (out->width & 1) || (out->height & 1))
    return fail(c, H2S_E_INVALID_ARG, "the scaled target needs positive, even width and height");
  if ((rc = check_frames(c, out, c->params.bits_out, "output", out_fmt))) return rc;
  const int W = in->width, H = in->height, ow = out->width, oh = out->height;
  // (RgbOut::check_ratio's limits)
  if (ow > 4 * 8192 || oh > 4 * 8192 || (double)W / ow > 12.0 || (double)H / oh > 12.0)
    return fail(c, H2S_E_UNSUPPORTED, "scaled output: resize ratio out of range");
  if (nframes == 0) return 0;
  DeviceGuard g(c->device);

  // the scratch: one chunk of the chain's frames, then a host output's staging
  const int per = std::min(nframes, kChunk);
  const bool host_out = out->location == H2S_LOC_HOST;
  const h2s_frames mid0 = scratch_frames(W, H, c->params.bits_out, nullptr);
  const size_t mid_bytes = (size_t)mid0.frame_pitch[0] * per;
  const size_t need = mid_bytes + (host_out ? frame_bytes(out, out_fmt) * (size_t)per : 0);
  if ((rc = c->scale_use.wait(c, s, "scaled output ordering"))) return rc;
  if (need > c->d_scale.cap && c->d_scale) {
    // an earlier call's kernels may still use the old scratch
    drain_launches(c);
    hipStreamSynchronize(s);
  }
  if ((rc = c->d_scale.reserve(c, need, "scaled output scratch"))) return rc;
  if ((rc = ensure_taps(c, W, H, ow, oh, s))) return queued_exit(c, s, rc);
  const h2s_frames mid = scratch_frames(W, H, c->params.bits_out, c->d_scale);
  const h2s_frames dout = device_view(out, c->d_scale + mid_bytes, out_fmt);

  // chunks in order on s: the dynamic peak's state sees the frames in order,
  // and chunk i + 1's conversion overwrites the scratch after chunk i's resize
  for (int f0 = 0; f0 < nframes; f0 += per) {
    const int nf = std::min(per, nframes - f0);
    const h2s_frames ci = frames_at(in, f0);
    if ((rc = process_frames(c, &ci, &mid, nf, s, in_fmt, PLANAR_420, f0))) return queued_exit(c, s, rc);
    const h2s_frames co = host_out ? dout : frames_at(&dout, f0);
    if ((rc = launch_chunk(c, &mid, &co, nf, out_fmt, s))) return queued_exit(c, s, rc);
    if (host_out) {
      const h2s_frames ho = frames_at(out, f0);
      const hipError_t e = copy_frames(&ho, &co, nf, s, out_fmt);
      if (e != hipSuccess) return queued_exit(c, s, hip_fail(c, e, "device->host copy"));
    }
  }
  if ((rc = c->scale_use.mark(c, s, "scaled output event"))) return queued_exit(c, s, rc);
  if (host_out) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return queued_exit(c, s, hip_fail(c, e, "stream synchronize"));
    return 0;
  }
  return note_launch(c, s);
}

}  // extern "C"
