// h2s_api_rgb.hip — the converted frames as an R'G'B' tensor on the device
// (h2s_process_rgb, include/h2s.h): h2s_process_scaled's pipeline with one more
// stage.  Chunk by chunk on the caller's stream: the chain runs unchanged into
// the scaled output's planar scratch at full size, k_scale420 (h2s_scale.hip)
// resizes the chunk into a second planar region of that scratch when the sizes
// differ, and k_rgb420 (h2s_rgb.hip) turns that region, or the full-size one,
// into the caller's tensor.  The scratch, its guard and the cached tap tables
// are h2s_process_scaled's.
#include "h2s_host.h"
#include "h2s_rgb.h"

using namespace h2s::host;
using h2s::RgbParams;

namespace {

int elem_size(int dtype) { return dtype == H2S_RGB_U8 ? 1 : (dtype == H2S_RGB_F32 ? 4 : 2); }

int check_rgb(h2s_ctx* c, const h2s_rgb_frames* o) {
  if (!o) return fail(c, H2S_E_INVALID_ARG, "RGB output is NULL");
  if (!o->data) return fail(c, H2S_E_INVALID_ARG, "RGB output data is NULL");
  if (o->width <= 0 || o->height <= 0 || (o->width & 1) || (o->height & 1))
    return fail(c, H2S_E_INVALID_ARG, "the RGB target needs positive, even width and height");
  if (o->dtype < H2S_RGB_U8 || o->dtype > H2S_RGB_F32) return fail(c, H2S_E_INVALID_ARG, "unknown RGB dtype");
  if (o->layout != H2S_RGB_HWC && o->layout != H2S_RGB_CHW) return fail(c, H2S_E_INVALID_ARG, "unknown RGB layout");
  for (int k = 0; k < 3; k++) {
    if (!isfinite(o->scale[k]) || !isfinite(o->bias[k]))
      return fail(c, H2S_E_INVALID_ARG, "RGB scale and bias must be finite");
    if (o->dtype == H2S_RGB_U8 && (o->scale[k] != 1.0f || o->bias[k] != 0.0f))
      return fail(c, H2S_E_INVALID_ARG, "H2S_RGB_U8 takes scale 1 and bias 0 (normalisation is for the float dtypes)");
  }
  const long long E = elem_size(o->dtype);
  const bool chw = o->layout == H2S_RGB_CHW;
  if (o->row_pitch % E || o->frame_pitch % E || (chw && o->plane_pitch % E))
    return fail(c, H2S_E_INVALID_ARG, "RGB pitches must be multiples of the element size");
  if ((uintptr_t)o->data % E) return fail(c, H2S_E_INVALID_ARG, "RGB data is not aligned to the element size");
  if (o->row_pitch < (chw ? 1 : 3) * E * o->width) return fail(c, H2S_E_INVALID_ARG, "RGB row_pitch is smaller than a row");
  if (chw && o->plane_pitch < o->row_pitch * o->height)
    return fail(c, H2S_E_INVALID_ARG, "RGB plane_pitch is smaller than a plane");
  if (o->frame_pitch < (chw ? 3 * o->plane_pitch : o->row_pitch * o->height))
    return fail(c, H2S_E_INVALID_ARG, "RGB frame_pitch is smaller than a frame");
  return 0;
}

// k_rgb420 over nf frames of the planar scratch set `src` into frames f0.. of the tensor
int launch_rgb(h2s_ctx* c, const h2s_frames* src, const h2s_rgb_frames* o, int f0, int nf, hipStream_t s) {
  const bool chw = o->layout == H2S_RGB_CHW;
  const int q = src->bits - c->k.shift_out;   // the chain's quantising depth
  const double sc = (double)(1 << (q - 8));
  RgbParams P{};
  P.y = (const uint8_t*)src->data[0], P.u = (const uint8_t*)src->data[1], P.v = (const uint8_t*)src->data[2];
  P.yls = src->linesize[0], P.cls = src->linesize[1], P.sfp = src->frame_pitch[0];
  P.dst = (uint8_t*)o->data + (long long)f0 * o->frame_pitch;
  P.rp = o->row_pitch, P.pp = chw ? o->plane_pitch : 0, P.fp = o->frame_pitch;
  P.w = o->width, P.h = o->height;
  P.shift = c->k.shift_out;
  P.yoff = (float)(16.0 * sc), P.coff = (float)(128.0 * sc);
  P.inv = o->dtype == H2S_RGB_U8 ? (float)(1.0 / sc) : (float)(1.0 / (255.0 * sc));
  for (int k = 0; k < 3; k++) P.scale[k] = o->scale[k], P.bias[k] = o->bias[k];
  P.vec = !((uintptr_t)o->data % 16 || o->row_pitch % 16 || o->frame_pitch % 16 || (chw && o->plane_pitch % 16));
  timing_begin(c, s);
  const hipError_t e = h2s::launch_rgb420(P, src->bits == 8 ? 1 : 2, o->dtype, o->layout, nf, s);
  timing_end(c, s);
  return e == hipSuccess ? 0 : hip_fail(c, e, "rgb kernel launch");
}

}  // namespace

extern "C" {

int h2s_process_rgb(h2s_ctx* c, const h2s_frames* in, const h2s_rgb_frames* out, int nframes, void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  hipStream_t s = (hipStream_t)hip_stream;
  const Format in_fmt = c->in_fmt;
  if (nframes < 0) return fail(c, H2S_E_INVALID_ARG, "nframes < 0");
  if (!c->params_set) return fail(c, H2S_E_INVALID_ARG, "h2s_set_params was not called");
  int rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", in_fmt))) return rc;
  if ((rc = check_rgb(c, out))) return rc;
  const int W = in->width, H = in->height, ow = out->width, oh = out->height;
  const bool scale = ow != W || oh != H;
  // (h2s_process_scaled's limits)
  if (scale && (ow > 4 * 8192 || oh > 4 * 8192 || (double)W / ow > 12.0 || (double)H / oh > 12.0))
    return fail(c, H2S_E_UNSUPPORTED, "RGB output: resize ratio out of range");
  if (nframes == 0) return 0;
  DeviceGuard g(c->device);

  // the scratch: one chunk of the chain's frames, then (sizes differ) the chunk at the target size
  const int per = std::min(nframes, kChunk);
  const int bits = c->params.bits_out;
  const h2s_frames mid0 = scratch_frames(W, H, bits, nullptr);
  const size_t mid_bytes = (size_t)mid0.frame_pitch[0] * per;
  const size_t need = mid_bytes + (scale ? (size_t)scratch_frames(ow, oh, bits, nullptr).frame_pitch[0] * per : 0);
  if ((rc = c->scale_use.wait(c, s, "RGB output ordering"))) return rc;
  if (need > c->d_scale.cap && c->d_scale) {
    // an earlier call's kernels may still use the old scratch
    drain_launches(c);
    hipStreamSynchronize(s);
  }
  if ((rc = c->d_scale.reserve(c, need, "RGB output scratch"))) return rc;
  if (scale && (rc = ensure_taps(c, W, H, ow, oh, s))) return queued_exit(c, s, rc);
  const h2s_frames mid = scratch_frames(W, H, bits, c->d_scale);
  const h2s_frames small = scratch_frames(ow, oh, bits, c->d_scale + mid_bytes);

  // chunks in order on s: the dynamic peak's state sees the frames in order, and
  // chunk i + 1's conversion overwrites the scratch after chunk i's last kernel
  for (int f0 = 0; f0 < nframes; f0 += per) {
    const int nf = std::min(per, nframes - f0);
    const h2s_frames ci = frames_at(in, f0);
    if ((rc = process_frames(c, &ci, &mid, nf, s, in_fmt, PLANAR_420, f0))) return queued_exit(c, s, rc);
    if (scale && (rc = launch_chunk(c, &mid, &small, nf, PLANAR_420, s))) return queued_exit(c, s, rc);
    if ((rc = launch_rgb(c, scale ? &small : &mid, out, f0, nf, s))) return queued_exit(c, s, rc);
  }
  if ((rc = c->scale_use.mark(c, s, "RGB output event"))) return queued_exit(c, s, rc);
  return note_launch(c, s);
}

}  // extern "C"
