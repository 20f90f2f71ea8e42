// h2s_api_preview.hip — the preview's two panes: the converted pane (the
// chain's 8-bit output, resized, matrixed to RGB24 and passed through the
// display gamma) and the source pane (the frames as decoded).  What the panes
// share is here once: the RGB output's checks, staging and download, the
// scratch reservation and its carving, and the tap tables.
#include "h2s_host.h"

using namespace h2s::host;
using h2s::KParams;

namespace {

// the caller's RGB24 frames, and where the kernels write them: in place for a
// device output, else into a tight staging copy that download() brings back
struct RgbOut {
  uint8_t* rgb;
  long long ls, fp;
  int w, h;
  bool host;
  uint8_t* d = nullptr;   // device side (stage)
  long long dls = 0, dfp = 0;

  int check(h2s_ctx* c, int nframes) const {
    if (nframes < 1) return fail(c, H2S_E_INVALID_ARG, "nframes must be >= 1");
    if (!rgb || w <= 0 || h <= 0 || ls < 3LL * w || (nframes > 1 && fp < ls * h))
      return fail(c, H2S_E_INVALID_ARG, "bad RGB output geometry");
    return 0;
  }
  // the resize from W x H, once the input set is known good; *scale: there is one
  int check_ratio(h2s_ctx* c, int W, int H, bool* scale) const {
    *scale = w != W || h != H;
    if (*scale && (w > 4 * 8192 || h > 4 * 8192 || (double)W / w > 12.0 || (double)H / h > 12.0))
      return fail(c, H2S_E_UNSUPPORTED, "preview resize ratio out of range");
    return 0;
  }
  size_t stage_bytes(int nframes) const { return host ? (size_t)w * 3 * h * nframes : 0; }
  void stage(uint8_t* scratch) {
    d = host ? scratch : rgb;
    dls = host ? 3LL * w : ls;
    dfp = host ? 3LL * w * h : fp;
  }
  hipError_t download(int nframes, hipStream_t s) const {
    hipError_t e = hipSuccess;
    for (int f = 0; host && f < nframes && e == hipSuccess; f++)
      e = hipMemcpy2DAsync(rgb + (long long)f * fp, ls, d + f * dfp, dls, 3 * (size_t)w, h, hipMemcpyDeviceToHost, s);
    return e;
  }
};

// the preview scratch (c->d_prev) as 256-byte aligned pieces: take() every
// piece, reserve() the sum, then at() gives each piece's address
struct Scratch {
  size_t size = 0;
  uint8_t* base = nullptr;
  size_t take(size_t bytes) {
    const size_t at = size;
    size += (bytes + 255) / 256 * 256;
    return at;
  }
  int reserve(h2s_ctx* c, hipStream_t s) {
    if (size > c->d_prev.cap && c->d_prev) {
      // a previous preview's kernels may still read the old scratch
      drain_launches(c);
      hipStreamSynchronize(s);
    }
    if (int rc = c->d_prev.reserve(c, size, "preview scratch")) return rc;
    base = c->d_prev;
    return 0;
  }
  template <class T = uint8_t>
  T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
};

// the tap tables of one resize (resize_taps): four axes, each with its own
// width T, the weights packed into one float array and the first taps into one
// int array (one upload each)
struct Taps {
  enum Axis { X, Y, CX, CY };
  int T[4] = {0, 0, 0, 0};
  size_t woff[4] = {0, 0, 0, 0}, soff[4] = {0, 0, 0, 0};
  std::vector<float> w;
  std::vector<int> s;
  const float* dw = nullptr;
  const int* ds = nullptr;
  void add(Axis a, int src, int dst) {
    woff[a] = w.size(), soff[a] = s.size();
    T[a] = resize_taps(src, dst, &w, &s);
  }
  hipError_t upload(float* w_dev, int* s_dev, hipStream_t st) {
    dw = w_dev, ds = s_dev;
    hipError_t e = hipMemcpyAsync(w_dev, w.data(), w.size() * 4, hipMemcpyHostToDevice, st);
    return e == hipSuccess ? hipMemcpyAsync(s_dev, s.data(), s.size() * 4, hipMemcpyHostToDevice, st) : e;
  }
  const float* wt(Axis a) const { return dw + woff[a]; }
  const int* st(Axis a) const { return ds + soff[a]; }
};

}  // namespace

extern "C" {

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

int h2s_preview_rgb24_batch(h2s_ctx* c, const h2s_frames* in, int nframes, uint8_t* rgb, int64_t rgb_linesize,
                            int64_t rgb_frame_pitch, int out_w, int out_h, double display_gamma, int rgb_location,
                            void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  RgbOut o{rgb, rgb_linesize, rgb_frame_pitch, out_w, out_h, rgb_location == H2S_LOC_HOST};
  int rc = o.check(c, nframes);
  if (rc) return rc;
  if (!(display_gamma > 0.0)) return fail(c, H2S_E_INVALID_ARG, "display gamma must be > 0");
  if (!c->params_set) return fail(c, H2S_E_INVALID_ARG, "h2s_set_params was not called");
  if (c->params.bits_out != 8)
    return fail(c, H2S_E_INVALID_ARG, "preview needs params.bits_out == 8 (the chain's yuv420p)");
  if ((rc = check_frames(c, in, c->params.bits_in, "input", c->in_fmt))) return rc;
  const int W = in->width, H = in->height;
  bool scale;
  if ((rc = o.check_ratio(c, W, H, &scale))) return rc;
  DeviceGuard g(c->device);
  hipStream_t s = (hipStream_t)hip_stream;
  const int ow2 = (out_w + 1) / 2, oh2 = (out_h + 1) / 2;
  Taps t;
  if (scale) {
    t.add(Taps::X, W, out_w), t.add(Taps::Y, H, out_h);
    t.add(Taps::CX, W / 2, ow2), t.add(Taps::CY, H / 2, oh2);
  }
  uint8_t glut[256];
  for (int i = 0; i < 256; i++) {
    // PIL point() with round() of pow(i/255, 1/gamma)*255 (round half to even)
    const double v = display_gamma == 1.0 ? (double)i : pow(i / 255.0, 1.0 / display_gamma) * 255.0;
    const double r = nearbyint(v);
    glut[i] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
  }
  // scratch: chain output (yuv420p), resized planes, tap tables, RGB, gamma LUT
  const size_t n = (size_t)nframes;
  const size_t yfp = (size_t)W * H * 3 / 2;                             // tight yuv420p frame
  const size_t sfp = (size_t)out_w * out_h + 2 * (size_t)ow2 * oh2;    // one resized frame
  Scratch sc;
  const size_t o_yuv = sc.take(yfp * n), o_syuv = sc.take(scale ? sfp * n : 0);
  const size_t o_w = sc.take(t.w.size() * 4), o_s = sc.take(t.s.size() * 4);
  const size_t o_rgb = sc.take(o.stage_bytes(nframes)), o_glut = sc.take(256);
  if ((rc = sc.reserve(c, s))) return rc;
  o.stage(sc.at(o_rgb));
  // the chain's output here is the call's own yuv420p scratch: planar, whatever
  // layout the context writes its callers' frames in
  h2s_frames y8{};
  y8.width = W, y8.height = H, y8.bits = 8, y8.location = H2S_LOC_DEVICE;
  y8 = tight(&y8, sc.at(o_yuv), PLANAR_420);
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
      const h2s_frames fi = frames_at(in, f), fo = frames_at(&y8, f);
      if ((e = hipMemsetAsync(c->d_pk, 0, pb, s)) != hipSuccess)
        return restored(queued_exit(c, s, hip_fail(c, e, "peak state reset")));
      // (frame f of the call: its Dolby Vision record, h2s_set_dovi)
      if ((rc = process_frames(c, &fi, &fo, 1, s, c->in_fmt, PLANAR_420, f))) return restored(rc);
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
  if (scale) {
    uint8_t* sy_ = sc.at(o_syuv);
    uint8_t* su_ = sy_ + (size_t)out_w * out_h;
    uint8_t* sv_ = su_ + (size_t)ow2 * oh2;
    const long long sp = (long long)sfp;
    e = t.upload(sc.at<float>(o_w), sc.at<int>(o_s), s);
    if (e == hipSuccess)
      e = h2s::launch_resize_u8(yp, W, H, W, fp, sy_, out_w, out_h, out_w, sp, t.wt(Taps::X), t.st(Taps::X),
                                t.T[Taps::X], t.wt(Taps::Y), t.st(Taps::Y), t.T[Taps::Y], nframes, s);
    auto chroma = [&](const uint8_t* src, uint8_t* dst) {
      return h2s::launch_resize_u8(src, W / 2, H / 2, W / 2, fp, dst, ow2, oh2, ow2, sp, t.wt(Taps::CX), t.st(Taps::CX),
                                   t.T[Taps::CX], t.wt(Taps::CY), t.st(Taps::CY), t.T[Taps::CY], nframes, s);
    };
    if (e == hipSuccess) e = chroma(up, su_);
    if (e == hipSuccess) e = chroma(vp, sv_);
    yp = sy_, up = su_, vp = sv_, yls = out_w, cls = ow2, fp = sp;
  }
  uint8_t* dglut = sc.at(o_glut);
  if (e == hipSuccess) e = hipMemcpyAsync(dglut, glut, 256, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = h2s::launch_yuv8_rgb24(yp, yls, up, vp, cls, fp, out_w, out_h, o.d, o.dls, o.dfp, dglut, nframes, s);
  if (e == hipSuccess) e = o.download(nframes, s);
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
  RgbOut o{rgb, rgb_linesize, rgb_frame_pitch, out_w, out_h, rgb_location == H2S_LOC_HOST};
  int rc = o.check(c, nframes);
  if (rc) return rc;
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
  if ((rc = check_frames(c, in, in->bits, "input", fmt))) return rc;
  const int W = in->width, H = in->height, bits = in->bits;
  bool scale;
  if ((rc = o.check_ratio(c, W, H, &scale))) return rc;
  DeviceGuard g(c->device);
  hipStream_t s = (hipStream_t)hip_stream;
  const int cw = W >> fmt.cxs(), ch = H >> fmt.cys(), ow2 = (out_w + 1) / 2;
  Taps t;
  if (scale) t.add(Taps::X, W, out_w), t.add(Taps::Y, H, out_h);
  t.add(Taps::CX, cw, ow2), t.add(Taps::CY, ch, out_h);
  // scratch: a host set's tight device copy, the tap tables, the RGB staging of a host output
  const bool host_in = in->location == H2S_LOC_HOST;
  Scratch sc;
  const size_t o_in = sc.take(host_in ? frame_bytes(in, fmt) * (size_t)nframes : 0);
  const size_t o_w = sc.take(t.w.size() * 4), o_s = sc.take(t.s.size() * 4), o_rgb = sc.take(o.stage_bytes(nframes));
  if ((rc = sc.reserve(c, s))) return rc;
  o.stage(sc.at(o_rgb));
  const h2s_frames din = device_view(in, sc.at(o_in), fmt);
  KParams k{};  // the source set as the conversion kernels bind it
  fill_geometry(&k, &din, nullptr, nframes, fmt, PLANAR_420);
  hipError_t e = t.upload(sc.at<float>(o_w), sc.at<int>(o_s), s);
  h2s::SrcPreviewParams P{};
  for (int p = 0; p < 3; p++) P.in[p] = k.in[p], P.ls[p] = k.in_ls[p], P.fp[p] = k.in_fp[p];
  P.cstep = k.in_cstep, P.sh = k.in_sh, P.mask = (1 << bits) - 1;
  P.W = W, P.H = H, P.cw = k.icw, P.ch = k.ich;
  P.ow = out_w, P.oh = out_h, P.ow2 = ow2;
  P.rgb = o.d, P.rls = o.dls, P.rfp = o.dfp;
  P.identity = scale ? 0 : 1;
  P.Tx = t.T[Taps::X], P.Ty = t.T[Taps::Y], P.Tcx = t.T[Taps::CX], P.Tcy = t.T[Taps::CY];
  P.wx = t.wt(Taps::X), P.wy = t.wt(Taps::Y), P.wcx = t.wt(Taps::CX), P.wcy = t.wt(Taps::CY);
  P.sx = t.st(Taps::X), P.sy = t.st(Taps::Y), P.scx = t.st(Taps::CX), P.scy = t.st(Taps::CY);
  const SourceConsts sk = source_consts(bits, fmt.full(), matrix);
  P.y_off = (int)sk.y_black, P.mid = (int)sk.mid;
  P.y_inv = (float)sk.y_scale, P.c_inv = (float)sk.c_scale;
  P.m_rcr = (float)sk.m_rcr, P.m_bcb = (float)sk.m_bcb, P.m_gcr = (float)sk.m_gcr, P.m_gcb = (float)sk.m_gcb;
  P.round8 = rgb_model == H2S_SRC_RGB_ROUND8;
  if (e == hipSuccess && host_in) e = copy_frames(&din, in, nframes, s, fmt);
  if (e == hipSuccess) {
    timing_begin(c, s);  // (h2s_set_timing: the kernel alone, without the copies around it)
    e = h2s::launch_source_rgb24(P, nframes, s);
    timing_end(c, s);
  }
  if (e == hipSuccess) e = o.download(nframes, s);
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

}  // extern "C"
