// h2s_api.hip — the C-ABI (include/h2s.h): contexts, table and LUT upload,
// frame validation, host staging, h2s_process and kernel timing.  Which kernels
// a call launches is decided once (Route) and carried out by launch_route over
// three primitives: launch_tiles, launch_columns and launch_two_pass.
// The host arithmetic behind the parameters is h2s_resolve.hip's, the dynamic
// peak h2s_api_peak.hip's and the preview h2s_api_preview.hip's (h2s_host.h)
#include <stdio.h>
#include <stdlib.h>

#include "h2s_host.h"

using namespace h2s::host;
using h2s::FastParams;
using h2s::KParams;

namespace {
thread_local std::string g_err;  // errors with no context
}  // namespace

namespace h2s {
namespace host {

int fail(h2s_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  else g_err = msg;
  return code;
}

int hip_fail(h2s_ctx* c, hipError_t e, const char* what) {
  return fail(c, H2S_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

static bool aligned(const void* p, long long a) { return ((uintptr_t)p % (uintptr_t)a) == 0; }

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
static bool planes_aligned(const h2s_frames* f, Format fmt, long long ay, long long ac) {
  for (int p = 0; p < fmt.planes(); p++) {
    const long long a = p ? ac : ay;
    if (!aligned(f->data[p], a) || f->linesize[p] % a || f->frame_pitch[p] % a) return false;
  }
  return true;
}

// vector path needs 16-B luma / 8-B chroma alignment of every row start
// (semi-planar: four pairs of the interleaved plane are one luma-sized access)
// (4:4:4 input: a chroma row is read like a luma row)
static bool vec_ok(const h2s_frames* f, bool out8, Format fmt) {
  const long long ay = out8 ? 8 : 16;
  return planes_aligned(f, fmt, ay, fmt.semi() || fmt.sub == H2S_SUB_444 ? ay : ay / 2);
}

// tile kernel: at least one 64-pixel tile, every row start 16-B aligned (8-B
// for 8-bit output), of the planes each set has
static bool tile_ok(const h2s_frames* in, const h2s_frames* out, bool out8, int tw, Format in_fmt, Format out_fmt) {
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
static bool is_tight(const h2s_frames* f, Format fmt) {
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
// The input's tags (h2s_set_input_tags): the S1 constants are rewritten for
// the set's range (source_kparams, h2s_resolve.hip: the limited-range terms
// resolve() wrote, or the full-range ones); resolve_fast folds the same from
// k.full.  No colour constant is computed here
void fill_geometry(KParams* k, const h2s_frames* in, const h2s_frames* out, int nframes, Format in_fmt,
                   Format out_fmt) {
  k->W = in->width;
  k->H = in->height;
  k->cw = in->width / 2;
  k->ch = in->height / 2;
  k->sub = in_fmt.sub, k->icw = in->width >> in_fmt.cxs(), k->ich = in->height >> in_fmt.cys();
  k->full = in_fmt.full() ? 1 : 0, k->vco = in_fmt.vco() ? 1 : 0;
  source_kparams(k, in->bits, in_fmt.full());
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

// set_params / set_lut rewrite device tables that this context's queued
// kernels may still read: wait for the events recorded after its own
// launches (include/h2s.h), not for the device
int drain_launches(h2s_ctx* c) {
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
int aux_stream(h2s_ctx* c, hipStream_t* out) {
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
int upload_table(h2s_ctx* c, DevBuf& buf, const void* src, size_t bytes, const char* what) {
  if (int rc = buf.reserve(c, bytes, what)) return rc;
  hipError_t e = table_copy(c, buf.p, src, bytes);
  return e == hipSuccess ? 0 : hip_fail(c, e, (std::string(what) + " upload").c_str());
}

// record that this context queued work on stream s (after the launches)
int note_launch(h2s_ctx* c, hipStream_t s) {
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

// an error exit of h2s_process after work was queued on s: record the launch
// event anyway, so that a later set_params / set_lut still waits for that work
// before rewriting the tables it reads (include/h2s.h); if even the event
// cannot be recorded, wait for the stream.  The caller's error stays the one
// reported.
int queued_exit(h2s_ctx* c, hipStream_t s, int rc) {
  const std::string msg = c->err;
  if (note_launch(c, s) != 0) (void)hipStreamSynchronize(s);
  c->err = msg;
  return rc;
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

int prepare(h2s_ctx* c, KParams* k, bool need_lut) {
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
  // Dolby Vision records (h2s_set_dovi): frame 0 of the call takes record 0
  k->dovi = c->dovi_n ? (const h2s::DoviRec*)c->d_dovi : nullptr;
  k->dovi_n = c->dovi_n, k->dovi_f0 = 0;
  return 0;
}

// k restricted to frames [f0, f0 + n)
KParams frame_range(const KParams& k, int f0, int n) {
  KParams kf = k;
  for (int p = 0; p < 3; p++) {
    kf.in[p] += (long long)f0 * kf.in_fp[p];
    kf.out[p] += (long long)f0 * kf.out_fp[p];
  }
  kf.nframes = n;
  kf.total = (long long)n * kf.ch * kf.ngx;
  kf.dovi_f0 += f0;
  return kf;
}

// the width the tile kernel covers: the whole 64-pixel tiles
static int tiled_width(const KParams& k) { return k.W & ~(h2s::TBW - 1); }

// the k_tile instance that converts k's frames (k: resolved, geometry filled)
static h2s::TileKey tile_key_of(const KParams& k, bool dbg) {
  return h2s::tile_key(k, k.in_cstep == 2 || k.out_cstep == 2, dbg);
}

// the tile kernel over the whole 64-pixel tiles of k's frames
hipError_t launch_tiles(const h2s_ctx* c, const KParams& k, const Route& r, const TileOpts& o) {
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
  F.dovi = k.dovi, F.dovi_n = k.dovi_n, F.dovi_f0 = k.dovi_f0;
  if (k.dovi) {
    // the k_tile<2, ...> instances stage luma as the code fraction y / (2^b - 1) and read chroma
    // back from its x8 upsampled centred codes; L'M'S' <= 1 stays inside the EOTF table, so every
    // tile takes the branch-free body; the table's scale is the PQ one whatever params.transfer_in says
    const double full = (double)((256 << k.x_sh) - 1);
    F.ys = (float)(1.0 / full), F.y_off_c = 0.0f;
    F.dv_cs = (float)(1.0 / (8.0 * full)), F.dv_cm = (float)((double)F.c_mid / full);
    F.safe_y = F.safe_c = HUGE_VALF;
    F.log2_lin_scale = F.log2_pq_scale;
  }
  return h2s::launch_fast(F, tile_key_of(k, o.dbg != 0), r.s);
}

// the generic kernel over a column range of k's frames (enum Columns, h2s_host.h)
hipError_t launch_columns(const KParams& k, const Route& r, Columns cols) {
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
hipError_t launch_route(const h2s_ctx* c, const KParams& k, const Route& r) {
  if (c->params.chroma_filter == H2S_CHROMA_BICUBIC) return launch_two_pass(c, k, r);
  if (!r.tile()) return launch_columns(k, r, COLUMNS_ALL);
  const hipError_t e = launch_tiles(c, k, r);
  return e == hipSuccess ? launch_columns(k, r, COLUMNS_RAGGED) : e;
}

// the tile kernel serves: both of the reference's chains (the CPU chain, and
// the libplacebo branch with the LUT on: k_tile<..., LP = 1>), the LUT on at
// N <= 177 (its lattice byte offsets are formed in float32, exact for
// multiples of 4 below 2^26 = 12 * 177^3 + margin) with every value finite
// and in [0, 1] (the CPU chain; the libplacebo branch: any), the default [EXT]
// switches, 10/12-bit input and BASELINE's operators; frames with a 64-wide
// tile and 16-byte aligned rows
static bool fast_params_ok(const h2s_ctx* c, const KParams& k) {
  const h2s_params& p = c->params;
  if (!c->fast_enabled || !h2s::tile_instance(tile_key_of(k, false))) return false;
  // Dolby Vision records: the tile kernel takes the shape profile 5 carries (dovi_tile_shape,
  // h2s_api_dovi.hip); any other record runs on the generic kernel
  if (k.dovi && !c->dovi_tile) return false;
  if (c->lp_exact && k.pipe == h2s::PIPE_LIBPLACEBO) return false;
  // the LUT off runs on the tile kernel for the libplacebo branch only (the
  // CPU chain's legacy closed form stays on the generic kernel)
  if (!k.lut_enabled && k.pipe != h2s::PIPE_LIBPLACEBO) return false;
  // the CPU chain forms lattice byte offsets in float32 (exact to N = 177);
  // the libplacebo branch reads its 8-bit table, any N
  if (k.lut_enabled && c->lut_n > 177 && !k.rgba8) return false;
  // the CPU chain's pre-multiplied lattice (k_build_lut_yuv) is built from clamped nodes, which
  // equals lut3d's blend followed by swscale's clip only while no node needs the clamp: a lattice
  // with a value outside [0, 1] (or not finite) runs on the generic kernel, which blends the raw
  // nodes and clips afterwards, as the oracle does; the 8-bit table is built that way for any lattice
  if (k.lut_enabled && !c->lut_unit && !k.rgba8) return false;
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

// frames [start, ...) of a batch
h2s_frames frames_at(const h2s_frames* f, int start) {
  h2s_frames t = *f;
  for (int p = 0; p < 3; p++) t.data[p] = (uint8_t*)f->data[p] + (long long)start * f->frame_pitch[p];
  return t;
}

// kernel timing (h2s_set_timing): one pair of the event ring around a call's
// launches on s, read back by h2s_kernel_ms
void timing_begin(h2s_ctx* c, hipStream_t s) {
  if (!c->timing) return;
  Event &e0 = c->ev0[c->ev_count % kEvRing], &e1 = c->ev1[c->ev_count % kEvRing];
  (void)e0.get(c, "timing event", hipEventDefault);
  (void)e1.get(c, "timing event", hipEventDefault);
  hipEventRecord(e0.ev, s);
}

void timing_end(h2s_ctx* c, hipStream_t s) {
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
  const int dovi_base = k.dovi_f0;   // (a chunk's Dolby Vision records count frames of the call)
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
    k.dovi_f0 = dovi_base + f0;
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
// dovi_f0: the call's first frame among the context's Dolby Vision records (a
// preview that converts frame by frame passes the frame's index)
int process_frames(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, int nframes, hipStream_t s,
                   Format in_fmt, Format out_fmt, int dovi_f0) {
  if (nframes < 0) return fail(c, H2S_E_INVALID_ARG, "nframes < 0");
  // the 4:2:0 front-end (h2s_set_input_decimation): it calls back with the 4:2:0 set
  if (decimating(c, in_fmt)) return process_decimated(c, in, out, nframes, s, in_fmt, out_fmt, dovi_f0);
  KParams k;
  int rc = prepare(c, &k);
  if (rc) return rc;
  k.dovi_f0 = dovi_f0;
  if ((rc = check_subsampling(c, k, in_fmt))) return rc;
  if ((rc = check_dovi(c, k, in_fmt, dovi_f0, nframes))) return rc;
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

}  // namespace host
}  // namespace h2s

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

int h2s_set_lut(h2s_ctx* c, const float* rgb, int n) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (!rgb || n < 2 || n > 256) return fail(c, H2S_E_INVALID_ARG, "LUT size must be in [2, 256]");
  DeviceGuard g(c->device);
  if (int rc = drain_launches(c)) return rc;
  const size_t cnt = (size_t)n * n * n;
  // zero records behind the lattice, as behind d_lut_yuv (ensure_lut_yuv): k_tile's stage-4 debug
  // plane blends the same four corners on this copy, and a coordinate clamped to exactly N-1 names
  // cell N-1, whose corners past the edge carry weight 0 but are read (up to 1 + N + N^2 records on)
  const size_t all = cnt + 1 + (size_t)n + (size_t)n * n;
  std::vector<float4> host(all, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  bool unit = true;  // (a NaN fails both comparisons)
  for (size_t i = 0; i < cnt; i++) {
    host[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.0f);
    for (int ch = 0; ch < 3; ch++) unit &= rgb[3 * i + ch] >= 0.0f && rgb[3 * i + ch] <= 1.0f;
  }
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
  if (int rc = c->d_lut.reserve(c, all * sizeof(float4), "LUT device")) return rc;
  hipError_t e = table_copy(c, c->d_lut, host.data(), all * sizeof(float4));
  if (e != hipSuccess) return hip_fail(c, e, "LUT upload");
  c->lut_n = n;
  c->lut_unit = unit;
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

int h2s_process(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, int nframes, void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  return process_frames(c, in, out, nframes, (hipStream_t)hip_stream, c->in_fmt, c->out_fmt);
}

int h2s_debug_float(h2s_ctx* c, const h2s_frames* in, int stage, float* out_rgb, int out_location,
                    void* hip_stream) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (stage < H2S_STAGE_LINEAR || stage > H2S_STAGE_YUV) return fail(c, H2S_E_INVALID_ARG, "bad stage");
  if (!out_rgb) return fail(c, H2S_E_INVALID_ARG, "out_rgb is NULL");
  hipStream_t s = (hipStream_t)hip_stream;
  if (!decimating(c, c->in_fmt)) return debug_float(c, in, c->in_fmt, stage, out_rgb, out_location, s);
  // the 4:2:0 front-end first (debug_float waits for s, so the scratch is free on return)
  Decimated d;
  h2s_frames view;
  int rc;
  if ((rc = decimate_begin(c, in, 1, s, c->in_fmt, &d))) return rc;
  DeviceGuard g(c->device);
  if ((rc = decimate_chunk(c, d, in, 1, s, &view))) return queued_exit(c, s, rc);
  rc = debug_float(c, &view, d.fmt, stage, out_rgb, out_location, s);
  const int rc_end = decimate_end(c, s);
  return rc ? rc : rc_end;
}

int h2s_query_path(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out) {
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (!decimating(c, c->in_fmt)) return query_path(c, in, out, c->in_fmt);
  // the answer for the 4:2:0 set the front-end makes (its scratch is 256-byte aligned, like a staged set)
  if (!c->params_set) return fail(c, H2S_E_INVALID_ARG, "h2s_set_params was not called");
  if (int rc = check_frames(c, in, c->params.bits_in, "input", c->in_fmt)) return rc;
  const uint8_t* fake = (const uint8_t*)(uintptr_t)4096;
  Format f420 = c->in_fmt;
  f420.sub = H2S_SUB_420, f420.loc = H2S_CHROMA_LEFT;
  const h2s_frames view = decimated_view(in, c->in_fmt, fake, fake);
  return query_path(c, &view, out, f420);
}

}  // extern "C"

namespace h2s {
namespace host {

// h2s_debug_float for a set of the form given (the context's own, or the 4:2:0 set of its front-end)
int debug_float(h2s_ctx* c, const h2s_frames* in, Format in_fmt, int stage, float* out_rgb, int out_location,
                hipStream_t s) {
  KParams k;
  int rc = prepare(c, &k);
  if (rc) return rc;
  if ((rc = check_subsampling(c, k, in_fmt))) return rc;
  if ((rc = check_dovi(c, k, in_fmt, 0, 1))) return rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", in_fmt))) return rc;
  DeviceGuard g(c->device);
  const size_t npx = (size_t)in->width * in->height, ob = npx * 3 * sizeof(float);
  // scratch: a tight device copy of the input (host input), the float planes
  // (host output) and one output frame for the tile kernel's own stores
  h2s_frames fo{};
  fo.width = in->width, fo.height = in->height, fo.bits = c->params.bits_out, fo.location = H2S_LOC_DEVICE;
  const size_t ib = in->location == H2S_LOC_HOST ? (frame_bytes(in, in_fmt) + 255) / 256 * 256 : 0;
  const size_t fb = (frame_bytes(&fo, PLANAR_420) + 255) / 256 * 256, pb = out_location == H2S_LOC_HOST ? ob : 0;
  Dev<uint8_t> scratch;  // freed on every exit, after s has been waited for
  if ((rc = scratch.reserve(c, ib + fb + pb + 256, "debug"))) return rc;
  uint8_t* base = scratch;
  const h2s_frames din = device_view(in, base, in_fmt);
  hipError_t e;
  if (in->location == H2S_LOC_HOST && (e = copy_frames(&din, in, 1, s, in_fmt)) != hipSuccess)
    return hip_fail(c, e, "debug copy");
  fo = tight(&fo, base + ib, PLANAR_420);   // (the call's own planar scratch frame)
  float* dout = out_location == H2S_LOC_HOST ? (float*)(base + ib + fb) : out_rgb;
  fill_geometry(&k, &din, &fo, 1, in_fmt, PLANAR_420);
  const bool out8 = c->params.bits_out == 8;
  const Route r{choose_path(c, k, &din, &fo, out8, in_fmt, PLANAR_420), false, out8, in_fmt, PLANAR_420, s};
  // the generic debug kernel covers every pixel; on the tile path the tile
  // kernel's debug instance then rewrites the tile columns with its own values
  // (where it has one: there are no debug instances of the tile kernel for
  // 4:2:2 / 4:4:4 input or for a top-left set, whose planes are the generic
  // kernel's whatever the path; a full-range set changes constants only)
  e = h2s::launch_debug(k, stage, dout, s);
  if (e == hipSuccess && r.tile() && h2s::tile_instance(tile_key_of(k, true))) {
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

// h2s_query_path for an input set of the form given
int query_path(h2s_ctx* c, const h2s_frames* in, const h2s_frames* out, Format in_fmt) {
  KParams k;
  int rc = prepare(c, &k);
  if (rc) return rc;
  if ((rc = check_subsampling(c, k, in_fmt))) return rc;
  if ((rc = check_dovi(c, k, in_fmt, 0, 1))) return rc;
  if ((rc = check_frames(c, in, c->params.bits_in, "input", in_fmt))) return rc;
  if ((rc = check_frames(c, out, c->params.bits_out, "output", c->out_fmt))) return rc;
  // host sets are staged into tight device copies, whose alignment decides
  uint8_t* fake = (uint8_t*)(uintptr_t)4096;
  const h2s_frames din = device_view(in, fake, in_fmt), dout = device_view(out, fake, c->out_fmt);
  fill_geometry(&k, &din, &dout, 1, in_fmt, c->out_fmt);
  return choose_path(c, k, &din, &dout, c->params.bits_out == 8, in_fmt, c->out_fmt);
}

}  // namespace host
}  // namespace h2s

extern "C" {

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
    case H2S_OPT_PRIVATE_BASE + 2:   // reserved: H2S_OPT_TEST_PEAK_FORM's key (the quad form's A/B, decided in round 6)
      return fail(c, H2S_E_INVALID_ARG, "option 0x7f000002 is reserved (the peak statistics form is no option)");
    case H2S_OPT_TEST_PEAK_BLOCKS:
      if (value < 1 || value > h2s::PEAK_BLOCKS_MAX) return fail(c, H2S_E_INVALID_ARG, "peak blocks must be in [1, 256]");
      c->peak_blocks = (int)value;
      return 0;
    case H2S_OPT_TEST_SCALE_UPLOADS:
      if (value != c->scale_taps.uploads)
        return fail(c, H2S_E_INVALID_ARG, "scaled-output tap uploads: " + std::to_string(c->scale_taps.uploads));
      return 0;
    case H2S_OPT_TEST_LADDER_UPLOADS:
      if (value != c->ladder_uploads)
        return fail(c, H2S_E_INVALID_ARG, "ladder tap uploads: " + std::to_string(c->ladder_uploads));
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
