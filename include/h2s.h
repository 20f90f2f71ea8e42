/*
 * h2s.h — C-ABI of libh2s, the MI355X-native HDR10/HLG -> SDR tone-mapping
 * hot path.  This is the drop-in boundary for the reference's CPU ffmpeg
 * filter chain.
 *
 * The reference (TORlN/HDR-to-SDR) has no native FFI of its own: its hot path
 * is the filtergraph string
 *
 *   zscale=t=linear:npl=100,tonemap={tm},zscale=t=bt709:m=bt709:r=tv,
 *   lut3d=file={lut}:interp=tetrahedral,setparams=...bt709,eq=gamma={g}
 *
 * (src/utils.py:38-42), formatted by ffmpeg_command._filter_args
 * (src/ffmpeg_command.py:227-247) and executed frame by frame inside an ffmpeg
 * child process (src/conversion.py:209-224).  Each entry point below names
 * the reference interface it replaces.  All signatures use plain C types:
 * pointers, sizes and POD structs — no torch or HIP types leak through.
 *
 * Threading: every function is callable from any thread.  A context must not
 * be used by two threads at once (one context per worker / GPU), and contexts
 * share no mutable global state.  h2s_process is asynchronous on the stream
 * it is given when both frame sets live in device memory; the caller
 * synchronises.  h2s_set_params and h2s_set_lut first wait for every launch
 * the context has queued (on any stream) to finish, so replacing the tables a
 * kernel in flight reads is safe; they wait on events recorded after the
 * context's own launches only, never on other contexts or on unrelated work
 * on the device.  One context may be given different streams from call to
 * call: scratch that its calls share (the BICUBIC plane, the peak state, and
 * the tables the first h2s_process after h2s_set_lut derives from the lattice
 * on its own stream) is ordered across those streams on the device.
 *
 * Errors: 0 on success, a negative H2S_E_* code otherwise; the message is
 * available from h2s_last_error(ctx) (or h2s_last_error(NULL) for failures
 * that happen before a context exists).  The Python host maps the codes to the
 * reference's exception types (ValueError / FileNotFoundError / RuntimeError,
 * src/ffmpeg_command.py:240-245, src/utils.py:185-186, src/utils.py:297-308).
 */
#ifndef H2S_H
#define H2S_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2S_ABI_VERSION 3
/* Minor revision within ABI 3 (h2s_abi_minor), for bindings that need to
 * detect additions and behaviour changes that keep every v3 signature:
 *   1: h2s_preview_rgb24_batch; the lp_p010 default TRUNCATE (the reference's
 *      format=p010 upload; 12-bit libplacebo-branch output changes);
 *   2: h2s_process with params.peak_detect is asynchronous on its stream (the
 *      peak statistics, smoothing and curve constants run on the device);
 *      h2s_peak_state / _reset / _feed wait for the context's queued work; a
 *      preview restores the context's peak state; the failure-injection test
 *      hook moved to the private option range (H2S_PRIVATE_TEST_HOOKS);
 *   3: H2S_OPT_LP_EXACT (then key 4);
 *   4: H2S_OPT_LP_EXACT moves to key 5 and key 4 is reserved (H2S_E_INVALID_ARG:
 *      a 3.0 / 3.1 client that set key 4 as the old failure-injection hook
 *      fails loudly instead of switching kernels); the libplacebo branch's
 *      exact path computes stages 1-3 in double precision (see below).
 * Added within 3.4, with no change of either number: h2s_set_frame_layout
 * (semi-planar nv12 / p010le / p012le frame sets); h2s_set_input_subsampling
 * (4:2:2 / 4:4:4 planar input on the CPU chain); h2s_set_input_tags (a
 * source's full-range and top-left chroma tags); h2s_preview_source_rgb24 /
 * _batch (the preview's source pane: the unconverted frame as RGB24);
 * h2s_set_dovi (Dolby Vision profile 5: per-frame RPU records);
 * h2s_scaled_size / h2s_process_scaled (convert and downscale in one call:
 * scaled 4:2:0 output); h2s_set_input_decimation (a 4:2:2 / 4:4:4 source
 * decimated to 4:2:0 on the device in front of either pipeline);
 * h2s_process_rgb (the converted frames as an R'G'B' tensor on the device:
 * u8 / half / bfloat16 / float32, HWC or CHW, normalised);
 * h2s_process_ladder (a rendition ladder, several sizes of the 4:2:0 output,
 * from one conversion of each frame).  No existing
 * struct, signature or default behaviour changes, so the symbol's presence in
 * the loaded library is the feature test. */
#define H2S_ABI_MINOR 4

/* ---- error codes ------------------------------------------------------- */
#define H2S_OK 0
#define H2S_E_INVALID_ARG (-1)  /* bad pointer / size / enum value        */
#define H2S_E_UNSUPPORTED (-2)  /* valid request this build cannot serve  */
#define H2S_E_HIP (-3)          /* HIP runtime error (message has detail) */
#define H2S_E_OOM (-4)          /* device or host allocation failed       */
#define H2S_E_LUT_MISSING (-5)  /* lut_enabled but no LUT loaded          */
#define H2S_E_PARSE (-6)        /* malformed .cube / filter text          */

/* ---- enums ------------------------------------------------------------- */
/* Input transfer of the source frames (frame tag read by zscale t=linear). */
enum h2s_transfer { H2S_TRC_PQ = 0, H2S_TRC_HLG = 1 };

/* Tone-map operators.  NONE..MOBIUS are ffmpeg vf_tonemap's `tonemap=`
 * values (the reference exposes reinhard/mobius/hable, src/utils.py:16);
 * BT2390 and SPLINE are the GPU-only operators the reference reaches through
 * libplacebo's `tonemapping=` (GPU_ONLY_TONEMAPPERS, src/utils.py:62-73,
 * :392-471).  SPLINE's tm_param is libplacebo's spline contrast (NaN = 0.5,
 * range 0..1.5). */
enum h2s_tonemap {
  H2S_TM_NONE = 0,
  H2S_TM_LINEAR = 1,
  H2S_TM_GAMMA = 2,
  H2S_TM_CLIP = 3,
  H2S_TM_REINHARD = 4,
  H2S_TM_HABLE = 5,
  H2S_TM_MOBIUS = 6,
  H2S_TM_BT2390 = 7,
  H2S_TM_SPLINE = 8
};

/* Output quantisation.  COMPAT8 reproduces the reference CPU chain's 8-bit
 * bottleneck (eq is 8-bit only, so ffmpeg converts to yuv420p before it and
 * shifts up to the -pix_fmt afterwards, src/ffmpeg_command.py:355-360, :501).
 * NATIVE quantises directly to bits_out. */
enum h2s_mode { H2S_MODE_COMPAT8 = 0, H2S_MODE_NATIVE = 1 };

/* Luma weights tonemap's desaturation uses: vf_tonemap reads the frame's
 * colorspace tag -- bt2020nc if the first zscale (no m=) carries it through,
 * or, if colorspace negotiation retags the float RGB frame, the libavutil RGB
 * entry {1,1,1} (the default).  Switchable because it cannot be pinned
 * without the bundled ffmpeg: the reference's only
 * pixel pair was made on its libplacebo branch, where no vf_tonemap runs. */
enum h2s_desat_luma {
  H2S_DESAT_LUMA_RGB = 0,    /* {1, 1, 1}                 */
  H2S_DESAT_LUMA_BT2020 = 1, /* {0.2627, 0.6780, 0.0593}  */
  H2S_DESAT_LUMA_BT709 = 2   /* {0.2126, 0.7152, 0.0722}  */
};

/* Where a frame set lives. */
enum h2s_location { H2S_LOC_DEVICE = 0, H2S_LOC_HOST = 1 };

/* How a frame set's chroma is stored (h2s_set_frame_layout).  PLANAR: three
 * planes, the code in the low bits (yuv420p / yuv420p10le / yuv420p12le).
 * SEMI: the Y plane and one plane of interleaved (Cb, Cr) pairs, 16-bit
 * samples with the code in the high bits (nv12 / p010le / p012le: what
 * hardware decoders produce and hardware encoders take). */
enum h2s_layout { H2S_LAYOUT_PLANAR = 0, H2S_LAYOUT_SEMI = 1 };

/* Chroma subsampling of an input frame set (h2s_set_input_subsampling).  The
 * output side is always 4:2:0. */
enum h2s_subsampling { H2S_SUB_420 = 0, H2S_SUB_422 = 1, H2S_SUB_444 = 2 };

/* Source tags of an input frame set (h2s_set_input_tags): the colour range of
 * its codes (ffprobe color_range tv / pc) and where its 4:2:0 chroma samples
 * sit (chroma_location left / topleft, HEVC chroma_sample_loc_type 0 / 2).
 * The output side is always limited range. */
enum h2s_range { H2S_RANGE_LIMITED = 0, H2S_RANGE_FULL = 1 };
enum h2s_chroma_loc { H2S_CHROMA_LEFT = 0, H2S_CHROMA_TOPLEFT = 1 };

/* The 4:2:0 front-end of a 4:2:2 / 4:4:4 input set (h2s_set_input_decimation). */
enum h2s_decimation { H2S_DECIMATE_OFF = 0, H2S_DECIMATE_BICUBIC = 1 };

/* Debug stages for h2s_debug_float: three float planes per pixel.
 * 1..4: R, G, B after the stage.  5: the quantiser's inputs, before rounding:
 * plane 0 = luma code (16 + 219 Y) * 2^(q-8), planes 1/2 = the pixel's Cb / Cr
 * in code units, 224 * 2^(q-8) * C (the 4:2:0 sample is 128 * 2^(q-8) plus
 * the chroma filter over these), q = the quantisation depth. */
enum h2s_stage {
  H2S_STAGE_LINEAR = 1,   /* after S1 zscale=t=linear:npl=100          */
  H2S_STAGE_TONEMAP = 2,  /* after S2 tonemap=                          */
  H2S_STAGE_GAMMA = 3,    /* after S3 zscale=t=bt709 (BT.1886 inverse)  */
  H2S_STAGE_LUT = 4,      /* after S4 lut3d=interp=tetrahedral          */
  H2S_STAGE_YUV = 5       /* S6 quantiser inputs (see above)            */
};

/* S6 chroma 4:4:4 -> 4:2:0 filter of the implicit swscale conversion
 * (cannot be pinned without the bundled ffmpeg).
 * BOX: the 2x2 mean of the quad (centre siting).  BICUBIC: swscale's default
 * bicubic (B = 0, C = 0.6) decimation, chroma sited left horizontally (on the
 * even luma column) and centred vertically, edge-clamped. */
enum h2s_chroma_filter { H2S_CHROMA_BOX = 0, H2S_CHROMA_BICUBIC = 1 };

/* Rounding of the 8-bit quantiser (S6 yuv420p, or the libplacebo branch's
 * rgba download).  NONE: round half up.  ORDERED: swscale's 8x8 ordered
 * dither offsets (ff_dither_8x8_128 / 128 of an LSB) instead of +0.5. */
enum h2s_dither { H2S_DITHER_NONE = 0, H2S_DITHER_ORDERED = 1 };

/* S1 chroma upsampler edge rule: the sample the
 * bilinear 2-tap reads past the plane's edge (row -1 above the first chroma
 * row, row ch below the last, column cw right of the last; left-sited chroma
 * never reads column -1).  ZIMG: -1 mirrors to 1, ch / cw fold to the last
 * sample (the round-1 model).  REPLICATE: every edge repeats its last
 * sample.  MIRROR: every edge mirrors about its last sample (ch -> ch-2). */
enum h2s_chroma_edge { H2S_EDGE_ZIMG = 0, H2S_EDGE_REPLICATE = 1, H2S_EDGE_MIRROR = 2 };

/* Format between S3 and S4 on the CPU chain: which
 * pixel format ffmpeg negotiates between zscale=t=bt709 and lut3d.  FLOAT:
 * gbrpf32, lut3d's float path (the round-1 model).  RGB48: 16-bit R'G'B' --
 * zscale rounds to 16 bits, lut3d's 16-bit path reads q (1/65535) (N-1) and
 * truncates its output to 16 bits, swscale converts from there. */
enum h2s_lut_input { H2S_LUT_IN_FLOAT = 0, H2S_LUT_IN_RGB48 = 1 };

/* How the libplacebo branch applies its PQ-domain curve (BT.2390 / SPLINE)
 * to colour.  libplacebo is absent: PARITY UNPINNED.  IPT (default): the
 * curve maps the intensity I of IPT-PQ -- linear BT.2020 -> XYZ -> LMS
 * (Hunt-Pointer-Estevez, D65-normalised), PQ-encoded in absolute
 * luminance, I = 0.4 L' + 0.4 M' + 0.2 S' (Ebner-Fairchild) -- and keeps
 * P and T; libplacebo tone-maps in IPT since v6, and on the reference's own
 * before/after pair this fits best (tests/test_website_fixture.py).
 * MAX_RGB: gain curve(max RGB) / max RGB on R, G, B (the round-2 model). */
enum h2s_lp_tone { H2S_LP_TONE_IPT = 0, H2S_LP_TONE_MAX_RGB = 1 };

/* libplacebo branch: the open options of the reference's stage
 * `libplacebo=...:range=tv:peak_detect=1:format=rgba` (src/utils.py:445-449),
 * each a named model (SURVEY.md App. B style; PARITY UNPINNED, libplacebo and
 * vf_libplacebo are absent from the image).
 * h2s_lp_range: FULL = the rgba download carries full-range codes
 *   round(255 v) (libplacebo ignores range= for an RGB output); LIMITED =
 *   range=tv applies to the RGB output: round(16 + 219 v), which lut3d and
 *   the auto-scale to -pix_fmt then read as full-range RGB.
 * h2s_lp_dither: NONE = the 8-bit download rounds to nearest; ORDERED = a
 *   16 x 16 Bayer matrix offsets each code before the truncation (a stand-in
 *   for libplacebo's default dither, whose blue-noise texture is not
 *   restated: it measures how much the dither matters).
 * h2s_lp_p010: the upload prefix (src/utils.py:430-431).  TRUNCATE (the
 *   default since ABI v3.1: the reference's default `format=p010,hwupload`
 *   prefix) = the 10-bit p010 container drops a 12-bit input's two low bits
 *   (code & ~3); KEEP = the CUDA-interop `hwmap=derive_device=vulkan` prefix,
 *   which maps the decoder's frame without a format conversion, so 12-bit
 *   input reaches libplacebo at full precision.  10-bit input: no effect. */
enum h2s_lp_range { H2S_LP_RANGE_FULL = 0, H2S_LP_RANGE_LIMITED = 1 };
enum h2s_lp_dither { H2S_LP_DITHER_NONE = 0, H2S_LP_DITHER_ORDERED = 1 };
enum h2s_lp_p010 { H2S_LP_P010_KEEP = 0, H2S_LP_P010_TRUNCATE = 1 };

/* S8 8-bit -> bits_out expansion after eq. */
enum h2s_expand { H2S_EXPAND_SHIFT = 0, H2S_EXPAND_REPLICATE = 1 };

/* Which of the reference's two chains the parameters describe.
 * CPU_CHAIN: FFMPEG_CONVERT_FILTER (src/utils.py:38-42): zscale -> tonemap ->
 *   zscale -> lut3d (float) -> yuv420p -> eq -> -pix_fmt.
 * LIBPLACEBO: build_libplacebo_filter (src/utils.py:392-471) with the LUT on:
 *   libplacebo tone map (BT.2390, spline, or libplacebo's own reinhard /
 *   hable / mobius, which the reference also routes there with GPU tone
 *   mapping on) -> BT.1886 encode against the SDR
 *   target -> 8-bit rgba download -> lut3d's 8-bit path (truncating output) ->
 *   Y'CbCr at the output depth (gamma = 1; the chain has no eq) or, with
 *   eq=gamma, yuv420p -> eq -> -pix_fmt.  With the LUT off the branch keeps
 *   libplacebo's own BT.709 conversion and nv12 (8-bit) download.
 * AUTO: LIBPLACEBO for BT2390 / SPLINE (the reference's GPU-only operators
 *   exist only there), CPU_CHAIN otherwise. */
enum h2s_pipeline { H2S_PIPE_AUTO = 0, H2S_PIPE_CPU_CHAIN = 1, H2S_PIPE_LIBPLACEBO = 2 };

/* Context options (h2s_set_option). */
enum h2s_option {
  H2S_OPT_FAST_PATH = 1,       /* 1 (default): the tile kernel where it applies; 0: generic kernel only */
  H2S_OPT_TILES_PER_BLOCK = 2, /* tile kernel: 64x32 tiles one block walks (1..64, default 8)          */
  H2S_OPT_HOST_SERIAL = 3,     /* host frames: 1 = one H2D, kernel, D2H per call (no chunk pipeline)   */
  /* 4: reserved (H2S_E_INVALID_ARG; was H2S_OPT_LP_EXACT in ABI 3.3), as is the private key           */
  /* H2S_OPT_PRIVATE_BASE + 2 (was H2S_OPT_TEST_PEAK_FORM): neither is given a new meaning             */
  H2S_OPT_LP_EXACT = 5         /* 1: the libplacebo branch on its exact path only (see below)           */
};
/* H2S_OPT_LP_EXACT: the libplacebo branch's 8-bit rgba download rounds a
 * float (255 x the BT.1886 encode).  The reference computes it in
 * libplacebo's float32 GLSL, so the restated reference is exact arithmetic;
 * the tile kernel (default, float32) lands within its stated error bound of
 * it and may round a code lying that close to a tie the other way (about
 * 0.1 % of codes; lut3d's 8-bit lattice step then spreads such a flip over a
 * few output steps).  With 1 the branch runs on the generic kernel's exact
 * path, stages 1-3 in double precision from the integer codes: output within
 * one step of the restated reference everywhere, at a multiple of the tile
 * kernel's time. */
/* Keys from H2S_OPT_PRIVATE_BASE up are the library's own test / debug hooks:
 * not part of the ABI, may change or vanish in any build. */
#define H2S_OPT_PRIVATE_BASE 0x7f000000
#ifdef H2S_PRIVATE_TEST_HOOKS
/* 1 = the next h2s_process call reports H2S_E_HIP right after queueing its
 * kernels (the error exits must still record the launch) */
#define H2S_OPT_TEST_FAIL_AFTER_LAUNCH (H2S_OPT_PRIVATE_BASE + 1)
/* H2S_OPT_PRIVATE_BASE + 2: reserved (H2S_E_INVALID_ARG; was H2S_OPT_TEST_PEAK_FORM, the statistics kernels' A/B) */
/* dynamic peak on the tile kernel: frames per pipelined chunk (0 = statistics for
 * the whole batch, then one conversion launch) */
#define H2S_OPT_TEST_PEAK_CHUNK (H2S_OPT_PRIVATE_BASE + 3)
/* peak statistics: blocks (partial records) per frame, 1..256 (default 64) */
#define H2S_OPT_TEST_PEAK_BLOCKS (H2S_OPT_PRIVATE_BASE + 4)
/* a query, not a setting: H2S_OK if the context has uploaded the scaled output's
 * tap tables exactly `value` times, else H2S_E_INVALID_ARG (the count is in
 * h2s_last_error) */
#define H2S_OPT_TEST_SCALE_UPLOADS (H2S_OPT_PRIVATE_BASE + 5)
/* the same query for h2s_process_ladder's own tap tables (one upload per
 * distinct rung size; h2s_process_scaled's count is not touched by a ladder) */
#define H2S_OPT_TEST_LADDER_UPLOADS (H2S_OPT_PRIVATE_BASE + 6)
#endif

/* Kernel path h2s_process takes for a given frame pair (h2s_query_path). */
enum h2s_path {
  H2S_PATH_TILE = 1,       /* k_tile only (width % 64 == 0)                      */
  H2S_PATH_TILE_TAIL = 2,  /* k_tile + k_process on the width % 64 columns       */
  H2S_PATH_GENERIC = 3,    /* k_process                                          */
  H2S_PATH_TWO_PASS = 4    /* k_process per-pixel chroma + bicubic decimation    */
};

/* ---- parameters ---------------------------------------------------------
 * Mirrors the values FFMPEG_CONVERT_FILTER.format(gamma, tonemapper,
 * lut_path) bakes into the chain string (src/ffmpeg_command.py:246-247) plus
 * the chain's hard-coded options (npl=100, desat default, interp) and the
 * output -pix_fmt (src/ffmpeg_command.py:355-360).                        */
typedef struct h2s_params {
  int32_t transfer_in;  /* enum h2s_transfer                               */
  int32_t bits_in;      /* 10 or 12 (yuv420p10le / yuv420p12le)            */
  int32_t bits_out;     /* 8, 10 or 12 (yuv420p / 10le / 12le)             */
  int32_t tonemap;      /* enum h2s_tonemap                                */
  double tm_param;      /* tonemap=param; NaN = vf_tonemap default         */
  double desat;         /* tonemap=desat; reference uses default 2.0       */
  double peak;          /* tonemap=peak; 0 = auto (side data / default)    */
  double npl;           /* zscale npl; reference: 100                      */
  double gamma;         /* eq=gamma; reference: ConversionRequest.gamma    */
  double maxcll;        /* frame side data MaxCLL (nits), 0 = absent       */
  double mastering_max; /* mastering display max luminance, 0 = absent     */
  int32_t lut_enabled;  /* 1: lut3d stage; 0: closed-form BT.2020->709     */
  int32_t mode;         /* enum h2s_mode                                   */
  int32_t desat_luma;   /* enum h2s_desat_luma                             */
  int32_t peak_detect;  /* BT.2390 / SPLINE: 1 = per-frame detected,
                         * temporally smoothed source peak (and, for SPLINE,
                         * average: the knee) (libplacebo peak_detect=1,
                         * src/utils.py:448); state lives in the context   */
  /* [EXT] switches the bundled ffmpeg would settle */
  int32_t chroma_filter; /* enum h2s_chroma_filter (S6)                     */
  int32_t dither;        /* enum h2s_dither (8-bit quantiser)               */
  int32_t expand;        /* enum h2s_expand (S8)                            */
  int32_t pipeline;      /* enum h2s_pipeline                               */
  /* libplacebo branch (BT.2390 / SPLINE); NaN = that branch's default      */
  double knee_offset;    /* BT.2390 knee offset: ks = (1+o) maxLum - o;
                          * libplacebo default 1.0, ITU-R BT.2390 0.5      */
  double target_black;   /* SDR target black (nits); NaN: LIBPLACEBO =
                          * white / 1000 (libplacebo's SDR contrast),
                          * CPU_CHAIN = 0 (no black-point adaptation)      */
  double target_white;   /* SDR target white (nits); NaN: LIBPLACEBO = 203
                          * (libplacebo's SDR white, BT.2408), CPU_CHAIN =
                          * npl                                            */
  int32_t chroma_edge;   /* enum h2s_chroma_edge (S1)                       */
  int32_t lut_input;     /* enum h2s_lut_input (S3 -> S4, CPU chain)        */
  int32_t lp_tone;       /* enum h2s_lp_tone (libplacebo branch)            */
  /* ABI v3: libplacebo branch options (enums above) */
  int32_t lp_range;      /* enum h2s_lp_range                               */
  int32_t lp_dither;     /* enum h2s_lp_dither                              */
  int32_t lp_p010;       /* enum h2s_lp_p010                                */
  int32_t reserved[2];   /* keeps the doubles below 8-byte aligned        */
  /* peak_detect=1 (libplacebo's pl_peak_detect_params as vf_libplacebo sets
   * them; NaN = vf_libplacebo's option defaults, in brackets):            */
  double pd_smoothing;   /* IIR smoothing period, frames [100]              */
  double pd_scene_low;   /* scene-change thresholds on the frame average,   */
  double pd_scene_high;  /*   % of the PQ range [5.5, 10]                   */
  double pd_percentile;  /* detected peak = this percentile of per-pixel
                          * PQ(max R,G,B); 100 = the maximum [99.995]       */
  double pd_min_peak;    /* lower bound on the detected peak, relative to
                          * the SDR target white [1.0]                      */
} h2s_params;

/* A batch of planar 4:2:0 frames (yuv420p / yuv420p10le / yuv420p12le).
 * Samples are uint8 when bits == 8, else little-endian uint16 holding the
 * value in the low bits (ffmpeg's *le layouts).  Frame f, plane p, row r
 * starts at data[p] + f*frame_pitch[p] + r*linesize[p] (bytes).          */
typedef struct h2s_frames {
  void *data[3];
  int64_t linesize[3];
  int64_t frame_pitch[3];
  int32_t width;    /* luma width  (even)  */
  int32_t height;   /* luma height (even)  */
  int32_t bits;     /* 8, 10 or 12         */
  int32_t location; /* enum h2s_location   */
} h2s_frames;

/* The same record describes a semi-planar set (H2S_LAYOUT_SEMI) when the
 * context's layout for that side says so:
 *   plane 0: the Y plane, as above;
 *   plane 1: the interleaved plane, width/2 (Cb, Cr) pairs per row and
 *     height/2 rows, so linesize[1] >= width * bytes per sample;
 *   plane 2: ignored (data NULL, linesize and frame_pitch 0 are fine).
 * bits == 8 (nv12, output only): one byte per sample.  bits == 10 / 12
 * (p010le / p012le; a decoder's "P016" too): little-endian 16-bit words with
 * the value in the high bits: on input code = word >> (16 - bits), whatever
 * the low bits hold (the h2s_lp_p010 TRUNCATE mask then applies to the code);
 * on output word = code << (16 - bits), low bits zero.  Pitches may be
 * padded as a decoder pads them; 16-bit planes need even linesize and
 * frame_pitch.  Row starts that are 16-byte aligned (8 for nv12) run on the
 * tile kernel, others on the generic one (h2s_query_path), as for planar. */

/* An input set of another chroma subsampling (h2s_set_input_subsampling;
 * planar only, codes in the low bits, bits 10 or 12) has chroma planes 1, 2 of
 *   H2S_SUB_422 (yuv422p10le / 12le): width/2 samples x height rows,
 *     linesize[1, 2] >= width/2 * 2 bytes;
 *   H2S_SUB_444 (yuv444p10le / 12le): width samples x height rows,
 *     linesize[1, 2] >= width * 2 bytes.
 * Width and height are still even: the output is 4:2:0.  A tight frame is
 * width * height * {3/2, 2, 3} samples. */

typedef struct h2s_ctx h2s_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
int h2s_abi_version(void);
int h2s_abi_minor(void);   /* H2S_ABI_MINOR of the loaded library */

/* Replaces spawning the ffmpeg child (src/conversion.py:209-224) and the
 * filter-graph setup it performs.  device = HIP device ordinal (the reference
 * always uses device 0: src/utils.py:99, src/ffmpeg_command.py:187). */
int h2s_create(int device, h2s_ctx **out);
void h2s_destroy(h2s_ctx *ctx);

/* Message for the last failure on ctx (or the calling thread when ctx is
 * NULL).  Never NULL; "" when there was none. */
const char *h2s_last_error(const h2s_ctx *ctx);

/* ---- LUT (lut3d=file=..., src/utils.py:40, :212-225) --------------------
 * rgb: n^3 float triples in .cube order (red fastest, then green, then blue),
 * i.e. exactly the order tools/generate_lut.py:97-109 writes.  The context
 * keeps its own device copy.  2 <= n <= 256; any float values are taken, as
 * lut3d takes them: the chain blends the nodes as given and the output clip
 * follows the blend.  The tile kernel's CPU-chain form assumes nodes in [0, 1],
 * so a lattice with any value outside [0, 1] or not finite (a creative or
 * overshooting .cube) runs the CPU chain on the generic kernel, and
 * h2s_query_path reports H2S_PATH_GENERIC; the libplacebo branch, whose 8-bit
 * table is built with the generic arithmetic, keeps its path for any lattice. */
int h2s_set_lut(h2s_ctx *ctx, const float *rgb, int n);

/* ---- params (FFMPEG_CONVERT_FILTER.format, src/utils.py:38-42) ----------- */
void h2s_params_default(h2s_params *p);
int h2s_set_params(h2s_ctx *ctx, const h2s_params *p);

/* ---- per-frame execution (the ffmpeg filter_frame loop) ------------------
 * Processes nframes frames from `in` into `out`.  Both sets must have the
 * same width/height; in->bits == params.bits_in, out->bits ==
 * params.bits_out.  hip_stream is a hipStream_t (NULL = default stream).
 * Device->device runs asynchronously, with params.peak_detect too (the peak
 * statistics, the smoothing and the per-frame curves are queued on the same
 * stream, ABI 3.2); any host-resident set is staged through context-owned
 * device buffers and the call returns after the copy back (PCIe-inclusive
 * path). */
int h2s_process(h2s_ctx *ctx, const h2s_frames *in, const h2s_frames *out,
                int nframes, void *hip_stream);

/* Debug/parity: three float planes (3*w*h floats) of frame 0 after `stage`
 * (enum h2s_stage), written to out_rgb (host or device per out_location).
 * Computed by the kernel h2s_process would use for this frame: the tile
 * kernel's own arithmetic (a debug instance of it) on the tile path, the
 * generic kernel otherwise (h2s_query_path; H2S_OPT_FAST_PATH = 0 forces the
 * generic one).  With peak_detect the curve uses the static peak (the
 * parameters' resolved peak), not the context's smoothed state: the debug
 * planes are a per-frame check of the arithmetic and leave that state
 * untouched.  With 4:2:2 / 4:4:4 input (h2s_set_input_subsampling) the planes
 * are the generic kernel's whatever h2s_query_path says: the tile kernel has
 * no debug instances for those inputs; the same holds for a top-left 4:2:0
 * set (h2s_set_input_tags), while a full-range set changes constants only and
 * keeps the tile kernel's debug instances.  Synchronous. */
int h2s_debug_float(h2s_ctx *ctx, const h2s_frames *in, int stage,
                    float *out_rgb, int out_location, void *hip_stream);

/* ---- options and introspection ------------------------------------------
 * h2s_set_option: enum h2s_option.  h2s_query_path: the enum h2s_path that
 * h2s_process(ctx, in, out, ...) would take with the current params, LUT and
 * options (negative H2S_E_* on invalid input). */
int h2s_set_option(h2s_ctx *ctx, int key, int64_t value);
int h2s_query_path(h2s_ctx *ctx, const h2s_frames *in, const h2s_frames *out);

/* ---- frame layout (enum h2s_layout; default PLANAR, PLANAR) ---------------
 * How every later call on the context reads its `in` frames and writes its
 * `out` frames: h2s_process and h2s_query_path (both), h2s_debug_float,
 * h2s_peak_stats and h2s_preview_rgb24 / _batch (`in`; their float, RGB and
 * statistics outputs are unaffected).  The two sides are independent.  The
 * kernels read and write the surfaces in place: no repack pass, and output
 * codes equal the planar ones sample for sample.  Only the arguments of later
 * launches change, so the call does not wait for queued work.  An unknown
 * value or a NULL ctx is H2S_E_INVALID_ARG. */
int h2s_set_frame_layout(h2s_ctx *ctx, int in_layout, int out_layout);

/* ---- input chroma subsampling (enum h2s_subsampling; default 420) --------
 * How every later call on the context reads the chroma planes of its `in`
 * frames: h2s_process (device and host-resident sets), h2s_query_path,
 * h2s_debug_float and h2s_preview_rgb24 / _batch.  The conversion kernels read
 * a 4:2:2 / 4:4:4 source at its own chroma resolution, as the reference's CPU
 * chain does (zscale takes what the decoder produced), instead of a 4:2:0
 * frame that swscale decimated first.  Model ([EXT], unpinned like the rest of
 * S1): 4:2:2 chroma is co-sited with the even luma column and
 * lines up with every luma row, so S1 is the horizontal pass alone on chroma
 * row y (C[2k] = c[k], C[2k+1] = c[k]/2 + c[k+1]/2, column width/2 by
 * params.chroma_edge); 4:4:4 is not resampled.  Everything after S1, and the
 * 4:2:0 output, is unchanged.  Only the arguments of later launches change, so
 * the call does not wait for queued work.  An unknown value or a NULL ctx is
 * H2S_E_INVALID_ARG.  With 422 / 444 set, each of these is H2S_E_UNSUPPORTED
 * (h2s_last_error says why), never another route:
 *   - H2S_LAYOUT_SEMI on the input side (p210 / p410);
 *   - the libplacebo pipeline (params resolve to H2S_PIPE_LIBPLACEBO, hence
 *     peak_detect too): the reference uploads format=p010 there, i.e. 4:2:0;
 *   - h2s_peak_stats.
 * h2s_set_input_decimation lifts all three by decimating to 4:2:0 first. */
int h2s_set_input_subsampling(h2s_ctx *ctx, int subsampling);

/* ---- input source tags (enum h2s_range, enum h2s_chroma_loc; default
 * LIMITED, LEFT) ------------------------------------------------------------
 * How every later call on the context interprets the codes and the chroma
 * siting of its `in` frames: h2s_process (device and host-resident sets),
 * h2s_query_path, h2s_debug_float, h2s_peak_stats and h2s_preview_rgb24 /
 * _batch.  The reference's chains honour both tags of the decoded frame
 * (zscale=t=linear has no rin=, so zimg takes the range from the frame;
 * vf_libplacebo reads the AVFrame), so both apply to both pipelines, with
 * peak_detect, and to planar and semi-planar input.  Model ([EXT], unpinned
 * like the rest of S1), for input depth b:
 *   H2S_RANGE_FULL: Y' = code / (2^b - 1), Cb, Cr = (code - 2^(b-1)) /
 *     (2^b - 1) (zimg's full-range integer to float conversion; every code is
 *     legal).  Nothing after S1's normalisation changes: the output stays
 *     BT.709 limited range.
 *   H2S_CHROMA_TOPLEFT (4:2:0 input): the horizontal pass is the left-sited
 *     one (C[2k] = c[k], C[2k+1] = c[k]/2 + c[k+1]/2); vertically the chroma
 *     row is co-sited with the even luma row: C[2m] = c[m], C[2m+1] = c[m]/2 +
 *     c[m+1]/2, row height/2 by params.chroma_edge exactly as column width/2
 *     (no row above the plane is read).  With 4:2:2 / 4:4:4 input there is no
 *     vertical pass: the tag is accepted and has no effect.
 * Other chroma locations (center, top, bottomleft, bottom) are not modelled.
 * Only the arguments of later launches change, so the call does not wait for
 * queued work.  An unknown value or a NULL ctx is H2S_E_INVALID_ARG. */
int h2s_set_input_tags(h2s_ctx *ctx, int range, int chroma_location);

/* ---- input decimation (enum h2s_decimation; default OFF) -------------------
 * The stage the reference's GPU chain starts with (format=p010,hwupload:
 * whatever the decoder produced, ffmpeg's auto-inserted swscale makes 4:2:0 of
 * it first, src/utils.py:431), as a device front-end.  OFF: every call behaves
 * and refuses exactly as h2s_set_input_subsampling says.  BICUBIC, while the
 * context's input subsampling is 4:2:2 or 4:4:4: every call that converts
 * `in` sees the 4:2:0 frames the front-end makes of it, on either pipeline:
 * h2s_process, h2s_process_scaled, h2s_query_path (it answers for the 4:2:0
 * set), h2s_debug_float, h2s_peak_stats and h2s_preview_rgb24 / _batch; with
 * peak_detect, with Dolby Vision records, with planar or semi-planar input
 * (p210le / p212le / p410le / p412le: words code << (16 - b)), device or host
 * frames.  With 4:2:0 input the setting has no effect, and
 * h2s_preview_source_rgb24 / _batch (the source as decoded) ignore it.
 * Model ([EXT], parity unpinned like the rest of the pixel stages; DESIGN.md
 * 4.14): S6's swscale-bicubic chroma model (H2S_CHROMA_BICUBIC; B = 0,
 * C = 0.6), for input depth b:
 *   - Luma is untouched: read in place from the caller's surface.
 *   - 4:4:4: horizontally 7 taps on source columns 2k-3 .. 2k+3 (left-sited).
 *   - 4:4:4 and 4:2:2: vertically 8 taps on source chroma rows 2m-3 .. 2m+4
 *     (centred: the `left` 4:2:0 siting).  4:2:2: that pass alone.
 *   - Indices are clamped to the plane (replicate).
 *   - Float32 on the integer codes, the vertical pass then the horizontal one,
 *     each an ascending fmaf chain from 0; v = floor(acc + 0.5) clamped to
 *     [0, 2^b - 1].  Range-agnostic: full-range codes pass through.
 *   - The chain behind it runs with the context's range tag and chroma
 *     location LEFT (a top-left tag on a 4:2:2 / 4:4:4 set has no effect, as
 *     without the front-end), on a 4:2:0 set of the context's own input layout
 *     and depth whose luma is the caller's and whose chroma is a context-owned
 *     device scratch of at most 16 frames: a longer batch runs in chunks,
 *     stream-ordered on hip_stream, so the dynamic peak's state sees the frames
 *     in order and the output does not depend on the chunking.  A host-resident
 *     `in` is staged chunk by chunk on hip_stream (serially: not the
 *     three-stream pipeline of h2s_process).
 * With h2s_set_timing the front-end launch is one more entry of the record, in
 * front of its chunk's conversion entry.  Only the arguments of later launches
 * change, so the call does not wait for queued work.  An unknown value or a
 * NULL ctx is H2S_E_INVALID_ARG. */
int h2s_set_input_decimation(h2s_ctx *ctx, int mode);

/* ---- Dolby Vision profile 5 (default: off) ---------------------------------
 * A profile-5 stream has no HDR10-compatible base layer: its codes are
 * IPT-PQ-c2 and mean something only after the frame's RPU has reshaped them.
 * The reference sends such a source to libplacebo even with GPU acceleration
 * off (src/ffmpeg_command.py:96-144); its CPU chain shows green and purple.
 * The RPU does not cross a rawvideo pipe, so the caller hands its numbers (a
 * few hundred per frame: ffprobe frame side data, an RPU tool) to the context
 * next to the frames.  Parsing the RPU bitstream is not part of this library.
 *
 * Model ([EXT], PARITY UNPINNED like the rest of the libplacebo branch:
 * libplacebo is absent).  It restates pl_shader_dovi_reshape
 * followed by libplacebo's Dolby Vision decode, written from memory of
 * libplacebo's source, not compared against it.  For input depth b (10 or 12)
 * and the frame's record R, per luma pixel:
 *   1. Signal: (y, cb, cr) = the luma code and the two chroma codes upsampled
 *      to luma resolution by the branch's S1 upsampler (left-sited bilinear,
 *      params.chroma_edge; the lp_p010 mask applies to the codes first);
 *      s = clamp((y, cb, cr) / (2^b - 1), 0, 1).  The range tag has no effect:
 *      an RPU is defined on the full-scale code fraction.
 *   2. Reshape: component c reads the unreshaped s of all three.  It has
 *      num_pivots in [2, 9] ascending pivots; piece k is the largest k <=
 *      num_pivots - 2 with pivots[k] <= s_c (k = 0 below the first pivot).
 *      method[k] 0, polynomial: r = a0 + a1 s_c + a2 s_c^2 (poly[k]).
 *      method[k] 1, MMR of order o = mmr_order[k] in {1, 2, 3}: with the terms
 *      t = (s0, s1, s2, s0 s1, s0 s2, s1 s2, s0 s1 s2),
 *      r = mmr_const[k] + sum_{i=1..o} sum_{j=0..6} mmr[k][i-1][j] t_j^i.
 *      r_c = clamp(r, pivots[0], pivots[num_pivots - 1]).
 *   3. Non-linear matrix: v = clamp(nonlinear (r - nonlinear_offset), 0, 1):
 *      L'M'S'.  The clamp to 1 is this model's own, not libplacebo's: beyond
 *      it lies more than 10000 nits.
 *   4. EOTF: lms = PQ_EOTF(v), 1 = 10000 nits.
 *   5. Linear matrix: rgb = linear lms: linear BT.2020 light, scaled to units
 *      of npl as S1 does; not clamped (S2 treats a negative channel as it does
 *      for any source).  `linear` is the complete L, M, S -> BT.2020 R, G, B
 *      matrix.
 * From here on the libplacebo branch runs unchanged: every operator, both
 * lp_tone forms, the LUT on or off, peak_detect, every output depth and
 * layout.  The trim metadata (L1 / L2 / L5 / L6) is not modelled: with
 * peak_detect the detected peak governs, as in the reference.
 *
 * h2s_set_dovi(ctx, rpu, n): n == 0 (rpu NULL or not) switches the front-end
 * off, the default: nothing else changes then, the same kernels run with
 * byte-identical output.  n == 1: one record for every frame.  n > 1: record
 * f for frame f of each later call; a later call with nframes > n is
 * H2S_E_INVALID_ARG.  The records are copied into context-owned device
 * memory; like h2s_set_params the call first waits for the context's queued
 * launches, so dynamic metadata costs one wait per batch (a stream-ordered
 * upload is out of scope).  Each of these is H2S_E_INVALID_ARG with a message:
 * a pivot count outside [2, 9]; pivots not ascending or outside [0, 1]; a
 * method or an order outside its enum; a coefficient that is not finite.
 *
 * With a record set: params.transfer_in is ignored; the pipeline must resolve
 * to LIBPLACEBO (H2S_PIPE_CPU_CHAIN, or AUTO with a CPU-chain operator, is
 * H2S_E_UNSUPPORTED: the reference has no such path and shows wrong colours
 * there); H2S_CHROMA_TOPLEFT is H2S_E_UNSUPPORTED; 4:2:2 / 4:4:4 input stays
 * the branch's own refusal; input may be planar or semi-planar, in device or
 * host memory (in the host chunk pipeline record indices count frames of the
 * call, not of the chunk).  The records are honoured by h2s_process and
 * h2s_query_path, h2s_debug_float (frame 0: record 0), h2s_peak_stats and the
 * statistics h2s_process queues under peak_detect (per-pixel PQ(max R, G, B)
 * of the decoded light, nearest chroma), and h2s_preview_rgb24 / _batch.
 * h2s_preview_source_rgb24 ignores them: the reference's extract_frame shows
 * the raw codes too, because swscale applies no RPU.
 * Routes: the tile kernel has instances for the shape profile 5 actually
 * carries -- luma polynomial pieces only (up to 8), each chroma component a
 * single piece, polynomial or MMR up to order 3 -- for the libplacebo
 * branch's five operators, planar and semi-planar (float32, like the rest of
 * that kernel; H2S_PATH_TILE / _TILE_TAIL).  A set in which any record has
 * another shape (a luma MMR, multi-piece chroma) runs on the generic kernel
 * (H2S_PATH_GENERIC; never a third route), as do tails, widths under 64,
 * H2S_OPT_FAST_PATH = 0 and H2S_OPT_LP_EXACT: there the front-end is in double
 * precision like the rest of its stages 1-3.  h2s_debug_float reports the
 * tile kernel's own arithmetic on the tile path. */
typedef struct h2s_dovi_curve {
  int32_t num_pivots;      /* 2..9 */
  float   pivots[9];
  int32_t method[8];       /* 0 polynomial, 1 MMR */
  float   poly[8][3];
  int32_t mmr_order[8];    /* 1..3 */
  float   mmr_const[8];
  float   mmr[8][3][7];
} h2s_dovi_curve;
typedef struct h2s_dovi_rpu {
  float nonlinear_offset[3], nonlinear[9], linear[9];   /* row-major */
  h2s_dovi_curve comp[3];
} h2s_dovi_rpu;
int h2s_set_dovi(h2s_ctx *ctx, const h2s_dovi_rpu *rpu, int n);

/* ---- dynamic peak (params.peak_detect, BT.2390 / spline) -----------------
 * h2s_peak_reset: forget the smoothing state (a new sequence / scene cut).
 * h2s_peak_state: the smoothed PQ-domain max / average after the last
 *   processed frame, the source peak (units of npl) it gave, and the number
 *   of frames folded in since the reset.  Any pointer may be NULL.
 * The state lives on the device and is updated in stream order by the
 * h2s_process calls that use it; h2s_peak_reset / _feed / _state first wait
 * for this context's queued work, then act synchronously. */
int h2s_peak_reset(h2s_ctx *ctx);
/* Frame-sharded runs (hdr2sdr/dist.py): the smoothing is a recurrence over
 * the whole sequence, so a rank that owns frames [a, b) first needs the
 * state frames [0, a) leave.  h2s_peak_stats: the per-frame statistics
 * h2s_process would fold in (max and mean of PQ(max R,G,B)), for device
 * frames, without converting them.  h2s_peak_feed: fold n frames' statistics
 * into the state in order, as h2s_process does.  Gathering every rank's
 * statistics and feeding the preceding ones makes the sharded output equal
 * to the sequential one. */
int h2s_peak_stats(h2s_ctx *ctx, const h2s_frames *in, int nframes, double *fmax, double *favg, void *hip_stream);
int h2s_peak_feed(h2s_ctx *ctx, const double *fmax, const double *favg, int n);
int h2s_peak_state(const h2s_ctx *ctx, double *max_pq, double *avg_pq, double *peak, int64_t *frames);

/* ---- preview (src/utils.py:719-765 extract_frame_with_conversion, the
 * GUI's adjust_gamma src/preview.py:108-117) ------------------------------
 * h2s_preview_size: the size FFMPEG_FILTER's trailing
 *   scale=W:H:force_original_aspect_ratio=decrease (src/utils.py:46-49) gives
 *   an in_w x in_h frame in a box_w x box_h box (PREVIEW_SIZE = 3840x2160,
 *   src/preview.py:29); upscales too, as ffmpeg's scale does.
 * h2s_preview_rgb24: frame 0 of `in` through the chain (ctx params; bits_out
 *   must be 8: the yuv420p the PNG encoder reads), the bicubic (B=0, C=0.6)
 *   resize to out_w x out_h when that differs from the frame size, BT.709
 *   limited Y'CbCr -> full-range RGB24 (nearest chroma), then the display
 *   gamma LUT round(255 (i/255)^(1/gamma)) on R, G, B (1.0 = identity).
 *   rgb: out_h rows of out_w*3 bytes, rgb_linesize apart, host or device per
 *   rgb_location.  Synchronous.
 * h2s_preview_rgb24_batch: the same for nframes frames of `in` (one size)
 *   into nframes RGB images rgb_frame_pitch bytes apart — the reference's
 *   batched preview (extract_frames_with_conversion_batch /
 *   extract_frames_with_gpu_conversion_batch, src/utils.py:617-626,
 *   :668-716, :803-824).  The CPU chain runs the batch as one tone-map
 *   launch; with params.peak_detect (the libplacebo branch) each frame starts
 *   from a fresh peak state, as each of the reference's per-frame ffmpeg runs
 *   does, and the context's own peak state is restored afterwards.  The resize and RGB kernels take the whole batch in one launch each.
 *   h2s_preview_rgb24 == the batch call with nframes = 1. */
int h2s_preview_size(int in_w, int in_h, int box_w, int box_h, int *out_w, int *out_h);
int h2s_preview_rgb24(h2s_ctx *ctx, const h2s_frames *in, uint8_t *rgb, int64_t rgb_linesize,
                      int out_w, int out_h, double display_gamma, int rgb_location,
                      void *hip_stream);
int h2s_preview_rgb24_batch(h2s_ctx *ctx, const h2s_frames *in, int nframes, uint8_t *rgb,
                            int64_t rgb_linesize, int64_t rgb_frame_pitch, int out_w, int out_h,
                            double display_gamma, int rgb_location, void *hip_stream);

/* ---- source pane (src/utils.py:827-859 extract_frame, :629-665
 * extract_frames_batch; the GUI's "before" image, src/preview.py:652-653,
 * :679-680) ------------------------------------------------------------------
 * h2s_preview_source_rgb24_batch: nframes source frames of `in` (one size), as
 *   decoded and with no tone mapping, as nframes RGB24 images: the restatement
 *   of `ffmpeg -i src -vf scale=W:H:force_original_aspect_ratio=decrease ...
 *   png`.  out_w x out_h comes from h2s_preview_size: always the aspect fit,
 *   on the libplacebo pipeline too (the source pane never goes through
 *   libplacebo).  rgb, rgb_linesize, rgb_frame_pitch, rgb_location and the
 *   argument checks (geometry, resize-ratio limits, NULLs) are those of
 *   h2s_preview_rgb24_batch.  Synchronous.
 *   No tone-map state: the call neither reads nor changes the params, the LUT,
 *   the options or the peak state, and works on a context that never had
 *   h2s_set_params.  The depth is in->bits, 10 or 12 (else H2S_E_INVALID_ARG).
 *   It reads the surfaces in place as the context's input side describes them:
 *   h2s_set_frame_layout (planar or semi-planar, padded pitches),
 *   h2s_set_input_subsampling (4:2:0, 4:2:2, 4:4:4 planar; 4:2:2 / 4:4:4 with a
 *   semi-planar input is H2S_E_UNSUPPORTED) and the range tag of
 *   h2s_set_input_tags.  The chroma-location tag is accepted and has no effect
 *   in this model (the chroma planes are resized centre-aligned whatever the
 *   tag says).  An unknown matrix or rgb_model is H2S_E_INVALID_ARG.
 *   Model ([EXT], parity unpinned like the rest of the preview tail; DESIGN.md
 *   4.4).  One swscale context, so nothing is rounded between the resize and
 *   the matrix.  For depth b the codes y, cb, cr are the low bits (planar) or
 *   word >> (16 - b) (semi-planar).
 *   Resize: luma W x H -> out_w x out_h; each chroma plane from its own cw x ch
 *     (W/2 x H/2, W/2 x H or W x H) to ow2 x out_h, ow2 = (out_w + 1) / 2:
 *     swscale treats packed RGB output (no full_chroma_int) as horizontally
 *     2:1 chroma, pixel (x, y) takes chroma (x >> 1, y).  Taps as in
 *     h2s_preview_rgb24: bicubic B = 0, C = 0.6, centre-aligned, widened by the
 *     ratio when downscaling, normalised, indices clamped at the edges;
 *     accumulated in float.  At equal size the luma taps are the identity.
 *   Normalisation: limited range Y' = (Y - 16 2^(b-8)) / (219 2^(b-8)), C = (C -
 *     2^(b-1)) / (224 2^(b-8)); H2S_RANGE_FULL Y' = Y / (2^b - 1), C = (C -
 *     2^(b-1)) / (2^b - 1).
 *   Matrix (enum h2s_src_matrix): R' = Y' + 2 (1 - Kr) Cr, B' = Y' + 2 (1 - Kb)
 *     Cb, G' = Y' - (2 Kr (1 - Kr) / Kg) Cr - (2 Kb (1 - Kb) / Kg) Cb, Kg = 1 -
 *     Kr - Kb; (Kr, Kb) = BT2020NC (0.2627, 0.0593), what a tagged HDR stream
 *     gets; BT709 (0.2126, 0.0722); BT601 (0.299, 0.114), swscale's default for
 *     an untagged stream.  Clipped to [0, 1].
 *   Output (enum h2s_src_rgb): TRUNC16 floor(65535 v + 0.5) >> 8 (for a 10/12-
 *     bit source ffmpeg hands the PNG encoder rgb48be, and PIL opens a 16-bit
 *     RGB PNG by taking each sample's high byte); ROUND8 floor(255 v + 0.5) (an
 *     rgb24 PNG).  No display gamma: the GUI's adjust_gamma never touches the
 *     original (src/preview.py:642).  extract_frame's single-frame form omits
 *     -vcodec, so ffmpeg codes a JPEG there: that lossy step is not modelled.
 * h2s_preview_source_rgb24 == the batch call with nframes = 1. */
enum h2s_src_matrix { H2S_SRC_MATRIX_BT2020NC = 0, H2S_SRC_MATRIX_BT709 = 1, H2S_SRC_MATRIX_BT601 = 2 };
enum h2s_src_rgb { H2S_SRC_RGB_TRUNC16 = 0, H2S_SRC_RGB_ROUND8 = 1 };
int h2s_preview_source_rgb24(h2s_ctx *ctx, const h2s_frames *in, uint8_t *rgb, int64_t rgb_linesize,
                             int out_w, int out_h, int matrix, int rgb_model, int rgb_location,
                             void *hip_stream);
int h2s_preview_source_rgb24_batch(h2s_ctx *ctx, const h2s_frames *in, int nframes, uint8_t *rgb,
                                   int64_t rgb_linesize, int64_t rgb_frame_pitch, int out_w, int out_h,
                                   int matrix, int rgb_model, int rgb_location, void *hip_stream);

/* ---- scaled 4:2:0 output: convert and downscale in one call ----------------
 * The reference's chain definition has this tail: FFMPEG_FILTER
 * (src/utils.py:46-49) is the export chain plus
 * scale=W:H:force_original_aspect_ratio=decrease.  [EXT], parity unpinned like
 * the rest of the preview tail.
 * h2s_scaled_size: h2s_preview_size's aspect fit of an in_w x in_h frame in a
 *   box_w x box_h box, each dimension then rounded down to even and not below
 *   2: what a 4:2:0 deliverable needs.  This is ffmpeg's scale option
 *   force_divisible_by=2, written from memory of libavfilter's scale_eval and
 *   not checked against it.
 * h2s_process_scaled: h2s_process, with out->width x out->height the target
 *   size (`in` keeps the source size; out->bits == params.bits_out).  The
 *   resize is a trailing scale= stage on the chain's quantised 4:2:0 output,
 *   before the S8 expansion, on both pipelines, with peak_detect or Dolby
 *   Vision records set (the chain in front is untouched):
 *   - Depth: q is the chain's quantising depth (8 in H2S_MODE_COMPAT8,
 *     bits_out in H2S_MODE_NATIVE and on the libplacebo branch at gamma 1);
 *     the resize's source codes are the chain's q-bit codes, what h2s_process
 *     would write >> (bits_out - q).
 *   - Planes: luma W x H -> ow x oh, each chroma plane W/2 x H/2 -> ow/2 x
 *     oh/2; ow and oh even and >= 2 (else H2S_E_INVALID_ARG).
 *   - Taps: those of h2s_preview_rgb24's resize: swscale bicubic B = 0,
 *     C = 0.6, centre-aligned, support widened by the ratio when downscaling,
 *     normalised float32 weights, source indices clamped at the edges.  No
 *     chroma-siting correction, as in the preview.
 *   - Arithmetic: float32, the horizontal pass then the vertical one, each an
 *     ascending fmaf chain from 0; v = floor(acc + 0.5) clamped to
 *     [0, 2^q - 1]; then S8 (H2S_EXPAND_SHIFT / _REPLICATE) to bits_out.
 *   - Limits: source / target <= 12 per axis and target <= 4 * 8192, else
 *     H2S_E_UNSUPPORTED.
 *   - Equal size: the call is h2s_process and nothing else (byte-identical).
 *   It honours h2s_set_frame_layout on both sides (planar or semi-planar
 *   output, padded pitches), h2s_set_input_subsampling, h2s_set_input_tags and
 *   h2s_set_dovi exactly as h2s_process does, and its other errors are
 *   h2s_process's.  Device -> device is asynchronous on hip_stream; a
 *   host-resident set is staged, and the call then returns after the stream
 *   has finished.  The full-size intermediate lives in a context-owned device
 *   scratch (planar 4:2:0 at bits_out) of at most 16 frames: a longer batch
 *   runs in chunks, stream-ordered, so the dynamic peak's state sees the
 *   frames in order and the output does not depend on the chunking.  The tap
 *   tables are cached in the context per (W, H, ow, oh) and uploaded once: a
 *   steady-state call makes no host -> device copy and no synchronisation; a
 *   new size waits for the context's queued launches first.  With
 *   h2s_set_timing the resize launch is one more entry of the record, after
 *   its chunk's h2s_process entry. */
int h2s_scaled_size(int in_w, int in_h, int box_w, int box_h, int *out_w, int *out_h);
int h2s_process_scaled(h2s_ctx *ctx, const h2s_frames *in, const h2s_frames *out,
                       int nframes, void *hip_stream);

/* ---- RGB tensor output: the converted frames as R'G'B' on the device -------
 * [EXT], parity unpinned like the rest of the preview tail.
 * h2s_process_rgb is h2s_process when out has the source's size and
 * h2s_process_scaled when the sizes differ, either followed by a
 * Y'CbCr -> R'G'B' stage on the chain's quantised 4:2:0 codes.  Everything in
 * front is untouched: both pipelines, peak_detect, Dolby Vision records, input
 * layouts, subsampling, tags and decimation.
 *   Let q be the chain's quantising depth (8 in H2S_MODE_COMPAT8, bits_out in
 *   H2S_MODE_NATIVE and on the libplacebo branch at gamma 1) and s = 2^(q-8).
 *   The codes y, u, v are what h2s_process / h2s_process_scaled would write,
 *   >> (bits_out - q).  Pixel (x, y) takes the chroma sample (x>>1, y>>1):
 *   nearest, as h2s_preview_rgb24 does.  In float32, with the preview's BT.709
 *   limited-range constants and operation order:
 *     Y = 1.16438356f * ((float)y - 16 s)   U = (float)u - 128 s   V = (float)v - 128 s
 *     cR = fmaf(1.79274107f, V, Y)
 *     cG = fmaf(-0.53290933f, V, fmaf(-0.21324861f, U, Y))
 *     cB = fmaf(2.11240179f, U, Y)
 *   - H2S_RGB_U8: floor(c * (1/s) + 0.5) clamped to [0, 255] (the product is
 *     exact).  At q = 8 this is h2s_preview_rgb24 at display gamma 1,
 *     operation for operation.
 *   - H2S_RGB_F32 / _F16 / _BF16: v = min(max(c * inv, 0), 1) with
 *     inv = (float)(1 / (255 s)); out_k = fmaf(scale[k], v, bias[k]), stored
 *     as float32 or rounded to nearest-even to half / bfloat16.  For an
 *     (x/255 - mean) / std normalisation: scale = 1/std, bias = -mean/std.
 *   No display gamma is applied.
 * Layouts: H2S_RGB_HWC interleaves R, G, B (a pixel is 3 elements, a row
 * 3 * width); H2S_RGB_CHW writes three planes plane_pitch bytes apart.  Every
 * pitch is in bytes and a multiple of the element size; data is aligned to the
 * element size.  Rows that start at multiples of 16 bytes (data and every
 * pitch used) are written with 16-byte stores, others element by element, to
 * the same values.
 * `in` is validated as h2s_process validates it and may be device or host
 * memory; the output is device memory only.  With a device input the call is
 * asynchronous on hip_stream.  With a host input the frames are staged as
 * h2s_process stages them and the call returns once that is done; the RGB
 * kernel is then still queued on hip_stream, so the consumer must be ordered
 * after that stream (or synchronise it) either way.
 * The size rules and limits are h2s_process_scaled's: width and height even
 * and >= 2, source / target <= 12 per axis and target <= 4 * 8192, else
 * H2S_E_UNSUPPORTED: a 3840x2160 -> 224x224 request is refused (17 : 1), such
 * a consumer resizes a 320x180 output further itself.  Batches longer than 16
 * frames run in chunks, stream-ordered, in the scaled output's scratch and
 * with its cached tap tables: a steady-state call makes no host -> device copy
 * and no synchronisation.  With h2s_set_timing the record gains one entry per
 * chunk for the RGB launch, after the chunk's conversion entry and, if the
 * sizes differ, its resize entry.
 * H2S_E_INVALID_ARG: NULL ctx / in / out / out->data; params not set;
 * nframes < 0; an odd or non-positive target size; an unknown dtype or layout;
 * H2S_RGB_U8 with a scale != 1 or a bias != 0; a non-finite scale or bias; a
 * pitch that is not a multiple of the element size; row_pitch smaller than one
 * row; CHW plane_pitch < row_pitch * height; frame_pitch smaller than one
 * frame's extent (HWC: row_pitch * height; CHW: 3 * plane_pitch); data not
 * aligned to the element size. */
enum h2s_rgb_dtype  { H2S_RGB_U8 = 0, H2S_RGB_F16 = 1, H2S_RGB_BF16 = 2, H2S_RGB_F32 = 3 };
enum h2s_rgb_layout { H2S_RGB_HWC = 0, H2S_RGB_CHW = 1 };
typedef struct h2s_rgb_frames {
  void   *data;                 /* device memory */
  int32_t width, height;        /* target size; even, >= 2 */
  int32_t dtype, layout;        /* enum h2s_rgb_dtype, enum h2s_rgb_layout */
  int64_t row_pitch;            /* bytes between rows */
  int64_t plane_pitch;          /* CHW: bytes between the R, G, B planes; HWC: ignored */
  int64_t frame_pitch;          /* bytes between frames */
  float   scale[3], bias[3];    /* float dtypes; U8 requires (1,1,1) / (0,0,0) */
} h2s_rgb_frames;
int h2s_process_rgb(h2s_ctx *ctx, const h2s_frames *in, const h2s_rgb_frames *out,
                    int nframes, void *hip_stream);

/* ---- rendition ladder: several sizes of the 4:2:0 output from one conversion
 * [EXT], like h2s_process_scaled.  A transcode box delivers a ladder from each
 * master (2160p, 1080p, 720p, 360p).  h2s_process_ladder writes outs[0 ..
 * n_outs - 1], each a frame set as h2s_process_scaled takes one: its width x
 * height are the rung's size, its depth is params.bits_out, its layout the
 * context's output layout, its pitches its own.  The rungs may come in any
 * order, may repeat a size and may have the source's own size; all of them
 * share one location.
 *   Per chunk of at most 16 frames the chain runs ONCE, as h2s_process_scaled
 *   runs it, into the context's full-size planar scratch, and every rung is
 *   made from that scratch on hip_stream, in rung order: a smaller (or larger)
 *   rung by h2s_process_scaled's resize, arithmetic and limits; a rung of the
 *   source's size by a copy of the finished codes into its layout and pitches.
 *   So a source frame is converted exactly once, the dynamic peak's state
 *   (params.peak_detect) advances by nframes whatever n_outs is and every rung
 *   is tone-mapped with one curve, and Dolby Vision record f belongs to frame
 *   f of the call.  Each rung's bytes are those of the separate call on an
 *   equal context: h2s_process_scaled for a scaled rung; for a source-size
 *   rung h2s_process into a set whose rows start at multiples of 16 bytes (the
 *   scratch's form, which decides the kernel route).
 *   n_outs == 1: the call is h2s_process_scaled(ctx, in, &outs[0], ...) and
 *   nothing else.
 * Every input option of h2s_process_scaled carries over (semi-planar, 4:2:2 /
 * 4:4:4 and host input, input tags, input decimation).  Device rungs are
 * asynchronous on hip_stream; host rungs are staged in the scratch behind the
 * intermediate and the call returns after the stream has finished.  The
 * ladder keeps tap tables of its own, up to H2S_LADDER_MAX sizes per context,
 * uploaded once each: a steady-state call makes no host -> device copy and no
 * synchronisation (a ninth size replaces one, after a wait for the context's
 * queued launches); h2s_process_scaled's cached tables are not touched.  With
 * h2s_set_timing a chunk records its conversion entry, then one entry per
 * rung in rung order.
 * H2S_E_INVALID_ARG: NULL ctx / in / outs; n_outs < 1 or > H2S_LADDER_MAX; a
 * rung with an odd or non-positive size, a NULL plane, the wrong depth or a
 * short pitch; rungs of differing location.  H2S_E_UNSUPPORTED: a rung beyond
 * h2s_process_scaled's limits (source / target > 12 on an axis, target >
 * 4 * 8192).  The message names the rung's index.  A refused call has queued
 * nothing, written no rung and left the peak state as it was. */
#define H2S_LADDER_MAX 8
int h2s_process_ladder(h2s_ctx *ctx, const h2s_frames *in, const h2s_frames *outs,
                       int n_outs, int nframes, void *hip_stream);

/* ---- .cube helpers (tools/generate_lut.py:28-119; lut3d's .cube parser) --
 * h2s_cube_generate: the BT.2020->BT.709 lattice, n^3 triples, .cube order,
 *   rounded exactly as the "%.6f" text the reference writes, then parsed to
 *   float32 (what lut3d holds after reading the file).
 * h2s_cube_format: the file text, byte-identical to
 *   '\n'.join(generate_cube_lines(n)) + '\n'.  Returns the byte count
 *   needed (excluding NUL); writes at most cap bytes.
 * h2s_cube_parse: parses .cube text (LUT_3D_SIZE header, comments, optional
 *   DOMAIN_MIN/MAX of 0/1) into float32 triples; *n_out gets the size.  Pass
 *   rgb=NULL to query the size first. */
int h2s_cube_generate(int n, float *rgb);
int64_t h2s_cube_format(int n, char *buf, int64_t cap);
int h2s_cube_parse(const char *text, int64_t len, float *rgb, int64_t cap_floats,
                   int *n_out);

/* Kernel-duration probe for bench.py: average device time (ms) of the last
 * `count` h2s_process launches recorded with HIP events on the launch stream
 * since the last reset (count <= 0 resets the record and returns 0).  A
 * h2s_preview_source_rgb24 / _batch call records its one kernel the same way
 * (the table and frame copies around it are outside the events). */
double h2s_kernel_ms(h2s_ctx *ctx, int count);
int h2s_set_timing(h2s_ctx *ctx, int enabled);

#ifdef __cplusplus
}
#endif
#endif /* H2S_H */
