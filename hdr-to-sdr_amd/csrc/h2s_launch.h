// h2s_launch.h — the one declaration of every host-callable kernel launcher.
// Included by the unit that defines a launcher (h2s_kernels.hip, h2s_peak.hip,
// h2s_fast.hip, h2s_preview.hip, h2s_scale.hip, h2s_decimate.hip, h2s_rgb.hip, h2s_repack.hip) and by every unit that calls one (the host
// units, h2s_testhooks.hip), so a signature or an
// enum value that drifts apart is a compile error, not a misrouted launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace h2s {

struct KParams;           // h2s_params.h
struct FastParams;
struct CurveConsts;
struct YuvLutConsts;
struct PeakModel;         // h2s_peak.h
struct PeakState;
struct PeakTail;
struct SrcPreviewParams;  // h2s_srcprev.h
struct ScaleParams;       // h2s_scale.h
struct DecimateParams;    // h2s_decimate.h
struct RgbParams;         // h2s_rgb.h
struct RepackParams;      // h2s_repack.h

// launch_process's form: PF_VEC the rows allow vector accesses, PF_OUT8 8-bit
// output, PF_C444 BICUBIC chroma pass 1 (luma + per-pixel chroma into P.chr444)
enum ProcessForm : unsigned { PF_VEC = 1, PF_OUT8 = 2, PF_C444 = 4 };

// h2s_kernels.hip
hipError_t launch_process(const KParams& P, unsigned form, hipStream_t s);
hipError_t launch_debug(const KParams& P, int stage, float* out, hipStream_t s);
hipError_t launch_chroma_bicubic(const KParams& P, const float* wx7, const float* wy8, bool out8, hipStream_t s);
hipError_t build_lut8x(const float4* lut, int n, unsigned* out, hipStream_t s);

// h2s_peak.hip
hipError_t launch_peak_stats(const KParams& P, float2* partial, const PeakTail& T, hipStream_t s);
hipError_t launch_peak_curves(double2* fstat, int n, const PeakModel& M, PeakState* st, CurveConsts* out,
                              hipStream_t s);

// h2s_fast.hip.  TileKey: which k_tile<TRC, TM, DESAT, LP, DBG, SEMI, SUB>
// a launch takes (tile_key builds it from the resolved parameters;
// tile_instance: there is such an instance, h2s_tile_sets.h's table)
struct TileKey {
  int trc, tm, desat, lp, dbg, semi, sub;
};
TileKey tile_key(const KParams& k, bool semi, bool dbg);
bool tile_instance(const TileKey& k);
hipError_t launch_fast(const FastParams& F, const TileKey& k, hipStream_t s);
hipError_t build_lut_yuv(const float4* rgb, float* yuv, int n, const YuvLutConsts& K, hipStream_t st);

// h2s_preview.hip (the tap tables: resize_taps, h2s_resolve.hip; one width per axis)
hipError_t launch_resize_u8(const uint8_t* src, int sw, int sh, long long sls, long long sfp, uint8_t* dst, int ow,
                            int oh, long long dls, long long dfp, const float* wx, const int* sx, int Tx,
                            const float* wy, const int* sy, int Ty, int nframes, hipStream_t s);
hipError_t launch_yuv8_rgb24(const uint8_t* yp, long long yls, const uint8_t* up, const uint8_t* vp, long long cls,
                             long long yuv_fp, int w, int h, uint8_t* rgb, long long rls, long long rgb_fp,
                             const uint8_t* glut, int nframes, hipStream_t s);
hipError_t launch_source_rgb24(const SrcPreviewParams& P, int nframes, hipStream_t s);

// h2s_scale.hip: every plane of nframes frames in one launch (src_bps: bytes of a scratch sample)
hipError_t launch_scale420(const ScaleParams& P, int src_bps, int nframes, hipStream_t s);

// h2s_decimate.hip: the chroma of nframes 4:2:2 / 4:4:4 frames (sub: enum h2s_subsampling) to 4:2:0 in one
// launch; it fills P's run and piece counts (run > 0: that run length, a test's; else its own pick)
hipError_t launch_decimate420(const DecimateParams& P, int sub, bool semi, int nframes, int run, hipStream_t s);

// h2s_rgb.hip: nframes planar 4:2:0 scratch frames to R'G'B' in one launch (src_bps: bytes of a scratch sample;
// dtype, layout: enum h2s_rgb_dtype, enum h2s_rgb_layout); it fills P's run and row-pair counts
hipError_t launch_rgb420(const RgbParams& P, int src_bps, int dtype, int layout, int nframes, hipStream_t s);

// h2s_repack.hip: every plane of nframes planar 4:2:0 scratch frames copied into a planar or semi-planar set of the
// same size in one launch (bps: bytes of a sample on both sides); it fills P's chunk and block counts
hipError_t launch_repack420(const RepackParams& P, int bps, bool semi, int nframes, hipStream_t s);

}  // namespace h2s
