// h2s_rgb.h — what k_rgb420 (h2s_rgb.hip) and its host side (h2s_api_rgb.hip)
// share: the launch record of the RGB tensor output (h2s_process_rgb) and the
// shape of a lane's piece of work.
#pragma once
#include <stdint.h>

namespace h2s {

constexpr int RGB_THREADS = 256;   // four waves, no LDS and no barrier: a lane's work is its own
constexpr int RGB_RUN = 16;        // luma columns of a lane's run (of both rows of its row pair)

// One launch: nframes planar 4:2:0 frames of the scaled-output scratch
// (scratch_frames, h2s_api_scale.hip: every row start 16-byte aligned and the
// rows padded to 16 bytes) to R'G'B' in the caller's tensor.  A scratch sample
// holds its q-bit code << shift
struct RgbParams {
  const uint8_t *y, *u, *v;
  long long yls, cls, sfp;   // luma and chroma row pitch, frame pitch of the scratch, bytes
  uint8_t* dst;
  long long rp, pp, fp;      // row, plane (CHW; HWC: unused) and frame pitch of the tensor, bytes
  int w, h;                  // even, >= 2
  int ngroups, npairs;       // runs of a row: ceil(w / RGB_RUN); row pairs: h / 2
  int shift;                 // bits_out - q
  float yoff, coff;          // 16 s and 128 s, s = 2^(q - 8)
  float inv;                 // U8: 1 / s; the float dtypes: (float)(1 / (255 s))
  float scale[3], bias[3];   // the float dtypes: out_k = fmaf(scale[k], v, bias[k])
  int vec;                   // every destination row start (of every plane and frame) is 16-byte aligned
};

}  // namespace h2s
