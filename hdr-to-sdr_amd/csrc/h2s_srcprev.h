// h2s_srcprev.h — launch parameters of the source-pane preview kernel
// (k_source_rgb24, h2s_preview.hip; h2s_preview_source_rgb24_batch): the
// unconverted source frame, resized and matrixed to RGB24 in one pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace h2s {

struct SrcPreviewParams {
  // the source set as the conversion kernels bind it (KParams, fill_geometry):
  // a semi-planar set has plane 2 = plane 1 one sample on, chroma samples cstep
  // apart and the code in the word's high bits (code = word >> sh); mask keeps
  // the depth's bits
  const uint8_t* in[3];
  long long ls[3], fp[3];
  int cstep, sh, mask;
  int W, H, cw, ch;  // luma and chroma plane sizes (cw x ch: W/2 x H/2, W/2 x H or W x H)
  // output: ow x oh pixels, ow2 = (ow + 1) / 2 chroma columns (pixel (x, y) takes chroma (x >> 1, y))
  int ow, oh, ow2;
  uint8_t* rgb;
  long long rls, rfp;
  // tap tables (resize_taps): per output index the first source tap and T
  // normalised weights; luma W -> ow, H -> oh (unused when identity), chroma
  // cw -> ow2, ch -> oh
  int identity;  // ow x oh == W x H: the luma taps are the sample itself
  int Tx, Ty, Tcx, Tcy;
  const float *wx, *wy, *wcx, *wcy;
  const int *sx, *sy, *scx, *scy;
  // Y' = y * y_inv, C = c * c_inv: the taps accumulate code - y_off and code -
  // mid (integers, exact; the weights are normalised, so this is the resized
  // plane less the offset), which keeps black and neutral chroma exactly 0
  int y_off, mid;
  float y_inv, c_inv;
  float m_rcr, m_gcb, m_gcr, m_bcb;
  int round8;  // H2S_SRC_RGB_ROUND8: floor(255 v + 0.5); else floor(65535 v + 0.5) >> 8
};

}  // namespace h2s
