// h2s_dovi.h — the Dolby Vision profile-5 front-end (h2s_set_dovi): from a
// pixel's full-scale code fractions and its frame's record to L'M'S', steps 2
// and 3 of the model in include/h2s.h ([EXT], PARITY UNPINNED: a restatement
// of pl_shader_dovi_reshape and libplacebo's Dolby Vision decode from memory
// of libplacebo's source).  One definition in T = double (the
// generic kernel's exact path, h2s_lpx.h) and T = float (the peak statistics).
#pragma once
#include <hip/hip_runtime.h>

#include "h2s_params.h"

namespace h2s {

// the record of frame f of the launch P binds
__device__ __forceinline__ const DoviRec* dovi_record(const KParams& P, int f) {
  return P.dovi + (P.dovi_n == 1 ? 0 : P.dovi_f0 + f);
}

// one component: its piece of s[c], the piece's polynomial or MMR over the
// unreshaped s of all three, clamped to the curve's own range
template <class T>
__device__ __forceinline__ T dovi_reshape(const DoviCurve& C, const T (&s)[3], int c) {
  const T x = s[c];
  const int last = C.num_pivots - 2;
  int k = 0;
  for (int i = 1; i <= last; i++) k = (T)C.pivots[i] <= x ? i : k;
  T r;
  if (C.method[k] == 0) {
    r = (T)C.poly[k][0] + (T)C.poly[k][1] * x + (T)C.poly[k][2] * (x * x);
  } else {
    const T t[7] = {s[0], s[1], s[2], s[0] * s[1], s[0] * s[2], s[1] * s[2], s[0] * s[1] * s[2]};
    r = (T)C.mmr_const[k];
    T p[7];
#pragma unroll
    for (int j = 0; j < 7; j++) p[j] = t[j];
    for (int i = 0; i < C.mmr_order[k]; i++) {
#pragma unroll
      for (int j = 0; j < 7; j++) {
        r += (T)C.mmr[k][i][j] * p[j];
        p[j] *= t[j];
      }
    }
  }
  const T lo = (T)C.pivots[0], hi = (T)C.pivots[last + 1];
  return r < lo ? lo : (r > hi ? hi : r);
}

// s (code / (2^b - 1), each in [0, 1]) -> v = clamp(N (r - off), 0, 1): L'M'S'
template <class T>
__device__ __forceinline__ void dovi_lms_pq(const DoviRec& R, const T (&s)[3], T (&v)[3]) {
  T d[3];
#pragma unroll
  for (int c = 0; c < 3; c++) d[c] = dovi_reshape<T>(R.comp[c], s, c) - (T)R.off[c];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const T x = (T)R.nl[3 * c] * d[0] + (T)R.nl[3 * c + 1] * d[1] + (T)R.nl[3 * c + 2] * d[2];
    v[c] = x > (T)0 ? (x < (T)1 ? x : (T)1) : (T)0;   // (NaN -> 0)
  }
}

}  // namespace h2s
