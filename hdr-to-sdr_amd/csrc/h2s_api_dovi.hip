// h2s_api_dovi.hip — Dolby Vision profile 5 on the host (h2s_set_dovi,
// include/h2s.h): the records' validation and upload, and what a call with
// records set is refused for.  The arithmetic is the kernels' (h2s_dovi.h).
#include <stddef.h>

#include "h2s_host.h"

using namespace h2s::host;
using h2s::KParams;

// the device's view of a record is the caller's struct, field for field
static_assert(sizeof(h2s::DoviCurve) == sizeof(h2s_dovi_curve) && sizeof(h2s::DoviRec) == sizeof(h2s_dovi_rpu),
              "DoviRec mirrors h2s_dovi_rpu");
static_assert(offsetof(h2s::DoviCurve, mmr) == offsetof(h2s_dovi_curve, mmr) &&
                  offsetof(h2s::DoviCurve, poly) == offsetof(h2s_dovi_curve, poly) &&
                  offsetof(h2s::DoviCurve, mmr_const) == offsetof(h2s_dovi_curve, mmr_const) &&
                  offsetof(h2s::DoviRec, comp) == offsetof(h2s_dovi_rpu, comp) &&
                  offsetof(h2s::DoviRec, lin) == offsetof(h2s_dovi_rpu, linear),
              "DoviRec mirrors h2s_dovi_rpu");

namespace {

bool all_finite(const float* v, int n) {
  for (int i = 0; i < n; i++)
    if (!isfinite(v[i])) return false;
  return true;
}

// "" or what is wrong with record i
std::string record_error(const h2s_dovi_rpu& r, int i) {
  const std::string at = "Dolby Vision record " + std::to_string(i);
  if (!all_finite(r.nonlinear_offset, 3) || !all_finite(r.nonlinear, 9) || !all_finite(r.linear, 9))
    return at + ": a matrix or offset entry is not finite";
  for (int c = 0; c < 3; c++) {
    const h2s_dovi_curve& k = r.comp[c];
    const std::string cc = at + ", component " + std::to_string(c);
    if (k.num_pivots < 2 || k.num_pivots > 9) return cc + ": num_pivots must be in [2, 9]";
    for (int p = 0; p < k.num_pivots; p++) {
      if (!(k.pivots[p] >= 0.0f && k.pivots[p] <= 1.0f)) return cc + ": pivots must lie in [0, 1]";
      if (p && !(k.pivots[p] > k.pivots[p - 1])) return cc + ": pivots must ascend";
    }
    for (int p = 0; p < k.num_pivots - 1; p++) {
      if (k.method[p] != 0 && k.method[p] != 1) return cc + ": method must be 0 (polynomial) or 1 (MMR)";
      if (k.method[p] == 0) {
        if (!all_finite(k.poly[p], 3)) return cc + ": a polynomial coefficient is not finite";
        continue;
      }
      if (k.mmr_order[p] < 1 || k.mmr_order[p] > 3) return cc + ": mmr_order must be in [1, 3]";
      if (!isfinite(k.mmr_const[p]) || !all_finite(&k.mmr[p][0][0], 7 * k.mmr_order[p]))
        return cc + ": an MMR coefficient is not finite";
    }
  }
  return "";
}

// the shape profile 5 actually carries, which the tile kernel's Dolby Vision
// instances take (h2s_tile_px.h dovi_tile_front): luma polynomial pieces only, each
// chroma component a single piece (polynomial, or MMR up to order 3)
bool dovi_tile_shape(const h2s_dovi_rpu& r) {
  for (int p = 0; p < r.comp[0].num_pivots - 1; p++)
    if (r.comp[0].method[p] != 0) return false;
  return r.comp[1].num_pivots == 2 && r.comp[2].num_pivots == 2;
}

}  // namespace

namespace h2s {
namespace host {

// what a call over frames [f0, f0 + nframes) of the context's records is
// refused for (k: resolved); no records: nothing
int check_dovi(h2s_ctx* c, const KParams& k, Format in_fmt, int f0, int nframes) {
  if (!c->dovi_n) return 0;
  if (k.pipe != h2s::PIPE_LIBPLACEBO)
    return fail(c, H2S_E_UNSUPPORTED,
                "Dolby Vision profile 5 runs on the libplacebo pipeline only (the reference's CPU chain has no RPU "
                "and shows wrong colours): set params.pipeline to H2S_PIPE_LIBPLACEBO or a libplacebo operator");
  if (in_fmt.loc == H2S_CHROMA_TOPLEFT)
    return fail(c, H2S_E_UNSUPPORTED, "Dolby Vision profile 5: top-left chroma siting is not modelled");
  if (c->dovi_n > 1 && (long long)f0 + nframes > c->dovi_n)
    return fail(c, H2S_E_INVALID_ARG,
                "frames " + std::to_string(f0) + ".." + std::to_string(f0 + nframes - 1) + " of the call need Dolby Vision records, " +
                    std::to_string(c->dovi_n) + " are set (h2s_set_dovi)");
  return 0;
}

}  // namespace host
}  // namespace h2s

extern "C" int h2s_set_dovi(h2s_ctx* c, const h2s_dovi_rpu* rpu, int n) {
  // (the records are judged first, context or not: a caller can validate
  // records with ctx NULL, where a valid set ends in "ctx is NULL")
  if (n < 0) return fail(c, H2S_E_INVALID_ARG, "n < 0");
  if (n > 0 && !rpu) return fail(c, H2S_E_INVALID_ARG, "rpu is NULL");
  for (int i = 0; i < n; i++) {
    const std::string e = record_error(rpu[i], i);
    if (!e.empty()) return fail(c, H2S_E_INVALID_ARG, e);
  }
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  if (n == 0 && c->dovi_n == 0) return 0;   // off, and nothing queued reads a record
  DeviceGuard g(c->device);
  // queued launches may still read the records this call replaces
  int rc = drain_launches(c);
  if (rc) return rc;
  if (n == 0) {
    c->dovi_n = 0;
    return 0;
  }
  hipStream_t aux;   // (fetched for its side effect: upload_table copies on the context stream)
  if ((rc = aux_stream(c, &aux))) return rc;
  c->dovi_n = 0;   // (a failed upload leaves the front-end off)
  if ((rc = upload_table(c, c->d_dovi, rpu, (size_t)n * sizeof(h2s_dovi_rpu), "Dolby Vision records"))) return rc;
  c->dovi_n = n;
  c->dovi_tile = true;
  for (int i = 0; i < n; i++) c->dovi_tile = c->dovi_tile && dovi_tile_shape(rpu[i]);
  return 0;
}
