// h2s_tile_sets.h — which k_tile<TRC, TM, DESAT, LP, DBG, SEMI, SUB> instances
// exist, and in which translation unit: the one table.  From it come the
// kernels each unit instantiates (H2S_TILE_UNIT, the whole of a stub unit),
// the extern declarations every other unit sees, the dispatch of a launch
// (launch_fast, h2s_fast.hip) and the host's predicate (tile_instance,
// h2s_launch.h), so a set or a case that one of them had and another lacked
// cannot be written.  Adding a set: DESIGN.md §4.1, "Adding an instance set".
#pragma once
#include "h2s_launch.h"
#include "h2s_tile.h"

// A family's cases X(TRC, TM, DESAT), in the order its units instantiate them:
// the CPU chain's (vf_tonemap's three operators with desat 0 off, 1 weighted
// luma, 2 RGB-coefficient luma; BT.2390 and spline have none) and the
// libplacebo branch's (LP: no desat), each for PQ (TRC 0) and HLG (TRC 1)
// input, and the libplacebo branch's on Dolby Vision records (TRC 2)
#define H2S_CASES_CPU(X, T) \
  X(T, 4, 0) X(T, 4, 1) X(T, 4, 2) X(T, 5, 0) X(T, 5, 1) X(T, 5, 2) X(T, 6, 0) X(T, 6, 1) X(T, 6, 2) X(T, 7, 0) X(T, 8, 0)
#define H2S_CASES_LP(X, T) X(T, 7, 0) X(T, 8, 0) X(T, 4, 0) X(T, 5, 0) X(T, 6, 0)
#define H2S_FAMILY_CPU(X) H2S_CASES_CPU(X, 0) H2S_CASES_CPU(X, 1)
#define H2S_FAMILY_LP(X) H2S_CASES_LP(X, 0) H2S_CASES_LP(X, 1)
#define H2S_FAMILY_DV(X) X(2, 4, 0) X(2, 5, 0) X(2, 6, 0) X(2, 7, 0) X(2, 8, 0)
#define H2S_TILE_FAMILIES(F) F(CPU) F(LP) F(DV)

// The instance sets S(UNIT, DBG, LP, SEMI, SUB, FAMILY): every case of FAMILY
// as k_tile<TRC, TM, DESAT, LP, DBG, SEMI, SUB>, explicitly instantiated in
// h2s_UNIT.hip and nowhere else.  One unit per set: the two chains' product
// instances each get the scheduler that measured fastest for them (_build.py
// SOURCE_FLAGS), and the parallel build stays parallel.
//  DBG 1: the debug instances (every h2s_stage, F.dbg_stage), 4:2:0 left-sited only
//  SEMI: the instances that also serve semi-planar frame sets; a launch with
//    planar sets on both sides takes the SEMI = false set (k_tile's comment)
//  SUB 1 / 2: 4:2:2 / 4:4:4 input, the CPU chain's product instances (SEMI: the
//    output side's layout branches); SUB 3: top-left 4:2:0 input, either
//    chain's product instances, planar or semi-planar on either side
#define H2S_TILE_SETS(S)                        \
  S(fast, 0, 0, false, 0, CPU)                  \
  S(fast_lp, 0, 1, false, 0, LP)                \
  S(fast_semi, 0, 0, true, 0, CPU)              \
  S(fast_lp_semi, 0, 1, true, 0, LP)            \
  S(fast_sub422, 0, 0, true, 1, CPU)            \
  S(fast_sub444, 0, 0, true, 2, CPU)            \
  S(fast_tl, 0, 0, true, 3, CPU)                \
  S(fast_lp_tl, 0, 1, true, 3, LP)              \
  S(debug, 1, 0, false, 0, CPU)                 \
  S(debug_lp, 1, 1, false, 0, LP)               \
  S(debug_semi, 1, 0, true, 0, CPU)             \
  S(debug_lp_semi, 1, 1, true, 0, LP)           \
  S(fast_lp_dv, 0, 1, false, 0, DV)             \
  S(fast_lp_dv_semi, 0, 1, true, 0, DV)         \
  S(debug_lp_dv, 1, 1, false, 0, DV)            \
  S(debug_lp_dv_semi, 1, 1, true, 0, DV)

namespace h2s {

enum TileSetId {
#define S(UNIT, DBG, LP, SEMI, SUB, FAMILY) SET_##UNIT,
  H2S_TILE_SETS(S)
#undef S
};
enum TileFamily {
#define F(NAME) FAMILY_##NAME,
  H2S_TILE_FAMILIES(F)
#undef F
};

// whether k's (trc, tm, desat) is a case of the family
inline bool family_case(int family, const TileKey& k) {
#define X(T, M, D) \
  if (k.trc == T && k.tm == M && k.desat == D) return true;
#define F(NAME) \
  if (family == FAMILY_##NAME) { H2S_FAMILY_##NAME(X) }
  H2S_TILE_FAMILIES(F)
#undef F
#undef X
  return false;
}

// the launch of set SET's instance for k's case (k's other fields chose the set: launch_fast)
template <int SET>
hipError_t launch_set(const FastParams& F, const TileKey& k, dim3 grid, size_t lds, hipStream_t s) {
#define X(T, M, D)                                                                                   \
  if (k.trc == T && k.tm == M && k.desat == D) {                                                     \
    hipLaunchKernelGGL((k_tile<T, M, D, set_lp, set_dbg, set_semi, set_sub>), grid, dim3(256), lds, s, F); \
    return hipGetLastError();                                                                        \
  }
#define S(UNIT, DBG, LP, SEMI, SUB, FAMILY)                            \
  if constexpr (SET == SET_##UNIT) {                                   \
    constexpr int set_dbg = DBG, set_lp = LP, set_sub = SUB;           \
    constexpr bool set_semi = SEMI;                                    \
    H2S_FAMILY_##FAMILY(X)                                             \
  }
  H2S_TILE_SETS(S)
#undef S
#undef X
  return hipErrorInvalidValue;
}

#define H2S_TILE_SET_SIGNATURE(UNIT) \
  hipError_t launch_set<SET_##UNIT>(const FastParams&, const TileKey&, dim3, size_t, hipStream_t);
#define S(UNIT, DBG, LP, SEMI, SUB, FAMILY) extern template H2S_TILE_SET_SIGNATURE(UNIT)
H2S_TILE_SETS(S)
#undef S

}  // namespace h2s

// the whole of h2s_UNIT.hip: the unit's set, instantiated here
#define H2S_TILE_UNIT(UNIT) \
  namespace h2s {           \
  template H2S_TILE_SET_SIGNATURE(UNIT) }
