// h2s_tile.h — the tile kernel k_tile (the specialised fast path of the fused
// tone-map kernel) and what is its own: the block's LDS, the prologue, the
// walk over tiles with its two barriers, the 8 steps of a tile.  The
// arithmetic of a pixel is h2s_tile_tone.h's and h2s_tile_px.h's, loads,
// staging and stores are h2s_tile_io.h's, and which instances exist, in which
// translation unit, is h2s_tile_sets.h's, through which h2s_fast*.hip (product
// instances) and h2s_debug*.hip (debug instances) include this file.
//
// Same chain as k_generic (h2s_kernels.hip) and oracle/h2s_oracle.c, restated
// for throughput on gfx950:
//  * one template instance per (transfer, operator, desat): the 8 steps a wave
//    runs per tile are straight-line code the compiler can interleave;
//  * chroma upsampling on integer-valued floats (exact), the 1/4, 1/8 and
//    depth-normalisation scales folded into the Y'CbCr->R'G'B' constants;
//  * the 3D-LUT lattice pre-multiplied into output Y'CbCr code space
//    (RGB->Y'CbCr is linear, and the host routes the CPU chain here only
//    while every lattice value is finite and in [0,1] -- h2s_set_lut records
//    it, fast_params_ok tests it -- so the swscale clip is a no-op and
//    blend-then-convert == convert-then-blend; any other lattice runs on the
//    generic kernel, which clips the blend); the tetrahedral blend then
//    yields quantiser inputs directly;
//  * lattice gathers are buffer loads (32-bit offsets, one SGPR base);
//  * eq's table sits in LDS.
// Geometry (k_tile): a block of 256 threads walks 8 consecutive 64 x 32 luma
// tiles, prefetching tile i+1 into registers while tile i computes.  A tile
// (Y, and U/V with their 1-row halo) is staged into LDS with coalesced
// 16-byte loads; then, in 8 steps, each wave processes one dense 8 x 8 pixel
// sub-block with one pixel per lane (lanes 4q..4q+3 = one 2x2 quad).  Dense
// sub-blocks keep the 64 lanes of every lattice gather on few cache lines;
// in a step the block's four waves take the four quarters of one 16 x 16
// macro-block (8 macro-blocks per tile, walked row by row), so the gathers the
// CU has in flight from one block share lattice lines in the L1 (the CPU
// chain's instances; the libplacebo instances, which gather nothing from the
// lattice, keep a 16-pixel column strip per wave: DESIGN.md §4.1, "Wave
// layout"; scripts/l1_wave_layout_sim.py);
// chroma is reduced per quad with DPP quad permutes and all outputs leave
// through LDS as 16-byte coalesced stores.  Measured balance (DESIGN.md
// §4.1): VALU ~70 % busy, LDS ~47 %, vector-memory return ~35 %.
// Tile I/O ("The tile I/O"): luma lies in LDS as the 16-bit
// codes that were loaded (luma_at): a step converts its sample and writes
// the output code over it, and the store phase moves 16 bytes unchanged.
// Every thread issues the same loads and the same two 16-byte stores per
// tile under no branch (tile_load, tile_store: what a thread does not need
// goes to an offset the buffer resource drops), and a tile is committed
// behind the previous tile's stores, so the compiler's counted waits for
// the loads never wait for a store.  Two barriers per tile.
#pragma once
#include "h2s_tile_io.h"

namespace h2s {

// frame f's curve record: a constant-address-space load with a block-uniform
// index, so the compiler emits scalar (s_load) reads
__device__ __forceinline__ CurveConsts curve_of(const CurveConsts* frames, int f) {
  typedef __attribute__((address_space(4))) const float cfloat;
  constexpr int n = (int)(sizeof(CurveConsts) / sizeof(float));
  cfloat* src = (cfloat*)frames + __builtin_amdgcn_readfirstlane(f) * n;
  CurveConsts r;
  float* dst = reinterpret_cast<float*>(&r);
#pragma unroll
  for (int i = 0; i < n; i++) dst[i] = src[i];
  return r;
}

// k_tile's amdgpu_waves_per_eu:
// 5 waves per SIMD = the LDS-bound occupancy (5 blocks of ~27.6 KB per CU;
// 3, 4 and 6 measured slower on the bench content, 6 by 4.5 % in round 3 at
// 80 VGPRs: profiles/r03/ablations/six_waves.log, blocks_per_cu.log): let
// the compiler use the VGPRs that allows
constexpr int TILE_WPE = 5;
// the libplacebo instances: the same 5 waves per SIMD for the register
// budget (96 VGPRs, 2-6 spilled); 4 (106 VGPRs, no spills) measured 8 %
// slower with the PQ-encode table's branch-free form (profiles/r05/lp_variants.log)
constexpr int TILE_WPE_LP = TILE_WPE;

// Each block walks F.tpb consecutive tiles (XCD-remapped, so neighbouring
// tiles and their lattice cells share one XCD's L2).  The loads of tile i+1
// are issued before tile i is computed, so after the first tile the block no
// longer waits on HBM latency.  Per tile: prefetch, barrier, 8 compute steps,
// barrier, store, commit the next tile's registers -> LDS (the first tile's
// commit precedes the loop; no barrier between store and commit, see the
// loop's end).  (A fifth wave doing all
// of the frame I/O, so that the compute waves' gathers never wait behind the
// prefetch in the shared vector-memory counter, measured 1.5x slower: its
// serial store + commit phase idles the four compute waves;
// profiles/r03/ablations/io_wave*.  Issuing the stores of tile i-1 and the
// loads of tile i+1 inside step 7, behind its gathers, measured 3-5 % slower:
// profiles/r03/ablations/late_io*.)
// DBG (0 or 1; 1 = the debug instances, never launched by h2s_process): run
// the whole chain and also write the three float planes of h2s_stage
// F.dbg_stage (1..5, a run-time field: one debug instance per chain serves
// every stage) for frame 0 to F.dbg (W x H each) from this kernel's own
// arithmetic — stage 4 blends the float4 RGB lattice F.dbg_lut with the same
// cell, corners and weights as the Y'CbCr lattice.
// LP = 1: the libplacebo branch (src/utils.py:444-460, BT.2390 / spline):
// BT.1886 encode against the target black, 8-bit rgba download, lut3d's 8-bit
// path on plain R'G'B' records (truncating output), BT.709 Y'CbCr at depth q
// SEMI: the instances that also serve semi-planar frame sets (F.in_semi /
// F.out_semi, h2s_set_frame_layout), with a block-uniform branch wherever the
// addressing or the packing differs.  They are separate instances because
// those branches cost registers whichever way they go (8-10 VGPRs and a dozen
// spilled SGPRs on the product instances): a launch with
// planar sets on both sides runs the SEMI = false instance, which compiles
// to what it was before the layouts existed
// SUB (the input's chroma subsampling, h2s_set_input_subsampling): 1 = 4:2:2,
// 2 = 4:4:4, CPU chain product instances only (LP 0, DBG 0; SEMI for the
// output side).  The staged chroma keeps hrow's allocation (so the block's LDS
// and the 5 blocks per CU): 4:2:2 as x1 centred floats, 32 rows of C422_ST,
// with the horizontal pass in the step; 4:4:4 as 16-bit centred codes, 32
// rows of C444_ST.  The step hands lin_tone the same x8 centred values (exact
// small integers), so everything after S0 is the 4:2:0 instance's code.  The
// SUB 0 instances compile to what they were before the parameter existed
// SUB 3 (h2s_set_input_tags, H2S_CHROMA_TOPLEFT): 4:2:0 input whose chroma rows
// are co-sited with the even luma rows, product instances of both chains (DBG
// 0; SEMI, so either side may be semi-planar).  Loads, staging and hrow are the
// 4:2:0 form's (rows cy0 - 1 .. cy0 + 16, of which row cy0 - 1 is not used);
// only the step's vertical combine differs: 4 h[cy] on even luma rows,
// 2 (h[cy] + h[cy + 1]) on odd ones, the same x8 exact integers
template <int TRC, int TM, int DESAT, int LP, int DBG = 0, bool SEMI = false, int SUB = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LP ? TILE_WPE_LP : TILE_WPE))) void k_tile(
    const FastParams F) {
  static_assert(DBG == 0 || DBG == 1, "the stage is F.dbg_stage, not a template value");
  static_assert(SUB == 0 || SUB == 3 || (LP == 0 && DBG == 0), "4:2:2 / 4:4:4 input: CPU chain product instances only");
  static_assert(SUB != 3 || (DBG == 0 && SEMI), "top-left 4:2:0 input: the SEMI product instances");
  constexpr bool S420 = SUB == 0 || SUB == 3;   // the input is 4:2:0 (4:2:0 loads and staging)
  constexpr int YST = row_stride<LP>(), HST = YST;
  static_assert(TBH * C422_ST <= (CBH + 2) * HST && TBH * C444_ST <= 2 * (CBH + 2) * HST, "hrow holds the SUB windows");
  __shared__ __attribute__((aligned(16))) unsigned char yin[YIN_BYTES];   // luma codes (luma_at); output codes overwrite them in place
  __shared__ float hrow[2][(CBH + 2) * HST];   // chroma rows (halo incl.) upsampled x2 horizontally
  __shared__ float csum[2][CBH * CBW];         // per chroma sample: sum of its 2x2 pixel contributions
  __shared__ float4 pq_lds[PQ_NSEG + 1];       // [0] = zero segment (pq_z): PQ EOTF, or HLG inverse OETF (!LP)
  __shared__ float4 pqi_lds[LP ? PQI_NTAB : 1];                   // PQ encode (lp_tone IPT)
  extern __shared__ uint16_t eq_lds[];         // eq table, codes pre-shifted to the output depth
  __shared__ int tflag[2];                     // per tile parity: some staged code outside the branch-free bound
  __shared__ int offtab[4];                    // +1 corner offsets along r, g, b (px_chain's TAG)
  __shared__ unsigned spread_lds[LP ? 256 : 1];   // LP, Morton table order: code c's bits at every third position
  // PQ: E is produced pre-scaled into table-segment units (the x PQ_SEG is
  // folded into the Y'CbCr->R'G'B' constants)
  constexpr int ESC = TRC == 0 || !LP ? PQ_SEG : 1;   // as px_chain

  const int t = threadIdx.x;
  const int lane = t & 63, w = t >> 6;
  const unsigned ntiles = F.nbx * F.nby * F.nframes;
  unsigned tile = (unsigned)xcd_remap(blockIdx.x, gridDim.x) * (unsigned)F.tpb;
  const unsigned tend = tile + (unsigned)F.tpb < ntiles ? tile + (unsigned)F.tpb : ntiles;

  // ---- prologue: first tile + tables, all issued before any wait ----
  TileGeo geo = tile_geo(F, tile);
  const LaneOfs lofs = lane_ofs<SEMI>(F, t);
  TileRegs<SEMI, SUB> cur = tile_load<SEMI, SUB>(F, geo, t, lofs);
  const __amdgpu_buffer_rsrc_t req = __builtin_amdgcn_make_buffer_rsrc((void*)F.eq_lut, (short)0, 2 * F.eq_n, 0x00020000);
  const unsigned eq0 = __builtin_amdgcn_raw_buffer_load_b16(req, 2 * t, 0, 0);  // out of range -> 0
  float4 pq0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const bool stage_pq = TRC != 1 || !LP || F.lp_ipt;   // block-uniform (TRC 2, Dolby Vision: the PQ EOTF of L'M'S')
  if (stage_pq && t < PQ_NSEG) {
    const __amdgpu_buffer_rsrc_t rpq = __builtin_amdgcn_make_buffer_rsrc((void*)F.pq_tab, (short)0, 16 * PQ_NSEG, 0x00020000);
    pq0 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rpq, 16 * t, 0, 0));
  }
  // codes at the output depth: shift, or bit replication (h2s_expand;
  // rep_rs = 8 - shift, or 31 for a plain shift: the 8-bit code >> 31 = 0)
  // (semi-planar 16-bit output: the luma word's high-bit alignment, F.out_sh,
  // is folded into the table, so the luma stores are the planar ones)
  const int eq_sh = SEMI ? F.out_sh : 0;
  if (t < F.eq_n) eq_lds[t] = (uint16_t)(((eq0 << F.shift_out) | (eq0 >> F.rep_rs)) << eq_sh);
  for (int i = t + 256; i < F.eq_n; i += 256) {  // native 10/12-bit tables
    const unsigned v = __builtin_amdgcn_raw_buffer_load_b16(req, 2 * i, 0, 0);
    eq_lds[i] = (uint16_t)(((v << F.shift_out) | (v >> F.rep_rs)) << eq_sh);
  }
  // the first segment (E' < 1/128) marked (cubic FLT_MAX t: 0 at E = 0,
  // > DARK_MARK above) wherever the table is the PQ EOTF (not the CPU chain's
  // HLG table): px_chain's dark re-run evaluates it exactly
  if (stage_pq && t < PQ_NSEG)
    pq_lds[t + 1] = (TRC == 0 || LP) && t == 0 ? make_float4(0.0f, 0.0f, 3.40282347e38f, 0.0f) : pq0;
  if (stage_pq && t == 255) pq_lds[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (t < 2) tflag[t] = 0;
  if (t < 3) offtab[t] = t == 0 ? 12 : (t == 1 ? F.og : F.ob);
  if (LP) {
    unsigned x = (unsigned)t;
    x = (x | (x << 8)) & 0x0F00Fu;
    x = (x | (x << 4)) & 0x0C30C3u;
    spread_lds[t] = (x | (x << 2)) & 0x249249u;
  }
  __syncthreads();   // the flags are zero before any thread's first commit sets one
  // (TRC 2: the max-RGB form encodes sig through this table too, tone<..., DV>)
  if (LP && (F.lp_ipt || TRC == 2)) {
    const __amdgpu_buffer_rsrc_t rpi = __builtin_amdgcn_make_buffer_rsrc((void*)F.pqi_tab, (short)0, 16 * PQI_NTAB, 0x00020000);
    for (int i = t; i < PQI_NTAB; i += 256)
      pqi_lds[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rpi, 16 * i, 0, 0));
  }

  // ---- per-lane step geometry: step m is the 16x16 macro-block (m & 3,
  // m >> 2) of the tile, of which wave w takes the 8x8 quarter (w & 1, w >> 1),
  // i.e. sub-block (2 (m&3) + (w&1), 2 (m>>2) + (w>>1)); lane = pixel (quad
  // q = lane>>2 in a 4x4 quad grid, position lane&3 in the quad).  The wave's
  // quarter goes into the per-lane bases below, the step into compile-time
  // LDS offsets (16 columns per m & 3, 16 rows per m >> 2).  One LDS
  // instruction still covers 8 rows x 8 columns from one base, and the wave's
  // quarter shifts that base by whole 8-sample chunks and whole groups of 8
  // luma (4 chroma) rows: the bank arguments at luma_at, row_stride, C422_ST
  // and C444_ST hold for every wave as they held for the strips ----
  // MB: the macro-block layout above, every CPU-chain instance.  The
  // libplacebo instances (LP) keep the layout this kernel had before it: wave w
  // walks the 16-pixel column strip w, step s = sub-block (2w + (s&1), s>>1).
  // Their rgba8 download rounds a value that float32 carries to about 1e-4 of
  // a code, and moving an 8x8 block to another unrolled step moved one such
  // tie of one instance's output ("Wave layout"): their bytes
  // stay what they were
  constexpr bool MB = !LP;
  auto SX = [](int s) { return MB ? 16 * (s & 3) : 8 * (s & 1); };    // step s's pixel offset from step 0's
  auto SY = [](int s) { return MB ? 16 * (s >> 2) : 8 * (s >> 1); };
  const int wx = MB ? w & 1 : 2 * w, wy = MB ? __builtin_amdgcn_readfirstlane(w >> 1) : 0;   // the wave's first sub-block
  const int qx = (lane >> 2) & 3, qy = lane >> 4, pxl = lane & 1, pyl = (lane >> 1) & 1;
  const int xl = 8 * wx + 2 * qx + pxl, yl = 8 * wy + 2 * qy + pyl;   // step 0's pixel (MB: (x, y) mod 16 at every step)
  uint16_t* ybase = reinterpret_cast<uint16_t*>(yin + luma_at(xl, yl));   // this lane's sample of step 0
  // vertical pass (centre siting): 3 x row cy + row cy-1 (top) / cy+1 (bottom)
  const float* h0 = hrow[0] + ((yl >> 1) + 1) * HST + xl;
  const float* h1 = hrow[1] + ((yl >> 1) + 1) * HST + xl;
  // (SUB 3, rows co-sited with the even luma row: row cy again (even luma rows) / cy+1 (odd))
  const int hb = SUB == 3 ? (pyl ? HST : 0) : (pyl ? HST : -HST);
  // SUB 1: the pixel's own chroma row, sample xl >> 1 and (odd columns) the one right of it
  const float* c0 = hrow[0] + yl * C422_ST + (xl >> 1);
  const float* c1 = hrow[1] + yl * C422_ST + (xl >> 1);
  // SUB 2: the pixel's own sample
  const int16_t* s0 = reinterpret_cast<const int16_t*>(hrow[0]) + yl * C444_ST + xl;
  const int16_t* s1 = reinterpret_cast<const int16_t*>(hrow[1]) + yl * C444_ST + xl;
  float* csb = csum[0] + csum_at(xl >> 1, yl >> 1);   // the quad's chroma sample of step 0

  // hot constants live in VGPRs for the whole kernel.  Staged samples:
  // luma Y*ys + y_off (+1 on PQ: pq_z's zero segment), chroma centred on its
  // midpoint code (exact), so E = Y' + a*{U,V} takes 4 FMAs
  const float yoff = in_vgpr(F.y_off_c) * (float)ESC + (ESC == PQ_SEG ? 1.0f : 0.0f);
  const float cmid = in_vgpr(F.c_mid);
  const float a_rv = in_vgpr(F.a_rv[1]) * (float)ESC, a_gv = in_vgpr(F.a_gv[1]) * (float)ESC,
              a_gu = in_vgpr(F.a_gu[1]) * (float)ESC, a_bu = in_vgpr(F.a_bu[1]) * (float)ESC;
  const float stride_g = in_vgpr(F.stride_g), stride_b = in_vgpr(F.stride_b);
  const int og = in_vgpr(F.og), ob = in_vgpr(F.ob), ocr = in_vgpr(F.cr), ocg = in_vgpr(F.cg), ocb = in_vgpr(F.cb);
  const float log2_nm1 = in_vgpr(F.log2_nm1), x_max = in_vgpr(F.x_max);
  const float ysc = in_vgpr(F.ys) * (float)ESC;   // zimg depth-conversion scale
  // S6 ordered dither (h2s_dither ORDERED, 8-bit quantiser): this lane's
  // pixel is (xl, yl) mod 8 at every step (tile and step origins are
  // multiples of 8), so its luma offset is one constant
  const float ydq = F.dither ? dither_off(xl, yl) - 0.5f : 0.0f;
  const StepK K{a_rv, a_gv, a_gu, a_bu, stride_g, stride_b, og, ob, ocr, ocg, ocb, log2_nm1, x_max,
                TM == 5 && !LP ? in_vgpr(F.hable_kb) : F.hable_kb, F.c111, rintf(1.0f / F.inv_nm1), offtab,
                LP ? in_vgpr(F.lp_k2) : 0.0f, LP ? in_vgpr(F.lp_k2 + 255.0f) : 0.0f, LP ? F.lp_cy + ydq : 0.0f,
                LP ? in_vgpr(F.lp_k1) : 0.0f};
  gu32* lut8v = LP ? in_vgpr64(F.lut8x) : nullptr;   // (a 64-bit VGPR base: no SGPRs to spill)
  // libplacebo branch: the rgba8 download offset of this lane's pixel at step
  // s (x mod 16 = xl + SX(s), y mod 16 = yl + SY(s) mod 16: tile origins are
  // multiples of 16; the strips' four positions are steps 0..3's)
  float qo[4];
#pragma unroll
  for (int i = 0; i < 4; i++)
    qo[i] = LP ? F.lp_qo + (F.lp_dith ? bayer16(xl + SX(i), yl + SY(i)) : 0.5f) -
                     (F.lut_off ? 0.0f : F.lp_k2 * F.lp_qs_f)
               : 0.5f;

  // the 8 compute steps of one tile; FB (fast body): no pixel of the tile can
  // reach the exact EOTF path and there is no BICUBIC scratch, so the 8 steps
  // are one straight-line block the scheduler can interleave
  auto steps = [&](const TileGeo& g, auto fast) {
    constexpr bool FB = decltype(fast)::value;
    constexpr int YR2 = YROW / 2;   // the luma tile's row stride in samples
    if constexpr (FB) {
      H2S_MARK("body: fast");
    } else {
      H2S_MARK("body: exact-capable");
    }
    // BT.2390 / spline: this tile's frame curve (dynamic peak: one record per
    // frame, read through the scalar cache; the frame index is block-uniform)
    CurveConsts cv = F;
    if ((TM == 7 || TM == 8 || LP) && F.cv_frames) cv = curve_of(F.cv_frames, g.f);
    // Dolby Vision (TRC 2): this tile's frame record (block-uniform, as the curve's)
    const CDoviRec* const dv =
        TRC == 2 ? (const CDoviRec*)F.dovi + __builtin_amdgcn_readfirstlane(F.dovi_n == 1 ? 0 : F.dovi_f0 + g.f) : nullptr;
    if constexpr (LP && TM == 7) {
      // the curve's constants that meet a second scalar operand in an FMA or
      // med3 (one scalar operand per VOP3 on gfx950): in VGPRs once per
      // tile instead of a v_mov per step (libplacebo instances, which have
      // the VGPRs; round 6)
      cv.b_e1b = in_vgpr(cv.b_e1b), cv.b_tb = in_vgpr(cv.b_tb), cv.b_c2 = in_vgpr(cv.b_c2);
      cv.b_lc = in_vgpr(cv.b_lc), cv.b_bk_b = in_vgpr(cv.b_bk_b), cv.b_bk_d = in_vgpr(cv.b_bk_d);
    } else if constexpr (LP && TM == 8) {
      cv.sp_qb_u = in_vgpr(cv.sp_qb_u), cv.sp_pb_u = in_vgpr(cv.sp_pb_u);
      cv.sp_srcmax = in_vgpr(cv.sp_srcmax), cv.sp_umax = in_vgpr(cv.sp_umax);
    }
    const __amdgpu_buffer_rsrc_t lut = __builtin_amdgcn_make_buffer_rsrc((void*)F.lut_yuv, (short)0, F.lut_bytes, 0x00020000);
    // A wave's sub-block whose 8 rows lie past the frame's last row computes
    // what is never stored, so it is skipped.  Macro-blocks: on the bottom tile
    // row of a 2160-row frame (16 live rows) that is macro-row 1, steps 4-7,
    // for every wave; with 8 or 24 live rows also the lower waves' quarters of
    // the last live macro-row.  Strips: whole step pairs.  The test is
    // wave-uniform (no barrier sits inside the steps) and applies to product
    // instances, not to the BICUBIC scratch path.  Only this exact-capable body
    // tests for it (k_tile sends such tiles here), so the fast body stays one
    // straight-line block
    // (live: the frame's rows from the first row of this wave's step-0 sub-block on)
    const int live = !FB && DBG == 0 && !F.chr444 ? F.H - g.py0 - 8 * wy : TBH;
    // the 2x2 chroma sums of step s (or, BICUBIC, the pixel's Cb, Cr into the
    // frame's 4:4:4 scratch, which k_chroma_bicubic decimates; the scratch
    // has whole tiles of rows: rows past F.H are written, never read)
    auto chroma_out = [&](int s, float oyv, float ozv) {
      if (!FB && F.chr444) {
        const int px = g.px0 + xl + SX(s), py = g.py0 + yl + SY(s);
        F.chr444[(long long)py * F.chr_w + px] = make_float2(oyv * F.inv_c56, ozv * F.inv_c56);
        return;
      }
      // chroma: 2x2 sums; the 4 lanes of a quad store the same value
      H2S_MARK("S6 chroma quad sums");
      const int oc = csum_at(SX(s) / 2, SY(s) / 2);   // (MB: whole 256-byte units, csum_at)
      const float su = quad_sum(oyv), sv = quad_sum(ozv);
      csb[oc] = su;
      csb[oc + CBH * CBW] = sv;
    };
    if constexpr (LP && DBG == 0) {
      if (!F.lut_off) {   // (launch-uniform)
        // The libplacebo branch's product steps, software-pipelined: step s's
        // lut3d table read (a 64 MiB table: its lines come from the L2 or the
        // MALL) is issued, then step s + 1's S1..S4 run, and only then is
        // step s finished (Y'CbCr, eq, the luma code into yin, the chroma
        // sums), so the read's latency hides behind a whole step of VALU work
        // instead of stalling each step (round 6)
        unsigned vp = 0;
#pragma unroll
        for (int s = 0; s <= 8; s++) {
          unsigned vn = 0;
          // (the bottom-tile skip: the same wave-uniform condition on step s
          // here and on step s - 1 below, so what is issued is finished)
          if (s < 8 && (FB || SY(s) < live)) {
            const int oy = SY(s) * YR2 + SX(s);
            const int oh = SY(s) / 2 * HST + SX(s);
            H2S_MARK("S0 step: staged Y, vertical chroma");
            const float ybs = fmaf((float)ybase[oy], ysc, yoff);
            // x8 upsampled, centred, exact (SUB 3: 4 h[cy], or 2 (h[cy] + h[cy+1]))
            const float U = SUB == 3 ? 2.0f * (h0[oh] + h0[oh + hb]) : fmaf(3.0f, h0[oh], h0[oh + hb]);
            const float V = SUB == 3 ? 2.0f * (h1[oh] + h1[oh + hb]) : fmaf(3.0f, h1[oh], h1[oh + hb]);
            float r, gg, bl;
            lin_tone<TRC, TM, DESAT, LP, 0, FB>(F, cv, pq_lds, pqi_lds, K, ybs, U, V, [](float, float, float) {},
                                                 r, gg, bl, dv);
            H2S_MARK("S3 encode");
            vn = lp_table_read(F, K, lut8v, spread_lds, r, gg, bl, qo[s & 3]);
          }
          if (s > 0 && (FB || SY(s - 1) < live)) {
            const int sp = s - 1;
            const float R8 = (float)(vp & 255u), G8 = (float)((vp >> 8) & 255u), B8 = (float)((vp >> 16) & 255u);
            H2S_MARK("S5 Y'CbCr");
            const f3 o = lp_ycbcr(F, K, R8, G8, B8);
            H2S_MARK("S7 eq");
            // luma code (eq applied, shifted) replaces the luma sample this lane read
            ybase[SY(sp) * YR2 + SX(sp)] = eq_lds[(int)o.x];
            chroma_out(sp, o.y, o.z);
          }
          vp = vn;
        }
        return;
      }
      H2S_MARK("body: lut off");
    }
#pragma unroll
    for (int s = 0; s < 8; s++) {
      if (!FB && SX(s) == 0 && SY(s) >= live) break;   // (wave-uniform)
      const int oy = SY(s) * YR2 + SX(s);   // compile-time LDS offsets
      const int oh = SY(s) / 2 * HST + SX(s);
      H2S_MARK("S0 step: staged Y, vertical chroma");
      const float ybs = fmaf((float)ybase[oy], ysc, yoff);   // (the staged luma: Y*ys + y_off, +1 on PQ)
      float U, V;
      if constexpr (SUB == 1) {   // 4 h at the pixel's row: 8 c[k], or 4 (c[k] + c[k+1])
        const int oc = SY(s) * C422_ST + SX(s) / 2;
        U = 4.0f * (c0[oc] + c0[oc + pxl]), V = 4.0f * (c1[oc] + c1[oc + pxl]);
      } else if constexpr (SUB == 2) {   // 8 (code - mid)
        const int oc = SY(s) * C444_ST + SX(s);
        U = 8.0f * (float)s0[oc], V = 8.0f * (float)s1[oc];
      } else if constexpr (SUB == 3) {   // 4 h[cy] (even luma rows), or 2 (h[cy] + h[cy+1])
        U = 2.0f * (h0[oh] + h0[oh + hb]), V = 2.0f * (h1[oh] + h1[oh + hb]);
      } else {
        U = fmaf(3.0f, h0[oh], h0[oh + hb]);   // x8 upsampled, centred, exact
        V = fmaf(3.0f, h1[oh], h1[oh + hb]);
      }
      const long long di = DBG && g.f == 0 && g.py0 + yl + SY(s) < F.H
                               ? (long long)(g.py0 + yl + SY(s)) * F.dbg_w + g.px0 + xl + SX(s)
                               : -1;
      float oyv, ozv;
      // luma code (eq applied, shifted) replaces the luma sample this lane read
      ybase[oy] = (uint16_t)px_chain<TRC, TM, DESAT, LP, DBG, FB>(
          F, cv, pq_lds, pqi_lds, eq_lds, lut8v, spread_lds, lut, K, ybs, U, V, di, oyv, ozv, LP ? qo[s & 3] : 0.5f, ydq, dv);
      chroma_out(s, oyv, ozv);   // (BICUBIC: this pixel's Cb, Cr into the 4:4:4 scratch)
    }
  };
  auto mask_in = [&](uint4& a) {   // h2s_lp_p010 TRUNCATE (block-uniform)
    a.x &= F.in_mask2, a.y &= F.in_mask2, a.z &= F.in_mask2, a.w &= F.in_mask2;
  };
  auto shift_in = [&](uint4& a) { a.x >>= F.in_sh, a.y >>= F.in_sh, a.z >>= F.in_sh, a.w >>= F.in_sh; };

  const int pl = __builtin_amdgcn_readfirstlane(t >> 6) & 1, rem = t & 63;   // chroma store role (t < 128)
  const bool cst = t < 128 && !F.chr444;
  // ---- commit the loaded tile's registers to LDS (tile: its index) ----
  // The loop below is rotated: the first tile is committed ahead of it and
  // every later one at the loop's end, behind the previous tile's stores.
  // There the vector-memory operations in flight are, oldest first, this
  // tile's loads, then the two stores every thread has just issued (the store
  // rule, put_luma), so the compiler's counted waits for the loads leave the
  // stores outstanding: no wave waits for a write acknowledgement.  (With the
  // commit at the loop's top, the entry from the prologue, where no store
  // follows the loads, made the same waits drain the stores.)
  auto commit = [&](unsigned ti) {
    H2S_MARK("tile: commit");
    // ---- commit this tile's registers to LDS ----
    if constexpr (SEMI && S420) {
      if (!F.in_semi) cur.uh = halo_half(F, geo, t, cur.uh);   // (geo: the tile being committed)
    }
    if (F.in_mask2 != 0xFFFFFFFFu) {   // h2s_lp_p010 TRUNCATE, semi-planar words (block-uniform)
      // semi-planar: the code sits in each 16-bit word's high bits; both
      // halves of a pair move down together and the mask (always set then)
      // clears what crossed from the high half, and the word's low junk bits
      if constexpr (SEMI && S420) {
        if (F.in_sh) {
          shift_in(cur.ya), shift_in(cur.ua);
          cur.uh >>= F.in_sh;
        }
      }
      mask_in(cur.ya), mask_in(cur.ua);
      if constexpr (SUB == 2) mask_in(cur.va);
      else cur.uh &= F.in_mask2;
    }
    const float my = stage_luma(yin, cur.ya, t >> 3, t & 7, ysc, yoff);
    float mc = 0.0f;
    if constexpr (SUB == 1) {
      mc = stage_chroma422(hrow[__builtin_amdgcn_readfirstlane(t >> 7)], cur.ua, cur.uh, t & 127, cmid);
    } else if constexpr (SUB == 2) {
      mc = stage_chroma444(hrow[0], hrow[1], cur.ua, cur.va, t >> 3, t & 7, (int)F.c_mid);
    } else if (SEMI && F.in_semi) {   // block-uniform
      if (t < 144) mc = stage_chroma_semi<HST>(hrow[0], hrow[1], cur.ua, cur.uh, t, cmid);
    } else if ((t & 127) < 72) {
      mc = stage_chroma<HST>(hrow[__builtin_amdgcn_readfirstlane(t >> 7)], cur.ua, cur.uh, t & 127, cmid);
    }
    // every thread waits for its chroma registers here, with or without a
    // chunk to commit: none stays in flight into the next prefetch, where
    // reusing the register would wait for it behind the stores
    if constexpr (SUB == 2) asm volatile("" ::"v"(cur.ua.w), "v"(cur.va.w));
    else asm volatile("" ::"v"(cur.ua.w), "v"(cur.uh));
    if ((my > F.safe_y || mc > F.safe_c)) tflag[ti & 1u] = 1;
  };
  commit(tile);
  for (;;) {
    H2S_MARK("tile: prefetch");
    const int par = (int)(tile & 1u);
    const TileGeo g = geo;
    const bool more = tile + 1 < tend;   // block-uniform
    if (more) {
      tile_next(F, geo);
      cur = tile_load<SEMI, SUB>(F, geo, t, lofs);  // in flight during this tile's compute
    }
    __syncthreads();
    // (a product instance's bottom tile with rows past the frame: the
    // exact-capable body, which skips their steps -- the same output)
    const bool fb = __builtin_amdgcn_readfirstlane(tflag[par]) == 0 && !F.chr444 && !(DBG == 0 && g.py0 + TBH > F.H);
    if (t == 0) tflag[par ^ 1] = 0;   // for the next tile: read by every wave of the previous one before this barrier
    if (fb)
      steps(g, std::integral_constant<bool, true>{});
    else
      steps(g, std::integral_constant<bool, false>{});
    H2S_MARK("tile: store");
    __syncthreads();

    // ---- write the tile: 16-byte (u16) / 8-byte (u8) non-temporal stores ----
    put_luma(F, g, read_luma(F, yin, t >> 3, t & 7), t >> 3, lofs.sy, t);
    // the chroma store of every thread (the store rule above put_luma): the
    // threads with a chroma role read and quantise their chunk, the others
    // (and rows past the frame) store nothing at ST_DROP
    const bool osemi = SEMI && F.out_semi;   // block-uniform
    u4v cv{0u, 0u, 0u, 0u};
    int cvo = ST_DROP;
    if (cst) {
      const int cr = osemi ? t >> 3 : rem >> 2;
      cv = osemi ? read_chroma_semi(F, csum[0], cr, t & 7) : read_chroma(F, csum[0], pl, cr, rem & 3);
      if (g.cy0 + cr < F.ch) cvo = lofs.sc;
    }
    put_chroma(F, g, cv, osemi ? 0 : pl, osemi, cvo, t);
    if (!more) break;
    commit(++tile);
    // No barrier before that commit.  What it writes before the next tile's
    // barrier 1 is ordered without one, for every instance form: the luma slot
    // (row t >> 3, chunk t & 7) is the slot this same thread has just read in
    // read_luma (a wave's LDS operations execute in order); hrow (4:2:0 rows,
    // the SUB 1 / 2 windows, the semi-planar rows alike) was last read in the
    // steps, before barrier 2; tflag[par ^ 1] was zeroed by thread 0 before
    // barrier 2 and is read after the next barrier 1.  csum, and yin by other
    // threads, are next written in the next tile's steps, behind its barrier
    // 1, which no wave passes before every wave has issued the stores above,
    // i.e. has its store-phase reads of yin and csum back.  The libplacebo and
    // debug instances and the BICUBIC scratch path keep nothing else in LDS
    // across tiles
  }
}

}  // namespace h2s
