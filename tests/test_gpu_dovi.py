"""Dolby Vision profile 5 on the GPU (h2s_set_dovi): the tile kernel's
instances (k_tile<2, ...>, float32), the generic kernel's (the exact path), the
peak-statistics instance, and the plumbing around them.  Expected values:
tests/dovi_ref.py.

1. the HDR10 twin end to end against the C oracle on the same codes, through
   the suite's own gates as they stand (lp_gate 'k_tile' / 'generic',
   float_gate 'k_tile' / 'k_debug'), static and detected peak, LUT off,
   semi-planar, host frames;
2. per-frame records (integer reshape twins), three maps in one launch;
3. first-order MMR against its folded identity-reshape record;
4. the realistic full-order record against the float64 restatement;
5. routing, refusals and state.

Shapes: 128 x 64 (whole tiles), 144 x 64 (tiles and a tail), 48 x 32 (below one
tile); three frames each.
"""
import ctypes

import numpy as np
import pytest

import dovi_ref as DR
import hdr2sdr
import oracle
from hdr2sdr import _abi
from hdr2sdr.dovi import DoviCurve, DoviRpu
from hdr2sdr.frames import FrameBatch
from test_gpu_parity import assert_close_int, lattice

pytestmark = pytest.mark.gpu

NF = 3
SHAPES = [(128, 64), (144, 64), (48, 32)]
ROUTE = {(128, 64): _abi.PATH_TILE, (144, 64): _abi.PATH_TILE_TAIL, (48, 32): _abi.PATH_GENERIC}
LUT_N = 65
_CACHE = {}

CHAINS = {
    'bt2390_10': dict(tonemapper='bt.2390', bits_in=10, bits_out=10),
    'spline_8': dict(tonemapper='spline', bits_in=10, bits_out=8),
    'hable_lp_12': dict(tonemapper='hable', pipeline='libplacebo', desat=0.0, bits_in=12, bits_out=12, lp_p010='keep'),
}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope='module')
def tm():
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.set_dovi(None)
    t.close()


def configure(tm, params, dovi=None):
    tm.set_params(params)
    if params.lut_enabled:
        tm.set_lut(lattice(LUT_N))
    tm.set_dovi(dovi)


def gpu(tm, src, bits_out, out_layout='planar', device='cuda'):
    import torch
    if device == 'cpu':
        dst = FrameBatch.empty_numpy(src.nframes, src.width, src.height, bits_out, out_layout)
        tm.process(src, dst)
        return dst.buf.astype(np.int64) if out_layout == 'planar' else dst
    dst = FrameBatch.empty_torch(src.nframes, src.width, src.height, bits_out, 'cuda', out_layout)
    tm.process(src.to_torch('cuda'), dst)
    torch.cuda.synchronize()
    return dst.to_numpy().buf.astype(np.int64) if out_layout == 'planar' else dst.to_numpy()


def path(tm, src, bits_out):
    return tm.query_path(src.to_torch('cuda'), FrameBatch.empty_torch(src.nframes, src.width, src.height, bits_out, 'cuda'))


def on_generic(tm, fn):
    """fn() with H2S_OPT_FAST_PATH 0: the generic kernel whatever the shape."""
    tm.set_option(_abi.OPT_FAST_PATH, 0)
    try:
        return fn()
    finally:
        tm.set_option(_abi.OPT_FAST_PATH, 1)


def twin(W, H, bits):
    return cached(('twin', W, H, bits), lambda: DR.twin_source(W, H, bits, NF))


def oracle_out(params, fb):
    return cached(('oracle', repr(params), fb.width, fb.height, fb.bits, id(fb)),
                  lambda: oracle.process(oracle.params_from(params.to_c()), lattice(LUT_N) if params.lut_enabled else None,
                                         fb.buf, fb.width, fb.height).astype(np.int64))


# ---- 1: the HDR10 twin ----------------------------------------------------------------------------
@pytest.mark.parametrize('wh', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('chain', sorted(CHAINS))
def test_hdr10_twin_matches_the_oracle(tm, chain, wh):
    """A frame under hdr10_equivalent against oracle.process on the same codes
    as plain HDR10: 0 unattributed samples, the attributed ones within k8
    (tests/lp_gate.py through assert_close_int, unchanged)."""
    W, H = wh
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    fb = twin(W, H, params.bits_in)
    configure(tm, params, DoviRpu.hdr10_equivalent(params.bits_in))
    assert path(tm, fb, params.bits_out) == ROUTE[wh]
    got = gpu(tm, fb, params.bits_out)
    want = oracle_out(params, fb)
    d = np.abs(got - want)
    print(f'DOVI-TWIN {chain} {W}x{H} path={ROUTE[wh]} max={int(d.max())} differ={float((d > 0).mean()):.4%}')
    assert_close_int(params, got, want, W, H, fb.buf, lut_n=LUT_N,
                     kernel='generic' if ROUTE[wh] == _abi.PATH_GENERIC else 'k_tile')
    if ROUTE[wh] != _abi.PATH_GENERIC:     # the same frames on the generic kernel alone
        assert on_generic(tm, lambda: path(tm, fb, params.bits_out)) == _abi.PATH_GENERIC
        gen = on_generic(tm, lambda: gpu(tm, fb, params.bits_out))
        d = np.abs(gen - want)
        print(f'DOVI-TWIN {chain} {W}x{H} generic max={int(d.max())} differ={float((d > 0).mean()):.4%}')
        assert_close_int(params, gen, want, W, H, fb.buf, lut_n=LUT_N, kernel='generic')
    # the record is what made it so: as IPT-PQ-c2 codes read by the identity record it is another picture
    tm.set_dovi(DoviRpu.identity(params.bits_in))
    assert (np.abs(gpu(tm, fb, params.bits_out) - want) > 1).mean() > 0.2


@pytest.mark.parametrize('stage', [1, 2, 3])
@pytest.mark.parametrize('kernel', ['k_tile', 'k_debug'])
@pytest.mark.parametrize('chain', ['bt2390_10', 'hable_lp_12', 'spline_8'])
def test_twin_debug_planes_pass_the_float_gate(tm, chain, kernel, stage):
    """The tile kernel's own Dolby Vision arithmetic (its debug instance, on
    the tile path) and the generic kernel's, through the unchanged float gate."""
    from float_gate import Planes, float_tolerance, judge_float
    W, H = 128, 64
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    fb = twin(W, H, params.bits_in)
    configure(tm, params, DoviRpu.hdr10_equivalent(params.bits_in))
    run = lambda: (path(tm, fb, params.bits_out), tm.debug_float(fb.to_torch('cuda'), stage))   # noqa: E731
    p, got = run() if kernel == 'k_tile' else on_generic(tm, run)
    assert p == (_abi.PATH_TILE if kernel == 'k_tile' else _abi.PATH_GENERIC)
    T = float_tolerance(params, kernel, stage, 'smooth', Planes(params, fb.buf, W, H, lut_n=LUT_N))
    report, fails = judge_float(params, kernel, 'smooth', stage, got, T)
    print(f'DOVI-FLOAT {chain} {kernel} stage {stage} max_rel={report["max_rel_err_rest"]:.3g}')
    assert not fails, '; '.join(fails)


@pytest.mark.parametrize('wh', [(128, 64), (48, 32)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('tmname', ['bt.2390', 'spline'])
def test_twin_with_peak_detect_matches_the_dynamic_oracle(tm, tmname, wh):
    """peak_detect = 1 on the device (the statistics kernel's Dolby Vision
    instance, the IIR, the per-frame curves): against oracle.process_dynamic
    with its knees, and h2s_peak_stats at test_peak_detect's tolerance."""
    W, H = wh
    params = hdr2sdr.TonemapParams(tonemapper=tmname, peak_detect=True, maxcll=4000.0)
    fb = twin(W, H, 10)
    configure(tm, params, DoviRpu.hdr10_equivalent(10))
    tm.reset_peak()
    got = gpu(tm, fb, 10)
    state = tm.peak_state()
    knees = []
    want, peaks = oracle.process_dynamic(oracle.params_from(params.to_c()), lattice(LUT_N), fb.buf, W, H, knees=knees)
    assert state['frames'] == NF and state['peak'] == pytest.approx(peaks[-1], rel=1e-4)
    assert path(tm, fb, 10) == ROUTE[wh]
    assert_close_int(params, got, want.astype(np.int64), W, H, fb.buf, lut_n=LUT_N,
                     kernel='generic' if ROUTE[wh] == _abi.PATH_GENERIC else 'k_tile', knees=knees)
    fmax, favg = tm.peak_stats(fb.to_torch('cuda'))
    mx, avg = oracle.peak_stats(oracle.params_from(params.to_c()), fb.buf, W, H)
    print(f'DOVI-STATS {tmname} {W}x{H} max rel {np.abs(fmax / mx - 1).max():.3g} avg rel {np.abs(favg / avg - 1).max():.3g}')
    np.testing.assert_allclose(fmax, mx, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(favg, avg, rtol=1e-5, atol=1e-6)


def test_twin_lut_off_semi_planar_and_host_frames(tm):
    W, H = 144, 64
    # LUT off (libplacebo's own BT.709 conversion, nv12 depth)
    params = hdr2sdr.TonemapParams(tonemapper='bt.2390', bits_out=8, lut_enabled=False)
    fb = twin(W, H, 10)
    configure(tm, params, DoviRpu.hdr10_equivalent(10))
    assert_close_int(params, gpu(tm, fb, 8), oracle_out(params, fb), W, H, fb.buf)
    # semi-planar in and out, and host frames (the chunk pipeline: NF > 1): the planar device bytes
    params = hdr2sdr.TonemapParams(**CHAINS['bt2390_10'])
    configure(tm, params, DoviRpu.hdr10_equivalent(10))
    want = gpu(tm, fb, 10)
    semi = gpu(tm, fb.to_layout('semi'), 10, out_layout='semi')
    assert np.array_equal(semi.to_layout('planar').buf.astype(np.int64), want)
    assert np.array_equal(gpu(tm, fb, 10, device='cpu'), want)


# ---- 2: per-frame records ---------------------------------------------------------------------------
# (tiles per block is the tile kernel's; 48 x 32 has the generic route only)
RECORD_CASES = [(wh, 'tile', tpb) for wh in SHAPES for tpb in (1, 8)] + [(wh, 'generic', 8) for wh in SHAPES[:2]]


@pytest.mark.parametrize('wh,route,tpb', RECORD_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_per_frame_records_match_their_twins(tm, wh, route, tpb):
    """Three luma maps in one launch: frame f under record f against the oracle
    on the mapped frame f (the HDR10 twin of the mapped codes), and against the
    library's own output for (mapped frames, the twin's record)."""
    W, H = wh
    params = hdr2sdr.TonemapParams(**CHAINS['bt2390_10'])
    src, recs, mapped = cached(('maps', W, H), lambda: DR.luma_map_pair(W, H, 10, NF))
    tm.set_option(_abi.OPT_TILES_PER_BLOCK, tpb)
    tm.set_option(_abi.OPT_FAST_PATH, 0 if route == 'generic' else 1)
    try:
        configure(tm, params, recs)
        # (128 x 64: 2 x 2 tiles per frame, so a block of 8 walks across both frame boundaries)
        assert path(tm, src, 10) == (_abi.PATH_GENERIC if route == 'generic' else ROUTE[wh])
        got = gpu(tm, src, 10)
        host = gpu(tm, src, 10, device='cpu')                # record indices count frames of the call, not of the chunk
        tm.set_dovi([recs[1], recs[0], recs[2]])
        swapped = gpu(tm, src, 10)
        tm.set_dovi(DoviRpu.hdr10_equivalent(10))
        own = gpu(tm, mapped, 10)
    finally:
        tm.set_option(_abi.OPT_TILES_PER_BLOCK, 8)
        tm.set_option(_abi.OPT_FAST_PATH, 1)
    want = oracle_out(params, mapped)
    tile = route == 'tile' and ROUTE[wh] != _abi.PATH_GENERIC
    assert_close_int(params, got, want, W, H, mapped.buf, lut_n=LUT_N, kernel='k_tile' if tile else 'generic')
    d = np.abs(got - own)
    print(f'DOVI-MAPS {W}x{H} {route} tpb={tpb} vs own twin: max={int(d.max())} differ={float((d > 0).mean()):.4%}')
    # a float32 a0 = k / (2^b - 1) moves a code's fraction by <= 2^-25 (exact path); the tile kernel's float32
    # reshape adds an ulp of the fraction: the agreement of two float32 forms of this branch
    assert (d > 0).mean() <= 1e-3 and (d <= 1).mean() >= 0.999
    assert np.array_equal(host, got)
    # swapping two records changes the frames they belong to, and only those
    assert (np.abs(swapped[:2] - want[:2]) > 1).mean() > 0.2 and np.array_equal(swapped[2], got[2])


# ---- 3: first-order MMR ---------------------------------------------------------------------------------
@pytest.mark.parametrize('wh', [(128, 64), (144, 64), (48, 32)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_first_order_mmr_equals_its_folded_record(tm, wh):
    """Chroma MMRs of order 1 (luma a polynomial: the shape the tile kernel
    takes) against the folded identity-reshape record, on the tile route and on
    the generic one, and the two routes against each other: equal within one
    step on >= 99.9 % of samples, the rest within k8."""
    import lp_gate
    W, H = wh
    params = hdr2sdr.TonemapParams(**CHAINS['bt2390_10'])
    fb = cached(('mmrsrc', W, H), lambda: DR.pull_in(DR.twin_source(W, H, 10, NF), (0.1, 0.9), 0.8))
    mmr, folded = DR.mmr_affine_pair(10, luma_mmr=False)
    assert DR.no_clamp_acts(fb, mmr) and DR.no_clamp_acts(fb, folded)
    out = {}
    for name, rec in (('mmr', mmr), ('folded', folded)):
        configure(tm, params, rec)
        assert path(tm, fb, 10) == ROUTE[wh]
        out[name, 'tile'] = gpu(tm, fb, 10)
        out[name, 'generic'] = on_generic(tm, lambda: gpu(tm, fb, 10))
    ref = out['mmr', 'generic']
    k8 = lp_gate.attribute(params, 'generic', ref, ref, fb.buf, W, H, LUT_N)['k8_bound_out_steps']
    pairs = [(('mmr', 'tile'), ('folded', 'tile')), (('mmr', 'generic'), ('folded', 'generic')),
             (('mmr', 'tile'), ('mmr', 'generic'))]
    for x, y in pairs:
        d = np.abs(out[x] - out[y])
        print(f'DOVI-MMR1 {W}x{H} {x} vs {y}: max={int(d.max())} beyond one step={float((d > 1).mean()):.4%}')
        assert (d <= 1).mean() >= 0.999 and d.max() <= k8
    # a luma MMR is no shape of the tile kernel's: the generic kernel, and the same agreement
    full, ffold = DR.mmr_affine_pair(10)
    configure(tm, params, full)
    assert path(tm, fb, 10) == _abi.PATH_GENERIC
    a = gpu(tm, fb, 10)
    tm.set_dovi(ffold)
    d = np.abs(a - gpu(tm, fb, 10))
    assert (d <= 1).mean() >= 0.999 and d.max() <= k8


# ---- 4: the full-order record ---------------------------------------------------------------------------
def stage1_tolerance(fb, rec, npl=100.0):
    """1e-3 relative plus ipt_cond.stage1_uncertainty of the restated LMS
    carried through |Lm|, per channel [3, H, W] (units of npl)."""
    from ipt_cond import stage1_uncertainty
    _, lms = DR.dovi_lms(fb.y[0], fb.u[0], fb.v[0], fb.bits, rec)
    want = DR.dovi_linear(fb.y[0], fb.u[0], fb.v[0], fb.bits, rec) / npl
    U = stage1_uncertainty(np.moveaxis(lms / npl, -1, 0), npl, 'smpte2084')
    U = np.einsum('ck,khw->chw', np.abs(DR.c_arrays(rec)['lin']), U)
    want = np.moveaxis(want, -1, 0)
    return want, 1e-3 * np.abs(want) + U


@pytest.mark.parametrize('kernel', ['k_tile', 'k_debug'])
@pytest.mark.parametrize('bits', [10, 12])
def test_full_order_record_stage1_matches_the_restatement(tm, bits, kernel):
    W, H = 144, 64
    params = hdr2sdr.TonemapParams(tonemapper='bt.2390', bits_in=bits, bits_out=10, lp_p010='keep')
    fb = cached(('smooth', W, H, bits),
                lambda: hdr2sdr.synth.synth_frames('smooth', NF, W, H, bits, device='cpu', seed=13).to_numpy())
    rec = DR.realistic_record(bits)
    configure(tm, params, rec)
    run = lambda: tm.debug_float(fb.to_torch('cuda'), 1).astype(np.float64)   # noqa: E731
    got = run() if kernel == 'k_tile' else on_generic(tm, run)      # (144 wide: tile columns and the tail's)
    want, tol = stage1_tolerance(fb, rec)
    err = np.abs(got - want)
    print(f'DOVI-FULL stage 1 bits {bits} {kernel}: max err / tol {float((err / np.maximum(tol, 1e-300)).max()):.3g}')
    assert (err <= tol).all()


@pytest.mark.parametrize('route', ['k_tile', 'generic', 'lp_exact'])
@pytest.mark.parametrize('form', ['ipt', 'max-rgb'])
def test_full_order_record_output_matches_the_restatement(tm, form, route):
    """Integer output against the float64 restatement under the bounds
    test_independent_libplacebo_branch_matches_oracle sets for two evaluations
    of this branch: max <= 8 x 2^(bits_out - 8), share of differing samples <=
    1e-2 (profiles/dovi/parity.md has the measured values)."""
    W, H = 144, 64
    params = hdr2sdr.TonemapParams(tonemapper='bt.2390', bits_out=10, lp_tone=form)
    fb = cached(('smooth', W, H, 10),
                lambda: hdr2sdr.synth.synth_frames('smooth', NF, W, H, 10, device='cpu', seed=13).to_numpy())
    rec = DR.realistic_record(10)
    configure(tm, params, rec)
    tm.set_option(_abi.OPT_LP_EXACT, 1 if route == 'lp_exact' else 0)
    tm.set_option(_abi.OPT_FAST_PATH, 0 if route == 'generic' else 1)
    try:
        assert path(tm, fb, 10) == (_abi.PATH_TILE_TAIL if route == 'k_tile' else _abi.PATH_GENERIC)
        got = gpu(tm, fb, 10)
    finally:
        tm.set_option(_abi.OPT_LP_EXACT, 0)
        tm.set_option(_abi.OPT_FAST_PATH, 1)
    want = cached(('restated', form), lambda: DR.restated(fb, rec, 10, LUT_N, ipt=form == 'ipt'))
    d = np.abs(got - want)
    print(f'DOVI-FULL {form} {route}: max={int(d.max())} differ={float((d > 0).mean()):.4%}')
    assert d.max() <= 8 * 4 and (d > 0).mean() <= 1e-2


def test_p010_truncation_applies_to_the_codes_first(tm):
    """12-bit input through the default format=p010 upload: the front-end
    reads the codes with their two low bits dropped, as the branch's S1 does."""
    W, H = 48, 32
    params = hdr2sdr.TonemapParams(tonemapper='bt.2390', bits_in=12, bits_out=10)      # lp_p010 'truncate'
    fb = hdr2sdr.synth.synth_frames('smooth', NF, W, H, 12, device='cpu', seed=13).to_numpy()
    assert (fb.buf & 3).any()
    rec = DR.realistic_record(12)
    configure(tm, params, rec)
    got = gpu(tm, fb, 10)
    d = np.abs(got - DR.restated(fb, rec, 10, LUT_N, mask=0xFFFC))
    assert d.max() <= 8 * 4 and (d > 0).mean() <= 1e-2
    cut = hdr2sdr.FrameBatch(fb.buf & 0xFFFC, W, H, 12)
    assert np.array_equal(gpu(tm, cut, 10), got)
    tm.set_params(params.with_(lp_p010='keep'))
    assert not np.array_equal(gpu(tm, fb, 10), got)


# ---- 5: routing, refusals and state -----------------------------------------------------------------------
def test_routing_of_records_the_tile_kernel_would_not_take(tm):
    """Two-piece chroma and a luma MMR report H2S_PATH_GENERIC and match the restatement."""
    W, H = 128, 64
    params = hdr2sdr.TonemapParams(**CHAINS['bt2390_10'])
    fb = twin(W, H, 10)
    base = DR.realistic_record(10)
    two_piece = base.with_(comp=(base.comp[0], DoviCurve.polynomial((0.0, 0.5, 1.0), [(0.0, 1.0), (0.02, 0.96)]),
                                 base.comp[2]))
    luma_mmr = base.with_(comp=(DoviCurve.mmr_single(0.01, [[0.97, 0.01, -0.01, 0.02, 0, 0, 0], [0.02, 0, 0, 0, 0, 0, 0]]),
                                base.comp[1], base.comp[2]))
    configure(tm, params, base)                      # the shape profile 5 carries: the tile kernel
    assert path(tm, fb, 10) == _abi.PATH_TILE
    tm.set_dovi([base, two_piece, base])             # one record of another shape sends the launch to the generic kernel
    assert path(tm, fb, 10) == _abi.PATH_GENERIC
    for name, rec in (('two_piece', two_piece), ('luma_mmr', luma_mmr)):
        configure(tm, params, rec)
        assert path(tm, fb, 10) == _abi.PATH_GENERIC
        d = np.abs(gpu(tm, fb, 10) - DR.restated(fb, rec, 10, LUT_N))
        print(f'DOVI-ROUTE {name}: max={int(d.max())} differ={float((d > 0).mean()):.4%}')
        assert d.max() <= 8 * 4 and (d > 0).mean() <= 1e-2


def test_refusals_and_off_state(tm):
    import torch
    W, H = 128, 64
    params = hdr2sdr.TonemapParams(**CHAINS['bt2390_10'])
    fb = twin(W, H, 10)
    src = fb.to_torch('cuda')
    dst = FrameBatch.empty_torch(NF, W, H, 10, 'cuda')
    configure(tm, params)
    before = gpu(tm, fb, 10)
    p_before = path(tm, fb, 10)
    assert p_before == _abi.PATH_TILE
    L = tm._L
    di, do = src.descriptor(), dst.descriptor()
    rec = DoviRpu.hdr10_equivalent(10)

    # nframes > n (n > 1); n == 1 serves any count
    tm.set_dovi([rec, rec])
    assert L.h2s_process(tm._ctx, ctypes.byref(di), ctypes.byref(do), 3, None) == _abi.H2S_E_INVALID_ARG
    assert b'Dolby Vision' in L.h2s_last_error(tm._ctx)
    assert L.h2s_process(tm._ctx, ctypes.byref(di), ctypes.byref(do), 2, None) == 0
    fmax, favg = np.zeros(3), np.zeros(3)
    assert L.h2s_peak_stats(tm._ctx, ctypes.byref(di), 3, fmax.ctypes.data, favg.ctypes.data, None) == \
        _abi.H2S_E_INVALID_ARG
    with pytest.raises(ValueError):
        tm.process(src, dst)

    # the CPU pipeline, explicit or resolved from AUTO
    tm.set_dovi(rec)
    for kw in (dict(tonemapper='bt.2390', pipeline='cpu'), dict(tonemapper='mobius')):
        tm.set_params(hdr2sdr.TonemapParams(**kw))
        assert L.h2s_process(tm._ctx, ctypes.byref(di), ctypes.byref(do), 3, None) == _abi.H2S_E_UNSUPPORTED
        assert L.h2s_query_path(tm._ctx, ctypes.byref(di), ctypes.byref(do)) == _abi.H2S_E_UNSUPPORTED
        out = np.empty((3, H, W), np.float32)
        assert L.h2s_debug_float(tm._ctx, ctypes.byref(di), 1, out.ctypes.data, _abi.LOC_HOST, None) == \
            _abi.H2S_E_UNSUPPORTED
    # top-left chroma
    tm.set_params(params)
    tl = FrameBatch(src.buf, W, H, 10, 'planar', '420', 'tv', 'topleft')
    with pytest.raises(ValueError, match='top-left'):
        tm.process(tl, dst)
    # 4:2:2 input stays the branch's own refusal
    s422 = FrameBatch.empty_torch(NF, W, H, 10, 'cuda', 'planar', '422')
    with pytest.raises(ValueError, match='4:2:2'):
        tm.process(s422, dst)
    # transfer_in is ignored
    tm.set_params(params)
    a = gpu(tm, fb, 10)
    tm.set_params(params.with_(transfer='arib-std-b67'))
    assert np.array_equal(gpu(tm, fb, 10), a)
    # an invalid record leaves the set as it was; off restores the HDR10 bytes and the route
    tm.set_params(params)
    bad = rec.to_c()
    bad.comp[0].num_pivots = 1
    assert L.h2s_set_dovi(tm._ctx, ctypes.byref(bad), 1) == _abi.H2S_E_INVALID_ARG
    assert np.array_equal(gpu(tm, fb, 10), a)
    tm.set_dovi(None)
    assert tm.dovi_records == 0 and path(tm, fb, 10) == p_before
    assert np.array_equal(gpu(tm, fb, 10), before)
    torch.cuda.synchronize()


def test_previewer_takes_records(tm):
    """The converted pane honours the records frame by frame (each preview
    frame from a fresh peak state); the source pane ignores them."""
    W, H = 128, 64
    src, recs, mapped = cached(('maps', W, H), lambda: DR.luma_map_pair(W, H, 10, NF))
    with hdr2sdr.Previewer(0, 'mobius', lattice=lattice(LUT_N), dovi=recs) as pv:
        assert pv.params.pipeline == 'libplacebo' and pv.params.peak_detect      # libplacebo, GPU toggle or not
        got = pv.convert_batch(src.to_torch('cuda'), 'iw', 'ih')
        orig = pv.original_batch(src.to_torch('cuda'), 'iw', 'ih')
        pv.set_dovi([recs[1], recs[0], recs[2]])
        swapped = pv.convert_batch(src.to_torch('cuda'), 'iw', 'ih')
        pv.set_dovi(DoviRpu.hdr10_equivalent(10))
        want = pv.convert_batch(mapped.to_torch('cuda'), 'iw', 'ih')
        pv.set_dovi(None)
        plain = pv.original_batch(src.to_torch('cuda'), 'iw', 'ih')
    for f in range(NF):
        d = np.abs(got[f].astype(np.int64) - want[f].astype(np.int64))
        assert (d > 2).mean() <= 1e-3, f       # (a one-step Y'CbCr flip is up to two RGB steps)
    assert (np.abs(swapped[0].astype(np.int64) - got[0].astype(np.int64)) > 2).mean() > 0.05
    assert np.array_equal(swapped[2], got[2])
    assert all(np.array_equal(a, b) for a, b in zip(orig, plain))


def test_planned_profile5_conversion_runs_end_to_end(tmp_path):
    """plan_from_argv(argv, props, dovi=...) -> decode pipe -> libh2s -> encode
    pipe where it raised before: the bytes are the twin's (oracle, dynamic peak)."""
    from test_dovi import p5_case
    from test_plan import _fake_pipes
    from hdr2sdr import plan as P
    W, H, N = 128, 64, 5
    argv, props = p5_case()
    src, recs, mapped = DR.luma_map_pair(W, H, 10, N)
    pl = P.plan_from_argv(argv, dict(props, width=W, height=H), hdr={'maxcll': 1000.0},
                          dovi=lambda first, count: recs[first:first + count])
    out = _fake_pipes(pl, tmp_path, src.buf)
    proc = P.start(pl, device=0, batch=2)
    list(proc.stderr)
    assert proc.wait(timeout=120) == 0 and proc.error is None and proc.frames == N
    got = np.fromfile(out, dtype=np.uint16).reshape(N, -1).astype(np.int64)
    knees = []
    want = oracle.process_dynamic(oracle.params_from(pl.params.to_c()), lattice(LUT_N), mapped.buf, W, H,
                                  knees=knees)[0].astype(np.int64)
    assert_close_int(pl.params, got, want, W, H, mapped.buf, lut_n=LUT_N, kernel='generic', knees=knees)
