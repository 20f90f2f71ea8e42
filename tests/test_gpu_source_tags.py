"""A source's full-range and top-left chroma tags on the GPU
(h2s_set_input_tags): the tile kernel's top-left instances of both chains, the
generic kernel's taps, the full-range constants and the fast body's bound, and
the plumbing around them.  Expected values: tests/source_tags_ref.py.

1. top-left == the library's own 4:2:2 path on the paired plane (CPU chain);
2. vertical ramps against the C oracle on the quarter-row twin, both chains,
   edge rows left out;
3. full-range grey steps against the C oracle on the limited twin: integer
   output, debug planes, peak statistics;
4. arbitrary content against the float64 restatement: <= 2 quantiser steps,
   <= 1 % of samples (test_arbitrary_chroma_matches_the_restatement's bounds);
5. the tag is honoured, the exact path is reached, other paths and forms,
   refusals and state.
"""
import ctypes

import numpy as np
import pytest

import hdr2sdr
import oracle
import source_tags_ref as TR
from hdr2sdr import _abi
from hdr2sdr.frames import FrameBatch
from hdr2sdr.synth import synth_frames
from test_gpu_parity import assert_close_int
from test_gpu_subsampling import B_CHAINS, SIZES, SOME, lat, LUT_N

pytestmark = pytest.mark.gpu

NF = 2
CHAINS = {
    'c2_hable_g22': dict(tonemapper='hable', gamma=2.2, bits_out=10),
    'mobius_hlg12': dict(tonemapper='mobius', bits_in=12, bits_out=12, transfer='arib-std-b67'),
    'reinhard_8': dict(tonemapper='reinhard', bits_out=8),
    'hable_pq12': dict(tonemapper='hable', bits_in=12, bits_out=10),
    # the libplacebo branch (bt.2390 and spline resolve to it; lp_tone IPT is its default)
    'bt2390_ipt': dict(tonemapper='bt.2390', lp_tone='ipt', bits_out=10),
    'spline': dict(tonemapper='spline', bits_out=10),
    # (lp_p010 keep: the format=p010 truncation would drop the low bits of the constructions' 12-bit codes)
    'bt2390_pq12': dict(tonemapper='bt.2390', bits_in=12, bits_out=10, lp_p010='keep'),
}
LP = ('bt2390_ipt', 'spline', 'bt2390_pq12')
_CACHE = {}


@pytest.fixture(scope='module')
def tm():
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.close()


def configure(tm, params):
    tm.set_params(params)
    if params.lut_enabled:
        tm.set_lut(lat())


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def oracle_out(params, fb):
    return cached(('oracle', repr(params), id(fb)),
                  lambda: oracle.process(oracle.params_from(params.to_c()), lat() if params.lut_enabled else None, fb.buf,
                                         fb.width, fb.height).astype(np.int64))


def gpu(tm, src, bits_out, out_layout='planar'):
    import torch
    dst = FrameBatch.empty_torch(src.nframes, src.width, src.height, bits_out, 'cuda', out_layout)
    tm.process(src.to_torch('cuda'), dst)
    torch.cuda.synchronize()
    return dst.to_numpy()


def paths(tm, src, bits_out):
    dst = FrameBatch.empty_torch(src.nframes, src.width, src.height, bits_out, 'cuda')
    return tm.query_path(src.to_torch('cuda'), dst)


def generic(tm, src, bits_out):
    """The run on the generic kernel (H2S_OPT_FAST_PATH 0)."""
    tm.set_option(_abi.OPT_FAST_PATH, 0)
    try:
        assert paths(tm, src, bits_out) in (_abi.PATH_GENERIC, _abi.PATH_TWO_PASS)
        return gpu(tm, src, bits_out)
    finally:
        tm.set_option(_abi.OPT_FAST_PATH, 1)


def even_source(kind, W, H, bits):
    """A 4:2:0 batch with even chroma codes, computed once."""
    return cached(('even', kind, W, H, bits),
                  lambda: TR.round2(synth_frames(kind, NF, W, H, bits, device='cpu', seed=11).to_numpy()))


def ramps(W, H, bits):
    return cached(('ramps', W, H, bits),
                  lambda: TR.ramp_pair(synth_frames('smooth', NF, W, H, bits, device='cpu', seed=13).to_numpy(),
                                       seed=W * 1000 + H))


def greys(W, H, bits, nframes=3):
    return cached(('greys', W, H, bits, nframes), lambda: TR.grey_steps(nframes, W, H, bits))


# ---- 1: top-left == the 4:2:2 path ------------------------------------------------
TL422 = ([('c2_hable_g22', wh, k) for wh in SIZES for k in ('uniform', 'smooth', 'edges')] +
         [(c, wh, 'uniform') for c in ('mobius_hlg12', 'reinhard_8') for wh in SOME])


@pytest.mark.parametrize('chain,wh,kind', TL422, ids=lambda v: str(v).replace(' ', ''))
def test_topleft_equals_the_422_path_on_the_paired_plane(tm, chain, wh, kind):
    W, H = wh
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    fb = even_source(kind, W, H, params.bits_in)
    configure(tm, params)
    src = TR.tagged(fb, 'tv', 'topleft')
    path = paths(tm, src, params.bits_out)
    assert path == SIZES[wh]
    got = gpu(tm, src, params.bits_out).buf.astype(np.int64)
    want = gpu(tm, TR.as_422(fb), params.bits_out).buf.astype(np.int64)
    d = np.abs(got - want)
    print(f'TAGS-422 {chain} {W}x{H} {kind} path={path} max={int(d.max())} differ={float((d > 0).mean()):.4%}')
    if path == _abi.PATH_TILE:
        assert np.array_equal(got, want)          # the staged values are the same exact integers
    else:   # (the 4:2:0 and 4:2:2 generic forms round a blend differently in the last bit)
        assert_close_int(params, got, want, W, H, fb.buf, lut_n=LUT_N)


@pytest.mark.parametrize('H', [32, 34])
@pytest.mark.parametrize('edge', ['zimg', 'replicate', 'mirror'])
def test_chroma_edge_rules_at_the_bottom_row(tm, edge, H):
    W = 64
    params = hdr2sdr.TonemapParams(chroma_edge=edge, **CHAINS['c2_hable_g22'])
    fb = even_source('uniform', W, H, 10)
    configure(tm, params)
    src = TR.tagged(fb, 'tv', 'topleft')
    assert paths(tm, src, 10) == _abi.PATH_TILE
    want = gpu(tm, TR.as_422(fb, edge), 10).buf.astype(np.int64)
    assert np.array_equal(gpu(tm, src, 10).buf.astype(np.int64), want)
    assert_close_int(params, generic(tm, src, 10).buf.astype(np.int64), want, W, H, fb.buf, lut_n=LUT_N)


@pytest.mark.parametrize('wh', [(64, 32), (70, 34)])
def test_bicubic_output_chroma_two_pass(tm, wh):
    W, H = wh
    params = hdr2sdr.TonemapParams(chroma_filter='bicubic', **CHAINS['c2_hable_g22'])
    fb = even_source('smooth', W, H, 10)
    configure(tm, params)
    src = TR.tagged(fb, 'tv', 'topleft')
    assert paths(tm, src, 10) == (_abi.PATH_TILE if wh == (64, 32) else _abi.PATH_TWO_PASS)
    got = gpu(tm, src, 10).buf.astype(np.int64)
    want = gpu(tm, TR.as_422(fb), 10).buf.astype(np.int64)
    assert_close_int(params, got, want, W, H, fb.buf, lut_n=LUT_N)
    assert not np.array_equal(got, gpu(tm, fb, 10).buf.astype(np.int64))


# ---- 2: vertical ramps against the oracle -------------------------------------------
RAMP_CASES = ([(c, wh, 'tile') for c in ('c2_hable_g22', 'bt2390_ipt', 'spline') for wh in SIZES] +
              [(c, wh, 'lp_exact') for c in ('bt2390_ipt', 'spline') for wh in SOME] +
              [(c, wh, 'tile') for c in ('hable_pq12', 'bt2390_pq12') for wh in [(192, 70), (208, 64)]])


@pytest.mark.parametrize('chain,wh,route', RAMP_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_vertical_ramps_match_the_oracle_on_the_quarter_row_twin(tm, chain, wh, route):
    W, H = wh
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    src, twin = ramps(W, H, params.bits_in)
    configure(tm, params)
    tm.set_option(_abi.OPT_LP_EXACT, 1 if route == 'lp_exact' else 0)
    try:
        path = paths(tm, src, params.bits_out)
        assert path == (_abi.PATH_GENERIC if route == 'lp_exact' else SIZES[wh])
        got = gpu(tm, src, params.bits_out).buf.astype(np.int64)
    finally:
        tm.set_option(_abi.OPT_LP_EXACT, 0)
    want = oracle_out(params, twin)
    kept = TR.without_edge_rows(got, want, W, H)
    d = np.abs(kept - want)
    print(f'TAGS-RAMP {chain} {W}x{H} {route} path={path} max={int(d.max())} differ={float((d > 0).mean()):.4%}')
    assert_close_int(params, kept, want, W, H, twin.buf, lut_n=LUT_N, kernel='exact' if route == 'lp_exact' else 'k_tile')
    # and the tag did something: the same samples read left-sited are another picture
    assert not np.array_equal(got, gpu(tm, TR.tagged(src), params.bits_out).buf.astype(np.int64))


# ---- 3: full-range grey steps against the oracle ---------------------------------------
GREY_CASES = [(c, wh) for c in ('c2_hable_g22', 'bt2390_ipt', 'spline') for wh in SOME + [(70, 34)]] + \
             [(c, wh) for c in ('hable_pq12', 'mobius_hlg12', 'bt2390_pq12') for wh in [(192, 70), (208, 64)]]


@pytest.mark.parametrize('chain,wh', GREY_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_full_range_grey_steps_match_the_oracle_on_the_limited_twin(tm, chain, wh):
    W, H = wh
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    full, twin = greys(W, H, params.bits_in)
    configure(tm, params)
    assert paths(tm, full, params.bits_out) == SIZES[wh]
    got = gpu(tm, full, params.bits_out).buf.astype(np.int64)
    want = oracle_out(params, twin)
    d = np.abs(got - want)
    print(f'TAGS-GREY {chain} {W}x{H} max={int(d.max())} differ={float((d > 0).mean()):.4%}')
    assert_close_int(params, got, want, W, H, twin.buf, lut_n=LUT_N)
    assert_close_int(params, generic(tm, full, params.bits_out).buf.astype(np.int64), want, W, H, twin.buf, lut_n=LUT_N,
                     kernel='exact')
    assert not np.array_equal(got, gpu(tm, TR.tagged(full), params.bits_out).buf.astype(np.int64))


@pytest.mark.parametrize('stage', [1, 5])
@pytest.mark.parametrize('kernel', ['k_tile', 'k_debug'])
@pytest.mark.parametrize('chain', ['c2_hable_g22', 'bt2390_ipt'])
def test_debug_planes_of_a_full_range_set(tm, chain, kernel, stage):
    """A full-range set keeps the tile kernel's debug instances (constants
    only); both kernels' planes against the oracle's planes of the limited
    twin, through the suite's float gate as it stands."""
    from float_gate import Planes, float_tolerance, judge_float
    W, H = 64, 32
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    full, twin = greys(W, H, params.bits_in, 1)
    configure(tm, params)
    tm.set_option(_abi.OPT_FAST_PATH, 1 if kernel == 'k_tile' else 0)
    try:
        assert paths(tm, full, params.bits_out) == (_abi.PATH_TILE if kernel == 'k_tile' else _abi.PATH_GENERIC)
        got = tm.debug_float(full.to_torch('cuda'), stage)
    finally:
        tm.set_option(_abi.OPT_FAST_PATH, 1)
    T = float_tolerance(params, kernel, stage, 'uniform', Planes(params, twin.buf, W, H, lut_n=LUT_N))
    report, fails = judge_float(params, kernel, 'uniform', stage, got, T)
    assert not fails, '; '.join(fails)


@pytest.mark.parametrize('wh', [(256, 128), (200, 96)])       # quad form; row / generic form
@pytest.mark.parametrize('layout', ['planar', 'semi'])
def test_peak_stats_of_a_full_range_set(wh, layout):
    """h2s_peak_stats reads the same constants: a full-range set's statistics
    against oracle.peak_stats of the limited twin, at test_peak_detect's
    tolerance for that comparison."""
    W, H = wh
    params = hdr2sdr.TonemapParams(tonemapper='bt.2390', peak_detect=True, maxcll=4000.0)
    full, twin = greys(W, H, 10, 3)
    with hdr2sdr.Tonemapper(0, params, lat()) as t:
        fmax, favg = t.peak_stats(full.to_layout(layout).to_torch('cuda'))
        tmax, tavg = t.peak_stats(twin.to_torch('cuda'))
    mx, avg = oracle.peak_stats(oracle.params_from(params.to_c()), twin.buf, W, H)
    np.testing.assert_allclose(fmax, mx, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(favg, avg, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(tmax, mx, rtol=1e-5, atol=1e-6)      # (the tags did not stick)


# ---- 4: arbitrary content against the float64 restatement --------------------------------
@pytest.mark.parametrize('tags', [('pc', 'left'), ('tv', 'topleft'), ('pc', 'topleft')], ids='-'.join)
@pytest.mark.parametrize('kind', ['uniform', 'smooth', 'ramp'])
@pytest.mark.parametrize('wh', [(64, 32), (192, 70), (208, 64), (70, 34)], ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('chain', ['hable_lut', 'reinhard_hlg12'])
def test_arbitrary_content_matches_the_restatement(tm, chain, wh, kind, tags):
    W, H = wh
    kw, rest = B_CHAINS[chain]
    params = hdr2sdr.TonemapParams(**kw)
    fb = cached(('synth', kind, W, H, params.bits_in),
                lambda: synth_frames(kind, NF, W, H, params.bits_in, device='cpu', seed=17).to_numpy())
    src = TR.tagged(fb, *tags)
    configure(tm, params)
    assert paths(tm, src, params.bits_out) == SIZES[wh]
    got = gpu(tm, src, params.bits_out)
    step = 1 << (params.bits_out - 8)           # compat8: the quantiser's step at the output depth
    for f in range(NF):
        want = TR.restated(src.y[f], src.u[f], src.v[f], *rest, color_range=tags[0], chroma_location=tags[1])
        for name, a, b in zip('YUV', (got.y[f], got.u[f], got.v[f]), want):
            d = np.abs(a.astype(np.int64) - b)
            print(f'TAGS-B {chain} {W}x{H} {kind} {tags} f{f} {name} max={int(d.max())} '
                  f'differ={float((d > 0).mean()):.4%}')
            assert d.max() <= 2 * step, (f, name, int(d.max()))
            assert (d > 0).mean() <= 1e-2, (f, name, float((d > 0).mean()))


# ---- 5: further checks ----------------------------------------------------------------------
@pytest.mark.parametrize('chain', ['c2_hable_g22', 'bt2390_ipt'])
@pytest.mark.parametrize('wh', list(SIZES), ids=lambda v: f'{v[0]}x{v[1]}')
def test_the_chroma_location_is_honoured(tm, chain, wh):
    """Vertical chroma structure: top-left output differs from left.  Chroma
    constant down every column: the two are equal sample for sample, on the
    route the size takes and on the generic kernel."""
    W, H = wh
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    edges = cached(('synth', 'edges', W, H, 10), lambda: synth_frames('edges', NF, W, H, 10, device='cpu', seed=17).to_numpy())
    flat = FrameBatch(edges.buf.copy(), W, H, 10)
    flat.u[...] = flat.u[:, :1]
    flat.v[...] = flat.v[:, :1]
    configure(tm, params)
    assert paths(tm, TR.tagged(edges, 'tv', 'topleft'), 10) == SIZES[wh]
    assert not np.array_equal(gpu(tm, TR.tagged(edges, 'tv', 'topleft'), 10).buf, gpu(tm, edges, 10).buf)
    assert np.array_equal(gpu(tm, TR.tagged(flat, 'tv', 'topleft'), 10).buf, gpu(tm, flat, 10).buf)
    assert np.array_equal(generic(tm, TR.tagged(flat, 'tv', 'topleft'), 10).buf, generic(tm, flat, 10).buf)
    assert not np.array_equal(generic(tm, TR.tagged(edges, 'tv', 'topleft'), 10).buf, generic(tm, edges, 10).buf)


@pytest.mark.parametrize('chain', ['c2_hable_g22', 'hable_pq12', 'mobius_hlg12'])   # PQ 10 / 12 bit, the HLG table form
def test_full_range_extremes_reach_the_exact_path(tm, chain):
    """Luma 2^b - 1 with chroma 0 and 2^b - 1 (E up to 1.94, past the PQ
    table's end at 1.875), and with chroma 94 % of the half-range (E = 1.883,
    inside the full-range codes but past the table too): the tile kernel must
    take the exact-capable body for those tiles, so its output equals the
    generic kernel's within the gate; the route is still TILE."""
    W, H = 128, 64
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    bits = params.bits_in
    top, mid = (1 << bits) - 1, 1 << (bits - 1)
    fb = synth_frames('smooth', 1, W, H, bits, device='cpu', seed=23).to_numpy()
    fb = FrameBatch(fb.buf.copy(), W, H, bits)
    fb.y[0, 4:12, 4:28] = top
    fb.u[0, 2:6, 2:6], fb.v[0, 2:6, 2:6] = 0, top
    fb.u[0, 2:6, 8:12], fb.v[0, 2:6, 8:12] = top, 0
    far = mid + (mid * 15) // 16                    # |c| = 93.75 % of the half-range
    fb.y[0, 36:44, 68:92] = top
    fb.u[0, 18:22, 34:38], fb.v[0, 18:22, 40:44] = far, far
    src = TR.tagged(fb, 'pc', 'left')
    configure(tm, params)
    assert paths(tm, src, params.bits_out) == _abi.PATH_TILE
    got = gpu(tm, src, params.bits_out).buf.astype(np.int64)
    want = generic(tm, src, params.bits_out).buf.astype(np.int64)
    d = np.abs(got - want)
    print(f'TAGS-EXACT {chain} {bits} max={int(d.max())} differ={float((d > 0).mean()):.4%}')
    assert_close_int(params, got, want, W, H, fb.buf, lut_n=LUT_N)


@pytest.mark.parametrize('tags', [('pc', 'left'), ('tv', 'topleft'), ('pc', 'topleft')], ids='-'.join)
@pytest.mark.parametrize('chain', ['c2_hable_g22', 'hable_pq12', 'bt2390_ipt'])
@pytest.mark.parametrize('wh', [(192, 96), (208, 64)], ids=['tile', 'tile_tail'])
def test_semi_planar_input_equals_the_planar_run(tm, wh, chain, tags):
    W, H = wh
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    fb = cached(('synth', 'smooth', W, H, params.bits_in),
                lambda: synth_frames('smooth', NF, W, H, params.bits_in, device='cpu', seed=17).to_numpy())
    src = TR.tagged(fb, *tags)
    semi = src.to_layout('semi')
    assert semi.layout == 'semi' and (semi.color_range, semi.chroma_location) == tags
    configure(tm, params)
    assert paths(tm, semi, params.bits_out) == SIZES[wh]
    want = gpu(tm, src, params.bits_out)
    assert np.array_equal(gpu(tm, semi, params.bits_out).buf, want.buf)
    out_semi = gpu(tm, semi, params.bits_out, 'semi')            # semi-planar output = the planar one repacked
    assert out_semi.layout == 'semi' and np.array_equal(out_semi.buf, want.to_layout('semi').buf)
    assert np.array_equal(gpu(tm, src, params.bits_out, 'semi').buf, out_semi.buf)
    assert not np.array_equal(want.buf, gpu(tm, fb, params.bits_out).buf)


@pytest.mark.parametrize('chain', ['c2_hable_g22', 'bt2390_ipt'])
@pytest.mark.parametrize('serial', [0, 1])
def test_host_sets_equal_the_device_run(tm, serial, chain):
    W, H, n = 192, 96, 3
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    fb = cached(('synth3', W, H), lambda: synth_frames('smooth', n, W, H, 10, device='cpu', seed=19).to_numpy())
    src = TR.tagged(fb, 'pc', 'topleft')
    configure(tm, params)
    want = gpu(tm, src, 10).buf
    dst = FrameBatch.empty_numpy(n, W, H, 10)
    tm.set_option(_abi.OPT_HOST_SERIAL, serial)
    try:
        tm.process(src, dst)
    finally:
        tm.set_option(_abi.OPT_HOST_SERIAL, 0)
    assert np.array_equal(dst.buf, want)
    assert not np.array_equal(want, gpu(tm, fb, 10).buf)


@pytest.mark.parametrize('pipeline', ['cpu', 'libplacebo'])
@pytest.mark.parametrize('wh', [(192, 96), (208, 64)], ids=['tile', 'tile_tail'])
def test_dynamic_peak_over_a_tagged_sequence(wh, pipeline):
    """peak_detect over three full-range, top-left frames of different
    brightness (grey steps: the limited twin is what the oracle reads): the
    tile run against the serial generic run, under the dynamic-peak tests'
    gate (assert_close_int with the oracle's per-frame knees), and both
    against the oracle's sequential flow on the twin."""
    W, H = wh
    params = hdr2sdr.TonemapParams(tonemapper='bt.2390', peak_detect=True, maxcll=4000.0, pipeline=pipeline)
    parts = [TR.grey_steps(1, W, H, 10, seed=s, levels=lv) for s, lv in ((1, (0, 1, 2)), (2, (0, 1)), (3, (0, 1, 2, 3)))]
    full = TR.tagged(FrameBatch(np.concatenate([p[0].buf for p in parts]), W, H, 10), 'pc', 'topleft')
    twin = np.concatenate([p[1].buf for p in parts])
    runs = {}
    for fast in (1, 0):
        with hdr2sdr.Tonemapper(0, params, lat()) as t:
            t.set_option(_abi.OPT_FAST_PATH, fast)
            dst = FrameBatch.empty_torch(3, W, H, 10, 'cuda')
            assert t.query_path(full.to_torch('cuda'), dst) == (SIZES[wh] if fast else _abi.PATH_GENERIC)
            runs[fast] = gpu(t, full, 10).buf.astype(np.int64)
            state = t.peak_state()
    knees = []
    want, peaks = oracle.process_dynamic(oracle.params_from(params.to_c()), lat(), twin, W, H, knees=knees)
    assert state['frames'] == 3 and state['peak'] == pytest.approx(peaks[-1], rel=1e-4)
    assert_close_int(params, runs[1], runs[0], W, H, twin, lut_n=LUT_N, knees=knees)
    assert_close_int(params, runs[1], want.astype(np.int64), W, H, twin, lut_n=LUT_N, knees=knees)


def test_preview_of_a_tagged_batch():
    from hdr2sdr import preview as PV
    W, H, box = 192, 96, (192, 96)
    full, twin = greys(W, H, 10, 1)
    with PV.Previewer(0, tonemapper='reinhard', lut_enabled=True, lattice=lat()) as pv:
        got = pv.convert(TR.tagged(full, 'pc', 'topleft'), box[0], box[1])
        plain = pv.convert(TR.tagged(full), box[0], box[1])
        ow, oh = PV.fit_size(W, H, *box)
        want = oracle.preview_rgb24(oracle.params_from(pv.params.to_c()), lat(), twin.buf, W, H, ow, oh, 1.0)
    d = np.abs(got.astype(int) - want.astype(int))
    assert d.max() <= 4 and (d > 1).mean() < 1e-2     # tests/test_preview.py's end-to-end bound
    assert not np.array_equal(got, plain)              # and the next, untagged batch was read untagged


def test_422_input_ignores_the_chroma_location(tm):
    W, H = 192, 70
    params = hdr2sdr.TonemapParams(**CHAINS['c2_hable_g22'])
    s422 = TR.as_422(even_source('smooth', W, H, 10))
    configure(tm, params)
    assert paths(tm, TR.tagged(s422, 'tv', 'topleft'), 10) == _abi.PATH_TILE
    want = gpu(tm, s422, 10).buf
    assert np.array_equal(gpu(tm, TR.tagged(s422, 'tv', 'topleft'), 10).buf, want)
    assert not np.array_equal(gpu(tm, TR.tagged(s422, 'pc', 'topleft'), 10).buf, want)     # (the range applies)
    got = tm.debug_float(TR.tagged(s422, 'tv', 'topleft').to_torch('cuda'), 1)
    assert np.array_equal(got, tm.debug_float(s422.to_torch('cuda'), 1))


@pytest.mark.parametrize('chain', ['c2_hable_g22', 'bt2390_ipt'])
def test_debug_planes_of_a_topleft_set_are_the_generic_kernels(tm, chain):
    """No debug instances of the tile kernel for top-left: the planes are
    k_debug's whatever the path (the 4:2:2 / 4:4:4 rule), and on the CPU chain
    they are the planes of the paired 4:2:2 plane up to the blend's last bit."""
    W, H = 64, 32
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    fb = even_source('smooth', W, H, 10)
    src = TR.tagged(fb, 'tv', 'topleft').to_torch('cuda')
    configure(tm, params)
    assert paths(tm, src, 10) == _abi.PATH_TILE
    on_tile = tm.debug_float(src, 1)
    tm.set_option(_abi.OPT_FAST_PATH, 0)
    try:
        assert np.array_equal(on_tile, tm.debug_float(src, 1))
    finally:
        tm.set_option(_abi.OPT_FAST_PATH, 1)
    assert not np.array_equal(on_tile, tm.debug_float(fb.to_torch('cuda'), 1))
    if chain not in LP:
        want = tm.debug_float(TR.as_422(fb).to_torch('cuda'), 1).astype(np.float64)
        assert np.all(np.abs(on_tile - want) <= 1e-3 * np.abs(want) + 1e-5)


# ---- refusals and state ------------------------------------------------------------------------
def test_refusals_raw_calls_and_defaults():
    import torch
    W, H = 64, 32
    fb = synth_frames('uniform', 1, W, H, 10, device='cpu', seed=3)
    src, dst = fb.to_torch('cuda'), FrameBatch.empty_torch(1, W, H, 10, 'cuda')
    params = hdr2sdr.TonemapParams(tonemapper='hable')
    with hdr2sdr.Tonemapper(0, params, lat()) as fresh:
        want = gpu(fresh, fb, 10).buf
    with hdr2sdr.Tonemapper(0, params, lat()) as t:
        L = t._L
        raw = lambda: L.h2s_process(t._ctx, ctypes.byref(src.descriptor()), ctypes.byref(dst.descriptor()), 1, None)  # noqa: E731
        for r, c in ((2, 0), (-1, 0), (0, 2), (0, -1), (1, 3)):
            assert L.h2s_set_input_tags(t._ctx, r, c) == _abi.H2S_E_INVALID_ARG
            assert L.h2s_last_error(t._ctx)
        assert L.h2s_set_input_tags(None, 0, 0) == _abi.H2S_E_INVALID_ARG
        # the refused values changed nothing, and the explicit defaults are the untagged call bit for bit
        assert L.h2s_set_input_tags(t._ctx, _abi.RANGE_LIMITED, _abi.CHROMA_LEFT) == 0
        assert raw() == 0
        torch.cuda.synchronize()
        assert np.array_equal(dst.to_numpy().buf, want)
        assert L.h2s_set_input_tags(t._ctx, _abi.RANGE_FULL, _abi.CHROMA_TOPLEFT) == 0
        assert L.h2s_set_input_tags(t._ctx, 7, 0) == _abi.H2S_E_INVALID_ARG      # the setting stays
        assert raw() == 0
        torch.cuda.synchronize()
        tagged = dst.to_numpy().buf.copy()
        assert not np.array_equal(tagged, want)
        assert np.array_equal(tagged, gpu(t, TR.tagged(fb.to_numpy(), 'pc', 'topleft'), 10).buf)


def test_refusals_through_python_and_no_stickiness(tm):
    W, H = 192, 96
    params = hdr2sdr.TonemapParams(**CHAINS['c2_hable_g22'])
    fb = cached(('synth', 'uniform', W, H, 10), lambda: synth_frames('uniform', NF, W, H, 10, device='cpu', seed=17).to_numpy())
    with pytest.raises(ValueError):
        tm.set_input_tags('full', 'left')
    with pytest.raises(ValueError):
        tm.set_input_tags('tv', 'center')
    with pytest.raises(ValueError):
        FrameBatch.empty_torch(1, W, H, 10, 'cuda', 'planar', '420', 'pc', 'bottom')
    configure(tm, params)
    gpu(tm, TR.tagged(fb, 'pc', 'topleft'), 10)
    after = gpu(tm, fb, 10).buf
    host = FrameBatch.empty_numpy(NF, W, H, 10)
    tm.process(TR.tagged(fb, 'pc', 'topleft'), host)            # (the staging path too)
    tm.process(fb, host)
    with hdr2sdr.Tonemapper(0, params, lat()) as fresh:
        want = gpu(fresh, fb, 10).buf
    assert np.array_equal(after, want) and np.array_equal(host.buf, want)
