"""4:2:2 / 4:4:4 input on the GPU (h2s_set_input_subsampling): the tile kernel's
SUB instances, the generic kernel's, and the plumbing around them.

A. exact upsamples of a 4:2:0 frame (tests/subsampling_ref.py) against the C
   oracle's result for that frame, with test_gpu_parity's own gate;
B. arbitrary full-resolution chroma against the float64 restatement with the
   model's upsampler: <= 2 quantiser steps, <= 1 % of samples (the sum and the
   union of the two budgets in use: GPU vs oracle 1 step / 0.5 %, oracle vs
   restatement 1 step at gamma 1 / 0.5 %);
C. host sets, semi-planar output, preview, debug planes, and no stickiness;
D. the refusals.
"""
import ctypes

import numpy as np
import pytest

import hdr2sdr
import oracle
import subsampling_ref as SR
from hdr2sdr import _abi
from hdr2sdr.frames import FrameBatch
from hdr2sdr.synth import synth_frames
from test_gpu_parity import assert_close_int

pytestmark = pytest.mark.gpu

LUT_N = 17
NF = 3
SUBS = ('422', '444')
# size -> the path of a chain the tile kernel serves (4:2:0, 4:2:2 and 4:4:4 alike)
SIZES = {(64, 32): _abi.PATH_TILE,        # one tile, every edge
         (192, 96): _abi.PATH_TILE,       # 3 x 3 tiles, the centre one on the interior scalar-origin loads
         (192, 70): _abi.PATH_TILE,       # a bottom tile with 6 live rows: chroma rows clamp too
         (208, 64): _abi.PATH_TILE_TAIL,  # 16 ragged columns on k_process
         (70, 34): _abi.PATH_GENERIC}     # ragged groups on the generic kernel
SOME = [(64, 32), (192, 70), (208, 64)]
CHAINS = {
    'c2_hable_g22': dict(tonemapper='hable', gamma=2.2, bits_out=10),
    'mobius_hlg12': dict(tonemapper='mobius', bits_in=12, bits_out=12, transfer='arib-std-b67'),
    'reinhard_8': dict(tonemapper='reinhard', bits_out=8),
    'hable_native': dict(tonemapper='hable', mode='native'),
    'hable_lut_off': dict(tonemapper='hable', lut_enabled=False),
}
_LAT = {}
_CACHE = {}


def lat():
    if LUT_N not in _LAT:
        _LAT[LUT_N] = hdr2sdr.generate_lattice(LUT_N)
    return _LAT[LUT_N]


@pytest.fixture(scope='module')
def tm():
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.close()


def configure(tm, params):
    tm.set_params(params)
    if params.lut_enabled:
        tm.set_lut(lat())


def source(kind, W, H, bits, edge='zimg'):
    """(4:2:0 batch with chroma multiples of 8, its exact 4:2:2 / 4:4:4 upsamples), computed once."""
    key = (kind, W, H, bits, edge)
    if key not in _CACHE:
        fb = SR.round8(synth_frames(kind, NF, W, H, bits, device='cpu', seed=11).to_numpy())
        _CACHE[key] = (fb, SR.exact_inputs(fb, edge))
    return _CACHE[key]


def oracle_420(params, fb):
    key = ('oracle', repr(params), id(fb))
    if key not in _CACHE:
        _CACHE[key] = oracle.process(oracle.params_from(params.to_c()), lat() if params.lut_enabled else None, fb.buf,
                                     fb.width, fb.height).astype(np.int64)
    return _CACHE[key]


def gpu(tm, src, bits_out, out_layout='planar'):
    import torch
    dst = FrameBatch.empty_torch(src.nframes, src.width, src.height, bits_out, 'cuda', out_layout)
    tm.process(src.to_torch('cuda'), dst)
    torch.cuda.synchronize()
    return dst.to_numpy()


def paths(tm, src, bits_out):
    dst = FrameBatch.empty_torch(src.nframes, src.width, src.height, bits_out, 'cuda')
    return tm.query_path(src.to_torch('cuda'), dst)


# ---- A: equivalence to the oracle's 4:2:0 result ---------------------------------
A_CASES = ([('c2_hable_g22', wh, k) for wh in SIZES for k in ('uniform', 'smooth', 'edges')] +
           [(c, wh, k) for c in list(CHAINS)[1:] for wh in SOME for k in ('uniform', 'smooth')])


@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('chain,wh,kind', A_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_exact_upsamples_match_the_oracle_on_the_420_frame(tm, chain, wh, kind, sub):
    W, H = wh
    params = hdr2sdr.TonemapParams(**CHAINS[chain])
    fb, ups = source(kind, W, H, params.bits_in)
    configure(tm, params)
    path = paths(tm, ups[sub], params.bits_out)
    assert path == paths(tm, fb, params.bits_out)
    if params.lut_enabled:
        assert path == SIZES[wh]
    else:
        assert path == _abi.PATH_GENERIC       # the CPU chain's LUT-off form runs on the generic kernel
    got = gpu(tm, ups[sub], params.bits_out).buf.astype(np.int64)
    # recorded, not asserted: the staged values are exact integers in both
    # forms, so the tile path should give the GPU's own 4:2:0 output
    same = np.array_equal(got, gpu(tm, fb, params.bits_out).buf.astype(np.int64))
    print(f'SUBSAMPLING-EQ {chain} {W}x{H} {kind} {sub} path={path} equals_gpu_420={same}')
    assert_close_int(params, got, oracle_420(params, fb), W, H, fb.buf, lut_n=LUT_N)


@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('edge', ['replicate', 'mirror'])
def test_chroma_edge_rules(tm, edge, sub):
    W, H = 64, 32
    params = hdr2sdr.TonemapParams(chroma_edge=edge, **CHAINS['c2_hable_g22'])
    fb, ups = source('uniform', W, H, 10, edge)
    configure(tm, params)
    assert paths(tm, ups[sub], 10) == _abi.PATH_TILE
    got = gpu(tm, ups[sub], 10).buf.astype(np.int64)
    assert_close_int(params, got, oracle_420(params, fb), W, H, fb.buf, lut_n=LUT_N)


@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('wh', [(64, 32), (70, 34)])
def test_bicubic_output_chroma_two_pass(tm, wh, sub):
    W, H = wh
    params = hdr2sdr.TonemapParams(chroma_filter='bicubic', **CHAINS['c2_hable_g22'])
    fb, ups = source('smooth', W, H, 10)
    configure(tm, params)
    assert paths(tm, ups[sub], 10) == paths(tm, fb, 10)
    got = gpu(tm, ups[sub], 10).buf.astype(np.int64)
    assert_close_int(params, got, oracle_420(params, fb), W, H, fb.buf, lut_n=LUT_N)


@pytest.mark.parametrize('sub', SUBS)
def test_generic_kernel_on_a_tile_sized_frame(tm, sub):
    W, H = 192, 70
    params = hdr2sdr.TonemapParams(**CHAINS['c2_hable_g22'])
    fb, ups = source('uniform', W, H, 10)
    configure(tm, params)
    tm.set_option(_abi.OPT_FAST_PATH, 0)
    try:
        assert paths(tm, ups[sub], 10) == _abi.PATH_GENERIC
        got = gpu(tm, ups[sub], 10).buf.astype(np.int64)
    finally:
        tm.set_option(_abi.OPT_FAST_PATH, 1)
    assert_close_int(params, got, oracle_420(params, fb), W, H, fb.buf, lut_n=LUT_N)


# ---- B: arbitrary full-resolution chroma ---------------------------------------------
B_CHAINS = {
    # (library parameters, the restatement's: bits_in, bits_out, hlg, operator, gamma, lut_n)
    'hable_lut': (dict(tonemapper='hable', bits_out=10), (10, 10, False, 'hable', 1.0, LUT_N)),
    'mobius_lut_off': (dict(tonemapper='mobius', bits_out=10, lut_enabled=False), (10, 10, False, 'mobius', 1.0, 0)),
    'reinhard_hlg12': (dict(tonemapper='reinhard', bits_in=12, bits_out=12, transfer='arib-std-b67'),
                       (12, 12, True, 'reinhard', 1.0, LUT_N)),
}


@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('kind', ['uniform', 'smooth', 'ramp'])
@pytest.mark.parametrize('wh', [(64, 32), (192, 70), (208, 64), (70, 34)], ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('chain', sorted(B_CHAINS))
def test_arbitrary_chroma_matches_the_restatement(tm, chain, wh, kind, sub):
    W, H = wh
    kw, rest = B_CHAINS[chain]
    params = hdr2sdr.TonemapParams(**kw)
    luma = synth_frames(kind, NF, W, H, params.bits_in, device='cpu', seed=17).to_numpy()
    src = SR.random_chroma(luma, sub, seed=W * 1000 + H)
    configure(tm, params)
    got = gpu(tm, src, params.bits_out)
    step = 1 << (params.bits_out - 8)           # compat8: the quantiser's step at the output depth
    for f in range(NF):
        want = SR.restated(sub, src.y[f], src.u[f], src.v[f], *rest)
        for name, a, b in zip('YUV', (got.y[f], got.u[f], got.v[f]), want):
            d = np.abs(a.astype(np.int64) - b)
            print(f'SUBSAMPLING-B {chain} {W}x{H} {kind} {sub} f{f} {name} max={int(d.max())} '
                  f'differ={float((d > 0).mean()):.4%}')
            assert d.max() <= 2 * step, (f, name, int(d.max()))
            assert (d > 0).mean() <= 1e-2, (f, name, float((d > 0).mean()))


# ---- C: plumbing -------------------------------------------------------------------------
@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('serial', [0, 1])
def test_host_sets_equal_the_device_run(tm, serial, sub):
    W, H = 192, 96
    params = hdr2sdr.TonemapParams(**CHAINS['c2_hable_g22'])
    _, ups = source('smooth', W, H, 10)
    configure(tm, params)
    want = gpu(tm, ups[sub], 10).buf
    dst = FrameBatch.empty_numpy(NF, W, H, 10)
    tm.set_option(_abi.OPT_HOST_SERIAL, serial)
    try:
        tm.process(ups[sub], dst)
    finally:
        tm.set_option(_abi.OPT_HOST_SERIAL, 0)
    assert np.array_equal(dst.buf, want)


@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('bits_out', [10, 8], ids=['p010le', 'nv12'])
@pytest.mark.parametrize('wh', [(192, 96), (208, 64)], ids=['tile', 'tile_tail'])
def test_semi_planar_output_equals_the_planar_one_repacked(tm, wh, bits_out, sub):
    W, H = wh
    params = hdr2sdr.TonemapParams(tonemapper='hable', gamma=2.2, bits_out=bits_out)
    _, ups = source('smooth', W, H, 10)
    configure(tm, params)
    planar = gpu(tm, ups[sub], bits_out)
    semi = gpu(tm, ups[sub], bits_out, 'semi')
    assert semi.layout == 'semi' and np.array_equal(semi.buf, planar.to_layout('semi').buf)


def test_preview_of_a_422_batch():
    from hdr2sdr import preview as PV
    W, H, box = 192, 96, (192, 96)
    fb, ups = source('smooth', W, H, 10)
    with PV.Previewer(0, tonemapper='reinhard', lut_enabled=True, lattice=lat()) as pv:
        got = pv.convert(ups['422'], box[0], box[1])
        ow, oh = PV.fit_size(W, H, *box)
        want = oracle.preview_rgb24(oracle.params_from(pv.params.to_c()), lat(), fb.buf, W, H, ow, oh, 1.0)
    d = np.abs(got.astype(int) - want.astype(int))
    assert d.max() <= 4 and (d > 1).mean() < 1e-2     # tests/test_preview.py's end-to-end bound


@pytest.mark.parametrize('stage', [1, 5])
def test_debug_planes_of_a_444_batch(tm, stage):
    """The generic kernel's planes of the exact 4:4:4 upsample against the
    oracle's planes of the 4:2:0 frame, through the suite's 1e-3 float gate as
    it stands (tests/float_gate.py: 1e-3 relative plus its stated conditioning
    allowances and floors; test_gpu_parity.check_float_stage's judge).  The
    bare |d| <= 1e-3 |want| + 1e-5 is printed beside it: measured 0.06 of that
    bound at stage 1 and 1.05 at stage 5 (planes in code units, 224 x C':
    chroma next to zero has no relative scale, which the gate's stage-5
    floor of 224 x 1e-5 is for)."""
    from float_gate import Planes, float_tolerance, judge_float
    W, H = 64, 32
    params = hdr2sdr.TonemapParams(**CHAINS['c2_hable_g22'])
    fb, ups = source('smooth', W, H, 10)
    configure(tm, params)
    got = tm.debug_float(ups['444'].to_torch('cuda'), stage)
    T = float_tolerance(params, 'k_debug', stage, 'smooth', Planes(params, fb.buf, W, H, lut_n=LUT_N))
    bare = np.abs(got.astype(np.float64) - T.want) / (1e-3 * np.abs(T.want) + 1e-5)
    print(f'SUBSAMPLING-DBG stage {stage}: bare 1e-3 bound used up to {float(bare.max()):.4f}')
    report, fails = judge_float(params, 'k_debug', 'smooth', stage, got, T)
    assert not fails, '; '.join(fails)


def test_the_setting_does_not_stick(tm):
    W, H = 192, 96
    params = hdr2sdr.TonemapParams(**CHAINS['c2_hable_g22'])
    fb, ups = source('uniform', W, H, 10)
    configure(tm, params)
    gpu(tm, ups['444'], 10)
    after = gpu(tm, fb, 10).buf
    host = FrameBatch.empty_numpy(NF, W, H, 10)
    tm.process(ups['444'], host)            # (the staging buffers too)
    tm.process(fb, host)
    with hdr2sdr.Tonemapper(0, params, lat()) as fresh:
        want = gpu(fresh, fb, 10).buf
    assert np.array_equal(after, want) and np.array_equal(host.buf, want)


# ---- D: refusals ----------------------------------------------------------------------------
def _raw(t, src_desc, dst_desc, n=1):
    return t._L.h2s_process(t._ctx, ctypes.byref(src_desc), ctypes.byref(dst_desc), n, None)


def test_refusals_raw_calls():
    import torch
    W, H = 64, 32
    src = FrameBatch.empty_torch(1, W, H, 10, 'cuda', 'planar', '444')
    src.buf.fill_(512)
    dst = FrameBatch.empty_torch(1, W, H, 10, 'cuda')
    with hdr2sdr.Tonemapper(0, hdr2sdr.TonemapParams(tonemapper='hable'), lat()) as t:
        L = t._L
        # semi-planar input + 4:2:2
        assert L.h2s_set_frame_layout(t._ctx, _abi.LAYOUT_SEMI, _abi.LAYOUT_PLANAR) == 0
        assert L.h2s_set_input_subsampling(t._ctx, _abi.SUB_422) == 0
        assert _raw(t, src.descriptor(), dst.descriptor()) == _abi.H2S_E_UNSUPPORTED
        assert b'semi' in L.h2s_last_error(t._ctx)
        assert L.h2s_query_path(t._ctx, ctypes.byref(src.descriptor()), ctypes.byref(dst.descriptor())) == \
            _abi.H2S_E_UNSUPPORTED
        assert L.h2s_set_frame_layout(t._ctx, _abi.LAYOUT_PLANAR, _abi.LAYOUT_PLANAR) == 0
        # peak statistics of a 4:2:2 batch
        fmax, favg = np.zeros(1), np.zeros(1)
        s422 = FrameBatch.empty_torch(1, W, H, 10, 'cuda', 'planar', '422')
        d = s422.descriptor()
        assert L.h2s_peak_stats(t._ctx, ctypes.byref(d), 1, fmax.ctypes.data, favg.ctypes.data, None) == \
            _abi.H2S_E_UNSUPPORTED
        assert L.h2s_last_error(t._ctx)
        # an unknown value on a live context; the setting stays
        assert L.h2s_set_input_subsampling(t._ctx, 3) == _abi.H2S_E_INVALID_ARG
        assert L.h2s_set_input_subsampling(t._ctx, -1) == _abi.H2S_E_INVALID_ARG
        assert L.h2s_last_error(t._ctx)
        # the libplacebo pipeline (bt.2390 resolves to it) + 4:4:4
        t.set_params(hdr2sdr.TonemapParams(tonemapper='bt.2390'))
        assert L.h2s_set_input_subsampling(t._ctx, _abi.SUB_444) == 0
        assert _raw(t, src.descriptor(), dst.descriptor()) == _abi.H2S_E_UNSUPPORTED
        assert b'libplacebo' in L.h2s_last_error(t._ctx)
        # back to 4:2:0 the same context converts again
        assert L.h2s_set_input_subsampling(t._ctx, _abi.SUB_420) == 0
        s420 = FrameBatch.empty_torch(1, W, H, 10, 'cuda')
        s420.buf.fill_(512)
        assert _raw(t, s420.descriptor(), dst.descriptor()) == 0
        torch.cuda.synchronize()


def test_refusals_through_python(tm):
    W, H = 64, 32
    s444 = FrameBatch.empty_torch(1, W, H, 10, 'cuda', 'planar', '444')
    s422 = FrameBatch.empty_torch(1, W, H, 10, 'cuda', 'planar', '422')
    dst = FrameBatch.empty_torch(1, W, H, 10, 'cuda')
    with pytest.raises(ValueError):
        FrameBatch.empty_torch(1, W, H, 10, 'cuda', 'semi', '422')
    configure(tm, hdr2sdr.TonemapParams(tonemapper='bt.2390'))
    with pytest.raises(ValueError, match='libplacebo'):
        tm.process(s444, dst)
    with pytest.raises(ValueError):
        tm.query_path(s444, dst)
    with pytest.raises(ValueError):
        tm.peak_stats(s422)
    with pytest.raises(ValueError):
        tm.set_input_subsampling('411')
    with pytest.raises(ValueError):
        tm.process(s422, s422)       # the output side is 4:2:0
    # a too-short 4:4:4 linesize is caught by the frame check
    configure(tm, hdr2sdr.TonemapParams(tonemapper='hable'))
    tm.set_input_subsampling('444')
    d = s422.descriptor()
    assert tm._L.h2s_process(tm._ctx, ctypes.byref(d), ctypes.byref(dst.descriptor()), 1, None) == \
        _abi.H2S_E_INVALID_ARG
    tm.set_input_subsampling('420')
