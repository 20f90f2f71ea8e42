"""The preview's source pane on the GPU (h2s_preview_source_rgb24 / _batch,
Previewer.original / original_batch / pair) against the float64 restatement in
tests/source_preview_ref.py.

Gate (the project's integer rule): every output byte within 1 of
the restatement and at most 0.5 % of a case's bytes differing at all; the
float32 restatement meets it on the same cases on the CPU
(tests/test_source_preview.py).  Flat frames and neutral chroma are exact
constructions with no tolerance."""
import ctypes
import functools

import numpy as np
import pytest

import hdr2sdr
import source_preview_ref as ref
from hdr2sdr import _abi
from hdr2sdr.preview import Previewer, source_rgb

pytestmark = pytest.mark.gpu

CASE_IDS = [c[0] for c in ref.CASES]
BY_ID = {c[0]: c for c in ref.CASES}


@pytest.fixture(scope='module')
def tm():
    """A context that never had params or a LUT: the source pane needs neither."""
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.close()


@functools.lru_cache(maxsize=None)
def _lattice():
    return hdr2sdr.generate_lattice(65)


@functools.lru_cache(maxsize=None)
def _frames(case_id, kind, nframes=1):
    return ref.case_frames(BY_ID[case_id], kind, nframes)


@functools.lru_cache(maxsize=None)
def _want(case_id, kind, matrix='bt2020nc', rgb='trunc16', nframes=1):
    ow, oh = ref.case_size(BY_ID[case_id])
    return ref.expected(_frames(case_id, kind, nframes), ow, oh, matrix, rgb)


def check_gate(got, want, what):
    mx, frac = ref.gate(np.asarray(got), want)
    print(f'{what}: max diff {mx}, {frac:.4%} of bytes differ')
    assert mx <= ref.MAX_DIFF and frac <= ref.MAX_FRACTION, what


def raw_call(tm, src, nframes, ow, oh, matrix=_abi.SRC_MATRIX_BT2020NC, model=_abi.SRC_RGB_TRUNC16, use=True):
    """The C call on anything with descriptor() (a FrameBatch, a RowPadded),
    host output: (rc, [nframes, oh, ow, 3])."""
    out = np.zeros((nframes, oh, ow, 3), dtype=np.uint8)
    if use:
        tm._use_layouts(src)
    d = src.descriptor()
    rc = _abi.lib().h2s_preview_source_rgb24_batch(tm._ctx, ctypes.byref(d), nframes, out.ctypes.data, 3 * ow,
                                                   3 * ow * oh, ow, oh, matrix, model, _abi.LOC_HOST,
                                                   tm._stream_ptr(None))
    return rc, out


# ---- the cases against the restatement ---------------------------------------------------
@pytest.mark.parametrize('kind', ref.CONTENTS)
@pytest.mark.parametrize('case_id', CASE_IDS)
def test_case_meets_the_gate_from_host_and_device(tm, case_id, kind):
    fb = _frames(case_id, kind)
    ow, oh = ref.case_size(BY_ID[case_id])
    host = source_rgb(tm, fb, ow, oh)[0]
    assert host.shape == (oh, ow, 3) and host.dtype == np.uint8
    check_gate(host, _want(case_id, kind)[0], f'{case_id} {kind}')
    dev = source_rgb(tm, fb.to_torch('cuda:0'), ow, oh)[0]
    assert np.array_equal(dev, host)


@pytest.mark.parametrize('rgb', ref.RGB_MODELS)
@pytest.mark.parametrize('matrix', ref.MATRICES)
@pytest.mark.parametrize('case_id,kind', [('box48x27', 'smooth'), ('odd47x26', 'edges'), ('full', 'edges')])
def test_matrices_and_rgb_models(tm, case_id, kind, matrix, rgb):
    ow, oh = ref.case_size(BY_ID[case_id])
    got = source_rgb(tm, _frames(case_id, kind), ow, oh, matrix, rgb)[0]
    check_gate(got, _want(case_id, kind, matrix, rgb)[0], f'{case_id} {kind} {matrix} {rgb}')


def test_models_and_matrices_differ_on_the_device(tm):
    fb = _frames('box48x27', 'smooth')
    outs = {(m, r): source_rgb(tm, fb, 48, 27, m, r)[0] for m in ref.MATRICES for r in ref.RGB_MODELS}
    assert not np.array_equal(outs['bt2020nc', 'trunc16'], outs['bt2020nc', 'round8'])
    assert not np.array_equal(outs['bt2020nc', 'trunc16'], outs['bt709', 'trunc16'])
    assert not np.array_equal(outs['bt709', 'trunc16'], outs['bt601', 'trunc16'])


# ---- semi-planar and padded surfaces ---------------------------------------------------------
@pytest.mark.parametrize('bits', [10, 12])
@pytest.mark.parametrize('W,H,ow,oh', [(66, 34, 66, 34), (66, 34, 41, 21)])
def test_padded_semi_planar_equals_its_planar_twin(tm, bits, W, H, ow, oh):
    from padded_frames import FILL, RowPadded
    planar = ref.synth_source('smooth', 2, W, H, bits)
    tight = source_rgb(tm, planar, ow, oh)
    check_gate(np.stack(tight), ref.expected(planar, ow, oh), f'planar {bits}-bit {W}x{H} -> {ow}x{oh}')
    # p010le / p012le: rows 64 bytes apart, the low bits of every word set (they are no part of the code)
    semi = planar.to_layout('semi')
    semi.buf[...] |= np.uint16((1 << (16 - bits)) - 1)
    surf = RowPadded(2, W, H, bits, 'semi', align=64).load(semi)
    before = surf.raw().copy()
    rc, got = raw_call(tm, surf, 2, ow, oh)
    assert rc == 0, tm._L.h2s_last_error(tm._ctx)
    assert np.array_equal(got, np.stack(tight))
    assert np.array_equal(surf.raw(), before) and (before == FILL).any()
    # the semi-planar tight batch through the Python surface, and a padded planar surface
    assert np.array_equal(np.stack(source_rgb(tm, semi, ow, oh)), np.stack(tight))
    rc, got = raw_call(tm, RowPadded(2, W, H, bits, 'planar', align=64).load(planar), 2, ow, oh)
    assert rc == 0 and np.array_equal(got, np.stack(tight))


@pytest.mark.parametrize('sub', ['422', '444'])
def test_padded_422_and_444_surfaces(tm, sub):
    from padded_frames import RowPadded
    fb = _frames(sub, 'edges')
    want = source_rgb(tm, fb, 40, 20)[0]
    rc, got = raw_call(tm, RowPadded(1, 64, 32, 10, 'planar', sub, align=64).load(fb), 1, 40, 20)
    assert rc == 0 and np.array_equal(got[0], want)


# ---- tags -------------------------------------------------------------------------------------
def test_full_range_tag_changes_the_result_and_topleft_does_not(tm):
    fb = _frames('full', 'edges')
    assert fb.color_range == 'pc'
    y = np.asarray(fb.y)
    assert y.min() < 64 and y.max() > 940   # codes outside the limited range
    full = source_rgb(tm, fb, 40, 20)[0]
    limited = source_rgb(tm, hdr2sdr.FrameBatch(fb.buf, 64, 32, 10, color_range='tv'), 40, 20)[0]
    assert not np.array_equal(full, limited)
    for rng in ('tv', 'pc'):
        left = hdr2sdr.FrameBatch(fb.buf, 64, 32, 10, color_range=rng, chroma_location='left')
        top = hdr2sdr.FrameBatch(fb.buf, 64, 32, 10, color_range=rng, chroma_location='topleft')
        for ow, oh in ((64, 32), (40, 20)):
            assert np.array_equal(source_rgb(tm, top, ow, oh)[0], source_rgb(tm, left, ow, oh)[0])


# ---- batches and device output ------------------------------------------------------------------
def test_three_frame_batch_equals_three_single_calls(tm):
    fb = _frames('odd47x26', 'smooth', 3)
    batch = source_rgb(tm, fb, 47, 26)
    assert len(batch) == 3
    check_gate(np.stack(batch), _want('odd47x26', 'smooth', nframes=3), 'batch of 3')
    assert not np.array_equal(batch[0], batch[1])
    for i in range(3):
        assert np.array_equal(source_rgb(tm, fb.slice(i, i + 1), 47, 26)[0], batch[i])
    dev = fb.to_torch('cuda:0')
    assert np.array_equal(np.stack(source_rgb(tm, dev, 47, 26)), np.stack(batch))


@pytest.mark.parametrize('ow,oh', [(47, 26), (48, 27)])
def test_device_rgb_with_padded_pitches(tm, ow, oh):
    import torch
    fb = _frames('odd47x26', 'edges', 2)       # 128x72
    host = np.stack(source_rgb(tm, fb, ow, oh))
    ls, rows = 3 * ow + 19, oh + 3             # (an odd linesize at ow 47: rows of every byte alignment)
    fp = ls * rows
    buf = torch.full((2 * fp + 7,), 0xA5, dtype=torch.uint8, device='cuda:0')
    dev = fb.to_torch('cuda:0')
    tm._use_layouts(dev)
    d = dev.descriptor()
    rc = _abi.lib().h2s_preview_source_rgb24_batch(tm._ctx, ctypes.byref(d), 2, buf.data_ptr() + 1, ls, fp, ow, oh,
                                                   _abi.SRC_MATRIX_BT2020NC, _abi.SRC_RGB_TRUNC16, _abi.LOC_DEVICE,
                                                   tm._stream_ptr(None))
    assert rc == 0, tm._L.h2s_last_error(tm._ctx)
    raw = buf.cpu().numpy()
    assert raw[0] == 0xA5 and np.all(raw[1 + 2 * fp:] == 0xA5)
    img = raw[1:1 + 2 * fp].reshape(2, rows, ls)
    assert np.array_equal(img[:, :oh, :3 * ow].reshape(2, oh, ow, 3), host)
    assert np.all(img[:, :oh, 3 * ow:] == 0xA5) and np.all(img[:, oh:] == 0xA5)


def test_single_frame_entry_point_is_the_batch_of_one(tm):
    fb = _frames('box48x27', 'smooth')
    out = np.zeros((27, 48, 3), dtype=np.uint8)
    tm._use_layouts(fb)
    d = fb.descriptor()
    rc = _abi.lib().h2s_preview_source_rgb24(tm._ctx, ctypes.byref(d), out.ctypes.data, 3 * 48, 48, 27,
                                             _abi.SRC_MATRIX_BT709, _abi.SRC_RGB_ROUND8, _abi.LOC_HOST,
                                             tm._stream_ptr(None))
    assert rc == 0
    assert np.array_equal(out, source_rgb(tm, fb, 48, 27, 'bt709', 'round8')[0])


# ---- exact constructions ----------------------------------------------------------------------
@pytest.mark.parametrize('case_id', CASE_IDS)
def test_flat_frames_come_out_uniform_and_exact(tm, case_id):
    _, W, H, _, bits, sub, rng = BY_ID[case_id]
    ow, oh = ref.case_size(BY_ID[case_id])
    codes = ref.flat_codes(bits, rng)
    fb = ref.flat_frame(W, H, bits, *codes, subsampling=sub, color_range=rng)
    for matrix in ref.MATRICES:
        want16 = ref.expected16(fb, ow, oh, matrix)
        assert np.all(want16 == want16[0, 0, 0]) and np.all((want16 % 256 >= 8) & (want16 % 256 <= 247))
        got = source_rgb(tm, fb, ow, oh, matrix)[0]
        assert np.array_equal(got, (want16[0] >> 8).astype(np.uint8)), (case_id, matrix, codes)


@pytest.mark.parametrize('case_id', ['identity', 'odd47x26', 'upscale', 'ratio12', '444', 'full12'])
def test_neutral_chroma_is_grey_everywhere(tm, case_id):
    _, W, H, _, bits, sub, rng = BY_ID[case_id]
    ow, oh = ref.case_size(BY_ID[case_id])
    src = _frames(case_id, 'edges')
    fb = hdr2sdr.FrameBatch(src.buf.copy(), W, H, bits, 'planar', sub, rng)
    fb.u[...] = 1 << (bits - 1)
    fb.v[...] = 1 << (bits - 1)
    for matrix in ref.MATRICES:
        for rgb in ref.RGB_MODELS:
            got = source_rgb(tm, fb, ow, oh, matrix, rgb)[0]
            assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 1], got[..., 2])
            assert len(np.unique(got)) > 8
            check_gate(got, ref.expected(fb, ow, oh, matrix, rgb)[0], f'neutral {case_id} {matrix} {rgb}')


# ---- refusals -----------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(tm):
    fb = _frames('ratio12', 'smooth')           # 384x16
    good = source_rgb(tm, fb, 32, 16)[0]

    def still_works():
        assert np.array_equal(source_rgb(tm, fb, 32, 16)[0], good)

    # 4:2:2 with a semi-planar input
    tm.set_frame_layout('semi', 'planar')
    tm.set_input_subsampling('422')
    rc, _ = raw_call(tm, fb, 1, 32, 16, use=False)
    assert rc == _abi.H2S_E_UNSUPPORTED and b'semi-planar' in tm._L.h2s_last_error(tm._ctx)
    still_works()
    # an 8-bit set
    rc, _ = raw_call(tm, hdr2sdr.FrameBatch.empty_numpy(1, 64, 32, 8), 1, 64, 32)
    assert rc == _abi.H2S_E_INVALID_ARG
    still_works()
    # unknown matrix / model
    for matrix, model in ((3, 0), (-1, 0), (0, 2), (0, -1)):
        rc, _ = raw_call(tm, fb, 1, 32, 16, matrix, model)
        assert rc == _abi.H2S_E_INVALID_ARG, (matrix, model)
        still_works()
    with pytest.raises(ValueError):
        source_rgb(tm, fb, 32, 16, matrix='bt470bg')
    # a ratio beyond 12 (384 / 31, 16 / 1)
    for ow, oh in ((31, 16), (32, 1)):
        rc, _ = raw_call(tm, fb, 1, ow, oh)
        assert rc == _abi.H2S_E_UNSUPPORTED, (ow, oh)
        still_works()
    # geometry and NULLs, as h2s_preview_rgb24_batch
    L, d = _abi.lib(), fb.descriptor()
    out = np.zeros((16, 32, 3), dtype=np.uint8)
    args = (_abi.SRC_MATRIX_BT2020NC, _abi.SRC_RGB_TRUNC16, _abi.LOC_HOST, None)
    assert L.h2s_preview_source_rgb24_batch(tm._ctx, ctypes.byref(d), 1, None, 96, 96 * 16, 32, 16, *args) == \
        _abi.H2S_E_INVALID_ARG
    assert L.h2s_preview_source_rgb24_batch(tm._ctx, None, 1, out.ctypes.data, 96, 96 * 16, 32, 16, *args) == \
        _abi.H2S_E_INVALID_ARG
    assert L.h2s_preview_source_rgb24_batch(tm._ctx, ctypes.byref(d), 0, out.ctypes.data, 96, 96 * 16, 32, 16,
                                            *args) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_preview_source_rgb24_batch(tm._ctx, ctypes.byref(d), 1, out.ctypes.data, 95, 96 * 16, 32, 16,
                                            *args) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_preview_source_rgb24_batch(tm._ctx, ctypes.byref(d), 2, out.ctypes.data, 96, 96 * 16 - 1, 32, 16,
                                            *args) == _abi.H2S_E_INVALID_ARG
    still_works()


# ---- the Python surface ----------------------------------------------------------------------------
def test_original_batch_groups_mixed_sizes():
    a, b = _frames('box48x27', 'smooth'), _frames('portrait', 'edges')       # 128x72, 36x64
    a2 = ref.synth_source('edges', 1, 128, 72, seed=99)
    with Previewer(0, tonemapper='reinhard', lut_enabled=False) as pv:
        assert pv.original_size(128, 72, 48, 27) == (48, 27) and pv.original_size(36, 64, 48, 27) == (15, 27)
        outs = pv.original_batch([a, b, a2], 48, 27)
        assert [o.shape for o in outs] == [(27, 48, 3), (27, 15, 3), (27, 48, 3)]
        for fb, o in zip((a, b, a2), outs):
            assert np.array_equal(o, pv.original(fb, 48, 27))
            check_gate(o, ref.expected(fb, o.shape[1], o.shape[0])[0], 'mixed batch')
        one = pv.original_batch(_frames('odd47x26', 'smooth', 3), 'iw', 'ih', matrix='bt601', rgb='round8')
        assert len(one) == 3 and one[0].shape == (72, 128, 3)
        check_gate(np.stack(one), ref.expected(_frames('odd47x26', 'smooth', 3), 128, 72, 'bt601', 'round8'), 'iw:ih')


@pytest.mark.parametrize('pipeline', ['cpu', 'libplacebo'])
def test_pair_is_original_plus_convert(pipeline):
    fb = ref.synth_source('smooth', 1, 128, 72, seed=31)
    kw = dict(tonemapper='bt.2390', use_gpu=True, lut_enabled=False) if pipeline == 'libplacebo' else \
        dict(tonemapper='hable', lattice=_lattice())
    with Previewer(0, **kw) as pv:
        assert pv.params.resolved_pipeline() == pipeline
        for box in ((64, 27), (128, 72)):
            # the source pane is the aspect fit on both pipelines; libplacebo's converted pane is the box itself
            assert pv.original_size(128, 72, *box) == hdr2sdr.fit_size(128, 72, *box)
            state = pv._tm.peak_state()
            conv = pv.convert(fb, *box, gamma=1.2)
            orig = pv.original(fb, *box)
            assert pv._tm.peak_state() == state
            assert np.array_equal(pv.convert(fb, *box, gamma=1.2), conv)     # unchanged by original() in between
            check_gate(orig, ref.expected(fb, orig.shape[1], orig.shape[0])[0], f'{pipeline} original {box}')
            for src in (fb, fb.to_torch('cuda:0')):
                o, c = pv.pair(src, *box, gamma=1.2)
                assert np.array_equal(o, orig) and np.array_equal(c, conv)
            assert pv._tm.peak_state() == state
        o, c = pv.pair(fb, 64, 27, matrix='bt709', rgb='round8')
        assert np.array_equal(o, pv.original(fb, 64, 27, 'bt709', 'round8')) and np.array_equal(c, pv.convert(fb, 64, 27))


def test_original_needs_no_params_and_no_lut(tm):
    assert tm.params is None and tm.lut_size == 0
    fb = _frames('identity', 'smooth')
    check_gate(source_rgb(tm, fb, 64, 32)[0], _want('identity', 'smooth')[0], 'bare context')
    # ... while the converted pane on the same context refuses
    out = np.zeros((32, 64, 3), dtype=np.uint8)
    d = fb.descriptor()
    assert _abi.lib().h2s_preview_rgb24(tm._ctx, ctypes.byref(d), out.ctypes.data, 192, 64, 32, 1.0, _abi.LOC_HOST,
                                        None) == _abi.H2S_E_INVALID_ARG
