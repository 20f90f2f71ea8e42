"""The preview's source pane without a device: the float64 restatement's own
known answers (tests/source_preview_ref.py), PIL's high-byte read of a 16-bit
PNG (which pins the TRUNC16 output model), ``source_box`` and the argument
handling of h2s_preview_source_rgb24 / _batch that needs no context."""
import ctypes
import io
import struct
import zlib
from fractions import Fraction

import numpy as np
import pytest

import hdr2sdr
import source_preview_ref as ref
from hdr2sdr import _abi
from hdr2sdr.preview import source_box

SIZES = [(64, 32, 64, 32), (66, 34, 66, 34), (128, 72, 48, 27), (128, 72, 47, 26), (32, 18, 80, 45),
         (36, 64, 20, 36), (384, 16, 32, 16)]


# ---- the restatement's known answers ----------------------------------------------
@pytest.mark.parametrize('bits', [10, 12])
@pytest.mark.parametrize('matrix', ref.MATRICES)
def test_limited_range_white_black_and_grey(bits, matrix):
    s = 1 << (bits - 8)
    mid = 1 << (bits - 1)
    for code, v in ((235 * s, Fraction(1)), (16 * s, Fraction(0)), (126 * s, Fraction(110, 219))):
        fb = ref.flat_frame(16, 8, bits, code, mid, mid)
        want16 = (65535 * v + Fraction(1, 2)).__floor__()
        want8 = (255 * v + Fraction(1, 2)).__floor__()
        assert np.all(ref.expected(fb, 16, 8, matrix, 'trunc16') == want16 >> 8)
        assert np.all(ref.expected(fb, 16, 8, matrix, 'round8') == want8)
    # (white, black, grey) -> (255, 0, 128) in both models
    assert [((65535 * v + Fraction(1, 2)).__floor__() >> 8, (255 * v + Fraction(1, 2)).__floor__())
            for v in (Fraction(1), Fraction(0), Fraction(110, 219))] == [(255, 255), (0, 0), (128, 128)]


def test_full_range_ends():
    for bits in (10, 12):
        top, mid = (1 << bits) - 1, 1 << (bits - 1)
        assert np.all(ref.expected(ref.flat_frame(16, 8, bits, top, mid, mid, color_range='pc'), 16, 8) == 255)
        assert np.all(ref.expected(ref.flat_frame(16, 8, bits, 0, mid, mid, color_range='pc'), 16, 8) == 0)
        # the limited reading of the same codes clips instead
        assert np.all(ref.expected(ref.flat_frame(16, 8, bits, 16 << (bits - 8), mid, mid, color_range='pc'), 16, 8) > 0)


@pytest.mark.parametrize('W,H,ow,oh', SIZES)
def test_flat_field_survives_every_resize(W, H, ow, oh):
    fb = ref.flat_frame(W, H, 10, 500, 400, 600)
    same = ref.expected16(ref.flat_frame(16, 8, 10, 500, 400, 600), 16, 8)[0, 0, 0]
    got = ref.expected16(fb, ow, oh)
    assert got.shape == (1, oh, ow, 3)
    assert np.all(got == same)


def test_resize_matrix_is_normalised_and_the_identity_at_equal_size():
    for src, dst in ((64, 64), (36, 20), (128, 47), (18, 45), (384, 32), (16, 32)):
        M = ref.resize_matrix(src, dst)
        assert np.allclose(M.sum(axis=1), 1.0, atol=1e-14)
    assert np.allclose(ref.resize_matrix(64, 64), np.eye(64), atol=1e-15)
    # ratio 12: ceil(4 * 12) + 1 = 49 taps, all inside one row's support
    assert (ref.resize_matrix(384, 32)[16] != 0).sum() <= 49


def test_saturated_patch_separates_the_matrices():
    fb = ref.flat_frame(16, 8, 10, 400, 800, 300)
    out = {m: ref.expected(fb, 16, 8, m)[0, 0, 0].astype(int) for m in ref.MATRICES}
    for a, b in (('bt2020nc', 'bt709'), ('bt2020nc', 'bt601'), ('bt709', 'bt601')):
        assert np.abs(out[a] - out[b]).max() >= 3, (a, b, out)
    # BT.2020: R = Y' + 1.4746 Cr, B = Y' + 1.8814 Cb, by hand
    Y, Cb, Cr = (400 - 64) / 876, (800 - 512) / 896, (300 - 512) / 896
    R, B = Y + 1.4746 * Cr, Y + 1.8814 * Cb
    G = (Y - 0.2627 * R - 0.0593 * B) / 0.678
    want = [int(np.floor(65535 * min(max(c, 0.0), 1.0) + 0.5)) >> 8 for c in (R, G, B)]
    assert out['bt2020nc'].tolist() == want


def test_trunc16_and_round8_differ_where_they_should():
    # 0.1: 6554 >> 8 = 25 but floor(26.0) = 26; 0.99: 64880 >> 8 = 253 but floor(252.95) = 252;
    # the two agree about the middle (255.996 v = 255 v + 0.5 at v = 0.502)
    v = np.array([0.0, 0.1, 0.4985, 0.5, 0.99, 1.0])
    assert ref.quantise(v, 'trunc16').tolist() == [0, 25, 127, 128, 253, 255]
    assert ref.quantise(v, 'round8').tolist() == [0, 26, 127, 128, 252, 255]
    ramp = np.linspace(0.0, 1.0, 4097)
    a, b = ref.quantise(ramp, 'trunc16').astype(int), ref.quantise(ramp, 'round8').astype(int)
    assert np.abs(a - b).max() == 1 and 0.2 < (a != b).mean() < 0.8


# ---- PIL's read of a 16-bit RGB PNG: the high byte ------------------------------------
def _png16(samples):
    """[h, w, 3] 16-bit samples -> the bytes of an RGB PNG of bit depth 16."""
    h, w, _ = samples.shape
    raw = b''.join(b'\x00' + samples[r].astype('>u2').tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data))
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 16, 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(raw)) + chunk(b'IEND', b''))


def test_pil_opens_a_16_bit_rgb_png_by_its_high_bytes():
    Image = pytest.importorskip('PIL.Image')
    s = np.array([[[0x807f, 0xfe80, 0x00ff], [0xffff, 0x0100, 0x7fff]],
                  [[0x8000, 0x80ff, 0xff00], [0x1234, 0xabcd, 0x00]]], dtype=np.uint16)
    img = Image.open(io.BytesIO(_png16(s)))
    got = np.asarray(img.convert('RGB'))
    assert got.dtype == np.uint8
    assert np.array_equal(got, (s >> 8).astype(np.uint8))
    assert got[0, 0, 0] == 128 and got[0, 0, 1] == 254


# ---- source_box ---------------------------------------------------------------------
def test_source_box_parses_the_references_scale():
    assert source_box(None) == ('iw', 'ih')
    assert source_box('scale=3840:2160:force_original_aspect_ratio=decrease') == (3840, 2160)
    assert source_box('scale=960:540:force_original_aspect_ratio=decrease') == (960, 540)
    assert hdr2sdr.source_box is source_box


@pytest.mark.parametrize('vf', [
    'scale=960:540', 'scale=960:540:force_original_aspect_ratio=increase', 'scale=960',
    'scale=0:540:force_original_aspect_ratio=decrease', 'scale=-1:540:force_original_aspect_ratio=decrease',
    'scale=960:540:force_original_aspect_ratio=decrease,eq=gamma=1.2', 'zscale=t=linear', '',
    'scale=960:540:force_original_aspect_ratio=decrease:flags=lanczos',
])
def test_source_box_refuses_anything_else(vf):
    with pytest.raises(ValueError):
        source_box(vf)


# ---- the entry points with no context ---------------------------------------------------
def test_null_context_is_invalid_arg():
    L = _abi.lib()
    fb = hdr2sdr.FrameBatch.empty_numpy(1, 16, 8, 10)
    d = fb.descriptor()
    out = np.zeros((8, 16, 3), dtype=np.uint8)
    assert L.h2s_preview_source_rgb24(None, ctypes.byref(d), out.ctypes.data, 48, 16, 8, _abi.SRC_MATRIX_BT2020NC,
                                      _abi.SRC_RGB_TRUNC16, _abi.LOC_HOST, None) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_preview_source_rgb24_batch(None, ctypes.byref(d), 1, out.ctypes.data, 48, 48 * 8, 16, 8,
                                            _abi.SRC_MATRIX_BT2020NC, _abi.SRC_RGB_TRUNC16, _abi.LOC_HOST,
                                            None) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_preview_source_rgb24(None, None, None, 0, 0, 0, 0, 0, 0, None) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_last_error(None)
    assert not out.any()


def test_bindings_name_the_enums_and_exports():
    assert 'h2s_preview_source_rgb24' in _abi.EXPORTS and 'h2s_preview_source_rgb24_batch' in _abi.EXPORTS
    assert _abi.SRC_MATRICES == {'bt2020nc': 0, 'bt709': 1, 'bt601': 2}
    assert _abi.SRC_RGB_MODELS == {'trunc16': 0, 'round8': 1}
    assert tuple(_abi.SRC_MATRICES) == ref.MATRICES and tuple(_abi.SRC_RGB_MODELS) == ref.RGB_MODELS


def test_python_refuses_unknown_names_before_any_call():
    from hdr2sdr.preview import source_rgb
    fb = hdr2sdr.FrameBatch.empty_numpy(1, 16, 8, 10)
    with pytest.raises(ValueError):
        source_rgb(None, fb, 16, 8, matrix='bt470bg')
    with pytest.raises(ValueError):
        source_rgb(None, fb, 16, 8, rgb='rgb48')


# ---- the GPU gate is reachable by the reference arithmetic alone ---------------------------
@pytest.mark.parametrize('kind', ref.CONTENTS)
@pytest.mark.parametrize('case', ref.CASES, ids=[c[0] for c in ref.CASES])
def test_float32_restatement_meets_the_gpu_gate(case, kind):
    fb = ref.case_frames(case, kind)
    ow, oh = ref.case_size(case)
    for matrix in ref.MATRICES:
        for rgb in ref.RGB_MODELS:
            want = ref.expected(fb, ow, oh, matrix, rgb)
            got = ref.expected(fb, ow, oh, matrix, rgb, dtype=np.float32)
            mx, frac = ref.gate(got, want)
            print(f'{case[0]} {kind} {matrix} {rgb}: max {mx}, {frac:.4%} differ')
            assert mx <= ref.MAX_DIFF and frac <= ref.MAX_FRACTION


def test_flat_codes_exist_for_every_depth_and_range():
    for bits in (10, 12):
        for rng in ('tv', 'pc'):
            y, cb, cr = ref.flat_codes(bits, rng)
            assert 16 << (bits - 8) <= y <= 235 << (bits - 8) and cb != cr
            for matrix in ref.MATRICES:
                v = ref.expected16(ref.flat_frame(66, 34, bits, y, cb, cr, color_range=rng), 47, 26, matrix)
                assert np.all(v == v[0, 0, 0]) and np.all((v % 256 >= 8) & (v % 256 <= 247))


def test_case_sizes():
    by_id = {c[0]: c for c in ref.CASES}
    assert ref.case_size(by_id['box48x27']) == (48, 27)
    assert ref.case_size(by_id['portrait']) == (20, 36)
    assert ref.case_size(by_id['odd47x26']) == (47, 26)
