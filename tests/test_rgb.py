"""The RGB tensor output without a GPU: the gates of tests/rgb_ref.py accept the
float32 evaluation of the model and refuse three mutants of it; the ctypes
mirror of h2s_rgb_frames has the C layout; Tonemapper.process_rgb's argument
checks; hdr2sdr.plan.RgbReader's mechanics with a stand-in decode process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rgb_ref as ref
from hdr2sdr import _abi, engine
from hdr2sdr import plan as P
from hdr2sdr.synth import synth_frames

from test_abi_exports import HEADER, declared_functions
from test_plan import GOLD, PROPS10

W, H = 128, 64
NORMS = {'plain': ref.normalisation(), 'imagenet': ref.normalisation(ref.IMAGENET_MEAN, ref.IMAGENET_STD)}


def code_planes(kind, q):
    """(y, u, v) q-bit code planes of one 128 x 64 frame."""
    rng = np.random.default_rng(q * 31 + len(kind))
    top, s = (1 << q) - 1, 1 << (q - 8)
    shape = ((H, W), (H // 2, W // 2), (H // 2, W // 2))
    if kind == 'random':          # every code, legal or not
        return tuple(rng.integers(0, top + 1, size=sh) for sh in shape)
    if kind == 'legal':           # the limited range
        hi = (235 * s, 240 * s, 240 * s)
        return tuple(rng.integers(16 * s, h + 1, size=sh) for sh, h in zip(shape, hi))
    if kind == 'flat':
        return tuple(np.full(sh, c * s) for sh, c in zip(shape, (97, 140, 111)))
    # 'smooth' / 'edges': a synthetic frame's own 10-bit codes, at depth q
    fb = synth_frames(kind, 1, W, H, 10, device='cpu', seed=0x26B).to_numpy()
    y, u, v = (p[0] for p in ref.planes_of(fb.buf, W, H))
    return tuple(p >> (10 - q) if q <= 10 else p << (q - 10) for p in (y, u, v))


@pytest.mark.parametrize('q', [8, 10, 12])
@pytest.mark.parametrize('kind', ['random', 'legal', 'flat', 'smooth', 'edges'])
def test_the_gates_accept_the_float32_evaluation(kind, q):
    """Without fused multiply-adds: at q = 8 no byte differs; at q = 10 and 12
    a value of c / s that lies within float32's rounding of k + 0.5 may land on
    the other side (seen: 1 or 2 bytes of 24576, 0.008 % at the most, against
    the gate's 0.1 %); the float outputs lie within 1.9e-7 of the float64 ones
    (un-normalised: values in [0, 1])."""
    y, u, v = code_planes(kind, q)
    for name, (scale, bias) in NORMS.items():
        for dt in ref.DTYPES:
            if dt == 'uint8' and name != 'plain':
                continue
            want = ref.expected(y, u, v, q, dt, scale, bias)
            got = ref.expected(y, u, v, q, dt, scale, bias, dtype=np.float32)
            ok, figures = ref.gate(got, want, dt, scale, bias)
            print(f'{kind} q = {q} {dt} {name}: {figures}')
            assert ok, (kind, q, dt, name, figures)
            if dt == 'uint8' and q == 8:
                assert np.array_equal(got, want)
            elif dt == 'float32' and name == 'plain':
                assert np.abs(got - want).max() <= 1.9e-7


MUTANTS = {'chroma row y': dict(chroma_row='same'), 'bt601': dict(coeffs=ref.BT601), 'no luma offset': dict(luma_offset=False)}


@pytest.mark.parametrize('q', [8, 10])
@pytest.mark.parametrize('kind', ['smooth', 'edges'])
@pytest.mark.parametrize('mutant', sorted(MUTANTS))
def test_mutants_fail_every_gate(mutant, kind, q):
    y, u, v = code_planes(kind, q)
    scale, bias = NORMS['plain']
    for dt in ref.DTYPES:
        want = ref.expected(y, u, v, q, dt)
        got = ref.expected(y, u, v, q, dt, dtype=np.float32, **MUTANTS[mutant])
        ok, figures = ref.gate(got, want, dt, scale, bias)
        assert not ok, (mutant, kind, q, dt, figures)


def test_bfloat16_rounding_is_torchs():
    x = np.random.default_rng(5).uniform(-3, 3, 4096).astype(np.float32)
    x[:4] = (1.0, 1.00390625, 1.01171875, 0.0)        # exact, and the two ties
    assert np.array_equal(ref.to_bfloat16(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())


# ---- the struct and the exports ------------------------------------------------------------
PROBE = r'''
#include <stddef.h>
#include <stdio.h>
#include "h2s.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(h2s_rgb_frames), offsetof(h2s_rgb_frames, data),
         offsetof(h2s_rgb_frames, width), offsetof(h2s_rgb_frames, height), offsetof(h2s_rgb_frames, dtype),
         offsetof(h2s_rgb_frames, layout), offsetof(h2s_rgb_frames, row_pitch), offsetof(h2s_rgb_frames, plane_pitch),
         offsetof(h2s_rgb_frames, frame_pitch), offsetof(h2s_rgb_frames, scale), offsetof(h2s_rgb_frames, bias));
  printf("%d %d %d %d %d %d\n", H2S_RGB_U8, H2S_RGB_F16, H2S_RGB_BF16, H2S_RGB_F32, H2S_RGB_HWC, H2S_RGB_CHW);
  return 0;
}
'''


def test_struct_layout_matches_c(tmp_path):
    c = tmp_path / 'probe.c'
    c.write_text(PROBE)
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.dirname(HEADER), str(c), '-o', str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    F = _abi.H2SRgbFrames
    assert [int(v) for v in lines[0].split()] == [ctypes.sizeof(F)] + [getattr(F, n).offset for n, _ in F._fields_]
    assert [n for n, _ in F._fields_] == ['data', 'width', 'height', 'dtype', 'layout', 'row_pitch', 'plane_pitch',
                                          'frame_pitch', 'scale', 'bias']
    assert [int(v) for v in lines[1].split()] == [_abi.RGB_U8, _abi.RGB_F16, _abi.RGB_BF16, _abi.RGB_F32,
                                                  _abi.RGB_HWC, _abi.RGB_CHW]


def test_the_header_declares_the_call_and_python_binds_it():
    assert 'h2s_process_rgb' in declared_functions()
    assert declared_functions() == sorted(_abi.EXPORTS)
    L = _abi.lib()
    assert L.h2s_process_rgb.argtypes[2]._type_ is _abi.H2SRgbFrames
    assert L.h2s_process_rgb(None, None, None, 1, None) == _abi.H2S_E_INVALID_ARG
    assert (L.h2s_abi_version(), L.h2s_abi_minor()) == (3, 4)       # the symbol's presence is the feature test


# ---- process_rgb's argument checks, against a stub library ---------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def h2s_process_rgb(self, ctx, di, do, n, stream):
        d = do._obj
        self.calls.append(dict(n=n, w=d.width, h=d.height, dtype=d.dtype, layout=d.layout, row=d.row_pitch,
                               plane=d.plane_pitch, frame=d.frame_pitch, scale=list(d.scale), bias=list(d.bias),
                               data=d.data))
        return 0

    def h2s_set_frame_layout(self, *a):
        return 0

    h2s_set_input_subsampling = h2s_set_input_tags = h2s_set_frame_layout


class _StubTensor:
    """What rgb_frames reads of a torch tensor, with is_cuda set: the checks
    before the library call see a device tensor on a machine without one."""

    def __init__(self, t):
        self._t = t
        self.is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _stub_tonemapper():
    tm = object.__new__(engine.Tonemapper)
    tm._L, tm._ctx, tm.device = _StubLib(), ctypes.c_void_p(1), 0
    tm._layouts, tm._subsampling, tm._tags = ('planar', 'planar'), '420', ('tv', 'left')
    tm.close = lambda: None
    return tm


def _src(n=2, w=64, h=32):
    from hdr2sdr import FrameBatch
    return FrameBatch.empty_numpy(n, w, h, 10)


def test_process_rgb_builds_the_record_from_the_strides():
    tm, src = _stub_tonemapper(), _src()
    out = _StubTensor(torch.zeros((2, 3, 32, 64), dtype=torch.float16))
    assert tm.process_rgb(src, out=out, dtype='float16', mean=ref.IMAGENET_MEAN, std=ref.IMAGENET_STD) is out
    call = tm._L.calls[-1]
    assert (call['n'], call['w'], call['h'], call['dtype'], call['layout']) == (2, 64, 32, _abi.RGB_F16, _abi.RGB_CHW)
    assert (call['row'], call['plane'], call['frame']) == (128, 128 * 32, 3 * 128 * 32)
    scale, bias = ref.normalisation(ref.IMAGENET_MEAN, ref.IMAGENET_STD)
    assert call['scale'] == scale and call['bias'] == bias
    # a padded and sliced view, in place: HWC rows of 64 pixels in rows of 80, frames 40 rows apart
    base = torch.zeros((2, 40, 80, 3), dtype=torch.uint8)
    view = _StubTensor(base[:, 4:36, 8:72])
    tm.process_rgb(src, out=view, layout='hwc', dtype=torch.uint8)
    call = tm._L.calls[-1]
    assert (call['row'], call['frame'], call['dtype'], call['layout']) == (240, 40 * 240, _abi.RGB_U8, _abi.RGB_HWC)
    assert call['data'] == base.data_ptr() + 4 * 240 + 8 * 3
    assert call['scale'] == [1.0] * 3 and call['bias'] == [0.0] * 3
    # nframes below the batch, and a one-frame tensor whose frame stride says nothing
    one = _StubTensor(torch.zeros((3, 32, 64), dtype=torch.float32).unsqueeze(0))
    tm.process_rgb(src, out=one, dtype='float32', nframes=1)
    assert (tm._L.calls[-1]['n'], tm._L.calls[-1]['frame']) == (1, 3 * 32 * 64 * 4)


@pytest.mark.parametrize('case', [
    dict(dtype='int8'), dict(dtype=torch.float64), dict(layout='nchw'),
    dict(mean=(0.5, 0.5, 0.5)),                                    # uint8 takes no normalisation
    dict(dtype='float32', mean=(0.5, 0.5)), dict(dtype='float32', std=(1.0, 0.0, 1.0)),
    dict(dtype='float32', mean=(0.0, float('nan'), 0.0)), dict(dtype='float16', std=(1.0, float('inf'), 1.0)),
    dict(size=(63, 32)), dict(size=(64, 0)), dict(size=(64, 31)), dict(nframes=3),
])
def test_process_rgb_refuses_before_the_library_is_called(case):
    tm = _stub_tonemapper()
    with pytest.raises(ValueError):
        tm.process_rgb(_src(), **case)
    assert tm._L.calls == []


@pytest.mark.parametrize('make,kw', [
    (lambda: torch.zeros((2, 3, 32, 64)), dict(dtype='float16')),                              # another dtype
    (lambda: torch.zeros((2, 32, 64, 3), dtype=torch.uint8), dict(layout='chw')),                # another layout
    (lambda: torch.zeros((2, 3, 32, 64), dtype=torch.uint8), dict(layout='hwc')),
    (lambda: torch.zeros((3, 32, 64), dtype=torch.uint8), {}),                                   # not 4-D
    (lambda: torch.zeros((2, 3, 32, 128), dtype=torch.uint8)[..., ::2], {}),                     # innermost stride 2
    (lambda: torch.zeros((2, 32, 64, 4), dtype=torch.uint8)[..., :3], dict(layout='hwc')),       # RGBA pixels
    (lambda: torch.zeros((2, 3, 64, 32), dtype=torch.uint8).transpose(2, 3), {}),                # columns first
    (lambda: torch.zeros((1, 3, 32, 64), dtype=torch.uint8).expand(2, 3, 32, 64), {}),           # frames overlap
    (lambda: torch.zeros((2, 1, 32, 64), dtype=torch.uint8).expand(2, 3, 32, 64), {}),           # planes overlap
    (lambda: torch.zeros((2, 3, 32, 63), dtype=torch.uint8), {}),                                # odd width
    (lambda: torch.zeros((1, 3, 32, 64), dtype=torch.uint8), {}),                                # fewer frames than the batch
    (lambda: torch.zeros((2, 3, 32, 64), dtype=torch.uint8), dict(size=(32, 16))),               # size is not out's
])
def test_process_rgb_refuses_an_output_it_cannot_write_in_place(make, kw):
    tm = _stub_tonemapper()
    with pytest.raises(ValueError):
        tm.process_rgb(_src(), out=_StubTensor(make()), **kw)
    assert tm._L.calls == []


def test_process_rgb_refuses_a_host_tensor():
    tm = _stub_tonemapper()
    with pytest.raises(ValueError, match='device'):
        tm.process_rgb(_src(), out=torch.zeros((2, 3, 32, 64), dtype=torch.uint8))
    assert tm._L.calls == []


# ---- RgbReader's mechanics -----------------------------------------------------------------
FRAME = 64 * 32 * 3 // 2


class _FakeRgb:
    """Stand-in GPU stage: the first sample of each frame, and what it was asked."""

    def __init__(self):
        self.calls, self.kw = [], []

    def process_rgb(self, src, nframes=None, **kw):
        self.calls.append(nframes)
        self.kw.append(kw)
        return np.array(src.buf[:nframes, 0])


def _plan(tmp_path, frames, tail=''):
    pl = P.plan_from_argv(GOLD['C2']['argv'], dict(PROPS10, width=64, height=32))
    raw = tmp_path / 'in.raw'
    frames.tofile(raw)
    pl.decode = [sys.executable, '-c',
                 f'import sys; sys.stdout.buffer.write(open({str(raw)!r}, "rb").read()); sys.stdout.flush(); {tail}']
    return pl


def _numbered(n):
    return np.arange(n, dtype=np.uint16)[:, None] * 8 + np.zeros((1, FRAME), np.uint16)


@pytest.mark.parametrize('nframes', [0, 1, 4, 9])
def test_rgb_reader_yields_batches_in_decode_order(tmp_path, nframes):
    """batch = 4: no frame, one, exactly a batch, two batches and one frame."""
    tm = _FakeRgb()
    rd = P.RgbReader(_plan(tmp_path, _numbered(nframes)), tm, batch=4, dtype='float16', layout='hwc')
    got = list(rd)
    assert [len(g) for g in got] == [4] * (nframes // 4) + ([nframes % 4] if nframes % 4 else [])
    assert np.array_equal(np.concatenate(got) if got else np.zeros(0), np.arange(nframes) * 8)
    assert rd.frames == nframes and sum(tm.calls) == nframes
    assert all(kw == dict(dtype='float16', layout='hwc') for kw in tm.kw)
    assert rd.dec.returncode == 0 and not rd._reader.is_alive()          # reaped on exhaustion
    assert list(rd) == []


@pytest.mark.parametrize('depth', [1, 3])
def test_rgb_reader_keeps_the_order_under_read_ahead(tmp_path, depth):
    tm = _FakeRgb()
    with P.RgbReader(_plan(tmp_path, _numbered(23)), tm, batch=2, depth=depth) as rd:
        got = np.concatenate(list(rd))
    assert np.array_equal(got, np.arange(23) * 8) and tm.calls == [2] * 11 + [1]


def test_rgb_reader_delivers_the_plans_scaled_size(tmp_path):
    pl = _plan(tmp_path, _numbered(1))
    pl.out_width, pl.out_height = 32, 16
    tm = _FakeRgb()
    list(P.RgbReader(pl, tm))
    assert tm.kw == [dict(size=(32, 16))]
    tm = _FakeRgb()
    list(P.RgbReader(_plan(tmp_path, _numbered(1)), tm, size=(48, 24)))
    assert tm.kw == [dict(size=(48, 24))]


def test_rgb_reader_raises_a_gpu_error_and_reaps_the_child(tmp_path):
    class Boom:
        def process_rgb(self, *a, **k):
            raise RuntimeError('libh2s error -3: device lost')
    rd = P.RgbReader(_plan(tmp_path, _numbered(5)), Boom(), batch=1)
    with pytest.raises(RuntimeError, match='device lost'):
        next(rd)
    assert isinstance(rd.error, RuntimeError) and rd.dec.returncode is not None and not rd._reader.is_alive()
    assert list(rd) == []


def test_rgb_reader_raises_a_decode_failure_after_the_frames_it_got(tmp_path):
    tm = _FakeRgb()
    rd = P.RgbReader(_plan(tmp_path, _numbered(3), tail='sys.exit(3)'), tm, batch=2)
    assert len(next(rd)) == 2 and len(next(rd)) == 1
    with pytest.raises(RuntimeError, match='exit code 3'):
        next(rd)
    assert rd.dec.returncode == 3


def test_rgb_reader_closed_early_reaps_the_child(tmp_path):
    rd = P.RgbReader(_plan(tmp_path, _numbered(40)), _FakeRgb(), batch=1, depth=1)
    next(rd)
    rd.close()
    assert rd.dec.returncode is not None and not rd._reader.is_alive()
    rd.close()
