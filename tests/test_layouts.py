"""Semi-planar frame layouts (nv12 / p010le / p012le) on the host side: the
FrameBatch views and repack helper, the C descriptor, the new export's
argument check, the planner's pipe formats and the executor's byte counts with
stand-in processes.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

from hdr2sdr import _abi
from hdr2sdr import plan as P
from hdr2sdr.frames import FrameBatch

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'filter_chains.json')))
PROPS10 = {'width': 3840, 'height': 2160, 'bit_depth': 10, 'color_transfer': 'smpte2084', 'frame_rate': 24.0}

W, H, F = 16, 8, 3


def _planar(bits, seed=0):
    rng = np.random.default_rng(seed)
    fb = FrameBatch.empty_numpy(F, W, H, bits)
    fb.buf[...] = rng.integers(0, 1 << bits, size=fb.buf.shape, dtype=np.uint16).astype(fb.buf.dtype)
    return fb


@pytest.mark.parametrize('bits', [8, 10, 12])
def test_to_layout_round_trip(bits):
    pl = _planar(bits, seed=bits)
    assert pl.layout == 'planar' and pl.to_layout('planar') is pl
    sp = pl.to_layout('semi')
    assert sp.layout == 'semi' and sp.buf.shape == pl.buf.shape and sp.buf.dtype == pl.buf.dtype
    sh = 0 if bits == 8 else 16 - bits
    assert sp.uv.shape == (F, H // 2, W // 2, 2)
    assert np.array_equal(sp.y, pl.y.astype(np.uint32) << sh)
    assert np.array_equal(sp.uv[..., 0], sp.u) and np.array_equal(sp.uv[..., 1], sp.v)
    assert np.array_equal(sp.u, pl.u.astype(np.uint32) << sh)
    assert np.array_equal(sp.v, pl.v.astype(np.uint32) << sh)
    if bits == 10:
        assert np.array_equal(sp.uv[..., 0], pl.u.astype(np.uint32) << 6)
    # the interleaved plane follows the Y plane: Cb, Cr, Cb, Cr ... per row
    row = sp.buf[1, W * H:W * H + W]
    assert np.array_equal(row[0::2], sp.u[1, 0]) and np.array_equal(row[1::2], sp.v[1, 0])
    back = sp.to_layout('planar')
    assert back.layout == 'planar' and np.array_equal(back.buf, pl.buf)
    # u / v of a semi batch are views: writing them writes the interleaved plane
    sp.u[0, 0, 0] = 0
    assert sp.uv[0, 0, 0, 0] == 0


def test_to_layout_drops_low_bits_and_rejects_unknown():
    pl = _planar(10, seed=5)
    sp = pl.to_layout('semi')
    sp.buf[...] |= 0x3F       # junk below the code
    assert np.array_equal(sp.to_layout('planar').buf, pl.buf)
    with pytest.raises(ValueError):
        pl.to_layout('packed')
    with pytest.raises(ValueError):
        FrameBatch(pl.buf, W, H, 10, 'packed')
    with pytest.raises(ValueError):
        pl.uv


def test_to_layout_torch_matches_numpy():
    torch = pytest.importorskip('torch')
    for bits in (8, 10, 12):
        pl = _planar(bits, seed=20 + bits)
        want = pl.to_layout('semi')
        t = pl.to_torch('cpu')
        got = t.to_layout('semi')
        assert got.layout == 'semi' and got.is_torch
        assert np.array_equal(got.to_numpy().buf, want.buf)
        assert got.to_numpy().layout == 'semi'
        assert np.array_equal(got.to_layout('planar').to_numpy().buf, pl.buf)
        assert isinstance(got.u, torch.Tensor) and tuple(got.uv.shape) == (F, H // 2, W // 2, 2)


def test_constructors_and_slice_keep_the_layout():
    assert FrameBatch.empty_numpy(2, W, H, 10).layout == 'planar'
    fb = FrameBatch.empty_numpy(4, W, H, 10, 'semi')
    assert fb.layout == 'semi' and fb.slice(1, 3).layout == 'semi' and fb.slice(1, 3).nframes == 2
    assert FrameBatch.empty_pinned(2, W, H, 8, 'semi').layout == 'semi'
    assert FrameBatch.empty_numpy(2, W, H, 12, layout='semi').to_torch('cpu').layout == 'semi'
    # positional construction as before the field existed
    assert FrameBatch(fb.buf, W, H, 10).layout == 'planar'


@pytest.mark.parametrize('bits', [8, 10, 12])
def test_semi_descriptor(bits):
    fb = FrameBatch.empty_numpy(F, W, H, bits, 'semi')
    d = fb.descriptor()
    bps = 1 if bits == 8 else 2
    base = fb.buf.ctypes.data
    assert d.data[0] == base and d.data[1] == base + W * H * bps
    assert d.linesize[0] == W * bps and d.linesize[1] == W * bps
    assert d.frame_pitch[0] == d.frame_pitch[1] == W * H * bps * 3 // 2
    assert not d.data[2] and d.linesize[2] == 0 and d.frame_pitch[2] == 0
    assert (d.width, d.height, d.bits) == (W, H, bits)
    # the planar descriptor is what it was
    dp = FrameBatch.empty_numpy(F, W, H, bits).descriptor()
    assert dp.linesize[1] == dp.linesize[2] == W // 2 * bps and dp.data[2]


def test_set_frame_layout_export():
    L = _abi.lib()
    assert 'h2s_set_frame_layout' in _abi.EXPORTS
    assert (_abi.LAYOUT_PLANAR, _abi.LAYOUT_SEMI) == (0, 1)
    assert L.h2s_set_frame_layout(None, 0, 0) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_set_frame_layout(None, 1, 1) == _abi.H2S_E_INVALID_ARG
    # an addition inside ABI 3.4: the symbol is the feature test
    assert (L.h2s_abi_version(), L.h2s_abi_minor()) == (3, 4)


def _p010_argv():
    argv = list(GOLD['C2']['argv'])
    argv[argv.index('-pix_fmt') + 1] = 'p010le'
    return argv


def test_plan_layouts_on_a_p010le_request():
    argv = _p010_argv()
    pl = P.plan_from_argv(argv, PROPS10)      # the default: today's argv
    enc = pl.encode
    assert enc[enc.index('-pix_fmt') + 1] == 'yuv420p10le' and pl.layout == 'planar' and pl.in_layout == 'planar'
    assert pl.decode[-2] == 'yuv420p10le'
    assert enc.count('p010le') == 1      # the encoder's own -pix_fmt, as the reference chose it
    auto = P.plan_from_argv(argv, PROPS10, out_layout='auto')
    assert auto.encode[auto.encode.index('-pix_fmt') + 1] == 'p010le' and auto.layout == 'semi'
    assert auto.in_layout == 'planar' and auto.decode == pl.decode
    assert auto.encode[:auto.encode.index('-pix_fmt') + 1] == enc[:enc.index('-pix_fmt') + 1]
    assert auto.encode[auto.encode.index('-pix_fmt') + 2:] == enc[enc.index('-pix_fmt') + 2:]
    assert auto.frame_bytes_out == pl.frame_bytes_out
    # a planar request stays planar under 'auto' (in_layout 'auto' is planar)
    same = P.plan_from_argv(GOLD['C2']['argv'], PROPS10, in_layout='auto', out_layout='auto')
    base = P.plan_from_argv(GOLD['C2']['argv'], PROPS10)
    assert (same.decode, same.encode, same.layout, same.in_layout) == (base.decode, base.encode, 'planar', 'planar')
    # explicit layouts on both sides, every depth's pipe name
    semi = P.plan_from_argv(argv, PROPS10, in_layout='semi', out_layout='semi')
    assert semi.decode[-2] == 'p010le' and semi.in_layout == 'semi' and semi.layout == 'semi'
    semi12 = P.plan_from_argv(GOLD['C5']['argv'], dict(PROPS10, bit_depth=12, color_transfer='arib-std-b67'),
                              in_layout='semi', out_layout='semi')
    assert semi12.decode[-2] == 'p012le'
    assert semi12.encode[semi12.encode.index('-pix_fmt') + 1] == 'p012le'
    semi8 = P.plan_from_argv(GOLD['default8']['argv'], PROPS10, out_layout='semi')
    assert semi8.encode[semi8.encode.index('-pix_fmt') + 1] == 'nv12' and semi8.decode[-2] == 'yuv420p10le'
    with pytest.raises(ValueError):
        P.plan_from_argv(argv, PROPS10, out_layout='packed')


class _CopyTonemapper:
    """Stand-in GPU stage: records the batches' layouts, copies the words."""

    def __init__(self):
        self.layouts = set()
        self.frames = 0

    def process(self, src, dst, stream=None, nframes=None):
        self.layouts.add((src.layout, dst.layout))
        self.frames += nframes
        dst.buf[:nframes] = src.buf[:nframes]


@pytest.mark.parametrize('layouts', [('planar', 'auto'), ('semi', 'semi'), ('semi', 'planar')])
def test_pipe_executor_byte_counts_with_layouts(tmp_path, layouts):
    """The executor's staging batches carry the plan's layouts, and a frame is
    the same number of bytes on the pipe in either layout."""
    w, h, n = 64, 32, 5
    pl = P.plan_from_argv(_p010_argv(), dict(PROPS10, width=w, height=h), in_layout=layouts[0], out_layout=layouts[1])
    want_out = 'semi' if layouts[1] in ('semi', 'auto') else 'planar'
    assert (pl.in_layout, pl.layout) == (layouts[0], want_out)
    assert pl.frame_bytes_in == pl.frame_bytes_out == w * h * 3
    frames = np.random.default_rng(3).integers(0, 1 << 16, size=(n, w * h * 3 // 2), dtype=np.uint16)
    raw, out = tmp_path / 'in.raw', tmp_path / 'out.raw'
    frames.tofile(raw)
    pl.decode = [sys.executable, '-c', f'import sys; sys.stdout.buffer.write(open({str(raw)!r}, "rb").read())']
    pl.encode = [sys.executable, '-c', f'import sys; open({str(out)!r}, "wb").write(sys.stdin.buffer.read())']
    tm = _CopyTonemapper()
    proc = P.H2SProcess(pl, tm, batch=2)
    list(proc.stderr)
    assert proc.wait(timeout=60) == 0
    assert os.path.getsize(out) == n * pl.frame_bytes_out
    assert np.array_equal(np.fromfile(out, dtype=np.uint16).reshape(n, -1), frames)
    assert tm.layouts == {(layouts[0], want_out)} and tm.frames == proc.frames == n
