"""The rendition ladder's host side without a GPU: plan_ladder against
plan_from_argv on the reference's own argv goldens, H2SLadderProcess's pipe
mechanics with stand-in processes and a stub GPU stage, the Python argument
checks of Tonemapper.process_ladder, and the new symbol in the header, the
binding and the library."""
import ctypes
import dataclasses
import json
import os
import re
import sys

import numpy as np
import pytest

from hdr2sdr import FrameBatch, Tonemapper, _abi
from hdr2sdr import plan as P

from conftest import REPO

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'filter_chains.json')))
PROPS10 = {'width': 3840, 'height': 2160, 'bit_depth': 10, 'color_transfer': 'smpte2084', 'frame_rate': 24.0}
BOXES = [None, (1920, 1080), (1280, 720), (640, 360)]     # the source size and three boxes


def rung_argv(cfg, i):
    """The reference's argv for rung i: its own output path and rate argument."""
    argv = [t.replace('out.mkv', f'out_{i}.mkv') for t in GOLD[cfg]['argv']]
    assert argv[-2:] == [f'out_{i}.mkv', '-y']
    return argv[:-2] + ['-maxrate', f'{8 >> i}M'] + argv[-2:]


# ---- plan_ladder ---------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', ['C2', 'C3', 'default8'])
def test_plan_ladder_is_plan_from_argv_per_rung(cfg):
    argvs = [rung_argv(cfg, i) for i in range(len(BOXES))]
    kw = dict(hdr={'maxcll': 1000.0}, out_layout='auto')
    lp = P.plan_ladder(argvs, PROPS10, BOXES, **kw)
    assert len(lp.rungs) == len(BOXES)
    for i, (argv, box) in enumerate(zip(argvs, BOXES)):
        want = P.plan_from_argv(argv, PROPS10, scale=box, **kw)
        got = lp.rungs[i]
        for f in dataclasses.fields(P.PipePlan):
            a, b = getattr(got, f.name), getattr(want, f.name)
            assert repr(a) == repr(b), (i, f.name)
        assert got.output_path == f'out_{i}.mkv'
    assert lp.decode == lp.rungs[0].decode == lp.rungs[3].decode
    assert lp.sizes == [(3840, 2160), (1920, 1080), (1280, 720), (640, 360)]
    assert lp.frame_bytes_in == 3840 * 2160 * 3
    assert repr(lp.params) == repr(lp.rungs[2].params)


def test_plan_ladder_argument_shapes():
    a = rung_argv('C2', 0)
    with pytest.raises(ValueError):
        P.plan_ladder([], PROPS10, [])
    with pytest.raises(ValueError):
        P.plan_ladder([a, a], PROPS10, [None])
    with pytest.raises(ValueError):
        P.plan_ladder([a] * 9, PROPS10, [None] * 9)
    with pytest.raises(ValueError):
        P.plan_ladder([a], PROPS10, [None], scale=(1920, 1080))
    assert len(P.plan_ladder([a] * 8, PROPS10, [None] * 8).rungs) == 8      # duplicates are fine


def _swap(argv, old, new):
    assert any(old in t for t in argv)
    return [t.replace(old, new) for t in argv]


@pytest.mark.parametrize('field,mutate', [
    ('input_path', lambda a: _swap(a, 'in.mkv', 'other.mkv')),
    ('params', lambda a: _swap(a, 'tonemap=hable', 'tonemap=mobius')),
    ('params', lambda a: _swap(a, 'yuv420p10le', 'yuv420p')),                 # another output depth
    ('lut_path', lambda a: _swap(a, 'file=<LUT>', 'file=other.cube')),
], ids=['input', 'tonemapper', 'depth', 'lut'])
def test_plan_ladder_names_the_rung_and_field_that_disagree(field, mutate):
    good = rung_argv('C2', 0)
    bad = mutate(rung_argv('C2', 2))
    with pytest.raises(ValueError) as e:
        P.plan_ladder([good, rung_argv('C2', 1), bad], PROPS10, [None, (1920, 1080), (1280, 720)])
    assert 'rung 2' in str(e.value) and field in str(e.value)


def test_plan_ladder_refuses_rungs_of_differing_layout():
    """out_layout='auto' is semi exactly for -pix_fmt p010le: such a rung beside planar ones."""
    good = rung_argv('C2', 0)
    bad = _swap(rung_argv('C2', 1), 'yuv420p10le', 'p010le')
    with pytest.raises(ValueError) as e:
        P.plan_ladder([good, bad], PROPS10, [None, (1920, 1080)], out_layout='auto')
    assert 'rung 1' in str(e.value) and 'layout' in str(e.value)


# ---- H2SLadderProcess ----------------------------------------------------------------------
W, H = 64, 32
SIZES = [(64, 32), (32, 16), (16, 8)]


class _StubLadder:
    """Stand-in GPU stage: rung i's frame f is filled with (first sample of source frame f) + i."""

    def __init__(self):
        self.calls = []

    def process_ladder(self, src, dsts, nframes=None, stream=None):
        self.calls.append(nframes)
        for i, d in enumerate(dsts):
            d.buf[:nframes] = src.buf[:nframes, :1] + i


def _fake_ladder(tmp_path, frames):
    lp = P.plan_ladder([rung_argv('C2', i) for i in range(3)], dict(PROPS10, width=W, height=H),
                       [None, (32, 16), (16, 8)])
    assert lp.sizes == SIZES
    raw = tmp_path / 'in.raw'
    frames.tofile(raw)
    lp.decode = [sys.executable, '-c', f'import sys; sys.stdout.buffer.write(open({str(raw)!r}, "rb").read())']
    outs = []
    for i, r in enumerate(lp.rungs):
        out = tmp_path / f'out_{i}.raw'
        r.encode = [sys.executable, '-c',
                    f'import sys; d = sys.stdin.buffer.read(); open({str(out)!r}, "wb").write(d); '
                    f'sys.stderr.write("rung {i} time=00:00:00.12\\n")']
        outs.append(out)
    return lp, outs


@pytest.mark.parametrize('nframes,batch', [(5, 2), (4, 4), (1, 8), (0, 3)])
def test_ladder_executor_feeds_every_encoder_its_own_rung(tmp_path, nframes, batch):
    frames = np.arange(nframes, dtype=np.uint16)[:, None] * 8 + np.zeros((1, W * H * 3 // 2), np.uint16)
    lp, outs = _fake_ladder(tmp_path, frames)
    tm = _StubLadder()
    proc = P.H2SLadderProcess(lp, tm, batch=batch)
    lines = list(proc.stderr)
    assert proc.wait(timeout=60) == 0 and proc.error is None
    assert any('rung 0 time=' in ln for ln in lines)            # stderr is rung 0's encoder
    for i, ((w, h), out) in enumerate(zip(SIZES, outs)):
        assert lp.rungs[i].frame_bytes_out == w * h * 3
        got = np.fromfile(out, dtype=np.uint16)
        assert got.size == nframes * w * h * 3 // 2              # exactly frames x frame_bytes_out
        got = got.reshape(nframes, w * h * 3 // 2)
        assert np.array_equal(got, np.arange(nframes, dtype=np.uint16)[:, None] * 8 + i + np.zeros_like(got))
    assert proc.frames == nframes and sum(tm.calls) == nframes
    if nframes == 5:
        assert tm.calls == [2, 2, 1]                             # one call per batch, the last one short


def test_ladder_executor_reports_gpu_failure_and_kills_everything(tmp_path):
    lp, _ = _fake_ladder(tmp_path, np.zeros((2, W * H * 3 // 2), np.uint16))
    killed = []

    class Boom:
        def process_ladder(self, *a, **k):
            raise RuntimeError('libh2s error -3: device lost')

    def popen(argv, **kw):
        import subprocess
        p = subprocess.Popen(argv, **kw)
        kill = p.kill
        p.kill = lambda: (killed.append(p), kill())[1]
        return p

    proc = P.H2SLadderProcess(lp, Boom(), batch=1, popen=popen)
    list(proc.stderr)
    assert proc.wait(timeout=60) == 1 and isinstance(proc.error, RuntimeError)
    assert set(killed) == set([proc.dec] + proc.encs) and len(proc.encs) == 3
    assert proc.returncode == 1 and proc.poll() == 1


def test_ladder_executor_returncode_is_the_first_failing_encoder(tmp_path):
    frames = np.zeros((2, W * H * 3 // 2), np.uint16)
    lp, _ = _fake_ladder(tmp_path, frames)
    lp.rungs[1].encode = [sys.executable, '-c', 'import sys; sys.stdin.buffer.read(); sys.exit(3)']
    lp.rungs[2].encode = [sys.executable, '-c', 'import sys; sys.stdin.buffer.read(); sys.exit(4)']
    proc = P.H2SLadderProcess(lp, _StubLadder(), batch=2)
    list(proc.stderr)
    assert proc.wait(timeout=60) == 3 and proc.error is None


# ---- Tonemapper.process_ladder: the checks come before the library -----------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f'the library was called ({name})')


def _tonemapper_without_library():
    tm = Tonemapper.__new__(Tonemapper)
    tm._L, tm._ctx = _NoLibrary(), ctypes.c_void_p()
    tm._layouts, tm._subsampling, tm._tags, tm._decimation = ('planar', 'planar'), '420', ('tv', 'left'), 'off'
    return tm


def test_process_ladder_validates_before_any_library_call():
    tm = _tonemapper_without_library()
    src = FrameBatch.empty_numpy(2, 64, 32, 10)

    def rung(w=32, h=16, n=2, bits=10, layout='planar', odd=False):
        r = FrameBatch.empty_numpy(n, w, h, bits, layout)
        if odd:             # (FrameBatch itself refuses an odd size: a foreign batch object may not)
            r.height -= 1
        return r

    bad = [
        [],                                        # no rung
        [rung()] * (_abi.LADDER_MAX + 1),          # too many
        [rung(), rung(n=1)],                       # a rung shorter than the batch
        [rung(), rung(odd=True)],                  # odd
        [rung(), rung(layout='semi')],             # layouts differ
        [rung(), rung(bits=8)],                    # depths differ
    ]
    for dsts in bad:
        with pytest.raises(ValueError):
            tm.process_ladder(src, dsts)
    with pytest.raises(ValueError):
        tm.process_ladder(src, [rung(), rung()], nframes=3)
    with pytest.raises(ValueError) as e:
        tm.process_ladder(src, [rung(), rung(), rung(odd=True)])
    assert 'rung 2' in str(e.value)
    # a good call does reach the library
    with pytest.raises(AssertionError):
        tm.process_ladder(src, [rung(64, 32), rung()])
    tm._ctx = None      # (nothing to destroy)


def test_ladder_needs_params():
    tm = _tonemapper_without_library()
    tm.params = None
    with pytest.raises(ValueError):
        tm.ladder(FrameBatch.empty_numpy(1, 64, 32, 10), [(32, 16)])
    tm._ctx = None


# ---- the symbol ----------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(REPO, 'include', 'h2s.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'^int h2s_process_ladder\(h2s_ctx \*ctx, const h2s_frames \*in, const h2s_frames \*outs,\s*'
                     r'int n_outs, int nframes, void \*hip_stream\);', code, flags=re.M)
    assert re.search(r'#define\s+H2S_LADDER_MAX\s+8\b', code) and _abi.LADDER_MAX == 8
    assert re.search(r'#define\s+H2S_OPT_TEST_LADDER_UPLOADS\s+\(H2S_OPT_PRIVATE_BASE \+ 6\)', code)
    assert _abi.OPT_TEST_LADDER_UPLOADS == 0x7f000000 + 6
    assert re.search(r'#define H2S_ABI_VERSION 3\b', code) and re.search(r'#define H2S_ABI_MINOR 4\b', code)
    assert 'h2s_process_ladder' in re.search(r'Added within 3\.4.*?\*/', header, flags=re.S).group(0)
    assert 'h2s_process_ladder' in _abi.EXPORTS
    L = _abi.lib()
    assert L.h2s_process_ladder.argtypes[3:5] == [ctypes.c_int, ctypes.c_int]
    # NULL handling needs no device
    assert L.h2s_process_ladder(None, None, None, 2, 1, None) == _abi.H2S_E_INVALID_ARG
