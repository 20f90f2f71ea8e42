"""A source's full-range and top-left chroma tags (h2s_set_input_tags), the
parts that need no GPU: the test constructions themselves
(tests/source_tags_ref.py), FrameBatch, the planner, the engine's use of the
setter and the ABI."""
import ctypes
import re

import numpy as np
import pytest

import hdr2sdr
import oracle
import source_tags_ref as TR
import subsampling_ref as SR
import test_oracle_independent as toi
from hdr2sdr import _abi
from hdr2sdr import plan as P
from hdr2sdr.frames import FrameBatch
from hdr2sdr.synth import synth_frames
from test_plan import GOLD, PROPS10

TM = {'reinhard': 4, 'hable': 5, 'mobius': 6}


# ---- the constructions' own identities ----------------------------------------
@pytest.mark.parametrize('edge', SR.EDGES)
def test_topleft_equals_the_422_model_of_the_paired_plane(edge):
    rng = np.random.default_rng(3)
    c = 2 * rng.integers(32, 480, size=(2, 9, 7))
    p = TR.vpair(c, edge)
    assert p.shape == (2, 18, 7) and np.array_equal(p[:, 0::2], c)
    dn = c[:, SR.edge_index(np.arange(9) + 1, 9, edge)]
    assert np.array_equal(2 * p[:, 1::2], c + dn)
    tl = TR.topleft_upsample(c, edge)
    assert tl.shape == (2, 18, 14)
    assert np.abs(SR.hpass(p.astype(np.float64), edge) - tl).max() == 0
    # rows: even = the chroma row itself, odd = the mean with the next; row ch by the edge rule
    assert np.array_equal(tl[:, 0::2, 0::2], c) and np.array_equal(2 * tl[:, 1::2, 0::2], c + dn)
    with pytest.raises(AssertionError):
        TR.vpair(c + 1, edge)
    fb = TR.round2(synth_frames('uniform', 2, 32, 16, 10, device='cpu', seed=1).to_numpy())
    s422 = TR.as_422(fb, edge)
    assert s422.subsampling == '422' and s422.u.shape == (2, 16, 16) and np.array_equal(s422.y, fb.y)


def test_topleft_differs_from_left_by_a_quarter_chroma_row():
    """On a vertical ramp the centre-sited upsample of c + b/4 is the top-left
    upsample of c except on luma rows 0 and H - 1: exactly those two differ."""
    ch, cw = 16, 6
    m = np.arange(ch)[:, None]
    a, b = 8 * np.arange(40, 40 + cw)[None, :], 4 * np.array([-5, -1, 0, 1, 3, 5])[None, :]
    c = a + b * m
    tl, left = TR.topleft_upsample(c), toi.upsample((c + b // 4).astype(np.float64))
    rows = np.nonzero((tl != left).any(axis=1))[0]
    assert list(rows) == [0, 2 * ch - 1]
    assert not np.array_equal(tl, toi.upsample(c.astype(np.float64)))


@pytest.mark.parametrize('bits', [10, 12])
def test_ramp_pair_and_edge_rows(bits):
    W, H = 64, 32
    luma = synth_frames('smooth', 2, W, H, bits, device='cpu', seed=9).to_numpy()
    src, twin = TR.ramp_pair(luma, seed=1)
    assert (src.chroma_location, src.color_range, twin.chroma_location) == ('topleft', 'tv', 'left')
    assert np.array_equal(src.y, luma.y) and np.array_equal(twin.y, luma.y)
    d = twin.u.astype(np.int64) - src.u.astype(np.int64)
    assert np.all(d == d[:, :1]) and np.any(d != 0)       # c' - c = b/4, constant down a column
    assert np.any(np.diff(src.u.astype(np.int64), axis=1) != 0)
    got, want = np.zeros((2, W * H * 3 // 2), np.int64), np.ones((2, W * H * 3 // 2), np.int64)
    kept = TR.without_edge_rows(got, want, W, H)
    assert kept[:, :W * H].reshape(2, H, W).sum(axis=(0, 2)).tolist() == [2 * W] + [0] * (H - 2) + [2 * W]
    assert kept[:, W * H:].reshape(2, 2, H // 2, W // 2).sum(axis=(0, 1, 3)).tolist() == \
        [2 * W] + [0] * (H // 2 - 2) + [2 * W]
    assert got.sum() == 0


@pytest.mark.parametrize('bits', [10, 12])
def test_grey_steps_normalise_alike(bits):
    full, twin = TR.grey_steps(3, 64, 32, bits)
    assert (full.color_range, full.chroma_location, twin.color_range) == ('pc', 'left', 'tv')
    top, s = (1 << bits) - 1, 1 << (bits - 8)
    assert sorted(np.unique(full.y)) == [0, top // 3, 2 * (top // 3), top]
    assert top // 3 == {10: 341, 12: 1365}[bits]
    assert sorted(np.unique(twin.y)) == [16 * s + 73 * s * k for k in range(4)]
    assert np.array_equal(full.y.astype(np.float64) / top, (twin.y.astype(np.float64) - 16 * s) / (219 * s))
    for fb in (full, twin):
        assert np.all(fb.u == 1 << (bits - 1)) and np.all(fb.v == 1 << (bits - 1))
    for f in range(3):   # every frame holds every level
        assert len(np.unique(full.y[f])) == 4


@pytest.mark.parametrize('kind', ['uniform', 'smooth', 'ramp'])
def test_restatement_of_the_twins_matches_the_oracle(kind):
    """The yardstick, not the feature: the float64 restatement given the tagged
    form of a frame agrees with the C oracle on the frame's untagged twin
    (test_oracle_independent's bounds: 1 step, 3 for luma with eq; <= 0.5 %)."""
    W, H, bits, lut_n, gamma = 64, 32, 10, 17, 2.2
    p = oracle.default_params(tonemap=TM['hable'], bits_in=bits, bits_out=10, gamma=gamma, lut_enabled=1)
    lat = hdr2sdr.generate_lattice(lut_n)
    rest = (bits, 10, False, 'hable', gamma, lut_n)
    luma = synth_frames(kind, 1, W, H, bits, device='cpu', seed=11).to_numpy()
    src, twin = TR.ramp_pair(luma, seed=2)
    full, ftwin = TR.grey_steps(1, W, H, bits)
    for tagged, untagged, rows in ((src, twin, slice(1, -1)), (full, ftwin, slice(None))):
        want = FrameBatch(oracle.process(p, lat, untagged.buf, W, H), W, H, 10)
        got = TR.restated(tagged.y[0], tagged.u[0], tagged.v[0], *rest, color_range=tagged.color_range,
                          chroma_location=tagged.chroma_location)
        for name, a, b in zip('YUV', (want.y[0], want.u[0], want.v[0]), got):
            d = np.abs(a.astype(np.int64) - b)[rows]
            assert d.max() <= 4 * (3 if name == 'Y' else 1), (name, int(d.max()))
            assert (d > 0).mean() <= 5e-3, (name, float((d > 0).mean()))
    # and the tags matter to it: the same samples untagged give another picture
    a = TR.restated(full.y[0], full.u[0], full.v[0], *rest, color_range='pc')
    b = TR.restated(full.y[0], full.u[0], full.v[0], *rest)
    assert not np.array_equal(a[0], b[0])


# ---- FrameBatch -------------------------------------------------------------
def test_frame_batch_validates_and_carries_the_tags():
    W, H = 16, 8
    fb = FrameBatch.empty_numpy(4, W, H, 10)
    assert (fb.color_range, fb.chroma_location) == ('tv', 'left')
    buf = np.zeros((1, W * H * 3 // 2), np.uint16)
    for bad in (dict(color_range='full'), dict(color_range='jpeg'), dict(chroma_location='center'),
                dict(chroma_location='top'), dict(chroma_location='bottomleft')):
        with pytest.raises(ValueError):
            FrameBatch(buf, W, H, 10, **bad)
    with pytest.raises(ValueError):
        FrameBatch.empty_numpy(1, W, H, 10, color_range='unknown')
    fb = FrameBatch.empty_numpy(4, W, H, 10, 'planar', '420', 'pc', 'topleft')
    tags = ('pc', 'topleft')
    for other in (fb.slice(1, 3), fb.to_numpy(), fb.to_layout('semi'), fb.to_layout('semi').to_layout('planar'),
                  FrameBatch.empty_pinned(2, W, H, 12, 'semi', '420', 'pc', 'topleft'),
                  FrameBatch.from_planes(fb.y, fb.u, fb.v, 10, color_range='pc', chroma_location='topleft')):
        assert (other.color_range, other.chroma_location) == tags
    assert fb.to_layout('semi').layout == 'semi'
    # a frame-sharded run hands each rank a slice: the tags travel with it
    assert [(s.color_range, s.chroma_location) for s in (fb.slice(0, 2), fb.slice(2, 4))] == [tags, tags]
    # 4:2:2 / 4:4:4 batches accept the tag (it has no effect there)
    assert FrameBatch.empty_numpy(1, W, H, 10, 'planar', '422', 'tv', 'topleft').chroma_location == 'topleft'
    pytest.importorskip('torch')
    t = fb.to_torch('cpu')
    assert (t.color_range, t.chroma_location) == tags and (t.to_numpy().color_range, t.slice(0, 1).chroma_location) == tags
    e = FrameBatch.empty_torch(1, W, H, 10, 'cpu', 'planar', '420', 'pc', 'topleft')
    assert (e.color_range, e.chroma_location) == tags
    # the descriptor is the buffer's: the tags change nothing in it
    a, b = fb.descriptor(), FrameBatch(fb.buf, W, H, 10).descriptor()
    assert bytes(a) == bytes(b)


# ---- planner ------------------------------------------------------------------
def test_plan_defaults_reproduce_the_untagged_plan():
    for name in ('C2', 'C3'):
        argv = GOLD[name]['argv']
        base = P.plan_from_argv(argv, PROPS10)
        assert (base.in_range, base.in_chroma_location) == ('tv', 'left')
        for kw in (dict(in_range='pc'), dict(in_chroma_location='topleft'), dict(in_range='auto', in_chroma_location='auto'),
                   dict(in_range='pc', in_chroma_location='topleft')):
            pl = P.plan_from_argv(argv, dict(PROPS10, color_range='pc', chroma_location='topleft'), **kw)
            # the decode argv is unchanged (the codes cross the pipe untouched), the encode side too
            assert pl.decode == base.decode and pl.encode == base.encode and pl.params == base.params


@pytest.mark.parametrize('tag,want', [(None, 'tv'), ('', 'tv'), ('unknown', 'tv'), ('unspecified', 'tv'), ('tv', 'tv'),
                                      ('pc', 'pc')])
def test_plan_auto_range(tag, want):
    props = dict(PROPS10) if tag is None else dict(PROPS10, color_range=tag)
    for name in ('C2', 'C3'):     # both pipelines
        assert P.plan_from_argv(GOLD[name]['argv'], props, in_range='auto').in_range == want
    assert P.plan_from_argv(GOLD['C2']['argv'], props).in_range == 'tv'          # not asked: today's behaviour


@pytest.mark.parametrize('tag,want', [(None, 'left'), ('', 'left'), ('unknown', 'left'), ('unspecified', 'left'),
                                      ('left', 'left'), ('topleft', 'topleft')])
def test_plan_auto_chroma_location(tag, want):
    props = dict(PROPS10) if tag is None else dict(PROPS10, chroma_location=tag)
    for name in ('C2', 'C3'):
        assert P.plan_from_argv(GOLD[name]['argv'], props, in_chroma_location='auto').in_chroma_location == want
    assert P.plan_from_argv(GOLD['C2']['argv'], props).in_chroma_location == 'left'


@pytest.mark.parametrize('tag', ['center', 'top', 'bottomleft', 'bottom'])
def test_plan_refuses_an_unmodelled_location(tag):
    argv = GOLD['C2']['argv']
    with pytest.raises(ValueError, match=tag):
        P.plan_from_argv(argv, dict(PROPS10, chroma_location=tag), in_chroma_location='auto')
    # only 'auto' reads the property
    assert P.plan_from_argv(argv, dict(PROPS10, chroma_location=tag)).in_chroma_location == 'left'
    with pytest.raises(ValueError):
        P.plan_from_argv(argv, PROPS10, in_chroma_location=tag)
    with pytest.raises(ValueError):
        P.plan_from_argv(argv, PROPS10, in_range='jpeg')
    with pytest.raises(ValueError, match='color_range'):
        P.plan_from_argv(argv, dict(PROPS10, color_range='mpeg'), in_range='auto')


class _Pipe:
    """A Popen stand-in: a decoder with `data` on stdout, an encoder that keeps what it is fed."""
    def __init__(self, argv, stdout=None, stderr=None, stdin=None, data=b''):
        import io
        self.argv, self.rc = argv, None
        self.stdout = io.BytesIO(data)
        self.stderr = io.BytesIO(b'')
        self.stdin = io.BytesIO()
        self.stdin.close = lambda: None

    def poll(self):
        return 0

    def wait(self, timeout=None):
        return 0

    def kill(self):
        pass

    terminate = kill


def test_pipe_runner_hands_the_tags_to_its_batches():
    pl = P.plan_from_argv(GOLD['C2']['argv'], dict(PROPS10, width=16, height=8, color_range='pc', chroma_location='topleft'),
                          in_range='auto', in_chroma_location='auto')
    assert (pl.in_range, pl.in_chroma_location) == ('pc', 'topleft')
    seen = []

    class TM:
        def process(self, src, dst, nframes=None):
            seen.append((src.color_range, src.chroma_location, dst.color_range, dst.chroma_location, nframes))

    frame = bytes(pl.frame_bytes_in)
    proc = P.H2SProcess(pl, TM(), batch=2, popen=lambda argv, **kw: _Pipe(argv, data=frame * 3, **kw))
    assert proc.wait(timeout=30) == 0 and proc.error is None and proc.frames == 3
    assert seen == [('pc', 'topleft', 'tv', 'left', 2), ('pc', 'topleft', 'tv', 'left', 1)]


# ---- engine -------------------------------------------------------------------
class _FakeLib:
    def __init__(self):
        self.calls = []

    def h2s_set_input_tags(self, ctx, r, c):
        self.calls.append(('tags', r, c))
        return 0

    def h2s_set_frame_layout(self, ctx, a, b):
        self.calls.append(('layout', a, b))
        return 0

    def h2s_set_input_subsampling(self, ctx, s):
        self.calls.append(('sub', s))
        return 0


def test_engine_sets_the_tags_once_per_change():
    tm = hdr2sdr.Tonemapper.__new__(hdr2sdr.Tonemapper)
    tm._L, tm._ctx = _FakeLib(), ctypes.c_void_p()
    tm._layouts, tm._subsampling, tm._tags = ('planar', 'planar'), '420', ('tv', 'left')
    W, H = 16, 8
    plain = FrameBatch.empty_numpy(1, W, H, 10)
    full = FrameBatch.empty_numpy(1, W, H, 10, color_range='pc')
    both = FrameBatch.empty_numpy(1, W, H, 10, color_range='pc', chroma_location='topleft')
    for src in (plain, plain, full, full, both, plain, plain):
        tm._use_layouts(src, plain)
    assert tm._L.calls == [('tags', 1, 0), ('tags', 1, 1), ('tags', 0, 0)]     # a tag never sticks
    tm._use_layouts(both)                          # calls without a destination batch too
    assert tm._L.calls[-1] == ('tags', 1, 1)
    for bad in (('full', 'left'), ('tv', 'center')):
        with pytest.raises(ValueError):
            tm.set_input_tags(*bad)
    assert tm._L.calls[-1] == ('tags', 1, 1)
    tm._ctx = None                                 # (nothing for __del__ to destroy)


# ---- ABI ------------------------------------------------------------------------
def test_abi_binds_and_exports_the_call():
    assert 'h2s_set_input_tags' in _abi.EXPORTS
    assert _abi.COLOR_RANGES == {'tv': 0, 'pc': 1} and _abi.CHROMA_LOCATIONS == {'left': 0, 'topleft': 1}
    L = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(L, 'h2s_set_input_tags')
    assert L.h2s_abi_version() == 3 and L.h2s_abi_minor() == 4     # the numbers stay
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'h2s.h')) as fh:
        hdr = fh.read()
    assert re.search(r'int h2s_set_input_tags\(h2s_ctx \*ctx, int range, int chroma_location\);', hdr)
    assert re.search(r'enum h2s_range\s*\{ H2S_RANGE_LIMITED = 0, H2S_RANGE_FULL = 1 \};', hdr)
    assert re.search(r'enum h2s_chroma_loc\s*\{ H2S_CHROMA_LEFT = 0, H2S_CHROMA_TOPLEFT = 1 \};', hdr)


def test_null_context_and_unknown_values_are_invalid_arg():
    L = ctypes.CDLL(_abi.LIB_PATH)
    L.h2s_set_input_tags.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.h2s_last_error.restype = ctypes.c_char_p
    L.h2s_last_error.argtypes = [ctypes.c_void_p]
    assert L.h2s_set_input_tags(None, 0, 0) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_last_error(None)
    assert L.h2s_set_input_tags(None, 2, 0) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_set_input_tags(None, 0, 2) == _abi.H2S_E_INVALID_ARG
