"""The 4:2:0 front-end on the GPU (h2s_set_input_decimation, k_decimate420).

1. the front-end alone (h2stest_decimate) against tests/decimate_ref.py under
   its tie-aware gate, at the smallest shapes at which the kernel can go wrong;
2. flat chroma is exact, and converts like the flat 4:2:0 set;
3. composition: with the setting on, every call equals, byte for byte, the same
   call on the 4:2:0 set made of the same luma and the hook's chroma (so the
   chain behind the front-end is unchanged);
4. a batch longer than the scratch equals frame by frame;
5. host frames equal device frames;
6. p210 / p410 sets equal their planar twins;
7. off is off.

The kernel's shapes: a lane owns 8 words of a chroma row, a wave 64 such chunks
(4:4:4: 62, its edge lanes load the halo), a run is 4 .. 32 output rows."""
import ctypes
import functools

import numpy as np
import pytest

import decimate_ref as R
import hdr2sdr
from hdr2sdr import _abi
from hdr2sdr.frames import FrameBatch
from hdr2sdr.preview import Previewer

pytestmark = pytest.mark.gpu

SUBS = ('422', '444')
FILL = 0x55
# widths: a strip of two chunks (16), ragged last chunks (70, 1044), whole chunks (144, 208), more than
# one wave strip in every form (1044: 2 .. 5 strips); heights: fewer rows than taps (4), run boundaries
# (R.WIDTHS x R.HEIGHTS and R.MORE)
PITCHES = ('tight', 'padded', 'odd')
LP = dict(tonemapper='bt.2390', maxcll=4000.0)
CHAINS = {
    'bt2390': dict(LP),
    'bt2390_lut_off_8': dict(LP, lut_enabled=False, bits_out=8),
    'spline_12': dict(tonemapper='spline', maxcll=4000.0, bits_in=12, bits_out=12),
    'hable_compat8': dict(tonemapper='hable', gamma=2.2),
    'hable_native_12': dict(tonemapper='hable', mode='native', bits_out=12),
    'hable_lut_off_8': dict(tonemapper='hable', lut_enabled=False, bits_out=8),
}


@functools.lru_cache(maxsize=None)
def _lattice():
    return hdr2sdr.generate_lattice(17)


_contexts = {}


def context(**kw):
    """One context per parameter set for the module; the setting is each test's to make."""
    key = tuple(sorted(kw.items()))
    if key not in _contexts:
        _contexts[key] = hdr2sdr.Tonemapper(0, hdr2sdr.TonemapParams(**kw), _lattice())
    tm = _contexts[key]
    tm.set_input_decimation('off')
    return tm


@pytest.fixture(scope='module', autouse=True)
def _close_contexts():
    yield
    for t in _contexts.values():
        t.close()
    _contexts.clear()


def hook():
    fn = _abi.lib().h2stest_decimate
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(_abi.H2SFrames), ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                   ctypes.c_int]
    return fn


class Surface:
    """A device 4:2:2 / 4:4:4 set of any form the front-end reads: planar or
    semi-planar (words code << (16 - bits)), rows tight, padded to 16 bytes
    and beyond, or a pitch that is no multiple of 16; frames further apart
    than a frame.  What FrameBatch is to Tonemapper."""
    color_range, chroma_location = 'tv', 'left'

    def __init__(self, y, u, v, bits, layout, sub, pitch='tight'):
        import torch
        self.nframes, self.height, self.width = y.shape
        self.bits, self.layout, self.subsampling = bits, layout, sub
        if layout == 'semi':
            sh = 16 - bits
            planes = [y.astype(np.uint16) << sh, (np.stack([u, v], axis=-1).astype(np.uint16) << sh).reshape(*u.shape[:2], -1)]
        else:
            planes = [y, u, v]
        self.geo, off = [], 0
        for p in planes:
            rowb = p.shape[-1] * 2
            ls = {'tight': rowb, 'padded': (rowb + 15) // 16 * 16 + 16, 'odd': rowb + 6 + (2 if (rowb + 6) % 16 == 0 else 0)}[pitch]
            self.geo.append((off, ls, p.shape[-2], rowb))
            off += ls * p.shape[-2]
        self.fp = off + {'tight': 0, 'padded': 64, 'odd': 2}[pitch]
        raw = np.full(self.nframes * self.fp, FILL, np.uint8)
        for p, (o, ls, rows, rowb) in zip(planes, self.geo):
            for f in range(self.nframes):
                raw[f * self.fp + o:][:rows * ls].reshape(rows, ls)[:, :rowb] = \
                    np.ascontiguousarray(p[f].astype('<u2')).view(np.uint8).reshape(rows, rowb)
        self.buf = torch.from_numpy(raw).cuda()

    def descriptor(self):
        d = _abi.H2SFrames()
        for p, (off, ls, _, _) in enumerate(self.geo):
            d.data[p] = self.buf.data_ptr() + off
            d.linesize[p], d.frame_pitch[p] = ls, self.fp
        d.width, d.height, d.bits, d.location = self.width, self.height, self.bits, _abi.LOC_DEVICE
        return d


def front_end(tm, src, run=0):
    """(Cb, Cr) [F, H/2, W/2] of the front-end alone, from either layout."""
    tm._use_layouts(src)
    F, ch, cw = src.nframes, src.height // 2, src.width // 2
    out = np.zeros((F, 2 * ch * cw), np.uint16)
    d = src.descriptor()
    rc = hook()(tm._ctx, ctypes.byref(d), F, out.ctypes.data, out.nbytes, run)
    assert rc == 0, _abi.lib().h2s_last_error(tm._ctx).decode()
    if src.layout == 'semi':
        pairs = out.reshape(F, ch, cw, 2)
        assert (pairs & ((1 << (16 - src.bits)) - 1) == 0).all()      # the code sits in the high bits
        pairs = pairs >> (16 - src.bits)
        return pairs[..., 0], pairs[..., 1]
    planes = out.reshape(F, 2, ch, cw)
    return planes[:, 0], planes[:, 1]


def check_gate(got, planes, sub, bits, kind, what, cap=True):
    for name, g, p in zip(('Cb', 'Cr'), got, planes):
        miss, tie, diff = R.gate(g, p, sub, bits)
        print(f'{what} {name}: {miss} miss, {tie:.3%} in the tie window, {diff} differ')
        assert miss == 0, what
        if kind == 'edges':
            assert 1 - tie >= R.EDGES_CLEAR, what
        elif cap:
            assert tie <= R.TIE_CAP, what


# ---- 1: the front-end alone -----------------------------------------------------------------
@pytest.mark.parametrize('bits', [10, 12])
@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('kind', R.CONTENTS)
def test_front_end_meets_the_gate(kind, sub, bits):
    """The four sizes of the composition tests: planar and semi-planar, and the two agree sample for sample."""
    tm = context(**dict(LP, bits_in=bits))
    for W, H in R.SIZES:
        y, u, v = R.content(kind, 1, W, H, sub, bits)
        planar = front_end(tm, Surface(y, u, v, bits, 'planar', sub))
        check_gate(planar, (u, v), sub, bits, kind, f'{kind} {sub} {bits} {W}x{H}')
        semi = front_end(tm, Surface(y, u, v, bits, 'semi', sub))
        assert all(np.array_equal(a, b) for a, b in zip(planar, semi))


@pytest.mark.parametrize('layout', ['planar', 'semi'])
@pytest.mark.parametrize('sub', SUBS)
def test_front_end_small_shapes_pitches_and_runs(sub, layout):
    """Every width x height of the kernel's edges, in the three pitches, at the
    host's own run length (4 rows at these sizes) and at forced runs of 8 and
    32 rows (70 and 66 source rows: a run boundary at 32, and one row past it).
    The tie share is capped where a plane has at least R.CAP_MIN_SAMPLES output
    samples: a plane of 16 samples has 6 % of them in the window with one tie."""
    for bits in (10, 12):
        tm = context(**dict(LP, bits_in=bits))
        for W, H in R.SMALL:
            y, u, v = R.content('noise', 1, W, H, sub, bits)
            got, cap = {}, (W // 2) * (H // 2) >= R.CAP_MIN_SAMPLES
            for pitch in PITCHES:
                got[pitch] = front_end(tm, Surface(y, u, v, bits, layout, sub, pitch))
                check_gate(got[pitch], (u, v), sub, bits, 'noise', f'{sub} {layout} {bits} {W}x{H} {pitch}', cap=cap)
            # the element path and the 16-byte path give the same codes
            assert all(np.array_equal(a, b) for p in PITCHES for a, b in zip(got[p], got['tight']))
            if H >= 66:
                for run in (8, 32):
                    forced = front_end(tm, Surface(y, u, v, bits, layout, sub, 'padded'), run)
                    assert all(np.array_equal(a, b) for a, b in zip(forced, got['tight'])), (W, H, run)


@pytest.mark.parametrize('layout', ['planar', 'semi'])
@pytest.mark.parametrize('sub', SUBS)
def test_front_end_three_frames_with_a_frame_pitch(sub, layout):
    tm = context(**LP)
    W, H = 70, 34
    y, u, v = R.content('smooth', 3, W, H, sub, 10)
    src = Surface(y, u, v, 10, layout, sub, 'padded')
    before = src.buf.cpu().numpy()
    check_gate(front_end(tm, src), (u, v), sub, 10, 'smooth', f'3 frames {sub} {layout}')
    assert np.array_equal(src.buf.cpu().numpy(), before)          # the source, its padding included, is only read


# ---- 2: the exact case ----------------------------------------------------------------------
def batch_420(y, cb, cr, bits, layout='planar'):
    fb = FrameBatch.from_planes(y, cb, cr, bits)
    return fb.to_layout(layout)


def process(tm, src, bits_out=None):
    import torch
    dst = FrameBatch.empty_torch(src.nframes, src.width, src.height, tm.params.bits_out, 'cuda')
    dst.buf.fill_(0x33)
    tm.process(src, dst)
    torch.cuda.synchronize()
    return dst.to_numpy().buf


def planar_source(y, u, v, bits, sub):
    return FrameBatch.from_planes(y, u, v, bits, sub).to_torch('cuda')


@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('chain', ['bt2390', 'hable_compat8'])
def test_flat_chroma_is_exact(chain, sub):
    tm = context(**CHAINS[chain])
    for (W, H), (cb, cr) in zip([(64, 32), (70, 34)], [(400, 1023), (0, 612)]):
        y, u, v = R.content('noise', 2, W, H, sub, 10)
        u[...], v[...] = cb, cr
        got = front_end(tm, Surface(y, u, v, 10, 'planar', sub))
        assert (got[0] == cb).all() and (got[1] == cr).all()
        tm.set_input_decimation('bicubic')
        on = process(tm, planar_source(y, u, v, 10, sub))
        tm.set_input_decimation('off')
        flat = batch_420(y, np.full((2, H // 2, W // 2), cb, np.uint16), np.full((2, H // 2, W // 2), cr, np.uint16), 10)
        assert np.array_equal(on, process(tm, flat.to_torch('cuda')))


# ---- 3: composition ---------------------------------------------------------------------------
def twins(tm, kind, nframes, W, H, sub, bits):
    """(the 4:2:2 / 4:4:4 device batch, the 4:2:0 one of its luma and the hook's chroma)."""
    y, u, v = R.content(kind, nframes, W, H, sub, bits)
    src = planar_source(y, u, v, bits, sub)
    cb, cr = [], []
    for f0 in range(0, nframes, 16):        # (the hook takes up to 16 frames)
        a, b = front_end(tm, src.slice(f0, min(f0 + 16, nframes)))
        cb.append(a), cr.append(b)
    return src, batch_420(y, np.concatenate(cb), np.concatenate(cr), bits).to_torch('cuda')


@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('chain', list(CHAINS))
def test_process_equals_the_420_set_of_the_hooks_chroma(chain, sub):
    kw = CHAINS[chain]
    tm = context(**kw)
    bits = kw.get('bits_in', 10)
    for W, H in R.SIZES:
        src, ref420 = twins(tm, 'smooth', 2, W, H, sub, bits)
        want = process(tm, ref420)
        dst = FrameBatch.empty_torch(2, W, H, tm.params.bits_out, 'cuda')
        want_path = tm.query_path(ref420, dst)
        tm.set_input_decimation('bicubic')
        assert tm.query_path(src, dst) == want_path
        got = process(tm, src)
        tm.set_input_decimation('off')
        assert np.array_equal(got, want), (chain, sub, W, H)


@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('tonemapper', ['bt.2390', 'spline'])
def test_peak_detect_output_state_and_statistics(tonemapper, sub):
    tm = context(tonemapper=tonemapper, peak_detect=True, maxcll=4000.0)
    for W, H in [(64, 32), (208, 64), (70, 34)]:
        src, ref420 = twins(tm, 'smooth', 3, W, H, sub, 10)
        tm.reset_peak()
        want, state, stats = process(tm, ref420), tm.peak_state(), tm.peak_stats(ref420)
        tm.set_input_decimation('bicubic')
        tm.reset_peak()
        got = process(tm, src)
        assert tm.peak_state() == state and state['frames'] == 3
        got_stats = tm.peak_stats(src)
        tm.set_input_decimation('off')
        assert np.array_equal(got, want), (W, H)
        assert all(np.array_equal(a, b) for a, b in zip(got_stats, stats))


@pytest.mark.parametrize('sub', SUBS)
def test_scaled_debug_and_preview_compose(sub):
    import torch
    W, H = 192, 70
    tm = context(**LP)
    src, ref420 = twins(tm, 'smooth', 2, W, H, sub, 10)

    def scaled(s):
        dst = FrameBatch.empty_torch(2, 96, 36, 10, 'cuda')
        tm.process_scaled(s, dst)
        torch.cuda.synchronize()
        return dst.to_numpy().buf

    want_scaled, want_dbg = scaled(ref420), [tm.debug_float(ref420, st) for st in (_abi.STAGE_TONEMAP, _abi.STAGE_YUV)]
    tm.set_input_decimation('bicubic')
    got_scaled, got_dbg = scaled(src), [tm.debug_float(src, st) for st in (_abi.STAGE_TONEMAP, _abi.STAGE_YUV)]
    tm.set_input_decimation('off')
    assert np.array_equal(got_scaled, want_scaled)
    assert all(np.array_equal(a, b) for a, b in zip(got_dbg, want_dbg))
    for kw in (dict(tonemapper='bt.2390', use_gpu=True), dict(tonemapper='hable')):
        with Previewer(0, lattice=_lattice(), **kw) as off, Previewer(0, lattice=_lattice(), decimate='bicubic', **kw) as on:
            want = off.convert_batch(ref420, 96, 36)
            got = on.convert_batch(src, 96, 36)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
            # the source pane shows the frames as decoded, whatever the setting
            assert np.array_equal(on.original(src, 96, 36), off.original(src, 96, 36))


def test_dolby_vision_records_follow_the_frames_across_chunks():
    """18 frames with a record each (three shapes in turn), with peak_detect:
    the second chunk's frames 16 and 17 take records 16 and 17, in the
    conversion and in h2s_peak_stats, as in the one launch of the 4:2:0 twin.
    A top-left tag on the 4:2:2 set changes nothing (the set the chain reads
    is left-sited)."""
    import dovi_ref as DR
    tm = context(**dict(LP, peak_detect=True))
    recs = [DR.luma_map_record(pieces, 10) for pieces in DR.LUMA_MAPS[:3]]
    src, ref420 = twins(tm, 'smooth', 18, 64, 32, '422', 10)
    tagged = FrameBatch(src.buf, 64, 32, 10, 'planar', '422', 'tv', 'topleft')
    tm.set_dovi([recs[f % 3] for f in range(18)])
    try:
        tm.reset_peak()
        want, state, stats = process(tm, ref420), tm.peak_state(), tm.peak_stats(ref420)
        # (frame 16 alone takes record 0: what a chunk that restarted the records would compute, and not the same)
        alone = tm.peak_stats(ref420.slice(16, 17))
        assert (alone[0][0], alone[1][0]) != (stats[0][16], stats[1][16])
        tm.set_input_decimation('bicubic')
        for s in (src, tagged):
            tm.reset_peak()
            assert np.array_equal(process(tm, s), want)
            assert tm.peak_state() == state
            assert all(np.array_equal(a, b) for a, b in zip(tm.peak_stats(s), stats))
    finally:
        tm.set_dovi(None)
        tm.set_input_decimation('off')


# ---- 4: chunking ------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [LP, dict(LP, peak_detect=True)], ids=['static', 'peak_detect'])
def test_a_batch_longer_than_the_scratch_equals_frame_by_frame(kw):
    """18 frames: one chunk of 16 and one of 2."""
    tm = context(**kw)
    W, H = 64, 32
    y, u, v = R.content('smooth', 18, W, H, '422', 10)
    src = planar_source(y, u, v, 10, '422')
    tm.set_input_decimation('bicubic')
    tm.reset_peak()
    whole, state = process(tm, src), tm.peak_state()
    tm.reset_peak()
    single = np.concatenate([process(tm, src.slice(f, f + 1)) for f in range(18)])
    assert tm.peak_state() == state
    stats = tm.peak_stats(src)
    parts = [tm.peak_stats(src.slice(f, f + 1)) for f in range(18)]
    tm.set_input_decimation('off')
    assert np.array_equal(whole, single)
    assert all(np.array_equal(stats[i], np.concatenate([p[i] for p in parts])) for i in (0, 1))


# ---- 5: host frames ---------------------------------------------------------------------------
@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('nframes', [1, 18])
def test_host_frames_equal_device_frames(nframes, sub):
    tm = context(**LP)
    W, H = 64, 32
    y, u, v = R.content('noise', nframes, W, H, sub, 10)
    host = FrameBatch.from_planes(y, u, v, 10, sub)
    tm.set_input_decimation('bicubic')
    want = process(tm, host.to_torch('cuda'))
    dst = FrameBatch.empty_numpy(nframes, W, H, 10)
    tm.process(host, dst)                                   # (returns after the stream has finished)
    assert np.array_equal(dst.buf, want)
    assert np.array_equal(tm.debug_float(host, _abi.STAGE_YUV), tm.debug_float(host.to_torch('cuda'), _abi.STAGE_YUV))
    tm.set_input_decimation('off')


# ---- 6: p210 / p410 -----------------------------------------------------------------------------
@pytest.mark.parametrize('bits', [10, 12])
@pytest.mark.parametrize('sub', SUBS)
def test_semi_planar_sets_equal_their_planar_twins(sub, bits):
    import torch
    tm = context(**dict(LP, bits_in=bits))
    for W, H in [(64, 32), (70, 34)]:
        y, u, v = R.content('smooth', 2, W, H, sub, bits)
        semi = FrameBatch.empty_numpy(2, W, H, bits, 'semi', sub, allow_semi_sub=True)
        sh = 16 - bits
        semi.y[...], semi.uv[..., 0], semi.uv[..., 1] = y << sh, u << sh, v << sh
        tm.set_input_decimation('bicubic')
        want = process(tm, planar_source(y, u, v, bits, sub))
        assert np.array_equal(process(tm, semi.to_torch('cuda')), want)
        out = FrameBatch.empty_numpy(2, W, H, 10)
        tm.process(semi, out)                               # a host p210 / p410 set
        assert np.array_equal(out.buf, want)
        # padded pitches: against the planar twin of the same pitches (rows 16 bytes apart send the 70-wide set
        # down the tile route, which its tight twin does not take)
        both = []
        for layout in ('semi', 'planar'):
            dst = FrameBatch.empty_torch(2, W, H, 10, 'cuda')
            tm.process(Surface(y, u, v, bits, layout, sub, 'padded'), dst)
            torch.cuda.synchronize()
            both.append(dst.to_numpy().buf)
        tm.set_input_decimation('off')
        assert np.array_equal(both[0], both[1])
        if W % 64 == 0:
            assert np.array_equal(both[0], want)


# ---- 7: off is off ------------------------------------------------------------------------------
def test_off_is_off_and_the_setting_toggles():
    import torch
    L = _abi.lib()
    tm = context(**dict(LP, peak_detect=True))
    W, H = 64, 32
    y, u, v = R.content('smooth', 1, W, H, '422', 10)
    src = planar_source(y, u, v, 10, '422')
    dst = FrameBatch.empty_torch(1, W, H, 10, 'cuda')
    y0, u0, v0 = R.content('smooth', 1, W, H, '444', 10)
    fb420 = batch_420(y0, u0[:, ::2, ::2], v0[:, ::2, ::2], 10).to_torch('cuda')

    def refused():
        tm._use_layouts(src, dst)
        di, do = src.descriptor(), dst.descriptor()
        fm = np.zeros(1)
        codes = [L.h2s_process(tm._ctx, ctypes.byref(di), ctypes.byref(do), 1, None),
                 L.h2s_query_path(tm._ctx, ctypes.byref(di), ctypes.byref(do)),
                 L.h2s_peak_stats(tm._ctx, ctypes.byref(di), 1, fm.ctypes.data, fm.ctypes.data, None)]
        return codes == [_abi.H2S_E_UNSUPPORTED] * 3

    assert refused()
    semi = FrameBatch.empty_torch(1, W, H, 10, 'cuda', 'semi', '422', allow_semi_sub=True)
    cpu = context(tonemapper='hable')
    with pytest.raises(ValueError, match='planar only'):
        cpu.process(semi, dst)
    for bad in (2, -1):
        assert L.h2s_set_input_decimation(tm._ctx, bad) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_set_input_decimation(None, 1) == _abi.H2S_E_INVALID_ARG
    with pytest.raises(ValueError):
        tm.set_input_decimation('box')
    tm.set_input_decimation('bicubic')
    tm.reset_peak()
    first = process(tm, src)
    tm.set_input_decimation('off')
    assert refused()
    tm.reset_peak()
    plain = process(tm, fb420)                       # a 4:2:0 call in between
    tm.set_input_decimation('bicubic')
    tm.reset_peak()
    assert np.array_equal(process(tm, fb420), plain)      # 4:2:0 input: the setting has no effect
    tm.reset_peak()
    assert np.array_equal(process(tm, src), first)
    tm.set_input_decimation('off')
    assert refused()
    torch.cuda.synchronize()


def test_timing_records_the_front_end_launch():
    tm = context(**LP)
    W, H = 192, 70
    y, u, v = R.content('smooth', 1, W, H, '444', 10)
    src = planar_source(y, u, v, 10, '444')
    tm.set_input_decimation('bicubic')
    tm.set_timing(True)
    try:
        process(tm, src)
        convert_ms = tm.kernel_ms(1)                   # the last entry: the chunk's conversion
        both_ms = tm.kernel_ms(2) * 2                  # and the front-end's entry in front of it
        assert 0.0 < convert_ms < both_ms
    finally:
        tm.set_timing(False)
        tm.set_input_decimation('off')
