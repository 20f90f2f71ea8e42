"""A rendition ladder from one conversion on the GPU (h2s_process_ladder,
Tonemapper.process_ladder) against the separate calls it replaces.

A rung is produced by the same kernels, from the same scratch contents, as the
separate call, so every comparison is byte for byte (np.array_equal), with no
tolerance anywhere:
  - a scaled rung against process_scaled on an equal context of its own;
  - a rung of the source's size against process into a surface whose rows lie
    16 bytes apart (RowPadded(..., align=16)): the library's scratch rows do, and
    that decides the chain's route (tests/test_gpu_scaled.py);
  - a semi-planar rung against its planar twin, interleaved in numpy.
One context per role and parameter set for the module; the dynamic-peak and
tap-cache cases make fresh ones, since they look at a context's state."""
import ctypes
import functools

import numpy as np
import pytest

import hdr2sdr
import source_preview_ref as spref
from hdr2sdr import _abi
from hdr2sdr.synth import synth_frames
from padded_frames import FILL, RowPadded

pytestmark = pytest.mark.gpu

C2 = dict(tonemapper='hable', gamma=2.2, bits_in=10, bits_out=10)    # compat8: q = 8
PEAK = dict(tonemapper='bt.2390', peak_detect=True, maxcll=4000.0)   # the libplacebo branch, dynamic peak
CONTENTS = ('smooth', 'uniform')


@functools.lru_cache(maxsize=None)
def _lattice():
    return hdr2sdr.generate_lattice(33)


def fresh(**kw):
    return hdr2sdr.Tonemapper(0, hdr2sdr.TonemapParams(**kw), _lattice())


_contexts = {}


def context(role, **kw):
    """One context per role ('ladder': the call under test; 'ref': the separate calls) and parameter set."""
    key = (role,) + tuple(sorted(kw.items()))
    if key not in _contexts:
        _contexts[key] = fresh(**kw)
    return _contexts[key]


@pytest.fixture(scope='module', autouse=True)
def _close_contexts():
    yield
    for t in _contexts.values():
        t.close()
    _contexts.clear()


@functools.lru_cache(maxsize=None)
def _source(kind, nframes, W, H, bits=10):
    return synth_frames(kind, nframes, W, H, bits, seed=0x1ADDE5).to_numpy()


def sync():
    import torch
    torch.cuda.synchronize()


def ladder(tm, src, sizes, layout='planar', nframes=None):
    """process_ladder into fresh tight device batches; their host copies."""
    n = src.nframes if nframes is None else nframes
    dsts = [hdr2sdr.FrameBatch.empty_torch(n, w, h, tm.params.bits_out, 'cuda:0', layout) for w, h in sizes]
    for d in dsts:
        d.buf.fill_(0x33)
    tm.process_ladder(src, dsts, nframes=n)
    sync()
    return [d.to_numpy() for d in dsts]


def separate(tm, src, size, nframes=None):
    """The separate call's planar bytes for one rung: process (rows 16 bytes apart) or process_scaled."""
    n = src.nframes if nframes is None else nframes
    ow, oh = size
    if (ow, oh) == (src.width, src.height):
        dst = RowPadded(n, ow, oh, tm.params.bits_out, align=16)
        tm.process(src, dst, nframes=n)
    else:
        dst = hdr2sdr.FrameBatch.empty_torch(n, ow, oh, tm.params.bits_out, 'cuda:0')
        tm.process_scaled(src, dst, nframes=n)
    sync()
    return dst.to_numpy().buf


def check_ladder(kw, src, sizes, what, layout='planar'):
    got = ladder(context('ladder', **kw), src, sizes, layout)
    ref = context('ref', **kw)
    for i, (size, g) in enumerate(zip(sizes, got)):
        want = separate(ref, src, size)
        assert np.array_equal(g.to_layout('planar').buf, want), f'{what}: rung {i} {size}'
    return got


# ---- 1-3: shapes at which a path changes -------------------------------------------------------
MIXED = [(192, 96), (128, 64), (96, 48), (16, 8)]      # 1 : 1, 1.5 : 1, 2 : 1, 12 : 1 on both axes (the LDS worst case)


@pytest.mark.parametrize('kind', CONTENTS)
@pytest.mark.parametrize('order', ['down', 'up'])
def test_tile_path_source_with_mixed_ratios(kind, order):
    src = _source(kind, 2, 192, 96).to_torch('cuda:0')
    check_ladder(C2, src, MIXED if order == 'down' else MIXED[::-1], f'mixed {order} {kind}')


@pytest.mark.parametrize('kind', CONTENTS)
def test_ragged_source(kind):
    """136 x 72: chroma rows of 68 samples (the repack's ragged last chunk), the scaler's ragged strip."""
    host = _source(kind, 2, 136, 72)
    # (a source with rows 16 bytes apart takes the tile kernel, a tight one, whose chroma rows are 136 bytes, the
    # generic kernel: either way the ladder and the separate call read the same source)
    src = RowPadded(2, 136, 72, 10, align=16).load(host)
    check_ladder(C2, src, [(136, 72), (70, 38)], f'ragged {kind}')
    check_ladder(C2, host.to_torch('cuda:0'), [(136, 72), (70, 38)], f'ragged tight source {kind}')


@pytest.mark.parametrize('kind', CONTENTS)
def test_several_row_runs(kind):
    src = _source(kind, 2, 96, 320).to_torch('cuda:0')
    check_ladder(C2, src, [(96, 320), (64, 160)], f'row runs {kind}')


def test_duplicate_rungs_and_all_source_size():
    src = _source('smooth', 2, 192, 96).to_torch('cuda:0')
    got = check_ladder(C2, src, [(96, 48), (192, 96), (96, 48), (192, 96)], 'duplicates')
    assert np.array_equal(got[0].buf, got[2].buf) and np.array_equal(got[1].buf, got[3].buf)
    check_ladder(C2, src, [(192, 96), (192, 96)], 'source size only')


# ---- 4: depths ---------------------------------------------------------------------------------
@pytest.mark.parametrize('expand', ['shift', 'replicate'])
@pytest.mark.parametrize('bits_out', [8, 10, 12])
def test_compat8_depths_and_expansions(bits_out, expand):
    kw = dict(C2, bits_out=bits_out, expand=expand)
    for kind in CONTENTS:
        check_ladder(kw, _source(kind, 2, 192, 96).to_torch('cuda:0'), [(192, 96), (96, 48)],
                     f'compat8 {bits_out} {expand} {kind}')


def test_native_depth():
    kw = dict(C2, bits_out=10, mode='native')
    for kind in CONTENTS:
        check_ladder(kw, _source(kind, 2, 192, 96).to_torch('cuda:0'), [(192, 96), (96, 48)], f'native {kind}')


# ---- 5: layouts --------------------------------------------------------------------------------
@pytest.mark.parametrize('bits_out', [8, 10, 12])
def test_semi_planar_rungs_equal_their_planar_twins(bits_out):
    """nv12 / p010le / p012le: a (Cb, Cr) pair is one word, a 16-bit code sits in its word's high bits."""
    kw = dict(C2, bits_out=bits_out)
    for kind in CONTENTS:
        src = _source(kind, 2, 192, 96).to_torch('cuda:0')
        got = check_ladder(kw, src, [(192, 96), (96, 48)], f'semi {bits_out} {kind}', layout='semi')
        if bits_out > 8:
            for g in got:
                assert (np.asarray(g.buf) & ((1 << (16 - bits_out)) - 1) == 0).all()
        # the ragged sizes too: the pairs' ragged last chunk
        host = _source(kind, 1, 136, 72)
        check_ladder(kw, RowPadded(1, 136, 72, 10, align=16).load(host), [(136, 72), (70, 38)],
                     f'semi ragged {bits_out} {kind}', layout='semi')


def test_semi_planar_and_422_input():
    for kind in CONTENTS:
        semi = _source(kind, 2, 192, 96).to_layout('semi').to_torch('cuda:0')
        check_ladder(C2, semi, [(192, 96), (96, 48)], f'p010 input {kind}')
    s422 = spref.synth_source('smooth', 2, 192, 96, 10, '422').to_torch('cuda:0')
    check_ladder(C2, s422, [(192, 96), (96, 48)], '4:2:2 input')


# ---- 6: destination pitches --------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['planar', 'semi'])
@pytest.mark.parametrize('align', [64, 10], ids=['aligned', 'unaligned'])
def test_padded_destination_pitches(align, layout):
    """Rows 64 bytes apart: the 16-byte stores.  Rows a multiple of 10 bytes apart (280 / 140 and 140 / 70 bytes:
    no multiple of 16 among them): the per-sample stores of both kernels.  No padding byte is written."""
    tm, ref = context('ladder', **C2), context('ref', **C2)
    sizes = [(136, 72), (70, 38)]
    for kind in CONTENTS:
        src = RowPadded(3, 136, 72, 10, align=16).load(_source(kind, 3, 136, 72))
        dsts = [RowPadded(3, w, h, 10, layout, align=align) for w, h in sizes]
        if align == 10:
            assert all(any(ls % 16 for _, ls, _, _ in d.planes) for d in dsts)
        tm.process_ladder(src, dsts)
        sync()
        for size, d in zip(sizes, dsts):
            assert np.array_equal(d.to_numpy().to_layout('planar').buf, separate(ref, src, size)), (kind, size)
            raw = d.raw()
            for f in range(3):
                for off, ls, rows, rowb in d.planes:
                    pad = raw[f * d.fp + off:][:rows * ls].reshape(rows, ls)[:, rowb:]
                    assert (pad == FILL).all()


# ---- 7: dynamic peak, every frame counted once -------------------------------------------------
def _brightness_steps(nframes, W, H):
    """Frames of differing brightness: the smoothed peak moves from frame to frame."""
    fb = _source('smooth', nframes, W, H)
    out = hdr2sdr.FrameBatch(np.array(fb.buf, copy=True), W, H, 10)
    for f in range(nframes):
        y = np.asarray(out.y[f]).astype(np.int64)
        out.y[f] = np.clip(64 + (y - 64) * (f + 2) // (nframes + 1), 64, 940).astype(out.buf.dtype)
    return out


def test_dynamic_peak_counts_every_frame_once():
    """The ladder {full, half} on A against process on B and process_scaled on C, all fresh: equal bytes, equal
    peak state (5 frames, not 10), and again after a second call on each."""
    W, H, N = 192, 96, 5
    a, b, c = fresh(**PEAK), fresh(**PEAK), fresh(**PEAK)
    try:
        assert a.params.resolved_pipeline() == 'libplacebo'
        batches = [_brightness_steps(N, W, H).to_torch('cuda:0'), _source('uniform', N, W, H).to_torch('cuda:0')]
        for call, src in enumerate(batches):
            full, half = ladder(a, src, [(W, H), (W // 2, H // 2)])
            want_full = separate(b, src, (W, H))
            want_half = separate(c, src, (W // 2, H // 2))
            assert np.array_equal(full.buf, want_full), f'call {call}: full rung'
            assert np.array_equal(half.buf, want_half), f'call {call}: half rung'
            assert a.peak_state() == b.peak_state() == c.peak_state()
            assert a.peak_state()['frames'] == N * (call + 1)
    finally:
        for t in (a, b, c):
            t.close()


# ---- 8: chunking -------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [C2, PEAK], ids=['static', 'peak_detect'])
def test_a_batch_longer_than_the_scratch_equals_frame_by_frame(kw):
    """18 frames: one chunk of 16 and one of 2."""
    tm = context('ladder', **kw)
    sizes = [(64, 32), (32, 16)]
    src = _source('smooth', 18, 64, 32).to_torch('cuda:0')
    tm.reset_peak()
    whole = ladder(tm, src, sizes)
    state = tm.peak_state()
    tm.reset_peak()
    single = [ladder(tm, src.slice(f, f + 1), sizes) for f in range(18)]
    for i in range(2):
        assert np.array_equal(whole[i].buf, np.concatenate([s[i].buf for s in single])), i
    assert tm.peak_state() == state
    if kw is PEAK:
        assert state['frames'] == 18


# ---- 9: Dolby Vision ---------------------------------------------------------------------------
def test_dolby_vision_records_follow_the_frame():
    import dovi_ref as DR
    W, H = 128, 64
    kw = dict(tonemapper='bt.2390', bits_in=10, bits_out=10)
    host, recs, _ = DR.luma_map_pair(W, H, 10, 2)
    src = host.to_torch('cuda:0')
    tm, ref = fresh(**kw), fresh(**kw)
    try:
        tm.set_dovi(recs)
        ref.set_dovi(recs)
        sizes = [(W, H), (W // 2, H // 2)]
        got = ladder(tm, src, sizes)
        for size, g in zip(sizes, got):
            assert np.array_equal(g.buf, separate(ref, src, size)), size
        # the two records do differ: swapped, the same frames convert differently
        ref.set_dovi(recs[::-1])
        assert not np.array_equal(got[0].buf, separate(ref, src, sizes[0]))
    finally:
        tm.close()
        ref.close()


# ---- 10: host ----------------------------------------------------------------------------------
def test_host_source_and_host_rungs_equal_the_device_result():
    tm = context('ladder', **C2)
    sizes = [(192, 96), (96, 48), (136, 72)]
    host = _source('uniform', 3, 192, 96)
    dsts = [hdr2sdr.FrameBatch.empty_numpy(3, w, h, 10) for w, h in sizes]
    tm.process_ladder(host, dsts)                       # (returns after the stream has finished)
    dev = ladder(tm, host.to_torch('cuda:0'), sizes)
    for d, g in zip(dsts, dev):
        assert np.array_equal(d.buf, g.buf)
    outs = tm.ladder(host, sizes)
    assert [(o.width, o.height, o.nframes) for o in outs] == [(w, h, 3) for w, h in sizes]
    assert all(np.array_equal(o.buf, d.buf) for o, d in zip(outs, dsts))
    # 18 host frames: two chunks through the one staging
    long = _source('smooth', 18, 64, 32)
    got = tm.ladder(long, [(64, 32), (32, 16)])
    dev = ladder(tm, long.to_torch('cuda:0'), [(64, 32), (32, 16)])
    assert all(np.array_equal(o.buf, d.buf) for o, d in zip(got, dev))


def test_mixed_rung_locations_are_refused():
    tm = context('ladder', **C2)
    src = _source('uniform', 1, 192, 96).to_torch('cuda:0')
    dev = hdr2sdr.FrameBatch.empty_torch(1, 192, 96, 10, 'cuda:0')
    with pytest.raises(ValueError):
        tm.process_ladder(src, [dev, hdr2sdr.FrameBatch.empty_numpy(1, 96, 48, 10)])
    rc, msg = raw_call(tm, src, [(192, 96), (96, 48)], edit=lambda outs: setattr(outs[1], 'location', _abi.LOC_HOST))
    assert rc == _abi.H2S_E_INVALID_ARG and 'rung 1' in msg


# ---- 11: one rung ------------------------------------------------------------------------------
def test_one_rung_is_process_scaled():
    tm, ref = context('ladder', **C2), context('ref', **C2)
    src = _source('uniform', 2, 136, 72).to_torch('cuda:0')
    assert np.array_equal(ladder(tm, src, [(70, 38)])[0].buf, separate(ref, src, (70, 38)))
    # the source's size: process_scaled's equal-size rule, h2s_process into the caller's own (tight) rows
    a = hdr2sdr.FrameBatch.empty_torch(2, 136, 72, 10, 'cuda')
    ref.process(src, a)
    sync()
    assert np.array_equal(ladder(tm, src, [(136, 72)])[0].buf, a.to_numpy().buf)


# ---- 12: the tap cache -------------------------------------------------------------------------
def test_tap_tables_are_uploaded_once_per_rung_size():
    tm = fresh(**C2)
    try:
        def count(key):
            return next(n for n in range(64) if _abi.lib().h2s_set_option(tm._ctx, key, n) == 0)

        src = _source('uniform', 1, 192, 96).to_torch('cuda:0')
        sizes = [(192, 96), (96, 48), (128, 64), (96, 48)]        # two distinct scaled sizes
        assert count(_abi.OPT_TEST_LADDER_UPLOADS) == 0
        first = ladder(tm, src, sizes)
        assert count(_abi.OPT_TEST_LADDER_UPLOADS) == 2
        for _ in range(5):
            again = ladder(tm, src, sizes)
            assert count(_abi.OPT_TEST_LADDER_UPLOADS) == 2
        assert count(_abi.OPT_TEST_SCALE_UPLOADS) == 0            # h2s_process_scaled's cache is not the ladder's
        one = separate(tm, src, (64, 32))                         # a process_scaled call in between
        assert count(_abi.OPT_TEST_SCALE_UPLOADS) == 1 and count(_abi.OPT_TEST_LADDER_UPLOADS) == 2
        after = ladder(tm, src, sizes)
        assert count(_abi.OPT_TEST_SCALE_UPLOADS) == 1 and count(_abi.OPT_TEST_LADDER_UPLOADS) == 2
        for f, a, b in zip(first, again, after):
            assert np.array_equal(f.buf, a.buf) and np.array_equal(f.buf, b.buf)
        assert np.array_equal(one, separate(context('ref', **C2), src, (64, 32)))
        # a ninth size replaces an entry that this call does not read, and the bytes stay right
        many = [(190 - 16 * k, 94 - 8 * k) for k in range(1, 9)]
        ladder(tm, src, many)
        assert count(_abi.OPT_TEST_LADDER_UPLOADS) == 2 + 8
        back = ladder(tm, src, sizes)
        assert count(_abi.OPT_TEST_LADDER_UPLOADS) == 2 + 8 + 2
        for f, b in zip(first, back):
            assert np.array_equal(f.buf, b.buf)
    finally:
        tm.close()


# ---- 13: errors --------------------------------------------------------------------------------
def raw_call(tm, src, sizes, edit=None, n_outs=None, nframes=1, null_outs=False, fill=None):
    """h2s_process_ladder through ctypes: (return code, h2s_last_error).  ``edit`` changes the descriptors
    (rung surfaces of the source's size: room for any target)."""
    dsts = [RowPadded(1, src.width, src.height, tm.params.bits_out, align=16) for _ in sizes]
    tm._use_layouts(src, dsts[0])
    outs = (_abi.H2SFrames * max(len(dsts), 1))(*[d.descriptor() for d in dsts])
    for o, (w, h) in zip(outs, sizes):
        o.width, o.height = w, h
    if edit:
        edit(outs)
    di = src.descriptor()
    L = _abi.lib()
    rc = L.h2s_process_ladder(tm._ctx, ctypes.byref(di), None if null_outs else outs,
                              len(dsts) if n_outs is None else n_outs, nframes, tm._stream_ptr(None))
    sync()
    if fill is not None:
        fill.extend(dsts)
    return rc, L.h2s_last_error(tm._ctx).decode()


def test_errors():
    tm = fresh(**C2)
    try:
        W, H = 192, 96
        src = _source('uniform', 1, W, H).to_torch('cuda:0')
        INV, UNS = _abi.H2S_E_INVALID_ARG, _abi.H2S_E_UNSUPPORTED
        ok = [(W, H), (96, 48), (16, 8)]                       # 12 : 1 on both axes is inside
        assert raw_call(tm, src, ok)[0] == 0
        assert raw_call(tm, src, ok, n_outs=0)[0] == INV
        assert raw_call(tm, src, ok, n_outs=-1)[0] == INV
        assert raw_call(tm, src, [(96, 48)] * 8)[0] == 0
        assert raw_call(tm, src, [(96, 48)] * 9)[0] == INV     # > H2S_LADDER_MAX
        assert raw_call(tm, src, ok, null_outs=True)[0] == INV
        assert _abi.lib().h2s_process_ladder(None, None, None, 2, 1, None) == INV
        for bad, code in (((95, 48), INV), ((96, 47), INV), ((0, 48), INV), ((96, -2), INV),    # odd, non-positive
                          ((14, 48), UNS), ((96, 6), UNS)):                                     # 13.7 : 1, 16 : 1
            for pos in range(3):
                sizes = list(ok)
                sizes[pos] = bad
                rc, msg = raw_call(tm, src, sizes)
                assert rc == code and f'rung {pos}' in msg, (bad, pos, rc, msg)
        # a rung of the wrong depth, without a plane, with a short pitch: h2s_process_scaled's checks, with the index
        for edit in (lambda o: setattr(o[2], 'bits', 8), lambda o: o[2].data.__setitem__(1, None),
                     lambda o: o[2].linesize.__setitem__(0, 2)):
            rc, msg = raw_call(tm, src, ok, edit=edit)
            assert rc == INV and 'rung 2' in msg, msg
        assert raw_call(tm, src, ok, nframes=-1)[0] == INV

        def too_wide(o):       # beyond 4 * 8192 (the pitches say there is room: the call is refused before any write)
            o[1].width = 4 * 8192 + 2
            for p in range(3):
                o[1].linesize[p] = 2 * o[1].width
        rc, msg = raw_call(tm, src, ok, edit=too_wide)
        assert rc == UNS and 'rung 1' in msg, msg
        with pytest.raises(ValueError):
            tm.process_ladder(src, [hdr2sdr.FrameBatch.empty_torch(1, W, H, 10, 'cuda'),
                                    hdr2sdr.FrameBatch.empty_torch(1, 14, 48, 10, 'cuda')])
        # a refused rung in position 2 of 3: nothing is written to rungs 0 and 1
        kept = []
        rc, msg = raw_call(tm, src, [(W, H), (96, 48), (14, 48)], fill=kept)
        assert rc == UNS and 'rung 2' in msg
        assert all((d.raw() == FILL).all() for d in kept)
        # and a correct call on the same context right afterwards is the reference's bytes
        ref = context('ref', **C2)
        for size, g in zip(ok, ladder(tm, src, ok)):
            assert np.array_equal(g.buf, separate(ref, src, size)), size
    finally:
        tm.close()


def test_a_refused_call_leaves_the_peak_state():
    tm = fresh(**PEAK)
    try:
        src = _source('smooth', 2, 192, 96).to_torch('cuda:0')
        ladder(tm, src, [(192, 96), (96, 48)])
        state = tm.peak_state()
        assert state['frames'] == 2
        rc, msg = raw_call(tm, src, [(192, 96), (14, 48)])
        assert rc == _abi.H2S_E_UNSUPPORTED and 'rung 1' in msg
        assert tm.peak_state() == state
    finally:
        tm.close()


# ---- 14: timing --------------------------------------------------------------------------------
def test_timing_records_the_conversion_then_every_rung():
    """17 frames (chunks of 16 and 1) x 3 rungs: 2 x (1 + 3) entries.  The newest entries are the second chunk's;
    the first chunk's conversion (16 frames) is the fifth from the end and outlasts the second's (1 frame)."""
    tm = context('ladder', **C2)
    W, H = 384, 192
    src = _source('smooth', 17, W, H).to_torch('cuda:0')
    sizes = [(W, H), (192, 96), (96, 48)]
    ladder(tm, src, sizes)                             # (the tables and the scratch exist)
    tm.set_timing(True)
    try:
        ladder(tm, src, sizes)
        total = [tm.kernel_ms(n) * n for n in range(1, 11)]        # (a count beyond the record is the whole record)
        entry = [total[0]] + [total[i] - total[i - 1] for i in range(1, 8)]     # newest first
        print('ladder timing entries, newest first (ms):', [round(v, 4) for v in entry])
        assert all(v > 0.0 for v in entry)
        assert tm.kernel_ms(8) == tm.kernel_ms(9) == tm.kernel_ms(10)          # exactly 8 entries
        conv2, conv1 = entry[3], entry[7]
        assert conv1 > conv2
    finally:
        tm.set_timing(False)
