"""The scaled 4:2:0 output on the GPU (h2s_process_scaled,
Tonemapper.process_scaled) against the float64 restatement in
tests/scaled_ref.py.

Every case takes its source codes from the same context's own h2s_process
output >> shift_out (that path is gated against the oracle elsewhere), written
to a surface whose rows lie 16 bytes apart as the library's scratch rows do, so
that both conversions take one route.  Gate (the project's
integer rule at depth q): every sample within 1 code of the restatement and at
most 0.5 % of a plane differing; the float32 restatement meets it on the same
contents and sizes on the CPU (tests/test_scaled.py).  Twins, chunking, the
equal size and flat frames are exact, with no tolerance."""
import ctypes
import functools

import numpy as np
import pytest

import hdr2sdr
import oracle
import scaled_ref as ref
import source_preview_ref as spref
from hdr2sdr import _abi
from hdr2sdr.synth import synth_frames
from padded_frames import FILL, RowPadded

pytestmark = pytest.mark.gpu

C2 = dict(tonemapper='hable', gamma=2.2, bits_in=10, bits_out=10)    # compat8: q = 8
CASE_IDS = [c[0] for c in ref.CASES]


@functools.lru_cache(maxsize=None)
def _lattice():
    return hdr2sdr.generate_lattice(33)


_contexts = {}


def context(**kw):
    """One context per parameter set for the module."""
    key = tuple(sorted(kw.items()))
    if key not in _contexts:
        _contexts[key] = hdr2sdr.Tonemapper(0, hdr2sdr.TonemapParams(**kw), _lattice())
    return _contexts[key]


@pytest.fixture(scope='module', autouse=True)
def _close_contexts():
    yield
    for t in _contexts.values():
        t.close()
    _contexts.clear()


def quant_bits(tm):
    return oracle.quant_bits(oracle.params_from(tm.params.to_c()))


@functools.lru_cache(maxsize=None)
def _source(kind, nframes, W, H, bits=10):
    return synth_frames(kind, nframes, W, H, bits, seed=0x5CA1E).to_numpy()


def chain_output(tm, src, nframes=None):
    """The context's own h2s_process output of a device batch, as a tight host
    buffer [F, W * H * 3 / 2] of bits_out codes."""
    import torch
    n = src.nframes if nframes is None else nframes
    mid = RowPadded(n, src.width, src.height, tm.params.bits_out, align=16)
    tm.process(src, mid, nframes=n)
    torch.cuda.synchronize()
    return mid.to_numpy().buf


def scaled(tm, src, ow, oh, layout='planar'):
    """process_scaled into a fresh tight device batch; the host copy of it."""
    import torch
    dst = hdr2sdr.FrameBatch.empty_torch(src.nframes, ow, oh, tm.params.bits_out, 'cuda:0', layout)
    dst.buf.fill_(0x33)
    tm.process_scaled(src, dst)
    torch.cuda.synchronize()
    return dst.to_numpy()


def check_gate(tm, got, mid, W, H, ow, oh, what):
    q, bo = quant_bits(tm), tm.params.bits_out
    want = ref.expected(mid, W, H, ow, oh, q, bo, tm.params.expand)
    mx, frac = ref.gate_planes(got, want, ow, oh, shift=bo - q)
    print(f'{what}: q = {q}, max diff {mx}, {frac:.4%} of the worst plane differs')
    assert mx <= ref.MAX_DIFF and frac <= ref.MAX_FRACTION, what
    # whatever differs, every sample is a legal expanded code
    g = np.asarray(got).astype(np.int64)
    assert np.array_equal(g, ref.expand(g >> (bo - q), q, bo, tm.params.expand)), what


# ---- the cases against the restatement ---------------------------------------------------
@pytest.mark.parametrize('kind', ref.CONTENTS)
@pytest.mark.parametrize('case_id', CASE_IDS)
def test_case_meets_the_gate(case_id, kind):
    _, W, H, ow, oh = ref.BY_ID[case_id]
    tm = context(**C2)
    src = _source(kind, 1, W, H).to_torch('cuda:0')
    got = scaled(tm, src, ow, oh)
    check_gate(tm, got.buf, chain_output(tm, src), W, H, ow, oh, f'{case_id} {kind}')


@pytest.mark.parametrize('expand', ['shift', 'replicate'])
@pytest.mark.parametrize('bits_out', [8, 10, 12])
def test_compat8_depths_and_expansions(bits_out, expand):
    tm = context(**dict(C2, bits_out=bits_out, expand=expand))
    assert quant_bits(tm) == 8
    _, W, H, ow, oh = ref.BY_ID['nonint']
    src = _source('uniform', 1, W, H).to_torch('cuda:0')
    got = scaled(tm, src, ow, oh)
    check_gate(tm, got.buf, chain_output(tm, src), W, H, ow, oh, f'compat8 {bits_out} {expand}')


@pytest.mark.parametrize('bits_out', [10, 12])
def test_native_depths(bits_out):
    tm = context(**dict(C2, bits_out=bits_out, mode='native'))
    assert quant_bits(tm) == bits_out
    _, W, H, ow, oh = ref.BY_ID['ragged']
    src = _source('smooth', 1, W, H).to_torch('cuda:0')
    got = scaled(tm, src, ow, oh)
    check_gate(tm, got.buf, chain_output(tm, src), W, H, ow, oh, f'native {bits_out}')


def test_three_frames_with_padded_pitches_on_both_sides():
    import torch
    _, W, H, ow, oh = ref.BY_ID['ragged']
    tm = context(**C2)
    host = _source('smooth', 3, W, H)
    src = RowPadded(3, W, H, 10, align=64).load(host)
    dst = RowPadded(3, ow, oh, 10, align=32)       # (70 x 38: rows of 140 and 70 bytes, 160 and 96 apart)
    tm.process_scaled(src, dst)
    torch.cuda.synchronize()
    check_gate(tm, dst.to_numpy().buf, chain_output(tm, src), W, H, ow, oh, 'padded')
    # a tight destination gets the same codes (from rows 16 bytes apart: a tight 136-wide source
    # would send the chain down its other route), and no byte of the padding is written
    assert np.array_equal(dst.to_numpy().buf, scaled(tm, RowPadded(3, W, H, 10, align=16).load(host), ow, oh).buf)
    raw = dst.raw()
    for f in range(3):
        for off, ls, rows, rowb in dst.planes:
            pad = raw[f * dst.fp + off:][:rows * ls].reshape(rows, ls)[:, rowb:]
            assert (pad == FILL).all()


def test_libplacebo_branch_with_peak_detect_keeps_the_state():
    tm = context(tonemapper='bt.2390', peak_detect=True, maxcll=4000.0)
    assert tm.params.resolved_pipeline() == 'libplacebo' and quant_bits(tm) == 10
    _, W, H, ow, oh = ref.BY_ID['2to1']
    src = _source('smooth', 3, W, H).to_torch('cuda:0')
    tm.reset_peak()
    mid = chain_output(tm, src)
    after_process = tm.peak_state()
    tm.reset_peak()
    got = scaled(tm, src, ow, oh)
    assert tm.peak_state() == after_process and after_process['frames'] == 3
    check_gate(tm, got.buf, mid, W, H, ow, oh, 'libplacebo peak_detect')


@pytest.mark.parametrize('bits_out', [8, 10])
def test_semi_planar_output_equals_its_planar_twin(bits_out):
    """nv12 / p010le written in place: a (Cb, Cr) pair is one word."""
    tm = context(**dict(C2, bits_out=bits_out))
    for case_id in ('ragged', '2to1'):
        _, W, H, ow, oh = ref.BY_ID[case_id]
        src = _source('uniform', 2, W, H).to_torch('cuda:0')
        planar = scaled(tm, src, ow, oh)
        semi = scaled(tm, src, ow, oh, 'semi')
        assert np.array_equal(semi.to_layout('planar').buf, planar.buf)
        if bits_out == 10:      # the code sits in the high bits of its word
            assert (np.asarray(semi.buf) & 0x3F == 0).all()


def test_semi_planar_output_with_unaligned_rows():
    """Rows 2 bytes off a 16-byte boundary: the scalar stores, pair words included."""
    import torch
    tm = context(**C2)
    _, W, H, ow, oh = ref.BY_ID['ragged']
    src = _source('uniform', 1, W, H).to_torch('cuda:0')
    planar = scaled(tm, src, ow, oh)
    dst = RowPadded(1, ow, oh, 10, 'semi', align=2)
    tm.process_scaled(src, dst)
    torch.cuda.synchronize()
    assert np.array_equal(dst.to_numpy().to_layout('planar').buf, planar.buf)


def test_semi_planar_and_422_input():
    tm = context(**C2)
    _, W, H, ow, oh = ref.BY_ID['nonint']
    host = _source('smooth', 1, W, H)
    semi = host.to_layout('semi').to_torch('cuda:0')
    check_gate(tm, scaled(tm, semi, ow, oh).buf, chain_output(tm, semi), W, H, ow, oh, 'p010 input')
    s422 = spref.synth_source('smooth', 1, W, H, 10, '422').to_torch('cuda:0')
    check_gate(tm, scaled(tm, s422, ow, oh).buf, chain_output(tm, s422), W, H, ow, oh, '4:2:2 input')


def test_host_resident_pair_equals_the_device_call():
    tm = context(**C2)
    _, W, H, ow, oh = ref.BY_ID['2to1']
    host = _source('uniform', 3, W, H)
    dst = hdr2sdr.FrameBatch.empty_numpy(3, ow, oh, 10)
    tm.process_scaled(host, dst)                      # (returns after the stream has finished)
    assert np.array_equal(dst.buf, scaled(tm, host.to_torch('cuda:0'), ow, oh).buf)
    out = tm(host, size=(ow, oh))
    assert (out.width, out.height, out.nframes) == (ow, oh, 3) and np.array_equal(out.buf, dst.buf)


@pytest.mark.parametrize('kw', [C2, dict(tonemapper='bt.2390', peak_detect=True, maxcll=4000.0)],
                         ids=['static', 'peak_detect'])
def test_a_batch_longer_than_the_scratch_equals_frame_by_frame(kw):
    """18 frames: one chunk of 16 and one of 2."""
    tm = context(**kw)
    W, H, ow, oh = 64, 32, 42, 20
    src = _source('smooth', 18, W, H).to_torch('cuda:0')
    tm.reset_peak()
    whole = scaled(tm, src, ow, oh).buf
    state = tm.peak_state()
    tm.reset_peak()
    single = np.concatenate([scaled(tm, src.slice(f, f + 1), ow, oh).buf for f in range(18)])
    assert np.array_equal(whole, single)
    assert tm.peak_state() == state


def test_equal_size_is_process():
    import torch
    tm = context(**C2)
    W, H = 136, 72
    src = _source('uniform', 2, W, H).to_torch('cuda:0')
    a = hdr2sdr.FrameBatch.empty_torch(2, W, H, 10, 'cuda')
    tm.process(src, a)
    torch.cuda.synchronize()
    assert np.array_equal(scaled(tm, src, W, H).buf, a.to_numpy().buf)


@pytest.mark.parametrize('case_id', CASE_IDS)
def test_flat_frame_stays_flat(case_id):
    _, W, H, ow, oh = ref.BY_ID[case_id]
    tm = context(**C2)
    src = spref.flat_frame(W, H, 10, 500, 400, 600).to_torch('cuda:0')
    mid = ref.planes_of(chain_output(tm, src), W, H)
    got = ref.planes_of(scaled(tm, src, ow, oh).buf, ow, oh)
    for m, g in zip(mid, got):
        assert (m == m.flat[0]).all()        # (a per-pixel chain: a flat source leaves it flat)
        assert (g == m.flat[0]).all()


def test_errors():
    tm = context(**C2)
    W, H = 192, 96
    src = _source('uniform', 1, W, H).to_torch('cuda:0')

    def call(ow, oh, bits=10):
        dst = hdr2sdr.FrameBatch.empty_torch(1, W, H, bits, 'cuda')    # (room for any target below)
        tm._use_layouts(src, dst)
        di, do = src.descriptor(), dst.descriptor()
        do.width, do.height = ow, oh
        return _abi.lib().h2s_process_scaled(tm._ctx, ctypes.byref(di), ctypes.byref(do), 1, tm._stream_ptr(None))

    assert call(96, 48) == 0
    assert call(95, 48) == _abi.H2S_E_INVALID_ARG        # an odd target
    assert call(96, 47) == _abi.H2S_E_INVALID_ARG
    assert call(0, 48) == _abi.H2S_E_INVALID_ARG
    assert call(14, 48) == _abi.H2S_E_UNSUPPORTED        # 192 / 14 = 13.7
    assert call(96, 6) == _abi.H2S_E_UNSUPPORTED         # 96 / 6 = 16
    assert call(16, 8) == 0                              # 12 on both axes is inside
    assert call(96, 48, bits=8) == _abi.H2S_E_INVALID_ARG   # out->bits != params.bits_out
    with pytest.raises(ValueError):
        tm.process_scaled(src, hdr2sdr.FrameBatch.empty_torch(1, 14, 48, 10, 'cuda'))
    import torch
    torch.cuda.synchronize()


def test_tap_tables_are_uploaded_once_per_size():
    """OPT_TEST_SCALE_UPLOADS answers OK exactly for the context's upload count."""
    tm = hdr2sdr.Tonemapper(0, hdr2sdr.TonemapParams(**C2), _lattice())
    try:
        def uploads():
            return next(n for n in range(16)
                        if _abi.lib().h2s_set_option(tm._ctx, _abi.OPT_TEST_SCALE_UPLOADS, n) == 0)

        W, H = 192, 96
        src = _source('uniform', 1, W, H).to_torch('cuda:0')
        assert uploads() == 0
        a1 = scaled(tm, src, 96, 48).buf
        assert uploads() == 1
        b = scaled(tm, src, 128, 64).buf               # another target: the tables are replaced
        assert uploads() == 2
        b2 = scaled(tm, src, 128, 64).buf              # the same target again: no upload
        assert uploads() == 2
        a2 = scaled(tm, src, 96, 48).buf
        assert uploads() == 3
        scaled(tm, src, W, H)                          # the equal size never touches them
        assert uploads() == 3
        assert np.array_equal(a1, a2) and np.array_equal(b, b2)
        check_gate(tm, b, chain_output(tm, src), W, H, 128, 64, 'second target')
    finally:
        tm.close()


def test_timing_records_the_resize_launch():
    tm = context(**C2)
    _, W, H, ow, oh = ref.BY_ID['2to1']
    src = _source('uniform', 1, W, H).to_torch('cuda:0')
    tm.set_timing(True)
    try:
        scaled(tm, src, ow, oh)
        resize_ms = tm.kernel_ms(1)                    # the last entry: the resize launch
        both_ms = tm.kernel_ms(2) * 2                  # and the chunk's h2s_process entry before it
        assert 0.0 < resize_ms < both_ms
    finally:
        tm.set_timing(False)
