"""The 4:2:0 front-end (h2s_set_input_decimation), the parts that need no GPU:
the gate of tests/decimate_ref.py judged on the float32 evaluation of the model
and on two mutants, the planner, FrameBatch and the ABI."""
import ctypes

import numpy as np
import pytest

import decimate_ref as R
from hdr2sdr import _abi
from hdr2sdr import plan as P
from hdr2sdr.frames import FrameBatch, frame_bytes
from test_plan import GOLD, PROPS10

SUBS = ('422', '444')


def test_taps_are_the_chroma_model():
    wx, wy = R.taps()
    assert np.allclose(wx * 80, [-3, 0, 23, 40, 23, 0, -3], atol=1e-12)
    assert np.allclose(wy * 640, [-9, -27, 77, 279, 279, 77, -27, -9], atol=1e-10)
    assert abs(np.abs(wx).sum() - 1.15) < 1e-12 and abs(wy[wy > 0].sum() - 1.1125) < 1e-12
    assert abs(R.delta(10) - 1.3e-3) < 1e-4 and abs(R.delta(12) - 5.3e-3) < 1e-4


# ---- the gate -----------------------------------------------------------------------------------
@pytest.mark.parametrize('bits', [10, 12])
@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('kind', R.CONTENTS)
def test_float32_evaluation_passes_the_gate_within_the_cap(kind, sub, bits):
    for W, H in R.SIZES:
        _, u, v = R.content(kind, 1, W, H, sub, bits)
        for plane in (u, v):
            for order in ('vh', 'hv'):
                miss, tie, diff = R.gate(R.decimate_f32(plane, sub, bits, order), plane, sub, bits)
                assert miss == 0, (W, H, order)
            if kind == 'edges':
                assert 1 - tie >= R.EDGES_CLEAR
            else:
                assert tie <= R.TIE_CAP, (W, H, tie)


@pytest.mark.parametrize('bits', [10, 12])
@pytest.mark.parametrize('sub', SUBS)
def test_float32_evaluation_passes_the_gate_at_the_small_shapes(sub, bits):
    for W, H in R.SMALL:
        _, u, v = R.content('noise', 1, W, H, sub, bits)
        for plane in (u, v):
            for order in ('vh', 'hv'):
                miss, tie, _ = R.gate(R.decimate_f32(plane, sub, bits, order), plane, sub, bits)
                assert miss == 0, (W, H, order)
            if (W // 2) * (H // 2) >= R.CAP_MIN_SAMPLES:
                assert tie <= R.TIE_CAP, (W, H, tie)


@pytest.mark.parametrize('bits', [10, 12])
@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('kind', R.CONTENTS)
def test_mutants_miss_the_gate(kind, sub, bits):
    for W, H in R.SIZES:
        _, u, _ = R.content(kind, 1, W, H, sub, bits)
        for mutant in (R.mutant_cosited, R.mutant_box):
            got = mutant(u, sub, bits)
            assert R.gate(got, u, sub, bits)[0] > 0, (mutant.__name__, W, H)
            assert R.beyond_one(got, u, sub, bits) > 0.03, (mutant.__name__, W, H)


def test_flat_planes_and_edges_are_exact_in_the_model():
    p = np.full((1, 10, 16), 777)
    for sub in SUBS:
        got, u = R.decimate(p, sub, 10)
        assert (got == 777).all() and np.allclose(u, 777, atol=1e-9)
        assert (R.decimate_f32(p, sub, 10) == 777).all()
    # replicate: a plane of two rows has every tap on them
    two = np.array([[[100] * 8, [300] * 8]])
    wy = R.taps()[1]
    assert np.allclose(R.decimate(two, '422', 10)[1], 100 * wy[:4].sum() + 300 * wy[4:].sum())


# ---- the planner --------------------------------------------------------------------------------
def test_plan_keeps_the_source_pix_fmt_for_the_gpu_front_end():
    W, H = PROPS10['width'], PROPS10['height']
    lp, cpu = GOLD['C3']['argv'], GOLD['C2']['argv']
    pl = P.plan_from_argv(lp, PROPS10, in_subsampling='422', decimate='gpu')
    assert (pl.in_subsampling, pl.decimate, pl.decode[-3:]) == ('422', 'gpu', ['-pix_fmt', 'yuv422p10le', '-'])
    assert pl.frame_bytes_in == W * H * 2 * 2 and pl.frame_bytes_out == W * H * 3
    pl = P.plan_from_argv(lp, dict(PROPS10, bit_depth=12, pix_fmt='yuv444p12le'), in_subsampling='auto', decimate='gpu')
    assert (pl.in_subsampling, pl.decimate, pl.decode[-2]) == ('444', 'gpu', 'yuv444p12le')
    # the default: today's argv, byte for byte
    for kw in ({}, dict(decimate='cpu')):
        pl = P.plan_from_argv(lp, dict(PROPS10, pix_fmt='yuv444p10le'), in_subsampling='444', **kw)
        base = P.plan_from_argv(lp, PROPS10)
        assert (pl.in_subsampling, pl.decimate, pl.decode[-2]) == ('420', 'cpu', 'yuv420p10le')
        assert pl.decode == base.decode and pl.encode == base.encode
    assert P.plan_from_argv(lp, dict(PROPS10, bit_depth=12), in_subsampling='422').decode[-2] == 'yuv420p12le'
    # a 4:2:0 source has nothing to decimate
    pl = P.plan_from_argv(lp, PROPS10, decimate='gpu')
    assert (pl.in_subsampling, pl.decimate, pl.decode[-2]) == ('420', 'cpu', 'yuv420p10le')
    # a CPU-chain plan reads the source natively, with or without it
    a = P.plan_from_argv(cpu, PROPS10, in_subsampling='422', decimate='gpu')
    b = P.plan_from_argv(cpu, PROPS10, in_subsampling='422')
    assert a.decimate == b.decimate == 'cpu' and a.decode == b.decode and a.decode[-2] == 'yuv422p10le'
    with pytest.raises(ValueError):
        P.plan_from_argv(lp, PROPS10, decimate='swscale')
    with pytest.raises(ValueError):       # the software decode pipe is planar
        P.plan_from_argv(lp, PROPS10, in_layout='semi', in_subsampling='422', decimate='gpu')


def test_h2s_process_sets_the_context_from_the_plan():
    import io

    class Tm:
        mode = None

        def set_input_decimation(self, mode):
            self.mode = mode

        def process(self, src, dst, nframes=None):
            pass

    class Proc:
        def __init__(self, *a, **k):
            self.stdout, self.stdin, self.stderr = io.BytesIO(b''), io.BytesIO(), io.BytesIO(b'')

        def poll(self):
            return 0

        def wait(self, timeout=None):
            return 0

        def kill(self):
            pass

    props = dict(PROPS10, width=64, height=32)
    for kw, want in ((dict(in_subsampling='422', decimate='gpu'), 'bicubic'), (dict(in_subsampling='422'), 'off')):
        tm = Tm()
        h = P.H2SProcess(P.plan_from_argv(GOLD['C3']['argv'], props, **kw), tm, batch=1, popen=Proc)
        h._thread.join(10), h._reader.join(10)
        assert tm.mode == want and h.error is None
        assert h._src[0].subsampling == ('422' if want == 'bicubic' else '420')


# ---- FrameBatch ---------------------------------------------------------------------------------
@pytest.mark.parametrize('sub,pairs_w', [('422', 8), ('444', 16)])
def test_frame_batch_semi_planar_subsampled_forms(sub, pairs_w):
    W, H = 16, 8
    for make in (FrameBatch.empty_numpy, FrameBatch.empty_pinned):
        with pytest.raises(ValueError):
            make(2, W, H, 10, 'semi', sub)
        fb = make(2, W, H, 10, 'semi', sub, allow_semi_sub=True)
        assert fb.buf.nbytes == 2 * frame_bytes(W, H, 10, sub) == 2 * (W * H + 2 * pairs_w * H) * 2
        assert fb.uv.shape == (2, H, pairs_w, 2) and fb.u.shape == fb.v.shape == (2, H, pairs_w)
        d = fb.descriptor()
        assert (d.linesize[0], d.linesize[1], d.linesize[2]) == (W * 2, pairs_w * 2 * 2, 0)
        assert d.data[1] - d.data[0] == W * H * 2 and not d.data[2]
        assert d.frame_pitch[0] == d.frame_pitch[1] == frame_bytes(W, H, 10, sub)
        assert fb.slice(0, 1).allow_semi_sub and fb.slice(0, 1).uv.shape == (1, H, pairs_w, 2)
    # the 4:2:0 semi-planar descriptor is what it was
    d = FrameBatch.empty_numpy(1, W, H, 10, 'semi').descriptor()
    assert d.linesize[1] == W * 2


# ---- ABI ------------------------------------------------------------------------------------------
def test_abi_binds_and_exports_the_call():
    assert 'h2s_set_input_decimation' in _abi.EXPORTS
    assert _abi.DECIMATIONS == {'off': 0, 'bicubic': 1}
    L = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(L, 'h2s_set_input_decimation') and hasattr(L, 'h2stest_decimate')
    assert L.h2s_abi_version() == 3 and L.h2s_abi_minor() == 4     # the numbers stay
    L.h2s_set_input_decimation.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.h2s_set_input_decimation(None, 1) == _abi.H2S_E_INVALID_ARG
    assert _abi.lib().h2s_last_error(None)
