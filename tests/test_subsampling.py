"""4:2:2 / 4:4:4 input (h2s_set_input_subsampling), the parts that need no GPU:
the test constructions themselves (tests/subsampling_ref.py), FrameBatch, the
planner and the ABI."""
import ctypes

import numpy as np
import pytest

import hdr2sdr
import oracle
import subsampling_ref as SR
from hdr2sdr import _abi
from hdr2sdr import plan as P
from hdr2sdr.frames import FrameBatch
from hdr2sdr.synth import synth_frames
from test_plan import GOLD, PROPS10

TM = {'reinhard': 4, 'hable': 5, 'mobius': 6}
# (tonemapper, bits_in, bits_out, hlg, gamma, lut_n): PQ 10 bit and HLG 12 bit, LUT 17 and off, gamma 1 and 2.2
YARDSTICK_CHAINS = [('hable', 10, 10, False, 2.2, 17), ('mobius', 10, 10, False, 1.0, 0),
                    ('reinhard', 12, 12, True, 1.0, 17), ('hable', 12, 12, True, 2.2, 0)]


@pytest.mark.parametrize('kind', ['uniform', 'smooth', 'ramp'])
@pytest.mark.parametrize('case', YARDSTICK_CHAINS, ids=lambda c: '-'.join(map(str, c)))
def test_exact_upsamples_restate_the_oracles_420_result(kind, case):
    """The yardstick, not the feature (it passes without it): the float64
    restatement fed the exact 4:2:2 / 4:4:4 upsamples of a 4:2:0 frame agrees
    with the C oracle on that frame within test_oracle_independent's own
    bounds (1 step, 3 for luma with eq; <= 0.5 % of samples)."""
    tm, bits_in, bits_out, hlg, gamma, lut_n = case
    W, H = 96, 64
    fb = SR.round8(synth_frames(kind, 1, W, H, bits_in, device='cpu', seed=11).to_numpy())
    p = oracle.default_params(tonemap=TM[tm], bits_in=bits_in, bits_out=bits_out, transfer_in=1 if hlg else 0,
                              gamma=gamma, lut_enabled=1 if lut_n else 0)
    lat = hdr2sdr.generate_lattice(lut_n) if lut_n else None
    want = FrameBatch(oracle.process(p, lat, fb.buf, W, H), W, H, bits_out)
    step = 1 << (bits_out - 8)
    for sub, src in SR.exact_inputs(fb).items():
        got = SR.restated(sub, src.y[0], src.u[0], src.v[0], bits_in, bits_out, hlg, tm, gamma, lut_n)
        for name, a, b in zip('YUV', (want.y[0], want.u[0], want.v[0]), got):
            d = np.abs(a.astype(np.int64) - b)
            bound = step * (1 if name != 'Y' or gamma == 1.0 else 3)
            assert d.max() <= bound, (sub, name, int(d.max()))
            assert (d > 0).mean() <= 5e-3, (sub, name, float((d > 0).mean()))


@pytest.mark.parametrize('edge', SR.EDGES)
def test_integer_upsamplers_are_the_s1_passes(edge):
    """hup(vup(c)) equals the float upsampler of the restatement (zimg rule)
    and vup / hup follow chroma_edge_at at both ends."""
    rng = np.random.default_rng(3)
    c = rng.integers(8, 120, size=(6, 10)) * 8
    v, h = SR.vup(c, edge), SR.hup(c, edge)
    assert v.shape == (12, 10) and h.shape == (6, 20)
    top = {'zimg': c[1], 'replicate': c[0], 'mirror': c[1]}[edge]
    bot = {'zimg': c[-1], 'replicate': c[-1], 'mirror': c[-2]}[edge]
    assert np.array_equal(4 * v[0], top + 3 * c[0]) and np.array_equal(4 * v[-1], 3 * c[-1] + bot)
    right = {'zimg': c[:, -1], 'replicate': c[:, -1], 'mirror': c[:, -2]}[edge]
    assert np.array_equal(2 * h[:, -1], c[:, -1] + right) and np.array_equal(h[:, 0::2], c)
    if edge == 'zimg':
        import test_oracle_independent as toi
        assert np.array_equal(SR.hup(v), toi.upsample(c.astype(np.float64)))
    assert np.array_equal(SR.hpass(v.astype(np.float64), edge), SR.hup(v, edge))
    odd = c.copy()
    odd[2, 3] += 2          # no longer a multiple of 8: the pass is not exact, and says so
    with pytest.raises(AssertionError):
        SR.vup(odd, edge)


# ---- FrameBatch -------------------------------------------------------------
@pytest.mark.parametrize('bits', [10, 12])
@pytest.mark.parametrize('sub,cw,ch,mult', [('422', 24, 32, 2), ('444', 48, 32, 3)])
def test_frame_batch_shapes_and_descriptor(sub, cw, ch, mult, bits):
    W, H, F = 48, 32, 3
    fb = FrameBatch.empty_numpy(F, W, H, bits, 'planar', sub)
    assert fb.subsampling == sub and fb.buf.shape == (F, W * H * mult)
    assert fb.y.shape == (F, H, W) and fb.u.shape == (F, ch, cw) and fb.v.shape == (F, ch, cw)
    fb.u[...] = 1
    fb.v[...] = 2
    assert np.all(fb.buf[:, :W * H] == 0) and np.all(fb.buf[:, W * H:W * H + cw * ch] == 1)
    assert np.all(fb.buf[:, W * H + cw * ch:] == 2)
    d = fb.descriptor()
    base = fb.buf.ctypes.data
    assert [d.data[p] for p in range(3)] == [base, base + W * H * 2, base + (W * H + cw * ch) * 2]
    assert [d.linesize[p] for p in range(3)] == [W * 2, cw * 2, cw * 2]
    assert [d.frame_pitch[p] for p in range(3)] == [W * H * mult * 2] * 3
    assert (d.width, d.height, d.bits) == (W, H, bits)
    assert hdr2sdr.frames.frame_bytes(W, H, bits, sub) == W * H * mult * 2


def test_frame_batch_carries_the_subsampling():
    W, H = 16, 8
    assert FrameBatch.empty_numpy(2, W, H, 10).subsampling == '420'
    fb = FrameBatch.empty_numpy(4, W, H, 10, subsampling='422')
    assert fb.slice(1, 3).subsampling == '422' and fb.slice(1, 3).nframes == 2
    assert fb.to_numpy().subsampling == '422'
    assert FrameBatch.empty_pinned(2, W, H, 12, 'planar', '444').subsampling == '444'
    pytest.importorskip('torch')
    t = fb.to_torch('cpu')
    assert t.subsampling == '422' and tuple(t.u.shape) == (4, H, W // 2) and t.to_numpy().subsampling == '422'
    assert FrameBatch.empty_torch(1, W, H, 10, 'cpu', 'planar', '444').buf.shape == (1, W * H * 3)
    y = np.zeros((1, H, W), np.uint16)
    assert FrameBatch.from_planes(y, np.ones((1, H, W), np.uint16), y, 10, '444').u.sum() == W * H


def test_frame_batch_refusals():
    buf = np.zeros((1, 16 * 8 * 2), np.uint16)
    with pytest.raises(ValueError):
        FrameBatch(buf, 16, 8, 10, 'semi', '422')
    with pytest.raises(ValueError):
        FrameBatch.empty_numpy(1, 16, 8, 10, 'semi', '444')
    with pytest.raises(ValueError):
        FrameBatch(buf, 16, 8, 10, 'planar', '411')
    for w, h in ((15, 8), (16, 7)):
        with pytest.raises(ValueError):
            FrameBatch.empty_numpy(1, w, h, 10, 'planar', '444')
    with pytest.raises(ValueError):
        FrameBatch.empty_numpy(1, 16, 8, 10, subsampling='422').to_layout('semi')


# ---- planner ------------------------------------------------------------------
def test_plan_pipes_the_source_subsampling():
    argv = GOLD['C2']['argv']
    W, H = PROPS10['width'], PROPS10['height']
    pl = P.plan_from_argv(argv, PROPS10)
    assert pl.in_subsampling == '420' and pl.decode[-2] == 'yuv420p10le' and pl.frame_bytes_in == W * H * 3
    pl = P.plan_from_argv(argv, PROPS10, in_subsampling='422')
    assert pl.in_subsampling == '422' and pl.decode[-3:] == ['-pix_fmt', 'yuv422p10le', '-']
    assert pl.frame_bytes_in == W * H * 2 * 2 and pl.frame_bytes_out == W * H * 3
    pl = P.plan_from_argv(argv, dict(PROPS10, bit_depth=12), in_subsampling='444')
    assert pl.decode[-2] == 'yuv444p12le' and pl.frame_bytes_in == W * H * 3 * 2
    # 'auto': ffprobe's pix_fmt when the properties carry it, else 4:2:0
    assert P.plan_from_argv(argv, PROPS10, in_subsampling='auto').in_subsampling == '420'
    for fmt, sub in (('yuv422p10le', '422'), ('yuv444p12le', '444'), ('yuv420p10le', '420'), ('gbrp10le', '420')):
        pl = P.plan_from_argv(argv, dict(PROPS10, pix_fmt=fmt), in_subsampling='auto')
        assert pl.in_subsampling == sub
    assert P.plan_from_argv(argv, dict(PROPS10, pix_fmt='yuv422p10le'), in_subsampling='auto').decode[-2] == 'yuv422p10le'
    # the libplacebo chain uploads format=p010: 4:2:0 whatever is asked
    pl = P.plan_from_argv(GOLD['C3']['argv'], dict(PROPS10, pix_fmt='yuv444p10le'), in_subsampling='444')
    assert pl.in_subsampling == '420' and pl.decode[-2] == 'yuv420p10le' and pl.frame_bytes_in == W * H * 3
    with pytest.raises(ValueError):
        P.plan_from_argv(argv, PROPS10, in_subsampling='411')
    with pytest.raises(ValueError):
        P.plan_from_argv(argv, PROPS10, in_layout='semi', in_subsampling='422')


# ---- ABI ------------------------------------------------------------------------
def test_abi_binds_and_exports_the_call():
    assert 'h2s_set_input_subsampling' in _abi.EXPORTS
    assert _abi.SUBSAMPLINGS == {'420': 0, '422': 1, '444': 2}
    L = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(L, 'h2s_set_input_subsampling')
    assert L.h2s_abi_version() == 3 and L.h2s_abi_minor() == 4     # the numbers stay


def test_null_context_and_unknown_value_are_invalid_arg():
    L = ctypes.CDLL(_abi.LIB_PATH)
    L.h2s_set_input_subsampling.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.h2s_last_error.restype = ctypes.c_char_p
    L.h2s_last_error.argtypes = [ctypes.c_void_p]
    assert L.h2s_set_input_subsampling(None, 0) == _abi.H2S_E_INVALID_ARG
    assert L.h2s_last_error(None)
    assert L.h2s_set_input_subsampling(None, 3) == _abi.H2S_E_INVALID_ARG
