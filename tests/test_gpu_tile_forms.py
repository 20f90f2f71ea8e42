"""GPU: the tile kernel's interior / border equalities on the frame forms
test_tile_interior_boundaries (planar 4:2:0) does not reach: semi-planar sets
on either side, and 4:2:2 / 4:4:4 input.

k_tile addresses a tile from launch-constant lane offsets plus one scalar
origin when its rows and its chroma window lie inside the frame, and clamps per
lane otherwise; each input form has its own window (4:2:0: cy0 >= 1,
cy0 + 17 <= ch, cx0 + 33 <= cw; 4:2:2: py0 + 32 <= H, cx0 + 33 <= icw; 4:4:4:
py0 + 32 <= H).  130x98 and 194x66 put tiles exactly on each equality
(cw = icw = 32k + 1, ch = 16m + 1); rows padded to 16 bytes send them through
the tile kernel (+ k_process for the W % 64 columns)."""
import numpy as np
import pytest

import hdr2sdr
import oracle
import subsampling_ref as SR
from hdr2sdr import _abi
from hdr2sdr.synth import synth_frames
from padded_frames import FILL, RowPadded
from test_gpu_parity import assert_close_int

pytestmark = pytest.mark.gpu

NF = 2
LUT_N = 17
SIZES = [(130, 98), (194, 66)]
_LAT = {}


def lat():
    if LUT_N not in _LAT:
        _LAT[LUT_N] = hdr2sdr.generate_lattice(LUT_N)
    return _LAT[LUT_N]


@pytest.fixture(scope='module')
def tm():
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.close()


def convert(tm, fb, bits_out, out_layout='planar'):
    """A host batch through the tile kernel on padded surfaces -> the tight host result."""
    import torch
    src = RowPadded(NF, fb.width, fb.height, fb.bits, fb.layout, fb.subsampling).load(fb)
    dst = RowPadded(NF, fb.width, fb.height, bits_out, out_layout)
    assert tm.query_path(src, dst) == _abi.PATH_TILE_TAIL
    tm.process(src, dst)
    torch.cuda.synchronize()
    raw = dst.raw().reshape(NF, -1)
    for _, ls, rows, rowb in dst.planes:      # nothing lands between the rows
        assert ls == rowb or (raw[:, :rows * ls].reshape(NF, rows, ls)[:, :, rowb:] == FILL).all()
        raw = raw[:, rows * ls:]
    return dst.to_numpy()


@pytest.mark.parametrize('W,H', SIZES)
@pytest.mark.parametrize('tmname', ['hable', 'bt.2390'])
def test_semi_planar_interior_boundaries(tm, W, H, tmname):
    """Semi-planar input and output equal the planar run repacked, exactly."""
    params = hdr2sdr.TonemapParams(tonemapper=tmname, gamma=2.2 if tmname == 'hable' else 1.0)
    tm.set_params(params)
    tm.set_lut(lat())
    planar = synth_frames('smooth', NF, W, H, 10, device='cpu', seed=11).to_numpy()
    src = {'planar': planar, 'semi': planar.to_layout('semi')}
    want = convert(tm, planar, 10)
    for il, ol in (('semi', 'semi'), ('semi', 'planar'), ('planar', 'semi')):
        got = convert(tm, src[il], 10, ol)
        assert got.layout == ol and np.array_equal(got.buf, want.to_layout(ol).buf), (il, ol)


@pytest.mark.parametrize('W,H', SIZES)
@pytest.mark.parametrize('sub', ['422', '444'])
def test_subsampled_input_interior_boundaries(tm, W, H, sub):
    """The exact 4:2:2 / 4:4:4 upsamples of a 4:2:0 frame: the oracle's result
    for that frame within the suite's gate, and the GPU's own 4:2:0 output
    exactly wherever the tile kernel wrote it (luma x < 64 floor(W / 64), chroma
    cx < 32 floor(W / 64); the columns right of that are k_process's, whose
    exact arithmetic is not the tile kernel's float32 bit for bit)."""
    params = hdr2sdr.TonemapParams(tonemapper='hable', gamma=2.2, bits_out=10)
    tm.set_params(params)
    tm.set_lut(lat())
    fb = SR.round8(synth_frames('smooth', NF, W, H, 10, device='cpu', seed=11).to_numpy())
    got = convert(tm, SR.exact_inputs(fb)[sub], 10)
    own = convert(tm, fb, 10)
    want = oracle.process(oracle.params_from(params.to_c()), lat(), fb.buf, W, H).astype(np.int64)
    assert_close_int(params, got.buf.astype(np.int64), want, W, H, fb.buf, lut_n=LUT_N)
    tw = W // 64 * 64
    for name, cols in (('y', tw), ('u', tw // 2), ('v', tw // 2)):
        a, b = getattr(got, name)[..., :cols], getattr(own, name)[..., :cols]
        print(f'TILE-FORMS {W}x{H} {sub} {name}: {int((a != b).sum())} of {a.size} tiled samples differ from the 4:2:0 run')
        assert np.array_equal(a, b), name
