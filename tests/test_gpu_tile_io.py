"""GPU: k_tile's per-tile frame I/O (commit, prefetch, stores, two barriers)
against the oracle, under the suite's integer gates (assert_close_int).

The tile loop commits a tile's registers to LDS behind the previous tile's
stores and with no barrier between them; every thread issues one 16-byte luma
and one 16-byte chroma store per tile (rows past the frame, threads without a
chroma role and the odd thread of an 8-bit pair store at an offset the buffer
resource drops); a bottom tile skips the step pairs whose rows lie past the
frame.  The shapes are the smallest at which each of these can go wrong:

* 64x32, 1 frame: one tile, no prefetch (the `more == false` exit at once);
* 128x48, 1 frame: a bottom tile row with 16 real rows (clamped load rows,
  dropped stores, skipped steps);
* 256x96, 3 frames: 36 tiles, 8 per block: blocks that walk a frame boundary
  and a last block of 4 tiles (LDS slots refilled with no third barrier);
* 192x64 with rows 256-byte aligned (a luma pitch of 512 > 2 W): nothing may
  land between the rows.

Contents: seeded noise of legal codes (every tile on the fast body), and the
same with patches of the extreme codes in every other tile (luma 0, black,
just above black, white, full scale, with extreme chroma), so that those tiles
take the exact-capable body and its dark re-run while their neighbours take
the fast body.  Surfaces are device buffers with padded rows; the bytes
between the rows must come back untouched."""
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

LUT_N = 17
# (W, H, frames, row alignment in bytes)
SHAPES = {
    '64x32x1': (64, 32, 1, 16),
    '128x48x1': (128, 48, 1, 16),
    '256x96x3': (256, 96, 3, 16),
    '192x64_pitch': (192, 64, 2, 256),
}
# parameters, input (layout, subsampling), output layout
FORMS = {
    'planar_10_10': (dict(tonemapper='hable', gamma=2.2, bits_out=10), ('planar', '420'), 'planar'),
    'planar_10_8': (dict(tonemapper='hable', gamma=2.2, bits_out=8), ('planar', '420'), 'planar'),
    'hlg_12_12': (dict(tonemapper='hable', gamma=1.0, bits_in=12, bits_out=12, transfer='arib-std-b67'),
                  ('planar', '420'), 'planar'),
    'p010_in_out': (dict(tonemapper='hable', gamma=2.2, bits_out=10), ('semi', '420'), 'semi'),
    'libplacebo_bt2390': (dict(tonemapper='bt.2390', gamma=1.0, bits_out=10), ('planar', '420'), 'planar'),
    'yuv444_in': (dict(tonemapper='hable', gamma=2.2, bits_out=10), ('planar', '444'), 'planar'),
}
CONTENTS = ['noise', 'extremes']

_lat = {}
_src = {}
_want = {}


def lat():
    if LUT_N not in _lat:
        _lat[LUT_N] = hdr2sdr.generate_lattice(LUT_N)
    return _lat[LUT_N]


@pytest.fixture(scope='module')
def tm():
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.close()


def source(content, shape, bits, rounded):
    """The seeded 4:2:0 host batch of a case (made once, never modified).
    rounded: chroma codes on multiples of 8, whose 4:4:4 upsample is exact."""
    key = (content, shape, bits, rounded)
    if key in _src:
        return _src[key]
    W, H, nf, _ = SHAPES[shape]
    fb = synth_frames('uniform', nf, W, H, bits, device='cpu', seed=4100 + W + H).to_numpy()
    if content == 'extremes':
        s = 1 << (bits - 10)
        rng = np.random.default_rng(977 + W + H)
        top = (1 << bits) - 1
        luma = np.array([0, 64 * s, 64 * s + 1, 66 * s, 70 * s, 940 * s, top])
        chroma = np.array([0, 64 * s, 512 * s, 960 * s, top])
        for f in range(nf):
            for ty in range((H + 31) // 32):
                for tx in range(W // 64):
                    if (tx + ty + f) & 1:
                        continue   # the neighbour stays on the fast body
                    y0 = 32 * ty + 2 * int(rng.integers(0, 4))
                    x0 = 64 * tx + 2 * int(rng.integers(0, 24))
                    h = min(16, H - y0)
                    fb.y[f, y0:y0 + h, x0:x0 + 16] = rng.choice(luma, (h, 16))
                    fb.u[f, y0 // 2:(y0 + h) // 2, x0 // 2:x0 // 2 + 8] = rng.choice(chroma, (h // 2, 8))
                    fb.v[f, y0 // 2:(y0 + h) // 2, x0 // 2:x0 // 2 + 8] = rng.choice(chroma, (h // 2, 8))
    if rounded:
        fb = SR.round8(fb)
    _src[key] = fb
    return fb


def oracle_result(form, content, shape):
    key = (form, content, shape)
    if key not in _want:
        kw, (_, sub), _ = FORMS[form]
        params = hdr2sdr.TonemapParams(**kw)
        W, H, _, _ = SHAPES[shape]
        fb = source(content, shape, params.bits_in, sub != '420')
        _want[key] = oracle.process(oracle.params_from(params.to_c()), lat(), fb.buf, W, H).astype(np.int64)
    return _want[key]


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('form', sorted(FORMS))
def test_tile_io_matches_oracle(tm, form, shape, content):
    import torch
    kw, (in_layout, sub), out_layout = FORMS[form]
    params = hdr2sdr.TonemapParams(**kw)
    W, H, nf, align = SHAPES[shape]
    fb = source(content, shape, params.bits_in, sub != '420')
    host = fb
    if sub != '420':
        host = SR.exact_inputs(fb)[sub]
    if in_layout == 'semi':
        host = host.to_layout('semi')
    tm.set_params(params)
    tm.set_lut(lat())
    src = RowPadded(nf, W, H, params.bits_in, in_layout, sub, align=align).load(host)
    dst = RowPadded(nf, W, H, params.bits_out, out_layout, align=align)
    assert tm.query_path(src, dst) == _abi.PATH_TILE
    tm.process(src, dst)
    torch.cuda.synchronize()
    raw = dst.raw().reshape(nf, -1)
    for _, ls, rows, rowb in dst.planes:      # nothing lands between the rows
        assert ls == rowb or (raw[:, :rows * ls].reshape(nf, rows, ls)[:, :, rowb:] == FILL).all()
        raw = raw[:, rows * ls:]
    got = dst.to_numpy()
    if out_layout == 'semi':
        got = got.to_layout('planar')
    want = oracle_result(form, content, shape)
    g = got.buf.astype(np.int64)
    d = np.abs(g - want)
    print(f'TILE-IO {form} {shape} {content}: {int((d > 0).sum())} of {d.size} samples differ, max {int(d.max())}')
    assert_close_int(params, g, want, W, H, fb.buf, lut_n=LUT_N)
