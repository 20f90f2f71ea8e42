"""GPU: k_tile's wave -> sub-block mapping (h2s_tile.h, "per-lane step
geometry"): in step m the four waves of a block are the four 8x8 quarters of
the tile's 16x16 macro-block (m & 3, m >> 2), and a quarter whose rows lie past
the frame's last row is skipped per wave.

The shapes are the smallest at which the mapping can go wrong.  Widths 64 and
128: one tile, and two (the macro walk crosses a tile edge and the LDS slots are
refilled).  Heights 8, 16, 24, 32, 40 and 56: the last tile row has 8, 16, 24
or 32 live rows, i.e. every combination of skipped and computed quarters
(8: only the upper waves' first macro-row; 16: all waves' first macro-row; 24:
the upper waves' second macro-row too), alone and under a full tile row.  Two
frames, against the oracle under the suite's integer gate (assert_close_int),
for the forms whose position-dependent values follow the mapping:

* C2's parameters, 10 -> 10 bit (the per-lane LDS bases and step offsets);
* the libplacebo branch (bt.2390): the software-pipelined loop's two halves,
  and with the download dither the per-lane Bayer offset;
* 8-bit output with ordered dither: the luma dither offset and the chroma
  dither rows;
* BICUBIC chroma: the 4:4:4 scratch coordinates;
* 4:2:2 and 4:4:4 input (their own per-lane chroma bases and step offsets);
* top-left 4:2:0 input, held to the library's own 4:2:2 path on the paired
  plane, exactly (test_gpu_source_tags' first check; the 4:2:2 path is held to
  the oracle here);
* a debug stage through h2s_debug_float (the debug-plane index), under the
  suite's float gate;
* a 128x40 launch against the same frames on the generic kernel."""
import numpy as np
import pytest

import hdr2sdr
import source_tags_ref as TR
import subsampling_ref as SR
from hdr2sdr import _abi
from hdr2sdr.frames import FrameBatch
from hdr2sdr.synth import synth_frames
from test_gpu_parity import assert_close_int, check_float_stage, lattice, run_both

pytestmark = pytest.mark.gpu

NF = 2
LUT_N = 17
WIDTHS = [64, 128]
HEIGHTS = [8, 16, 24, 32, 40, 56]
FORMS = {
    'c2_10_10': dict(tonemapper='hable', gamma=2.2, bits_out=10),
    'lp_bt2390': dict(tonemapper='bt.2390', gamma=1.0, bits_out=10),
    'lp_bt2390_download_dither': dict(tonemapper='bt.2390', gamma=1.0, bits_out=10, lp_dither='ordered'),
    'c2_8bit_ordered_dither': dict(tonemapper='hable', gamma=2.2, bits_out=8, dither='ordered'),
    'c2_bicubic': dict(tonemapper='hable', gamma=2.2, bits_out=10, chroma_filter='bicubic'),
}
C2 = FORMS['c2_10_10']
_CACHE = {}


@pytest.fixture(scope='module')
def tm():
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.close()


def on_tile(tm, src, bits_out):
    dst = FrameBatch.empty_torch(src.nframes, src.width, src.height, bits_out, 'cuda')
    return tm.query_path(src.to_torch('cuda'), dst) == _abi.PATH_TILE


def gpu(tm, src, bits_out):
    import torch
    dst = FrameBatch.empty_torch(src.nframes, src.width, src.height, bits_out, 'cuda')
    tm.process(src.to_torch('cuda'), dst)
    torch.cuda.synchronize()
    return dst.to_numpy().buf.astype(np.int64)


def rounded_source(W, H):
    """A 4:2:0 batch whose chroma codes are multiples of 8 (its 4:2:2 / 4:4:4
    upsamples are exact), made once."""
    if (W, H) not in _CACHE:
        _CACHE[W, H] = SR.round8(synth_frames('smooth', NF, W, H, 10, device='cpu', seed=11).to_numpy())
    return _CACHE[W, H]


@pytest.mark.parametrize('H', HEIGHTS)
@pytest.mark.parametrize('W', WIDTHS)
@pytest.mark.parametrize('form', sorted(FORMS))
def test_macro_block_steps_match_oracle(tm, form, W, H):
    params = hdr2sdr.TonemapParams(**FORMS[form])
    got, want, wh = run_both(tm, params, 'smooth', W, H, nframes=NF, lut_n=LUT_N)
    assert on_tile(tm, synth_frames('smooth', NF, W, H, params.bits_in, device='cpu', seed=11), params.bits_out)
    d = np.abs(got - want)
    print(f'TILE-MACRO {form} {W}x{H}: {int((d > 0).sum())} of {d.size} samples differ, max {int(d.max())}')
    assert_close_int(params, got, want, *wh, lut_n=LUT_N)


@pytest.mark.parametrize('H', HEIGHTS)
@pytest.mark.parametrize('W', WIDTHS)
@pytest.mark.parametrize('sub', ['422', '444'])
def test_macro_block_steps_subsampled_input(tm, sub, W, H):
    """The exact 4:2:2 / 4:4:4 upsamples of a 4:2:0 frame against the oracle's
    result for that frame."""
    import oracle
    params = hdr2sdr.TonemapParams(**C2)
    tm.set_params(params)
    tm.set_lut(lattice(LUT_N))
    fb = rounded_source(W, H)
    src = SR.exact_inputs(fb)[sub]
    assert on_tile(tm, src, 10)
    got = gpu(tm, src, 10)
    want = oracle.process(oracle.params_from(params.to_c()), lattice(LUT_N), fb.buf, W, H).astype(np.int64)
    d = np.abs(got - want)
    print(f'TILE-MACRO {sub} {W}x{H}: {int((d > 0).sum())} of {d.size} samples differ, max {int(d.max())}')
    assert_close_int(params, got, want, W, H, fb.buf, lut_n=LUT_N)


@pytest.mark.parametrize('H', HEIGHTS)
@pytest.mark.parametrize('W', WIDTHS)
def test_macro_block_steps_topleft_input(tm, W, H):
    """Top-left 4:2:0 input stages the same exact integers as the 4:2:2 path
    on the paired plane: equal outputs, sample for sample."""
    params = hdr2sdr.TonemapParams(**C2)
    tm.set_params(params)
    tm.set_lut(lattice(LUT_N))
    fb = TR.round2(synth_frames('smooth', NF, W, H, 10, device='cpu', seed=11).to_numpy())
    src = TR.tagged(fb, 'tv', 'topleft')
    assert on_tile(tm, src, 10)
    got = gpu(tm, src, 10)
    assert np.array_equal(got, gpu(tm, TR.as_422(fb), 10))
    assert not np.array_equal(got, gpu(tm, fb, 10))   # (the tag did something)


@pytest.mark.parametrize('H', [40, 56])
@pytest.mark.parametrize('cfg,stage', [('C2_hable_pq10', 4), ('C3_bt2390_libplacebo', 3)])
def test_macro_block_steps_debug_planes(tm, cfg, stage, H):
    """The debug instances write each pixel's plane sample at the mapping's
    position (rows past the frame: nowhere)."""
    check_float_stage(tm, 'k_tile', cfg, 'uniform', stage, W=128, H=H)


@pytest.mark.parametrize('form', ['c2_10_10', 'lp_bt2390'])
def test_macro_block_steps_equal_generic_kernel(tm, form):
    """128x40 on the tile kernel against the same frames on the generic
    kernel (test_switch_pair_tile_equals_generic's check)."""
    params = hdr2sdr.TonemapParams(**FORMS[form])
    W, H = 128, 40
    host = synth_frames('smooth', NF, W, H, params.bits_in, device='cpu', seed=9)
    tm.set_params(params)
    tm.set_lut(lattice(LUT_N))
    assert on_tile(tm, host, params.bits_out)
    tile = gpu(tm, host, params.bits_out)
    tm.set_option(_abi.OPT_FAST_PATH, 0)
    try:
        assert not on_tile(tm, host, params.bits_out)
        gen = gpu(tm, host, params.bits_out)
    finally:
        tm.set_option(_abi.OPT_FAST_PATH, 1)
    assert_close_int(params, tile, gen, W, H, host.to_numpy().buf, lut_n=LUT_N)
    assert (tile == gen).mean() > 0.99
