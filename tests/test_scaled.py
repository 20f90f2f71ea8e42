"""The scaled 4:2:0 output without a GPU: the size rule, the planner's
``scale=`` and the restatement in tests/scaled_ref.py itself.

The GPU gate (tests/test_gpu_scaled.py) holds the kernel to the float64
restatement within 1 code on at most 0.5 % of a plane.  Here the float32
evaluation of the same chains is held to that gate on every content x size the
GPU test uses, with the oracle's chain output as the stand-in intermediate: the
cap is reachable by the model's own arithmetic.  Two mutants of the model
(left-aligned sampling, unwidened 4-tap support) must miss it."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import hdr2sdr
import oracle
import scaled_ref as ref
from hdr2sdr import plan as P
from hdr2sdr.synth import synth_frames

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'filter_chains.json')))
PROPS10 = {'width': 3840, 'height': 2160, 'bit_depth': 10, 'color_transfer': 'smpte2084', 'frame_rate': 24.0}

# hand-computed: av_rescale (round half up) of the box by the aspect, min with
# the box, then each dimension down to even
SIZES = [
    ((3840, 2160, 1920, 1080), (1920, 1080)),
    ((4096, 1716, 1920, 1080), (1920, 804)),     # 1920 * 1716 / 4096 = 804.4
    ((2160, 3840, 1920, 1080), (608, 1080)),     # portrait: 1080 * 2160 / 3840 = 607.5 -> 608
    ((1280, 720, 3840, 2160), (3840, 2160)),     # a box larger than the source: upscaled, as ffmpeg's scale does
    ((1000, 562, 333, 333), (332, 186)),         # 333 -> 332; 333 * 562 / 1000 = 187.1 -> 187 -> 186
    ((3840, 2160, 1280, 720), (1280, 720)),
    ((4000, 2, 100, 100), (100, 2)),             # 100 * 2 / 4000 rounds to 0: not below 2
]


@pytest.mark.parametrize('args,want', SIZES)
def test_scaled_size_hand_computed(args, want):
    assert hdr2sdr.scaled_size(*args) == want
    assert all(v % 2 == 0 and v >= 2 for v in hdr2sdr.scaled_size(*args))


def test_scaled_size_rejects_empty():
    with pytest.raises(ValueError):
        hdr2sdr.scaled_size(0, 10, 10, 10)


def test_scaled_size_python_and_c_agree():
    try:
        L = hdr2sdr.lib()
    except ImportError:
        pytest.skip('libh2s.so is not built')
    rng = np.random.default_rng(5)
    cases = [a for a, _ in SIZES] + [tuple(int(v) for v in rng.integers(1, 9000, 4)) for _ in range(300)]
    for a in cases:
        w, h = ctypes.c_int(), ctypes.c_int()
        assert L.h2s_scaled_size(*a, ctypes.byref(w), ctypes.byref(h)) == 0
        assert (w.value, h.value) == hdr2sdr.scaled_size(*a), a
    assert L.h2s_scaled_size(0, 1, 1, 1, ctypes.byref(w), ctypes.byref(h)) == hdr2sdr._abi.H2S_E_INVALID_ARG


# ---- the planner ---------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', ['C2', 'C5', 'default8'])
@pytest.mark.parametrize('box', [(1920, 1080), (1280, 720)])
def test_plan_with_scale_sizes_the_encode_pipe(cfg, box):
    pl = P.plan_from_argv(GOLD[cfg]['argv'], PROPS10, scale=box)
    assert (pl.out_width, pl.out_height) == box and (pl.width, pl.height) == (3840, 2160) and pl.scaled
    assert pl.encode[pl.encode.index('-s') + 1] == f'{box[0]}x{box[1]}'
    bps = 1 if pl.params.bits_out == 8 else 2
    assert pl.frame_bytes_out == box[0] * box[1] * 3 // 2 * bps
    assert pl.frame_bytes_in == 3840 * 2160 * 3 // 2 * 2
    base = P.plan_from_argv(GOLD[cfg]['argv'], PROPS10)
    assert pl.decode == base.decode                      # the decode side does not change
    i = pl.encode.index('-s') + 1
    assert pl.encode[:i] + pl.encode[i + 1:] == base.encode[:i] + base.encode[i + 1:]   # -s alone does


def test_plan_scale_fits_the_aspect():
    pl = P.plan_from_argv(GOLD['C2']['argv'], dict(PROPS10, width=4096, height=1716), scale=(1920, 1080))
    assert (pl.out_width, pl.out_height) == (1920, 804)
    assert pl.encode[pl.encode.index('-s') + 1] == '1920x804'


ARGV_GOLDENS = sorted(k for k, v in GOLD.items() if isinstance(v, dict) and 'argv' in v)


@pytest.mark.parametrize('cfg', ARGV_GOLDENS)
def test_plan_without_scale_is_unchanged(cfg):
    props = dict(PROPS10, bit_depth=12, color_transfer='arib-std-b67') if cfg == 'C5' else PROPS10
    base = P.plan_from_argv(GOLD[cfg]['argv'], props)
    pl = P.plan_from_argv(GOLD[cfg]['argv'], props, scale=None)
    assert (pl.decode, pl.encode) == (base.decode, base.encode)
    assert (pl.out_width, pl.out_height) == (pl.width, pl.height) == (3840, 2160) and not pl.scaled
    assert pl.encode[pl.encode.index('-s') + 1] == '3840x2160'
    bps = 1 if pl.params.bits_out == 8 else 2
    assert pl.frame_bytes_out == 3840 * 2160 * 3 // 2 * bps
    # a box of the source's own size is no scaling either
    same = P.plan_from_argv(GOLD[cfg]['argv'], props, scale=(3840, 2160))
    assert (same.decode, same.encode, same.scaled) == (base.decode, base.encode, False)


def test_pipeplan_defaults_to_the_source_size():
    pl = P.PipePlan(decode=[], encode=[], params=hdr2sdr.TonemapParams(), lut_path=None, width=64, height=32,
                    input_path='a', output_path='b')
    assert (pl.out_width, pl.out_height, pl.scaled) == (64, 32, False)


# ---- the restatement -------------------------------------------------------------------------
PARAMS = hdr2sdr.TonemapParams(tonemapper='hable', gamma=2.2, bits_in=10, bits_out=10)   # C2, compat8: q = 8


@functools.lru_cache(maxsize=None)
def _lattice():
    return hdr2sdr.generate_lattice(33)


@functools.lru_cache(maxsize=None)
def _intermediate(case_id, kind):
    """The oracle's chain output for a case's source: the stand-in intermediate."""
    _, W, H, _, _ = ref.BY_ID[case_id]
    src = synth_frames(kind, 1, W, H, 10, seed=0x5CA1E).to_numpy()
    return oracle.process(oracle.params_from(PARAMS.to_c()), _lattice(), src.buf, W, H)


@functools.lru_cache(maxsize=None)
def _want(case_id, kind):
    _, W, H, ow, oh = ref.BY_ID[case_id]
    return ref.expected(_intermediate(case_id, kind), W, H, ow, oh, 8, 10)


@pytest.mark.parametrize('kind', ref.CONTENTS)
@pytest.mark.parametrize('case_id', sorted(ref.BY_ID))
def test_float32_evaluation_meets_the_gate(case_id, kind):
    _, W, H, ow, oh = ref.BY_ID[case_id]
    got = ref.expected(_intermediate(case_id, kind), W, H, ow, oh, 8, 10, dtype=np.float32)
    mx, frac = ref.gate_planes(got, _want(case_id, kind), ow, oh, shift=2)
    print(f'{case_id} {kind}: float32 vs float64 max diff {mx}, {frac:.4%} of the worst plane')
    assert mx <= ref.MAX_DIFF and frac <= ref.MAX_FRACTION


def test_expected_output_is_expanded_codes():
    want = _want('2to1', 'uniform')
    assert want.shape == (1, 96 * 48 * 3 // 2)
    assert (want & 3 == 0).all() and want.max() <= 255 << 2     # shift expansion of 8-bit codes
    rep = ref.expected(_intermediate('2to1', 'uniform'), 192, 96, 96, 48, 8, 10, 'replicate')
    assert np.array_equal(rep >> 2, want >> 2) and np.array_equal(rep & 3, rep >> 8)


def test_flat_plane_stays_flat():
    for W, H, ow, oh in [(192, 96, 96, 48), (64, 64, 128, 128), (384, 192, 32, 16)]:
        for dt in (np.float64, np.float32):
            out = ref.resize_plane(np.full((H, W), 137), ow, oh, 255, dt)
            assert (out == 137).all()


@pytest.mark.parametrize('kind', ref.CONTENTS)
@pytest.mark.parametrize('mutant', [{'centre': False}, {'widen': False}])
def test_mutants_miss_the_gate(mutant, kind):
    """Left-aligned sampling, and 4 unwidened taps at 2 : 1, are other resizes."""
    y, u, v = (p[0] >> 2 for p in ref.planes_of(_intermediate('2to1', kind), 192, 96))
    true = ref.scaled(y, u, v, 96, 48, 8)
    wrong = ref.scaled(y, u, v, 96, 48, 8, **mutant)
    for t, w in zip(true, wrong):
        mx, frac = ref.gate(w, t)
        print(f'{mutant} {kind}: max diff {mx}, {frac:.4%}')
        assert mx > ref.MAX_DIFF or frac > ref.MAX_FRACTION
