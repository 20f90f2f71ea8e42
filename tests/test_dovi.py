"""Dolby Vision profile 5 without a GPU: the ABI's struct layouts and record
validation, ``DoviRpu.from_fixed_point``, the planner and ``from_request`` with
and without ``dovi=``, and the preconditions of the constructions the GPU tests
take their expected values from (tests/dovi_ref.py)."""
import ctypes
import json
import math
import os
import subprocess
import types

import numpy as np
import pytest

import dovi_ref as DR
import hdr2sdr
import oracle
import test_oracle_independent as toi
from hdr2sdr import _abi
from hdr2sdr import chain as C
from hdr2sdr import dovi as D
from hdr2sdr import plan as P
from hdr2sdr.dovi import DoviCurve, DoviRpu
from hdr2sdr.synth import synth_frames

from conftest import REPO

HEADER = os.path.join(REPO, 'include', 'h2s.h')

PROBE = r'''
#include <stddef.h>
#include <stdio.h>
#include "h2s.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(h2s_dovi_curve), offsetof(h2s_dovi_curve, pivots),
         offsetof(h2s_dovi_curve, method), offsetof(h2s_dovi_curve, poly), offsetof(h2s_dovi_curve, mmr_order),
         offsetof(h2s_dovi_curve, mmr_const), offsetof(h2s_dovi_curve, mmr), sizeof(h2s_dovi_rpu),
         offsetof(h2s_dovi_rpu, nonlinear), offsetof(h2s_dovi_rpu, linear), offsetof(h2s_dovi_rpu, comp),
         sizeof(((h2s_dovi_curve *)0)->mmr[0]));
  return 0;
}
'''


def test_struct_layouts_match_c(tmp_path):
    c = tmp_path / 'probe.c'
    c.write_text(PROBE)
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.dirname(HEADER), str(c), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    K, R = D.H2SDoviCurve, D.H2SDoviRpu
    assert got == [ctypes.sizeof(K), K.pivots.offset, K.method.offset, K.poly.offset, K.mmr_order.offset,
                   K.mmr_const.offset, K.mmr.offset, ctypes.sizeof(R), R.nonlinear.offset, R.linear.offset,
                   R.comp.offset, 3 * 7 * 4]


def test_symbol_is_exported_and_bound():
    assert 'h2s_set_dovi' in _abi.EXPORTS
    assert _abi.lib().h2s_set_dovi.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert _abi.lib().h2s_abi_minor() == 4          # the symbol's presence is the feature test


def _rc(rec, n=1):
    """h2s_set_dovi on no context: the records are judged first, so a valid
    set ends in "ctx is NULL" and an invalid one in its own message."""
    L = _abi.lib()
    arr = (D.H2SDoviRpu * 1)(rec)
    rc = L.h2s_set_dovi(None, ctypes.addressof(arr), n)
    return rc, L.h2s_last_error(None).decode()


def test_validation_errors():
    good = DR.realistic_record(10).to_c()
    rc, msg = _rc(good)
    assert rc == _abi.H2S_E_INVALID_ARG and msg == 'ctx is NULL'

    def broken(edit):
        r = DR.realistic_record(10).to_c()
        edit(r)
        rc, msg = _rc(r)
        assert rc == _abi.H2S_E_INVALID_ARG and msg != 'ctx is NULL', msg
        return msg

    def set_(path, value):
        def edit(r):
            obj = r
            for p in path[:-1]:
                obj = obj[p] if isinstance(p, int) else getattr(obj, p)
            if isinstance(path[-1], int):
                obj[path[-1]] = value
            else:
                setattr(obj, path[-1], value)
        return edit

    assert 'num_pivots' in broken(set_(('comp', 0, 'num_pivots'), 1))
    assert 'num_pivots' in broken(set_(('comp', 2, 'num_pivots'), 10))
    assert 'ascend' in broken(set_(('comp', 0, 'pivots', 3), 0.01))
    assert '[0, 1]' in broken(set_(('comp', 1, 'pivots', 1), 1.5))
    assert '[0, 1]' in broken(set_(('comp', 1, 'pivots', 0), -0.1))
    assert 'method' in broken(set_(('comp', 0, 'method', 7), 2))
    assert 'mmr_order' in broken(set_(('comp', 1, 'mmr_order', 0), 4))
    assert 'mmr_order' in broken(set_(('comp', 2, 'mmr_order', 0), 0))
    assert 'finite' in broken(set_(('comp', 0, 'poly', 2, 1), math.nan))
    assert 'finite' in broken(set_(('comp', 1, 'mmr', 0, 2, 6), math.inf))
    assert 'finite' in broken(set_(('comp', 2, 'mmr_const', 0), math.nan))
    assert 'finite' in broken(set_(('linear', 4), math.inf))
    assert 'finite' in broken(set_(('nonlinear_offset', 1), math.nan))
    # what a piece does not use is not judged: an MMR coefficient of a polynomial
    # piece, a piece past the last pivot
    for path in (('comp', 0, 'mmr', 0, 0, 0), ('comp', 1, 'poly', 5, 0), ('comp', 1, 'method', 3)):
        r = DR.realistic_record(10).to_c()
        set_(path, math.nan if path[-2] != 'method' else 9)(r)
        assert _rc(r)[1] == 'ctx is NULL'
    L = _abi.lib()
    assert L.h2s_set_dovi(None, None, 1) == _abi.H2S_E_INVALID_ARG and b'NULL' in L.h2s_last_error(None)
    assert L.h2s_set_dovi(None, None, -1) == _abi.H2S_E_INVALID_ARG


def test_dataclass_checks():
    with pytest.raises(ValueError):
        DoviCurve(pivots=(0.0,))
    with pytest.raises(ValueError):
        DoviCurve(pivots=(0.0, 0.5, 1.0))                    # two pieces, one of each array
    with pytest.raises(ValueError):
        DoviRpu(nonlinear=(1.0,) * 8)
    with pytest.raises(ValueError):
        DoviRpu.identity(8)
    with pytest.raises(ValueError):
        D.records_to_c([DoviRpu(), 'x'])
    ident = DoviRpu.identity(12).to_c()
    assert list(ident.nonlinear) == list(ident.linear) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert ident.comp[1].num_pivots == 2 and list(ident.comp[1].poly[0]) == [0.0, 1.0, 0.0]
    assert _rc(ident)[1] == 'ctx is NULL'
    assert len(D.records_to_c(DoviRpu())) == 1 and len(D.records_to_c([DoviRpu()] * 3)) == 3


def test_from_fixed_point_arithmetic():
    den = 1 << 23
    r = DoviRpu.from_fixed_point(
        10, pivots=[[0, 256, 1023], [0, 1023], [64, 960]], methods=[[0, 0], [1], [0]],
        poly_coef=[[[den // 4, den, -den // 2], [0, 2 * den]], [None], [[den // 8, den // 2]]],
        mmr_order=[[0, 0], [2], [0]], mmr_constant=[[0, 0], [den // 16], [0]],
        mmr_coef=[[None, None], [[[den, 0, 0, 0, 0, 0, den // 2], [0, -den, 0, 0, 0, 0, 0], [9] * 7]], [None]],
        coef_log2_denom=23, ycc_to_rgb_matrix=[8192, 0, 4096, 8192, -2048, 0, 8192, 0, 0],
        ycc_to_rgb_offset=[0, 1 << 27, 1 << 26], rgb_to_lms_matrix=[16384, 0, 0, 0, 8192, 8192, 0, 0, 16384])
    assert r.comp[0].pivots == (0.0, 256 / 1023, 1.0) and r.comp[2].pivots == (64 / 1023, 960 / 1023)
    assert r.comp[0].poly == ((0.25, 1.0, -0.5), (0.0, 2.0, 0.0)) and r.comp[2].poly == ((0.125, 0.5, 0.0),)
    assert r.comp[1].method == (1,) and r.comp[1].mmr_order == (2,) and r.comp[1].mmr_const == (1 / 16,)
    assert r.comp[1].mmr[0][0] == (1.0, 0, 0, 0, 0, 0, 0.5) and r.comp[1].mmr[0][1][1] == -1.0
    assert r.comp[1].mmr[0][2] == (0.0,) * 7                 # past the order: not taken
    assert r.nonlinear == (1.0, 0.0, 0.5, 1.0, -0.25, 0.0, 1.0, 0.0, 0.0)
    assert r.nonlinear_offset == (0.0, 0.5, 0.25)
    want = np.array(D.LMS_TO_BT2020) @ np.array([[1, 0, 0], [0, 0.5, 0.5], [0, 0, 1.0]])
    assert np.allclose(np.array(r.linear).reshape(3, 3), want, rtol=0, atol=1e-15)
    assert np.abs(np.array(D.LMS_TO_BT2020).sum(axis=1) - 1.0).max() < 2e-4
    other = DoviRpu.from_fixed_point(
        12, [[0, 4095]] * 3, [[0]] * 3, [[[0, den]]] * 3, [[0]] * 3, [[0]] * 3, [[None]] * 3, 23,
        [8192, 0, 0, 0, 8192, 0, 0, 0, 8192], [0, 0, 0], [16384, 0, 0, 0, 16384, 0, 0, 0, 16384], lms_to_bt2020=np.eye(3))
    assert other == DoviRpu.identity(12)
    assert _rc(r.to_c())[1] == 'ctx is NULL' and _rc(DR.realistic_record(12).to_c())[1] == 'ctx is NULL'


# ---- the planner and from_request ----------------------------------------------------------
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'filter_chains.json')))
RULES = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'request_rules.json')))
PROPS10 = {'width': 3840, 'height': 2160, 'bit_depth': 10, 'color_transfer': 'smpte2084', 'frame_rate': 24.0}


def p5_case():
    case = next(c for c in RULES['cases'] if c.get('props', {}).get('dovi_profile') == 5
                and 'filter_complex' in c and c['pix_fmt'] == 'yuv420p10le')
    argv = list(GOLD['C3']['argv'])
    argv[argv.index('-filter_complex') + 1] = case['filter_complex']
    return argv, dict(PROPS10, **case['props'])


def test_planner_with_and_without_dovi():
    argv, props = p5_case()
    with pytest.raises(ValueError) as e:
        P.plan_from_argv(argv, props)
    assert str(e.value) == C.DOVI_P5_ERROR                   # the refusal is what it was
    rec = DoviRpu.hdr10_equivalent(10)
    pl = P.plan_from_argv(argv, props, dovi=rec)
    assert pl.dovi is rec and pl.params.resolved_pipeline() == 'libplacebo' and pl.params.peak_detect
    # the unspecified transfer such streams carry is no error
    for trc in ('unknown', 'unspecified', 'bt709', ''):
        assert P.plan_from_argv(argv, dict(props, color_transfer=trc), dovi=rec).params.transfer == 'smpte2084'
    fn = lambda first, count: [rec] * count   # noqa: E731
    assert P.plan_from_argv(argv, props, dovi=fn).dovi is fn
    # records for a source that is not profile 5, and a profile-5 argv on the CPU chain
    with pytest.raises(ValueError):
        P.plan_from_argv(GOLD['C3']['argv'], PROPS10, dovi=rec)
    with pytest.raises(ValueError):
        P.plan_from_argv(GOLD['C2']['argv'], props, dovi=rec)
    assert D.resolve_records(rec, 5, 3) == [rec]
    assert D.resolve_records(lambda a, n: [rec] * n, 5, 3) == [rec] * 3
    with pytest.raises(ValueError):
        D.resolve_records(lambda a, n: [rec] * (n + 1), 0, 3)


def test_run_loop_sets_the_records_per_batch(tmp_path):
    from test_plan import _fake_pipes
    argv, props = p5_case()
    asked = []

    def dovi(first, count):
        asked.append((first, count))
        return [DoviRpu.hdr10_equivalent(10)] * count

    class Fake:
        def __init__(self):
            self.log = []

        def set_dovi(self, recs):
            self.log.append(('dovi', len(recs)))

        def process(self, src, dst, stream=None, nframes=None):
            self.log.append(('process', nframes))
            dst.buf[:nframes] = src.buf[:nframes]

    pl = P.plan_from_argv(argv, dict(props, width=64, height=32), dovi=dovi)
    frames = np.full((5, 64 * 32 * 3 // 2), 512, np.uint16)
    _fake_pipes(pl, tmp_path, frames)
    tm = Fake()
    proc = P.H2SProcess(pl, tm, batch=2)
    list(proc.stderr)
    assert proc.wait(timeout=60) == 0 and proc.error is None
    assert asked == [(0, 2), (2, 2), (4, 1)]
    assert tm.log == [('dovi', 2), ('process', 2), ('dovi', 2), ('process', 2), ('dovi', 1), ('process', 1)]


def test_from_request_with_and_without_dovi():
    req = types.SimpleNamespace(tonemapper='Mobius', gamma=1.0, bit_depth=10, use_gpu=False, lut_enabled=True)
    props = {'is_dolby_vision': True, 'dovi_profile': 5}
    with pytest.raises(ValueError) as e:
        hdr2sdr.TonemapParams.from_request(req, properties=props)
    assert str(e.value) == C.DOVI_P5_ERROR
    p = hdr2sdr.TonemapParams.from_request(req, properties=props, dovi=DoviRpu.hdr10_equivalent(10))
    assert p.pipeline == 'libplacebo' and p.peak_detect and p.tonemapper == 'mobius' and p.desat == 0.0
    # the libplacebo probe does not decide: the engine runs the branch natively
    p2 = hdr2sdr.TonemapParams.from_request(req, properties=props, libplacebo_available=False,
                                            dovi=lambda a, n: [DoviRpu()] * n)
    assert p2 == p
    # dovi= changes nothing for another source
    assert hdr2sdr.TonemapParams.from_request(req, dovi=DoviRpu()) == hdr2sdr.TonemapParams.from_request(req)


def test_sharded_runs_refuse_records():
    from hdr2sdr import dist
    with pytest.raises(ValueError, match='Dolby Vision'):
        dist.sync_peak_state(types.SimpleNamespace(dovi_records=3), None, 8)


# ---- the constructions' preconditions -----------------------------------------------------------
@pytest.mark.parametrize('bits', [10, 12])
def test_twin_domain_and_identity(bits):
    """Construction 1: 'smooth' seed 13 lies inside the twin's domain as it is,
    and there the restated model under hdr10_equivalent is the HDR10 decode."""
    fb = synth_frames('smooth', 2, 128, 64, bits, device='cpu', seed=13).to_numpy()
    e = DR.e_prime(fb)
    assert e.min() >= 0.0 and e.max() <= 1.0 and DR.inside(fb)
    assert np.array_equal(DR.twin_source(128, 64, bits, 2).buf, fb.buf)      # not pulled in
    for kind in ('ramp', 'uniform', 'edges'):
        assert not DR.inside(synth_frames(kind, 2, 128, 64, bits, device='cpu', seed=13).to_numpy())
    rec = DoviRpu.hdr10_equivalent(bits)
    v, _ = DR.dovi_lms(fb.y[0], fb.u[0], fb.v[0], bits, rec)
    assert np.abs(v - e[0]).max() < 5e-7                      # float32 fields of the record
    got = DR.dovi_linear(fb.y[0], fb.u[0], fb.v[0], bits, rec)
    want = DR.hdr10_linear(fb.y[0], fb.u[0], fb.v[0], bits)
    assert np.abs(got - want).max() <= 2e-5 * want.max()
    for W, H in ((144, 64), (48, 32)):                        # the other test shapes
        assert DR.inside(DR.twin_source(W, H, bits))


@pytest.mark.parametrize('bits', [10, 12])
def test_luma_map_twins(bits):
    """Construction 2 (its own assertions run inside luma_map_pair), and the
    three records differ."""
    src, recs, mapped = DR.luma_map_pair(128, 64, bits)
    assert len({r.comp[0] for r in recs}) == 3
    for f in range(3):
        a = DR.dovi_linear(src.y[f], src.u[f], src.v[f], bits, recs[f])
        b = DR.dovi_linear(mapped.y[f], mapped.u[f], mapped.v[f], bits, DoviRpu.hdr10_equivalent(bits))
        assert np.abs(a - b).max() <= 1e-5 * b.max()
        c = DR.dovi_linear(src.y[f], src.u[f], src.v[f], bits, recs[(f + 1) % 3])
        assert np.abs(c - b).max() > 1e-2 * b.max()           # another frame's record is another picture


def test_mmr_affine_twins():
    """Construction 3: the folded record gives the same light where no clamp acts."""
    fb = DR.pull_in(DR.twin_source(128, 64, 10), (0.1, 0.9), 0.8)
    for luma_mmr in (True, False):       # every component an MMR; the shape the tile kernel takes
        mmr, folded = DR.mmr_affine_pair(10, luma_mmr=luma_mmr)
        assert DR.no_clamp_acts(fb, mmr) and DR.no_clamp_acts(fb, folded)
        assert all(k.method == (1,) and k.mmr_order == (1,) for k in mmr.comp[1:]) and folded.comp == (DoviCurve(),) * 3
        assert mmr.comp[0].method == ((1,) if luma_mmr else (0,))
        a = DR.dovi_linear(fb.y[0], fb.u[0], fb.v[0], 10, mmr)
        b = DR.dovi_linear(fb.y[0], fb.u[0], fb.v[0], 10, folded)
        assert np.abs(a - b).max() <= 2e-5 * b.max()
        assert np.abs(a - DR.hdr10_linear(fb.y[0], fb.u[0], fb.v[0], 10)).max() > 1e-2 * b.max()


@pytest.mark.parametrize('bits_in,bits_out,lut_n', [(10, 10, 65), (10, 8, 33), (12, 12, 65)])
@pytest.mark.parametrize('ipt', [False, True])
def test_tail_copy_equals_chain_lp(bits_in, bits_out, lut_n, ipt):
    """Construction 4: lp_tail from chain_lp's own stage 1 is chain_lp, sample
    for sample, on HDR10 content: the copy cannot drift."""
    fb = synth_frames('smooth', 1, 96, 64, bits_in, device='cpu', seed=13).to_numpy()
    want = toi.chain_lp(fb.y[0], fb.u[0], fb.v[0], bits_out, lut_n, ipt=ipt, bits_in=bits_in)
    got = DR.lp_tail(DR.hdr10_linear(fb.y[0], fb.u[0], fb.v[0], bits_in), bits_out, lut_n, ipt=ipt)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert np.array_equal(DR.upsample(np.asarray(fb.u[0], dtype=np.float64)), toi.upsample(fb.u[0].astype(np.float64)))


def test_restatement_of_the_twin_matches_the_oracle():
    """The whole restatement (model + tail) under the HDR10 twin against the C
    oracle, under the bounds test_independent_libplacebo_branch_matches_oracle sets."""
    W, H = 96, 64
    fb = DR.twin_source(W, H, 10, 1)
    p = oracle.default_params(tonemap=7, bits_in=10, bits_out=10, pipeline=2, lp_tone=0)
    got = oracle.process(p, hdr2sdr.generate_lattice(65), fb.buf, W, H).astype(np.int64)
    want = DR.restated(fb, DoviRpu.hdr10_equivalent(10), 10, 65, ipt=True)
    d = np.abs(got - want)
    assert d.max() <= 8 and (d > 0).mean() <= 1e-2


def test_realistic_record_is_what_it_says():
    for bits in (10, 12):
        r = DR.realistic_record(bits)
        assert r == DR.realistic_record(bits) and r != DR.realistic_record(bits, seed=8)       # seeded
        assert r.comp[0].num_pivots == 9 and r.comp[0].method == (0,) * 8
        assert all(k.method == (1,) and k.mmr_order == (3,) for k in r.comp[1:])
        x = np.linspace(0, 1, 4097)
        s = np.stack([x, np.full_like(x, 0.5), np.full_like(x, 0.5)], -1)[None]
        out = DR.reshape(s, r)[0]
        # (a three-point quadratic per eighth: loosest in the first, where x^1.15 bends most)
        assert np.abs(out[:, 0] - x ** 1.15).max() < 2e-3 and (np.diff(out[:, 0]) >= 0).all()
        assert np.abs(out[:, 1:] - 0.5).max() < 0.12          # chroma near the identity
