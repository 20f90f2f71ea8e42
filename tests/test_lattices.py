"""CPU: the LUT stage on lattices other than the bundled gamut map
(tests/lattices_ref.py), before the GPU suite relies on them
(tests/test_gpu_lattices.py).

* The C oracle against the float64 restatement (tests/test_oracle_independent.py
  chain / chain_lp, handed the lattice) on the rough, the overshooting and the
  tiny lattices: whole frames through both pipelines under that module's own
  bounds, and the stage-4 plane against the float64 walk of the oracle's own
  stage-3 plane within float32 rounding.
* The fixtures discriminate: a wrong tetrahedron on the bumpy lattices and
  node clamping on the overshooting one move a stated share of 200 000 seeded
  coordinates by more than one 8-bit step.
* The integer gate (test_gpu_parity.assert_close_int) rejects exactly those two
  errors when they are put through the whole chain, and accepts the
  restatement without them.
* An overshooting .cube survives the parser unclamped.
"""
import functools

import numpy as np
import pytest

import hdr2sdr
import lattices_ref as LR
import oracle
from float_gate import lattice_max_step
from hdr2sdr.synth import synth_frames
from test_gpu_parity import assert_close_int
from test_oracle_independent import TM, chain, chain_lp, tetrahedral

W, H = 96, 64
LATTICES = {
    'bumpy17': lambda: LR.bumpy(17),
    'overshoot17': lambda: LR.overshoot(17, 1.15),
    'random2': lambda: LR.random_unit(2),
    'random3': lambda: LR.random_unit(3),
}


@functools.lru_cache(maxsize=None)
def lat_of(name):
    a = LATTICES[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frame(kind, seed):
    return synth_frames(kind, 1, W, H, 10, device='cpu', seed=seed).to_numpy()


# ---- 1. the oracle against the float64 restatement --------------------------
@pytest.mark.parametrize('kind', ['smooth', 'ramp', 'uniform'])
@pytest.mark.parametrize('case', [('hable', 2.2, False), ('mobius', 1.0, True)], ids=['hable-g2.2', 'mobius-native'])
@pytest.mark.parametrize('name', sorted(LATTICES))
def test_oracle_cpu_chain_matches_restatement(name, case, kind):
    """tests/test_oracle_independent.py's CPU-chain check and bounds, on these lattices."""
    tm, gamma, native = case
    lat = lat_of(name)
    n = round(lat.shape[0] ** (1 / 3))
    fb = frame(kind, 11)
    p = oracle.default_params(tonemap=TM[tm], gamma=gamma, mode=1 if native else 0)
    got = hdr2sdr.FrameBatch(oracle.process(p, lat, fb.buf, W, H), W, H, 10)
    want = chain(fb.y[0], fb.u[0], fb.v[0], 10, 10, False, tm, gamma, n, native=native, lat=LR.cube(lat))
    step = 1 if native else 4
    for plane, a, b in zip('YUV', (got.y[0], got.u[0], got.v[0]), want):
        d = np.abs(a.astype(np.int64) - b)
        bound = step * (1 if plane != 'Y' or gamma == 1.0 else 3)
        assert d.max() <= bound, (plane, int(d.max()))
        assert (d > 0).mean() <= 5e-3, (plane, float((d > 0).mean()))


@pytest.mark.parametrize('kind', ['smooth', 'ramp', 'uniform'])
@pytest.mark.parametrize('form', ['max-rgb', 'ipt'])
@pytest.mark.parametrize('name', sorted(LATTICES))
def test_oracle_libplacebo_branch_matches_restatement(name, form, kind):
    """The libplacebo branch (rgba8 download, lut3d's truncating 8-bit path)
    under tests/test_oracle_independent.py's bounds, on these lattices."""
    lat = lat_of(name)
    n = round(lat.shape[0] ** (1 / 3))
    fb = frame(kind, 13)
    p = oracle.default_params(tonemap=7, pipeline=2, lp_tone=1 if form == 'max-rgb' else 0)
    got = hdr2sdr.FrameBatch(oracle.process(p, lat, fb.buf, W, H), W, H, 10)
    want = chain_lp(fb.y[0], fb.u[0], fb.v[0], 10, n, ipt=form == 'ipt', lat=LR.cube(lat))
    k8 = 4
    for plane, a, b in zip('YUV', (got.y[0], got.u[0], got.v[0]), want):
        d = np.abs(a.astype(np.int64) - b)
        assert d.max() <= 8 * k8, (plane, int(d.max()))
        assert (d > 0).mean() <= 1e-2, (plane, float((d > 0).mean()))


@pytest.mark.parametrize('kind', ['smooth', 'uniform'])
@pytest.mark.parametrize('name', sorted(LATTICES))
def test_oracle_stage4_is_the_float64_walk_of_its_stage3(name, kind):
    """oracle.debug_float stage 4 (lut3d's raw blend, not clipped) against the
    float64 walk at the oracle's own stage-3 values.  Bound, from float32
    alone: the coordinate s3 (N-1) rounds by 2^-24 (N-1) per axis and moves the
    blend by at most the lattice's steepest step per unit; the three weight
    differences, four products and three sums each round by 2^-24 of values
    <= max |node|: 2^-24 (3 (N-1) max_step + 10 max|node|), doubled."""
    lat = lat_of(name)
    n = round(lat.shape[0] ** (1 / 3))
    fb = frame(kind, 11)
    p = oracle.default_params(tonemap=TM['hable'], gamma=2.2)
    s3 = oracle.debug_float(p, lat, fb.buf, W, H, 3).astype(np.float64)
    s4 = oracle.debug_float(p, lat, fb.buf, W, H, 4).astype(np.float64)
    assert np.isfinite(s3).all()
    want = tetrahedral(LR.cube(lat), np.clip(np.moveaxis(s3, 0, -1) * (n - 1), 0, n - 1))
    tol = 2.0 ** -23 * (3 * (n - 1) * lattice_max_step(n, lat) + 10 * float(np.abs(lat).max()))
    err = np.abs(np.moveaxis(s4, 0, -1) - want)
    assert err.max() <= tol, (float(err.max()), tol)
    if name == 'overshoot17':      # the plane is the raw blend: the clip comes after it
        assert want.min() < 0.0 or want.max() > 1.0


@pytest.mark.parametrize('kind', ['smooth', 'uniform'])
@pytest.mark.parametrize('name', sorted(LATTICES))
def test_oracle_libplacebo_stage4_is_the_float64_8bit_path(name, kind):
    """The branch's stage 4 (lut3d's 8-bit output / 255) against the float64
    walk at the oracle's own download codes (oracle.lp_download), truncated
    and clipped as lut3d's 8-bit path does.  Equal codes in, so the outputs
    differ only where the float32 and float64 blends straddle an integer: by
    one 8-bit step, on at most the restatement tests' 1 % of values."""
    lat = lat_of(name)
    n = round(lat.shape[0] ** (1 / 3))
    fb = frame(kind, 13)
    p = oracle.default_params(tonemap=7, pipeline=2)
    q = np.floor(oracle.lp_download(p, lat, fb.buf, W, H))
    s4 = np.rint(oracle.debug_float(p, lat, fb.buf, W, H, 4).astype(np.float64) * 255.0)
    o = tetrahedral(LR.cube(lat), np.moveaxis(q, 0, -1) / 255.0 * (n - 1))
    want = np.clip(np.trunc(o * 255.0), 0, 255)
    d = np.abs(np.moveaxis(s4, 0, -1) - want)
    assert d.max() <= 1, float(d.max())
    assert (d > 0).mean() <= 1e-2, float((d > 0).mean())


# ---- 2. the fixtures discriminate -------------------------------------------
@pytest.mark.parametrize('n,amp', [(17, 0.02), (33, 0.02), (17, 0.01), (33, 0.01)])
def test_bumpy_lattice_discriminates_between_tetrahedra(n, amp):
    """Measured: 0.595 / 0.575 at amp 0.02 and 0.389 / 0.347 at amp 0.01 for
    N = 17 / 33 (the bundled lattices: 0.14 / 0.06)."""
    share = float((LR.swap_error(LR.bumpy(n, amp), LR.points()) > 1.0).mean())
    print(f'LATTICE swap_error bumpy({n}, {amp}): {share:.3f} of coordinates beyond one 8-bit step')
    assert share >= 0.30, share


def test_overshoot_lattice_discriminates_the_clamp_order():
    """Measured: 0.254 of the coordinates, up to 15.6 steps."""
    lat = LR.overshoot(17, 1.15)
    assert lat.min() < 0.0 and lat.max() > 1.0
    e = LR.clamp_order_error(lat, LR.points())
    print(f'LATTICE clamp_order_error overshoot(17, 1.15): {float((e > 1.0).mean()):.3f} beyond one step, '
          f'max {float(e.max()):.1f}')
    assert (e > 1.0).mean() >= 0.10, float((e > 1.0).mean())
    # and nothing on a lattice inside [0, 1]
    assert LR.clamp_order_error(LR.bumpy(17), LR.points(20_000)).max() == 0.0


def test_fixtures_are_seeded_and_shaped():
    for n in (17, 33):
        a, b = LR.bumpy(n), LR.bumpy(n)
        assert a.dtype == np.float32 and a.shape == (n ** 3, 3) and np.array_equal(a, b)
        assert a.min() >= 0.0 and a.max() <= 1.0
        assert not np.array_equal(a, LR.bumpy(n, seed=2))
        # the noise does not steepen the lattice's steepest step by more than itself
        assert lattice_max_step(n, a) <= lattice_max_step(n) + 2 * 0.02
    for n in (2, 3):
        a = LR.random_unit(n)
        assert a.dtype == np.float32 and a.shape == (n ** 3, 3) and np.array_equal(a, LR.random_unit(n))
        assert a.min() >= 0.0 and a.max() <= 1.0
    o = LR.overshoot(17, 1.15)
    assert o.dtype == np.float32 and o.shape == (17 ** 3, 3)
    assert abs(float(o.min()) + 0.075) < 1e-6 and abs(float(o.max()) - 1.075) < 1e-6


# ---- 3. the integer gate rejects both errors ---------------------------------
GATE = hdr2sdr.TonemapParams(tonemapper='hable', gamma=2.2, bits_out=10)


def _through_chain(lat, kind, **kw):
    """(oracle output, the float64 restatement's output with kw, source): [1, W H 3/2] int64."""
    n = round(lat.shape[0] ** (1 / 3))
    fb = frame(kind, 11)
    want = oracle.process(oracle.params_from(GATE.to_c()), lat, fb.buf, W, H).astype(np.int64)
    y, u, v = chain(fb.y[0], fb.u[0], fb.v[0], 10, 10, False, 'hable', 2.2, n, lat=LR.cube(lat), **kw)
    got = np.concatenate([y.ravel(), u.ravel(), v.ravel()])[None].astype(np.int64)
    return want, got, fb.buf


@pytest.mark.parametrize('kind', ['uniform', 'smooth'])
@pytest.mark.parametrize('name', ['bumpy17', 'bumpy33'])
def test_gate_rejects_a_wrong_tetrahedron_on_bumpy_lattices(name, kind):
    lat = LR.bumpy(int(name[5:]))
    want, good, src = _through_chain(lat, kind)
    assert_close_int(GATE, good, want, W, H, src, lat=lat)
    want, bad, src = _through_chain(lat, kind, tetra=LR.tetrahedral_swapped)
    with pytest.raises(AssertionError, match='beyond|max diff'):
        assert_close_int(GATE, bad, want, W, H, src, lat=lat)


@pytest.mark.parametrize('kind', ['uniform', 'smooth'])
def test_gate_rejects_node_clamping_on_the_overshoot_lattice(kind):
    lat = LR.overshoot(17, 1.15)
    want, good, src = _through_chain(lat, kind)
    assert_close_int(GATE, good, want, W, H, src, lat=lat)
    want, bad, src = _through_chain(lat, kind, tetra=LR.tetrahedral_clamped_nodes)
    with pytest.raises(AssertionError, match='beyond|max diff'):
        assert_close_int(GATE, bad, want, W, H, src, lat=lat)


@pytest.mark.parametrize('name', ['bumpy17', 'overshoot17', 'random3'])
def test_libplacebo_gate_with_the_lattice_handed_through(name):
    """tests/lp_gate.py on another lattice (tests/test_lp_gate.py's checks):
    k8 is that lattice's; the oracle's float32 form of the branch is accepted
    (every flip attributed to a download tie), a one-code bias is rejected."""
    import math
    import lp_gate
    lat = lat_of(name)
    n = round(lat.shape[0] ** (1 / 3))
    p = hdr2sdr.TonemapParams(tonemapper='bt.2390', bits_out=10)
    op = oracle.params_from(p.to_c())
    src = synth_frames('smooth', 2, 128, 64, 10, device='cpu', seed=5).to_numpy().buf
    want = oracle.process(op, lat, src, 128, 64).astype(np.int64)
    with oracle.lp_form(f32=True):
        f32 = oracle.process(op, lat, src, 128, 64).astype(np.int64)
    rep, fails = lp_gate.check(p, 'generic', f32, want, src, 128, 64, lattice=lat)
    assert not fails, (rep, fails)
    assert rep['k8_steps'] == math.ceil(lattice_max_step(n, lat) * (n - 1)) + 1
    assert_close_int(p, f32, want, 128, 64, src, kernel='generic', lat=lat)
    with oracle.lp_form(bias=1):
        biased = oracle.process(op, lat, src, 128, 64).astype(np.int64)
    rep, fails = lp_gate.check(p, 'k_tile', biased, want, src, 128, 64, lattice=lat)
    assert rep['unattributed'] > 0 and fails, rep


def test_float_gate_reads_the_lattice_from_the_planes():
    """Planes(lat=) carries the lattice: the planes, the slope term and the
    k8 bound are that lattice's, and the defaults stay the bundled one's."""
    from float_gate import FLOAT_CFGS, Planes, float_tolerance, judge_float, lattice_slope
    lat = lat_of('bumpy17')
    src = synth_frames('uniform', 1, 128, 64, 10, device='cpu', seed=3).to_numpy().buf
    params = hdr2sdr.TonemapParams(**FLOAT_CFGS['C2_hable_pq10'])
    P = Planes(params, src, 128, 64, lat=lat)
    assert P.lut_n == 17 and P.lat_given and not Planes(params, src, 128, 64).lat_given
    assert np.array_equal(P[4], oracle.debug_float(P.op, lat, src, 128, 64, 4).astype(np.float64))
    T = float_tolerance(params, 'k_tile', 4, 'uniform', P)
    _, fails = judge_float(params, 'k_tile', 'uniform', 4, T.want.copy(), T)
    assert not fails, fails
    rough, smooth = lattice_slope(17, P[3], lat), lattice_slope(17, P[3])
    assert rough.shape == smooth.shape and rough.mean() > 1.2 * smooth.mean()
    lp = hdr2sdr.TonemapParams(**FLOAT_CFGS['C3_bt2390_libplacebo'])
    tiny = lat_of('random2')
    Tl = float_tolerance(lp, 'k_tile', 4, 'uniform', Planes(lp, src, 128, 64, lat=tiny))
    assert Tl.flip_lim == (int(np.ceil(lattice_max_step(2, tiny))) + 1) / 255.0


# ---- 4. an overshooting .cube through the parser ------------------------------
def test_parse_cube_keeps_overshoot_values(tmp_path):
    lat = LR.overshoot(5, 1.15)
    text = 'LUT_3D_SIZE 5\n' + ''.join('%.6f %.6f %.6f\n' % tuple(float(c) for c in row) for row in lat)
    want = np.array([[float('%.6f' % float(c)) for c in row] for row in lat], dtype=np.float64).astype(np.float32)
    assert want.min() < 0.0 and want.max() > 1.0
    got = hdr2sdr.parse_cube(text)
    assert got.dtype == np.float32 and got.shape == (125, 3)
    assert np.array_equal(got, want)
    assert np.array_equal(oracle.parse_cube(text), want)
    # Tonemapper.load_cube's parser path (hdr2sdr.lut.load_cube: the file, read as bytes)
    path = tmp_path / 'overshoot5.cube'
    path.write_text(text, newline='\n')
    assert np.array_equal(hdr2sdr.load_cube(str(path)), want)
