"""GPU: the LUT stage on lattices other than the bundled gamut map
(tests/lattices_ref.py), through the suite's existing gates handed the
lattice in force (assert_close_int / check_float_stage with lat=).

Every other LUT test runs generate_lattice(n): smooth, nearly affine inside
most cells, every node in [0, 1].  Here:

* bumpy(n, AMP): the bundled lattice plus seeded node noise.  A wrong
  tetrahedron moves more than half of all coordinates by more than one 8-bit
  step on it (tests/test_lattices.py), so k_tile's selection (axis tags, max3 /
  min3 / med3, the LDS offset table, the scalar-gather key) is judged in every
  cell, on the tile kernel, the generic kernel, the tile + tail seam and the
  stage-4 float plane;
* overshoot(17, 1.15): nodes in [-0.075, 1.075].  lut3d blends the raw nodes
  and swscale clips the blend; k_tile's pre-multiplied lattice is built from
  clamped nodes, which differs by up to 15.6 steps, so h2s_set_lut routes such a
  lattice's CPU chain to the generic kernel (H2S_PATH_GENERIC), while the
  libplacebo branch (8-bit table, generic arithmetic) stays on the tile path;
* random_unit(2), random_unit(3): one or two cells per axis, every over-range
  code on the last cell's far face (the padded records, weight 0);
* a same-size replacement and a shrink on one context (the derived lattices'
  rebuild paths), bit for bit back to the first output.

Frames are 128x64x2 (two tile columns, two tile rows) or 80x34x2 (one tile
column plus a 16-column tail, a ragged bottom tile row).

Amplitude and differ-shares.  AMP = 0.02 (the issue's first choice; 0.01 was
not needed).  The share of samples that differ from the oracle at all (budget
0.5 %, assert_close_int's max_frac), from this module's LATTICE lines on an
MI355X, none beyond one step:

  bumpy, CPU chain, 128x64x2      k_tile                      generic
    N = 17  uniform/smooth/edges  0.012 / 0.008 / 0.008 %     0 / 0 / 0
    N = 33  uniform/smooth/edges  0.012 / 0.008 / 0.016 %     0.004 % / 0 / 0
    N = 17  native, uniform       0.045 %                     0
  tile + tail, 80x34x2            N = 17: 0.012 % (uniform), 0 (edges); N = 33: 0 / 0
  tiny, CPU chain                 k_tile <= 0.016 %, generic 0
  libplacebo branch (k_tile)      <= 0.049 % differ, every sample beyond one
                                  step attributed to a download tie, max 8 steps

The bundled 17^3 and 33^3 lattices give 0.008 % on the same 'edges' frame (the
'replace' lines): the rough lattice's rounding flips stay a factor of 10 under
the budget.

Stage-4 float plane on bumpy(17) (share of values that pass the 1e-3 gate only
through the lattice-slope conditioning term; caps 3 % uniform, 2 % smooth):
k_tile C2 0.22 % (uniform), 0.14 % (smooth); generic 0; the libplacebo branch
0, with 0.02 % of pixels flipped at the download.  A survey outside the suite
on BT.2390 over the CPU pipeline, whose frames put 42-56 % of their stage-4
values below 0.02, gave k_tile 2.5 % / 3.3 % (uniform / smooth) at N = 17 and
4.9 % / 7.2 % at N = 33, the same at amp 0.01 and 0.02, every value inside its
tolerance, against 0.2 % / 0.1 % on the bundled lattices: next to black the
clipped noise is the node value, so the interpolant's relative slope is of
order N - 1 per unit whatever the amplitude, and k_tile's stage-3 floor (1e-5
absolute) reaches 1e-3 relative there.  That is the rough lattice's own
conditioning, stated here and not gated: section 2 uses section 1's
configuration, whose frames are not dominated by near-black values.

The overshoot case against the library as it was before h2s_set_lut recorded
the lattice's range (k_tile, clamped nodes; path TILE / TILE_TAIL): 128x64
uniform 7.43 % of samples differ, 1.50 % of pixels and chroma pairs beyond one
step, max 8 steps ('chroma max diff 2 quantiser steps'); edges 3.02 % / 0.48 %
/ 8; 80x34 uniform 6.62 % / 1.18 % / 7; edges 2.50 % / 0.37 % / 6.  On the
generic kernel: 0 samples differ in all four.
"""
import numpy as np
import pytest

import hdr2sdr
import lattices_ref as LR
import lp_gate
import oracle
from hdr2sdr import _abi
from hdr2sdr.synth import synth_frames
from float_gate import lattice
from test_gpu_parity import assert_close_int, check_float_stage, run_both

pytestmark = pytest.mark.gpu

AMP = 0.02
NF = 2
CPU = dict(tonemapper='hable', gamma=2.2, bits_out=10)          # the CPU chain, 10-bit compat8
LP = dict(tonemapper='bt.2390', gamma=1.0, bits_out=10)         # the libplacebo branch (C3)

LATTICES = {
    'bumpy17': lambda: LR.bumpy(17, AMP),
    'bumpy33': lambda: LR.bumpy(33, AMP),
    'overshoot17': lambda: LR.overshoot(17, 1.15),
    'random2': lambda: LR.random_unit(2),
    'random3': lambda: LR.random_unit(3),
    'bundled17': lambda: lattice(17),
    'bundled33': lambda: lattice(33),
}
_lat, _src, _want = {}, {}, {}


def lat_of(name):
    if name not in _lat:
        _lat[name] = LATTICES[name]()
        _lat[name].setflags(write=False)
    return _lat[name]


def source(kind, W, H, bits=10):
    key = (kind, W, H, bits)
    if key not in _src:
        _src[key] = synth_frames(kind, NF, W, H, bits, device='cpu', seed=11)
    return _src[key]


def reference(kw, name, kind, W, H):
    """The oracle's output of a case, computed once and shared by the kernels."""
    key = (tuple(sorted(kw.items())), name, kind, W, H)
    if key not in _want:
        params = hdr2sdr.TonemapParams(**kw)
        _want[key] = oracle.process(oracle.params_from(params.to_c()), lat_of(name),
                                    source(kind, W, H, params.bits_in).to_numpy().buf, W, H).astype(np.int64)
        _want[key].setflags(write=False)
    return _want[key]


@pytest.fixture(scope='module')
def tm():
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.close()


def convert(tm, kw, name, kind, W, H, kernel):
    """One launch on `kernel` ('k_tile': the route's own choice; 'generic':
    H2S_OPT_FAST_PATH 0).  Returns (params, got, want, src, path)."""
    import torch
    params = hdr2sdr.TonemapParams(**kw)
    cpu = source(kind, W, H, params.bits_in)
    tm.set_params(params)
    tm.set_lut(lat_of(name))
    tm.set_option(_abi.OPT_FAST_PATH, 1 if kernel == 'k_tile' else 0)
    try:
        src = cpu.to_torch('cuda')
        dst = hdr2sdr.FrameBatch.empty_torch(NF, W, H, params.bits_out, 'cuda')
        path = tm.query_path(src, dst)
        tm.process(src, dst)
        torch.cuda.synchronize()
    finally:
        tm.set_option(_abi.OPT_FAST_PATH, 1)
    return params, dst.to_numpy().buf.astype(np.int64), reference(kw, name, kind, W, H), cpu.to_numpy().buf, path


def report(label, params, got, want, W, H):
    """The LATTICE line: the share of samples that differ at all, the share
    beyond one quantiser step (luma before eq) and the largest difference."""
    by, bc, step = lp_gate.beyond_samples(params, got, want, W, H)
    d = np.abs(got - want)
    print(f'LATTICE {label}: differ {float((d > 0).mean()):.4%}, beyond one step '
          f'{float((by.sum() + bc.sum()) / (by.size + bc.size)):.4%} of pixels and chroma pairs, '
          f'max {int(-(-int(d.max()) // step))} steps')


def tile_path(W):
    return _abi.PATH_TILE if W % 64 == 0 else _abi.PATH_TILE_TAIL


# ---- 1. bumpy lattices, the CPU chain ----------------------------------------
@pytest.mark.parametrize('kind', ['uniform', 'smooth', 'edges'])
@pytest.mark.parametrize('kernel', ['k_tile', 'generic'])
@pytest.mark.parametrize('name', ['bumpy17', 'bumpy33'])
def test_bumpy_cpu_chain(tm, name, kernel, kind):
    params, got, want, src, path = convert(tm, CPU, name, kind, 128, 64, kernel)
    report(f'bumpy-cpu {name} {kernel} {kind} 128x64', params, got, want, 128, 64)
    assert path == (_abi.PATH_TILE if kernel == 'k_tile' else _abi.PATH_GENERIC)
    assert_close_int(params, got, want, 128, 64, src, lat=lat_of(name))


@pytest.mark.parametrize('kernel', ['k_tile', 'generic'])
def test_bumpy_cpu_chain_native(tm, kernel):
    """mode='native': the quantiser step is 4x finer than compat8's."""
    kw = dict(CPU, mode='native')
    params, got, want, src, path = convert(tm, kw, 'bumpy17', 'uniform', 128, 64, kernel)
    report(f'bumpy-cpu-native bumpy17 {kernel} uniform 128x64', params, got, want, 128, 64)
    assert path == (_abi.PATH_TILE if kernel == 'k_tile' else _abi.PATH_GENERIC)
    assert_close_int(params, got, want, 128, 64, src, lat=lat_of('bumpy17'))


@pytest.mark.parametrize('kind', ['uniform', 'edges'])
@pytest.mark.parametrize('name', ['bumpy17', 'bumpy33'])
def test_bumpy_tile_plus_tail_seam(tm, name, kind):
    """80x34: k_tile on the first 64 columns, k_process on the other 16 (and a
    bottom tile row of 2 rows): both sides of the seam on a rough lattice."""
    params, got, want, src, path = convert(tm, CPU, name, kind, 80, 34, 'k_tile')
    report(f'bumpy-cpu {name} tile+tail {kind} 80x34', params, got, want, 80, 34)
    assert path == _abi.PATH_TILE_TAIL
    assert_close_int(params, got, want, 80, 34, src, lat=lat_of(name))


# ---- 2. bumpy lattice, the stage-4 float plane --------------------------------
# The CPU-chain configuration is the one of section 1 (C2: Hable, gamma 2.2,
# 10-bit compat8).  Its 'smooth' frame is 128x128: the float gate refuses to
# judge a frame of which 1 % or more lies at vf_tonemap's desaturation kink
# (whatever the kernel or lattice: the share is the oracle's), and the smooth
# gradient's kink band covers 1.01 % of 128x64 pixels, 0.64 % of 128x128.
FLOAT_CASES = [('C2_hable_pq10', 'uniform', 128, 64), ('C2_hable_pq10', 'smooth', 128, 128),
               ('C3_bt2390_libplacebo', 'uniform', 128, 64), ('C3_bt2390_libplacebo', 'smooth', 128, 64)]


@pytest.mark.parametrize('cfg,kind,W,H', FLOAT_CASES)
@pytest.mark.parametrize('kernel', ['k_tile', 'k_debug'])
def test_bumpy_float_stage4(tm, kernel, cfg, kind, W, H):
    rep = check_float_stage(tm, kernel, cfg, kind, 4, W=W, H=H, lat=lat_of('bumpy17'))
    print(f'LATTICE float-stage4 bumpy17 {kernel} {cfg} {kind} {W}x{H}: floor_only {rep["floor_only_frac"]:.4f}, '
          f'max rel err {rep["max_rel_err_rest"]:.2e}, flips {rep.get("flip_frac", 0.0):.4%}')


# ---- 3. overshoot, the CPU chain: the generic kernel --------------------------
@pytest.mark.parametrize('kind', ['uniform', 'edges'])
@pytest.mark.parametrize('W,H', [(128, 64), (80, 34)])
def test_overshoot_cpu_chain_runs_on_the_generic_kernel(tm, W, H, kind):
    """Nodes outside [0, 1]: clip(blend(nodes)), as the oracle.  Against the
    library before h2s_set_lut recorded the lattice's range this case ran on
    k_tile (clamped nodes) and failed the hard bound; DESIGN.md 4.3."""
    params, got, want, src, path = convert(tm, CPU, 'overshoot17', kind, W, H, 'k_tile')
    report(f'overshoot-cpu overshoot17 {kind} {W}x{H} path {path}', params, got, want, W, H)
    assert_close_int(params, got, want, W, H, src, lat=lat_of('overshoot17'))
    assert path == _abi.PATH_GENERIC


# ---- 4. overshoot and bumpy, the libplacebo branch ----------------------------
@pytest.mark.parametrize('kind', ['uniform', 'smooth'])
@pytest.mark.parametrize('name', ['overshoot17', 'bumpy17', 'bumpy33'])
def test_libplacebo_branch_stays_on_the_tile_path(tm, name, kind):
    params, got, want, src, path = convert(tm, LP, name, kind, 128, 64, 'k_tile')
    report(f'libplacebo {name} {kind} 128x64', params, got, want, 128, 64)
    assert path == _abi.PATH_TILE
    assert_close_int(params, got, want, 128, 64, src, lat=lat_of(name))


# ---- 6. tiny lattices through the whole chain ----------------------------------
@pytest.mark.parametrize('kind', ['uniform', 'edges'])
@pytest.mark.parametrize('kernel', ['k_tile', 'generic'])
@pytest.mark.parametrize('pipe', ['cpu', 'libplacebo'])
@pytest.mark.parametrize('name', ['random2', 'random3'])
def test_tiny_lattices(tm, name, pipe, kernel, kind):
    """N = 2 and 3: every coordinate in or on the last cell; an over-range
    code ('edges') clamps to s = N - 1, where k_tile reads the zero records
    behind the lattice with weight 0."""
    kw = CPU if pipe == 'cpu' else LP
    params, got, want, src, path = convert(tm, kw, name, kind, 128, 64, kernel)
    report(f'tiny {name} {pipe} {kernel} {kind} 128x64', params, got, want, 128, 64)
    assert path == (_abi.PATH_TILE if kernel == 'k_tile' else _abi.PATH_GENERIC)
    assert_close_int(params, got, want, 128, 64, src, lat=lat_of(name))


# ---- 7. replacing the lattice on one context ------------------------------------
@pytest.mark.parametrize('pipe', ['cpu', 'libplacebo'])
def test_same_size_replacement_and_shrink_on_one_context(pipe):
    """bundled 33 -> bumpy 33 (same size: the derived lattice is rebuilt in
    place) -> bumpy 17 (the shrink: the 17^3 lattice's zero pad lies where 33^3
    data was) -> bundled 17 -> bundled 33 again, 'edges' content (over-range
    codes read the pad) after each h2s_set_lut; each output within the gate of
    the oracle with the lattice in force, the last equal to the first."""
    params = hdr2sdr.TonemapParams(**(CPU if pipe == 'cpu' else LP))
    t = hdr2sdr.Tonemapper(0)
    try:
        outs = []
        for name in ('bundled33', 'bumpy33', 'bumpy17', 'bundled17', 'bundled33'):
            got, want, (W, H, src) = run_both(t, params, 'edges', 128, 64, lat=lat_of(name))
            report(f'replace {pipe} -> {name}', params, got, want, W, H)
            assert_close_int(params, got, want, W, H, src, lat=lat_of(name))
            outs.append(got)
        assert np.array_equal(outs[-1], outs[0])
        assert not np.array_equal(outs[1], outs[0]) and not np.array_equal(outs[2], outs[1])
    finally:
        t.close()
