"""Lattices other than the bundled BT.2020 -> BT.709 gamut map, and what
they discriminate, for the LUT stage's tests (tests/test_lattices.py on the
CPU, tests/test_gpu_lattices.py on the GPU).  numpy only; every lattice is
seeded; all are float32 [n^3, 3] in .cube order (red fastest).

Why they exist.  The bundled lattice is smooth and nearly affine inside most
cells, with every node in [0, 1].  A kernel that picks a wrong tetrahedron
errs only to second order on it (swap_error: median 0.05 8-bit steps at 17^3),
and a kernel that clamps nodes where lut3d + swscale clamp the blend gives the
same result on it (clamp_order_error: 0).  So:

* bumpy(n, amp, seed): the bundled lattice plus uniform node noise in +-amp,
  clipped to [0, 1]: every cell discriminates between tetrahedra, and the
  steepest step between neighbouring nodes stays about the bundled one's (at
  amp 0.02: 0.42 against 0.44 at 17^3, 0.34 against 0.33 at 33^3);
* overshoot(n, gain): 0.5 + (bundled - 0.5) gain, not clipped: nodes outside
  [0, 1], as a creative or overshooting .cube has them;
* random_unit(n, seed): uniform in [0, 1] at n = 2 and 3, one or two cells per
  axis, so every coordinate sits in or on the last cell.

The float64 tetrahedral walk is tests/test_oracle_independent.py's
(tetrahedral, chain, chain_lp): stated once, there; the mutants below are that
walk with its arguments changed.
"""
import numpy as np

import hdr2sdr
from test_oracle_independent import tetrahedral

STEP8 = 255.0        # lattice values per 8-bit step


def bumpy(n, amp=0.02, seed=1):
    rng = np.random.default_rng([n, seed])
    base = hdr2sdr.generate_lattice(n).astype(np.float64)
    return np.clip(base + rng.uniform(-amp, amp, base.shape), 0.0, 1.0).astype(np.float32)


def overshoot(n, gain=1.15):
    return (0.5 + (hdr2sdr.generate_lattice(n).astype(np.float64) - 0.5) * gain).astype(np.float32)


def random_unit(n, seed=1):
    assert n in (2, 3), n
    return np.random.default_rng([n, seed]).uniform(0.0, 1.0, (n ** 3, 3)).astype(np.float32)


def cube(lat):
    """[n^3, 3] -> float64 [b][g][r][c], as the float64 walk indexes it."""
    n = round(lat.shape[0] ** (1 / 3))
    assert n ** 3 == lat.shape[0], lat.shape
    return np.asarray(lat, dtype=np.float64).reshape(n, n, n, 3)


def points(count=200_000, seed=5):
    """Seeded unit coordinates (count, 3), uniform in [0, 1)."""
    return np.random.default_rng(seed).uniform(0.0, 1.0, (count, 3))


def tetrahedral_swapped(lat, s):
    """The walk with the middle and the smallest fraction's axes exchanged:
    the neighbouring tetrahedron of the right cell (its affine interpolant at
    s), what a selection error at one comparison computes."""
    return tetrahedral(lat, s, walk=(0, 2, 1))


def tetrahedral_clamped_nodes(lat, s):
    """The walk on nodes clamped to [0, 1] first (what a pre-multiplied
    Y'CbCr lattice built from clamp01(node) computes)."""
    return tetrahedral(np.clip(lat, 0.0, 1.0), s)


def swap_error(lat, pts):
    """Per coordinate of pts (count, 3; unit coordinates), in 8-bit steps: the
    largest channel difference between the correct tetrahedron and the one
    with the mid / min axes exchanged."""
    a = cube(lat)
    s = pts * (a.shape[0] - 1)
    return np.abs(tetrahedral(a, s) - tetrahedral_swapped(a, s)).max(axis=-1) * STEP8


def clamp_order_error(lat, pts):
    """Per coordinate, in 8-bit steps: clip(blend(nodes)) (lut3d, then the
    swscale clip) against blend(clip(nodes))."""
    a = cube(lat)
    s = pts * (a.shape[0] - 1)
    return np.abs(np.clip(tetrahedral(a, s), 0.0, 1.0) - tetrahedral_clamped_nodes(a, s)).max(axis=-1) * STEP8
