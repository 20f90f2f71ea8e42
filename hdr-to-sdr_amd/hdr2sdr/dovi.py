"""Dolby Vision profile 5: a frame's RPU as the numbers libh2s applies.

A profile-5 stream has no HDR10-compatible base layer; its codes are IPT-PQ-c2
and mean something only after the frame's RPU has reshaped them.  The reference
sends such a source to libplacebo (src/ffmpeg_command.py:96-144).  The rawvideo
pipe drops the RPU, but it is a few hundred numbers per frame, which a caller
can obtain elsewhere (ffprobe frame side data, an RPU tool) and hand to the
context next to the frames: ``Tonemapper.set_dovi`` (``h2s_set_dovi``).  The
model is stated in include/h2s.h and DESIGN.md §4.12 ([EXT], parity unpinned).
Parsing the RPU bitstream is not part of this package.

``DoviCurve`` / ``DoviRpu`` mirror ``h2s_dovi_curve`` / ``h2s_dovi_rpu``;
``DoviRpu.from_fixed_point`` takes the integers as ffmpeg's ``AVDOVIMetadata``
carries them.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Any, Sequence

import numpy as np

MAX_PIVOTS = 9
MAX_PIECES = 8
METHOD_POLY, METHOD_MMR = 0, 1

# L, M, S -> linear BT.2020 R, G, B: the constant libplacebo multiplies in
# front of an RPU's rgb_to_lms matrix, as recalled from libplacebo's source
# ([EXT], unpinned: not compared against it; each row sums to 1 within 2e-4).
# An argument of from_fixed_point for that reason
LMS_TO_BT2020 = ((3.06441879, -2.16597676, 0.10155818),
                 (-0.65612108, 1.78554118, -0.12943749),
                 (0.01736321, -0.04725154, 1.03004253))


class H2SDoviCurve(ctypes.Structure):
    _fields_ = [
        ('num_pivots', ctypes.c_int32),
        ('pivots', ctypes.c_float * 9),
        ('method', ctypes.c_int32 * 8),
        ('poly', (ctypes.c_float * 3) * 8),
        ('mmr_order', ctypes.c_int32 * 8),
        ('mmr_const', ctypes.c_float * 8),
        ('mmr', ((ctypes.c_float * 7) * 3) * 8),
    ]


class H2SDoviRpu(ctypes.Structure):
    _fields_ = [
        ('nonlinear_offset', ctypes.c_float * 3),
        ('nonlinear', ctypes.c_float * 9),
        ('linear', ctypes.c_float * 9),
        ('comp', H2SDoviCurve * 3),
    ]


def _poly3(a: Any) -> 'tuple[float, float, float]':
    v = [float(x) for x in a] + [0.0, 0.0, 0.0]
    return (v[0], v[1], v[2])


_ZERO_MMR = ((0.0,) * 7,) * 3


@dataclass(frozen=True)
class DoviCurve:
    """A component's reshaping curve, ``h2s_dovi_curve`` field for field with
    the arrays as long as they are used: ascending ``pivots`` (2..9 values in
    [0, 1]; ``num_pivots`` is their count) and, per piece k < num_pivots - 1,
    ``method[k]`` (0 polynomial, 1 MMR), ``poly[k]`` (a0, a1, a2),
    ``mmr_order[k]`` (1..3), ``mmr_const[k]`` and ``mmr[k][order][7]``."""
    pivots: 'tuple[float, ...]' = (0.0, 1.0)
    method: 'tuple[int, ...]' = (METHOD_POLY,)
    poly: 'tuple[tuple[float, float, float], ...]' = ((0.0, 1.0, 0.0),)
    mmr_order: 'tuple[int, ...]' = (1,)
    mmr_const: 'tuple[float, ...]' = (0.0,)
    mmr: 'tuple[tuple[tuple[float, ...], ...], ...]' = (_ZERO_MMR,)

    def __post_init__(self) -> None:
        if not 2 <= len(self.pivots) <= MAX_PIVOTS:
            raise ValueError(f'a Dolby Vision curve has 2..{MAX_PIVOTS} pivots, got {len(self.pivots)}')
        n = len(self.pivots) - 1
        for name in ('method', 'poly', 'mmr_order', 'mmr_const', 'mmr'):
            if len(getattr(self, name)) != n:
                raise ValueError(f'{len(self.pivots)} pivots need {n} pieces, {name} has {len(getattr(self, name))}')

    @property
    def num_pivots(self) -> int:
        return len(self.pivots)

    @classmethod
    def identity(cls) -> 'DoviCurve':
        return cls()

    @classmethod
    def polynomial(cls, pivots: Any, coefs: Any) -> 'DoviCurve':
        """Polynomial pieces: ``coefs[k]`` = (a0, a1[, a2]) on [pivots[k], pivots[k + 1])."""
        n = len(pivots) - 1
        return cls(tuple(float(p) for p in pivots), (METHOD_POLY,) * n, tuple(_poly3(c) for c in coefs),
                   (1,) * n, (0.0,) * n, (_ZERO_MMR,) * n)

    @classmethod
    def mmr_single(cls, const: float, coef: Any, pivots: Any = (0.0, 1.0)) -> 'DoviCurve':
        """One MMR piece of order len(coef): ``coef[i][j]`` multiplies t_j^(i + 1)."""
        c = np.asarray(coef, dtype=np.float64).reshape(-1, 7)
        rows = tuple(tuple(float(v) for v in row) for row in c) + ((0.0,) * 7,) * (3 - c.shape[0])
        return cls(tuple(float(p) for p in pivots), (METHOD_MMR,), ((0.0, 1.0, 0.0),), (int(c.shape[0]),),
                   (float(const),), (rows,))

    def to_c(self) -> H2SDoviCurve:
        c = H2SDoviCurve()
        c.num_pivots = len(self.pivots)
        for i, p in enumerate(self.pivots):
            c.pivots[i] = p
        for k in range(MAX_PIECES):   # unused pieces: a valid identity
            c.mmr_order[k] = 1
            c.poly[k][1] = 1.0
        for k in range(len(self.pivots) - 1):
            c.method[k] = self.method[k]
            c.mmr_order[k] = self.mmr_order[k]
            c.mmr_const[k] = self.mmr_const[k]
            for j in range(3):
                c.poly[k][j] = self.poly[k][j]
            for i, row in enumerate(self.mmr[k]):
                for j, v in enumerate(row):
                    c.mmr[k][i][j] = v
        return c


_I3 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


@dataclass(frozen=True)
class DoviRpu:
    """One frame's record: ``nonlinear_offset`` (3), ``nonlinear`` (3 x 3, row
    major: reshaped signal - offset -> L'M'S'), ``linear`` (3 x 3: L, M, S ->
    linear BT.2020 R, G, B) and the three components' curves."""
    nonlinear_offset: 'tuple[float, ...]' = (0.0, 0.0, 0.0)
    nonlinear: 'tuple[float, ...]' = _I3
    linear: 'tuple[float, ...]' = _I3
    comp: 'tuple[DoviCurve, DoviCurve, DoviCurve]' = field(default_factory=lambda: (DoviCurve(),) * 3)

    def __post_init__(self) -> None:
        if len(self.nonlinear_offset) != 3 or len(self.nonlinear) != 9 or len(self.linear) != 9 or len(self.comp) != 3:
            raise ValueError('a Dolby Vision record has a 3-vector, two 3 x 3 matrices and three curves')

    def to_c(self) -> H2SDoviRpu:
        r = H2SDoviRpu()
        for i in range(3):
            r.nonlinear_offset[i] = self.nonlinear_offset[i]
            r.comp[i] = self.comp[i].to_c()
        for i in range(9):
            r.nonlinear[i] = self.nonlinear[i]
            r.linear[i] = self.linear[i]
        return r

    def with_(self, **kw: Any) -> 'DoviRpu':
        from dataclasses import replace
        return replace(self, **kw)

    @classmethod
    def identity(cls, bits: int = 10) -> 'DoviRpu':
        """Identity reshaping, no offset, both matrices the identity: the code
        fractions are read as PQ-coded linear BT.2020 R, G, B (``bits`` has no
        effect; it is here for symmetry with the other constructors).  As a
        timing input it is the floor of the front-end's cost, not a
        representative record: it has no luma pieces to select and no MMR."""
        if bits not in (10, 12):
            raise ValueError(f'bits must be 10 or 12, got {bits}')
        return cls()

    @classmethod
    def hdr10_equivalent(cls, bits: int = 10) -> 'DoviRpu':
        """The record under which a frame decodes as plain limited-range
        BT.2020-NCL PQ (HDR10): identity reshaping, the offset of the limited
        range's black and neutral codes, ``nonlinear`` the BT.2020-NCL matrix
        times the limited range's scales, ``linear`` the identity.  In real
        arithmetic stage 1 is then the HDR10 decode wherever E' lies in [0, 1]
        after upsampling."""
        if bits not in (10, 12):
            raise ValueError(f'bits must be 10 or 12, got {bits}')
        s, full = float(1 << (bits - 10)), float((1 << bits) - 1)
        off = (64.0 * s / full, 512.0 * s / full, 512.0 * s / full)
        kr, kb = 0.2627, 0.0593
        kg = 1.0 - kr - kb
        ncl = np.array([[1.0, 0.0, 2.0 * (1.0 - kr)],
                        [1.0, -2.0 * kb * (1.0 - kb) / kg, -2.0 * kr * (1.0 - kr) / kg],
                        [1.0, 2.0 * (1.0 - kb), 0.0]])
        d = np.diag([full / (876.0 * s), full / (896.0 * s), full / (896.0 * s)])
        return cls(nonlinear_offset=off, nonlinear=tuple(float(v) for v in (ncl @ d).reshape(-1)))

    @classmethod
    def from_fixed_point(cls, bits: int, pivots: 'Sequence[Sequence[int]]', methods: 'Sequence[Sequence[int]]',
                         poly_coef: 'Sequence[Sequence[Sequence[int]]]', mmr_order: 'Sequence[Sequence[int]]',
                         mmr_constant: 'Sequence[Sequence[int]]', mmr_coef: 'Sequence[Sequence[Any]]',
                         coef_log2_denom: int, ycc_to_rgb_matrix: 'Sequence[int]',
                         ycc_to_rgb_offset: 'Sequence[int]', rgb_to_lms_matrix: 'Sequence[int]',
                         lms_to_bt2020: Any = LMS_TO_BT2020) -> 'DoviRpu':
        """A record from an RPU's integers as ffmpeg's ``AVDOVIMetadata``
        carries them (AVDOVIDataMapping / AVDOVIColorMetadata):

        * ``pivots[c]``: component c's pivots in code units of the ``bits``-deep
          signal (-> / (2^bits - 1));
        * ``methods[c][k]`` 0 polynomial / 1 MMR; ``poly_coef[c][k]`` up to
          three integers, ``mmr_constant[c][k]``, ``mmr_coef[c][k][i][j]`` (i <
          ``mmr_order[c][k]``, j < 7): fixed point with ``coef_log2_denom``
          fractional bits;
        * ``ycc_to_rgb_matrix`` (9, scaled by 2^13), ``ycc_to_rgb_offset`` (3,
          scaled by 2^28): the non-linear matrix and its offset;
        * ``rgb_to_lms_matrix`` (9, scaled by 2^14); ``linear`` =
          ``lms_to_bt2020 @ rgb_to_lms_matrix`` ([EXT], unpinned: the mapping of
          an RPU's matrices onto libplacebo's decode is restated from memory)."""
        if bits not in (10, 12):
            raise ValueError(f'bits must be 10 or 12, got {bits}')
        full, den = float((1 << bits) - 1), float(1 << int(coef_log2_denom))
        curves = []
        for c in range(3):
            pv = tuple(float(p) / full for p in pivots[c])
            n = len(pv) - 1
            meth, poly, order, const, mmr = [], [], [], [], []
            for k in range(n):
                is_mmr = int(methods[c][k]) == METHOD_MMR
                meth.append(METHOD_MMR if is_mmr else METHOD_POLY)
                poly.append((0.0, 1.0, 0.0) if is_mmr else _poly3(float(v) / den for v in poly_coef[c][k]))
                o = int(mmr_order[c][k]) if is_mmr else 1
                order.append(o)
                const.append(float(mmr_constant[c][k]) / den if is_mmr else 0.0)
                rows = [[0.0] * 7 for _ in range(3)]
                if is_mmr:
                    coef = np.asarray(mmr_coef[c][k], dtype=np.float64)[:o, :7] / den
                    for i in range(o):
                        rows[i] = [float(v) for v in coef[i]]
                mmr.append(tuple(tuple(r) for r in rows))
            curves.append(DoviCurve(pv, tuple(meth), tuple(poly), tuple(order), tuple(const), tuple(mmr)))
        nl = np.asarray(ycc_to_rgb_matrix, dtype=np.float64).reshape(3, 3) / float(1 << 13)
        off = np.asarray(ycc_to_rgb_offset, dtype=np.float64).reshape(3) / float(1 << 28)
        r2l = np.asarray(rgb_to_lms_matrix, dtype=np.float64).reshape(3, 3) / float(1 << 14)
        lin = np.asarray(lms_to_bt2020, dtype=np.float64).reshape(3, 3) @ r2l
        return cls(tuple(float(v) for v in off), tuple(float(v) for v in nl.reshape(-1)),
                   tuple(float(v) for v in lin.reshape(-1)), tuple(curves))


def records_to_c(rpus: 'DoviRpu | Sequence[DoviRpu]') -> Any:
    """A ctypes array of ``h2s_dovi_rpu`` from one record or a sequence."""
    if isinstance(rpus, DoviRpu):
        rpus = [rpus]
    rpus = list(rpus)
    for r in rpus:
        if not isinstance(r, DoviRpu):
            raise ValueError(f'expected DoviRpu records, got {type(r).__name__}')
    arr = (H2SDoviRpu * len(rpus))()
    for i, r in enumerate(rpus):
        arr[i] = r.to_c()
    return arr


def resolve_records(dovi: Any, first_frame: int, count: int) -> 'list[DoviRpu]':
    """What ``dovi=`` (a single ``DoviRpu`` or a callable ``dovi(first_frame,
    count) -> list[DoviRpu]``) gives for frames [first_frame, first_frame +
    count) of a stream."""
    if isinstance(dovi, DoviRpu):
        return [dovi]
    recs = list(dovi(first_frame, count))
    if len(recs) not in (1, count):
        raise ValueError(f'dovi({first_frame}, {count}) returned {len(recs)} records (expected 1 or {count})')
    return recs
