"""The tile kernel's instance sets in user-level coordinates: which frame
forms, chains, transfers, operators and desaturation settings have a k_tile
instance of their own, stated here from the library's interface (not read
from csrc/h2s_tile_sets.h, which this checks), with the sources that give some
sets an exact twin.  Used by tests/test_gpu_tile_sets.py and by
scripts/format_checksums.py --tile-sets.

A row is (set, transfer, operator, desat): one k_tile instance.  Every launch
is 192 x 96 (3 x 3 tiles: the centre one on tile_load's interior addressing,
the others on the border forms), 2 frames, 10 bits in and out, a 17^3 LUT.
"""
import dataclasses

import numpy as np

import dovi_ref as DR
import hdr2sdr
import subsampling_ref as SR
from hdr2sdr.synth import synth_frames

W, H, NF, BITS, LUT_N, SEED = 192, 96, 2, 10, 17, 11


@dataclasses.dataclass(frozen=True)
class Set:
    name: str            # the translation unit's, csrc/h2s_<name>.hip
    chain: str           # 'cpu' | 'lp' (the libplacebo branch) | 'dv' (the branch on Dolby Vision records)
    layout: str = 'planar'      # of the input and the output set
    sub: str = '420'
    loc: str = 'left'
    debug: bool = False  # the chain's debug instances (debug_float)


SETS = [
    Set('fast', 'cpu'), Set('fast_lp', 'lp'),
    Set('fast_semi', 'cpu', 'semi'), Set('fast_lp_semi', 'lp', 'semi'),
    Set('fast_sub422', 'cpu', sub='422'), Set('fast_sub444', 'cpu', sub='444'),
    Set('fast_tl', 'cpu', loc='topleft'), Set('fast_lp_tl', 'lp', loc='topleft'),
    Set('debug', 'cpu', debug=True), Set('debug_lp', 'lp', debug=True),
    Set('debug_semi', 'cpu', 'semi', debug=True), Set('debug_lp_semi', 'lp', 'semi', debug=True),
    Set('fast_lp_dv', 'dv'), Set('fast_lp_dv_semi', 'dv', 'semi'),
    Set('debug_lp_dv', 'dv', debug=True), Set('debug_lp_dv_semi', 'dv', 'semi', debug=True),
]
OPERATORS = ('reinhard', 'hable', 'mobius', 'bt.2390', 'spline')
# vf_tonemap's desaturation: off, on the weighted luma, on the RGB-coefficient
# luma (its default); BT.2390, spline and the libplacebo branch have none
DESAT = {'off': dict(desat=0.0), 'weighted': dict(desat=2.0, desat_luma='bt2020'), 'rgb': dict(desat=2.0, desat_luma='rgb')}
TRANSFERS = {'pq': 'smpte2084', 'hlg': 'arib-std-b67'}
DEBUG_STAGE = 5


def cases(chain):
    """(transfer, operator, desat) of a chain, every one an instance of each of its sets."""
    if chain == 'cpu':
        return [(t, op, d) for t in TRANSFERS for op in OPERATORS
                for d in (DESAT if op in ('reinhard', 'hable', 'mobius') else ('off',))]
    return [(t, op, 'off') for t in (TRANSFERS if chain == 'lp' else ('pq',)) for op in OPERATORS]


ROWS = [(s, t, op, d) for s in SETS for t, op, d in cases(s.chain)]


def row_id(row):
    s, t, op, d = row
    return f'{s.name}/{t}/{op}/{d}'


def params(row):
    s, t, op, d = row
    return hdr2sdr.TonemapParams(tonemapper=op, transfer=TRANSFERS[t], bits_in=BITS, bits_out=BITS,
                                 pipeline='cpu' if s.chain == 'cpu' else 'libplacebo', **DESAT[d])


def dovi_record():
    """The record of the 'dv' sets: full order (8 luma pieces, order-3 MMR chroma)."""
    return DR.realistic_record(BITS)


def base_source():
    """The 4:2:0 planar batch every source derives from (chroma multiples of 8: exact_inputs)."""
    return SR.round8(synth_frames('smooth', NF, W, H, BITS, device='cpu', seed=SEED).to_numpy())


def column_constant(fb):
    """A copy of a planar 4:2:0 numpy batch whose chroma is its first row down
    every column: the left-sited vertical pass (3 h[cy] + h[cy -+ 1]) and the
    top-left one (4 h[cy], 2 (h[cy] + h[cy + 1])) then both give 4 h exactly."""
    out = hdr2sdr.FrameBatch(fb.buf.copy(), fb.width, fb.height, fb.bits)
    for p in (out.u, out.v):
        p[...] = p[..., :1, :]
    return out


def sources(base):
    """{set name: (the set's source, its twin's or None)}: numpy batches.  The
    twin is a planar left-sited 4:2:0 batch whose output the set's output
    equals sample for sample (a semi-planar set's: repacked)."""
    flat = column_constant(base)
    ups = SR.exact_inputs(base)
    out = {}
    for s in SETS:
        if s.sub != '420':
            src, twin = ups[s.sub], base
        elif s.loc == 'topleft':
            src, twin = dataclasses.replace(flat, chroma_location='topleft'), flat
        elif s.layout == 'semi':
            src, twin = base.to_layout('semi'), base
        else:
            src, twin = base, None
        out[s.name] = (src, twin)
    return out
