"""Expected values for 4:2:2 / 4:4:4 input (h2s_set_input_subsampling).

The C oracle reads 4:2:0 only, so the tests take their expected values from
two constructions:

A. *Exact upsamples.*  S1 brings a 4:2:0 chroma plane to 4:4:4 with a
   horizontal left-sited pass (C[2k] = c[k], C[2k+1] = (c[k] + c[k+1]) / 2) and
   a vertical centre-sited pass ((c[m-1] + 3 c[m]) / 4, (3 c[m] + c[m+1]) / 4).
   When the 4:2:0 codes are multiples of 8 both passes give integers, so
   ``vup(c)`` is a 4:2:2 plane and ``hup(vup(c))`` a 4:4:4 plane whose pixels
   are exactly what S1 makes of the 4:2:0 frame: the library's result for them
   is held to the oracle's result for the 4:2:0 frame.

B. *The float64 restatement* (tests/test_oracle_independent.py ``chain``) with
   its upsampler replaced by the model's: the horizontal pass alone on chroma
   row y for 4:2:2, the identity for 4:4:4.  It takes any full-resolution
   chroma.
"""
import numpy as np

import hdr2sdr
import test_oracle_independent as toi

EDGES = ('zimg', 'replicate', 'mirror')


def edge_index(i, n, edge):
    """chroma_edge_at: the sample read at positions i of an n-sample row."""
    i = np.asarray(i).copy()
    neg = i < 0
    i[neg] = 0 if edge == 'replicate' else -i[neg]
    over = i > n - 1
    i[over] = 2 * (n - 1) - i[over] if edge == 'mirror' else n - 1
    return np.clip(i, 0, n - 1)


def _exact_div(a, d):
    assert not np.any(a % d), 'the construction needs chroma codes that are multiples of 8'
    return a // d


def vup(c, edge='zimg'):
    """[..., ch, cw] integer codes -> [..., 2 ch, cw]: the vertical pass, exact."""
    c = np.asarray(c).astype(np.int64)
    ch = c.shape[-2]
    m = np.arange(ch)
    up, dn = edge_index(m - 1, ch, edge), edge_index(m + 1, ch, edge)
    out = np.empty(c.shape[:-2] + (2 * ch, c.shape[-1]), dtype=np.int64)
    out[..., 0::2, :] = _exact_div(c[..., up, :] + 3 * c, 4)
    out[..., 1::2, :] = _exact_div(3 * c + c[..., dn, :], 4)
    return out


def hup(c, edge='zimg'):
    """[..., h, cw] integer codes -> [..., h, 2 cw]: the horizontal pass, exact."""
    c = np.asarray(c).astype(np.int64)
    cw = c.shape[-1]
    nxt = edge_index(np.arange(cw) + 1, cw, edge)
    out = np.empty(c.shape[:-1] + (2 * cw,), dtype=np.int64)
    out[..., 0::2] = c
    out[..., 1::2] = _exact_div(c + c[..., nxt], 2)
    return out


def round8(fb):
    """A copy of a 4:2:0 numpy batch with chroma rounded to multiples of 8
    (clamped to <= 2^bits - 8, so an 'edges' code stays a code)."""
    out = hdr2sdr.FrameBatch(fb.buf.copy(), fb.width, fb.height, fb.bits)
    top = (1 << fb.bits) - 8
    for p in (out.u, out.v):
        p[...] = np.minimum((p.astype(np.int64) + 4) // 8 * 8, top).astype(p.dtype)
    return out


def exact_inputs(fb420, edge='zimg'):
    """{'422': batch, '444': batch}: the exact upsamples of a 4:2:0 numpy
    batch whose chroma codes are multiples of 8 (round8)."""
    y = np.asarray(fb420.y)
    u2, v2 = vup(fb420.u, edge), vup(fb420.v, edge)
    return {'422': hdr2sdr.FrameBatch.from_planes(y, u2, v2, fb420.bits, '422'),
            '444': hdr2sdr.FrameBatch.from_planes(y, hup(u2, edge), hup(v2, edge), fb420.bits, '444')}


def hpass(c, edge='zimg'):
    """The 4:2:2 model in float64: (h, cw) -> (h, 2 cw), horizontal pass only."""
    cw = c.shape[-1]
    nxt = edge_index(np.arange(cw) + 1, cw, edge)
    h = np.empty(c.shape[:-1] + (2 * cw,))
    h[..., 0::2] = c
    h[..., 1::2] = 0.5 * c + 0.5 * c[..., nxt]
    return h


def restated(subsampling, y, u, v, *args, edge='zimg', **kw):
    """toi.chain on one frame whose chroma planes have ``subsampling``."""
    old = toi.upsample
    toi.upsample = {'420': old, '422': lambda c: hpass(c, edge), '444': lambda c: c}[subsampling]
    try:
        return toi.chain(y, u, v, *args, **kw)
    finally:
        toi.upsample = old


def random_chroma(fb420, subsampling, seed):
    """A batch with fb420's luma and seeded uniform chroma codes over the legal
    range at ``subsampling``'s own resolution."""
    rng = np.random.default_rng(seed)
    s = 1 << (fb420.bits - 8)
    out = hdr2sdr.FrameBatch.empty_numpy(fb420.nframes, fb420.width, fb420.height, fb420.bits, 'planar', subsampling)
    out.y[...] = fb420.y
    for p in (out.u, out.v):
        p[...] = rng.integers(16 * s, 240 * s + 1, size=p.shape).astype(p.dtype)
    return out
