"""Expected values for tagged input (h2s_set_input_tags): full-range codes
(color_range pc) and top-left sited 4:2:0 chroma.

The C oracle reads limited-range, left-sited 4:2:0 only, so the tests take
their expected values from four constructions.  Each asserts its own
preconditions.

1. *Top-left == the 4:2:2 path.*  For a 4:2:0 plane c of even codes, the 4:2:2
   plane p[2m] = c[m], p[2m+1] = (c[m] + c[edge(m+1)]) / 2 is exact in integers,
   and the 4:2:2 model's horizontal pass of p equals the top-left upsample of c
   everywhere (``as_422``).  So the library's output for (c, topleft) is held to
   its own output for (p, 4:2:2), a path gated against the oracle already.

2. *Vertical ramps.*  Per column, c[m] = a(x) + b(x) m with a a multiple of 8 and
   b a multiple of 4.  The left-sited plane c' = c + b/4 has the same S1 output
   as top-left c on every luma row except rows 0 and H - 1 (``ramp_pair``), so
   (c, topleft) is held to the oracle's result for c' with output luma rows 0,
   H - 1 and output chroma rows 0, H/2 - 1 left out (``without_edge_rows``).

3. *Grey steps.*  Full-range luma code 341 k (10-bit) / 1365 k (12-bit), k =
   0..3, with neutral chroma 2^(b-1) normalises to exactly what the limited
   codes 64 + 292 k / 256 + 1168 k with neutral chroma do (k / 3, 0, 0): a frame
   of those levels sent as full range is held to the oracle's result for the
   limited twin (``grey_steps``).

4. *The float64 restatement* (tests/test_oracle_independent.py ``chain``) on
   arbitrary content, with its upsampler replaced by the top-left model's and,
   for full range, float pseudo-codes that its limited-range normalisation
   turns into the full-range values (``restated``).
"""
from fractions import Fraction

import numpy as np

import hdr2sdr
import test_oracle_independent as toi
from subsampling_ref import edge_index, hpass

FULL, TOPLEFT = 'pc', 'topleft'


# ---- the model, float64 ------------------------------------------------------------
def topleft_upsample(c, edge='zimg'):
    """4:2:0 plane (ch, cw) -> (2 ch, 2 cw): horizontal left-sited pass, then the
    vertical pass co-sited with the even luma row: C[2m] = c[m], C[2m+1] =
    c[m]/2 + c[m+1]/2, row ch by the edge rule."""
    h = hpass(np.asarray(c, dtype=np.float64), edge)
    ch = h.shape[-2]
    dn = edge_index(np.arange(ch) + 1, ch, edge)
    v = np.empty(h.shape[:-2] + (2 * ch, h.shape[-1]))
    v[..., 0::2, :] = h
    v[..., 1::2, :] = 0.5 * h + 0.5 * h[..., dn, :]
    return v


def tagged(fb, color_range='tv', chroma_location='left'):
    """fb's samples (shared, not copied) read with the given tags."""
    return hdr2sdr.FrameBatch(fb.buf, fb.width, fb.height, fb.bits, fb.layout, fb.subsampling, color_range,
                              chroma_location)


# ---- 1: top-left == the 4:2:2 path ---------------------------------------------------
def round2(fb):
    """A copy of a 4:2:0 numpy batch with chroma codes rounded down to even."""
    out = hdr2sdr.FrameBatch(fb.buf.copy(), fb.width, fb.height, fb.bits)
    for p in (out.u, out.v):
        p[...] = p & ~np.asarray(1, dtype=p.dtype)
    return out


def vpair(c, edge='zimg'):
    """[..., ch, cw] even integer codes -> [..., 2 ch, cw]: p[2m] = c[m],
    p[2m+1] = (c[m] + c[edge(m+1)]) / 2, exact."""
    c = np.asarray(c).astype(np.int64)
    assert not np.any(c % 2), 'the construction needs even chroma codes'
    ch = c.shape[-2]
    dn = edge_index(np.arange(ch) + 1, ch, edge)
    out = np.empty(c.shape[:-2] + (2 * ch, c.shape[-1]), dtype=np.int64)
    out[..., 0::2, :] = c
    out[..., 1::2, :] = (c + c[..., dn, :]) // 2
    return out


def as_422(fb420, edge='zimg'):
    """The 4:2:2 batch whose horizontal pass is the top-left upsample of the
    4:2:0 numpy batch fb420 (even chroma codes), checked here in float64."""
    u2, v2 = vpair(fb420.u, edge), vpair(fb420.v, edge)
    for c, p in ((fb420.u, u2), (fb420.v, v2)):
        assert np.array_equal(hpass(p.astype(np.float64), edge), topleft_upsample(c, edge))
    return hdr2sdr.FrameBatch.from_planes(np.asarray(fb420.y), u2, v2, fb420.bits, '422')


# ---- 2: vertical ramps ----------------------------------------------------------------
def ramp_pair(luma420, seed):
    """(tagged top-left batch c, left-sited twin c') with luma420's luma and,
    per column, c[m] = a + b m: a a multiple of 8 in [320, 640] s, b a multiple
    of 4 with |b| (ch - 1) + |b| / 4 <= 256 s (s = 2^(bits - 10)), so that every
    code of c and c' = c + b/4 is a legal chroma code."""
    rng = np.random.default_rng(seed)
    s = 1 << (luma420.bits - 10)
    F, ch, cw = np.asarray(luma420.u).shape
    bmax = (256 * s // ch) // 4
    assert bmax >= 1
    src = hdr2sdr.FrameBatch(luma420.buf.copy(), luma420.width, luma420.height, luma420.bits)
    twin = hdr2sdr.FrameBatch(luma420.buf.copy(), luma420.width, luma420.height, luma420.bits)
    m = np.arange(ch)[None, :, None]
    for ps, pt in ((src.u, twin.u), (src.v, twin.v)):
        a = 8 * rng.integers(40 * s, 80 * s + 1, size=(F, 1, cw))
        b = 4 * rng.integers(-bmax, bmax + 1, size=(F, 1, cw))
        c = a + b * m
        ct = c + b // 4
        assert c.min() >= 64 * s and c.max() <= 960 * s and ct.min() >= 64 * s and ct.max() <= 960 * s
        # the identity: every luma row but the first and the last
        assert np.array_equal(topleft_upsample(c)[..., 1:-1, :], toi_upsample_batch(ct)[..., 1:-1, :])
        ps[...] = c.astype(ps.dtype)
        pt[...] = ct.astype(pt.dtype)
    return tagged(src, 'tv', TOPLEFT), twin


def toi_upsample_batch(c):
    """test_oracle_independent.upsample (left-sited, centre-sited vertically) per frame."""
    return np.stack([toi.upsample(f.astype(np.float64)) for f in c])


def without_edge_rows(got, want, W, H):
    """got [F, W*H*3/2] with output luma rows 0 and H - 1 and output chroma
    rows 0 and H/2 - 1 taken from want: those rows are left out of a gate."""
    got = got.copy()
    ysz, cw, ch = W * H, W // 2, H // 2
    gy, wy = got[:, :ysz].reshape(-1, H, W), want[:, :ysz].reshape(-1, H, W)
    gy[:, [0, H - 1]] = wy[:, [0, H - 1]]
    gc, wc = got[:, ysz:].reshape(-1, 2, ch, cw), want[:, ysz:].reshape(-1, 2, ch, cw)
    gc[:, :, [0, ch - 1]] = wc[:, :, [0, ch - 1]]
    return got


# ---- 3: grey steps ---------------------------------------------------------------------
def grey_steps(nframes, W, H, bits, seed=5, levels=(0, 1, 2, 3)):
    """(full-range tagged batch, limited twin): the levels k in 16-pixel blocks
    (frame 0 onwards alternately: seeded blocks, vertical stripes, horizontal
    stripes), neutral chroma."""
    rng = np.random.default_rng(seed)
    s = 1 << (bits - 8)
    top = (1 << bits) - 1
    fstep, lstep, l0 = top // 3, 73 * s, 16 * s
    for k in range(4):   # the two normalisations agree exactly
        assert Fraction(fstep * k, top) == Fraction(lstep * k, 219 * s) == Fraction(k, 3)
    full = hdr2sdr.FrameBatch.empty_numpy(nframes, W, H, bits)
    twin = hdr2sdr.FrameBatch.empty_numpy(nframes, W, H, bits)
    yy, xx = np.mgrid[0:H, 0:W]
    lv = np.asarray(levels)
    for f in range(nframes):
        if f % 3 == 0:
            blocks = rng.integers(0, len(lv), size=((H + 15) // 16, (W + 15) // 16))
            k = lv[blocks[yy // 16, xx // 16]]
        elif f % 3 == 1:
            k = lv[(xx // 8) % len(lv)]
        else:
            k = lv[(yy // 2) % len(lv)]
        full.y[f] = (fstep * k).astype(full.buf.dtype)
        twin.y[f] = (l0 + lstep * k).astype(twin.buf.dtype)
    for fb in (full, twin):
        fb.u[...] = 1 << (bits - 1)
        fb.v[...] = 1 << (bits - 1)
    return tagged(full, FULL, 'left'), twin


# ---- 4: the float64 restatement -----------------------------------------------------
def restated(y, u, v, bits_in, *rest, color_range='tv', chroma_location='left', **kw):
    """toi.chain on one tagged 4:2:0 frame.  Full range: float pseudo-codes
    y' = 16 s + 219 s code / (2^b - 1), u' = 128 s + 224 s (code - 2^(b-1)) /
    (2^b - 1), which chain's limited-range normalisation turns into the
    full-range values; top-left: chain's upsampler replaced by the model's."""
    y, u, v = (np.asarray(p).astype(np.float64) for p in (y, u, v))
    if color_range == FULL:
        s, top, mid = float(1 << (bits_in - 8)), float((1 << bits_in) - 1), float(1 << (bits_in - 1))
        y = 16 * s + 219 * s * y / top
        u, v = (128 * s + 224 * s * (c - mid) / top for c in (u, v))
    old = toi.upsample
    if chroma_location == TOPLEFT:
        toi.upsample = topleft_upsample
    try:
        return toi.chain(y, u, v, bits_in, *rest, **kw)
    finally:
        toi.upsample = old

