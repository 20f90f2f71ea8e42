"""Expected values for Dolby Vision profile 5 (h2s_set_dovi).

The C oracle knows nothing of Dolby Vision, so the tests take their expected
values from constructions that reduce to paths it already gates, and from a
float64 restatement (the pattern of tests/source_tags_ref.py).  Each
construction asserts its own preconditions.

1. *The HDR10 twin.*  ``DoviRpu.hdr10_equivalent(b)`` is, in real arithmetic,
   the limited-range BT.2020-NCL PQ decode, so a frame with that record must
   give what the oracle gives for the same codes as plain HDR10 wherever E' lies
   in [0, 1] after upsampling (``twin_source``; ``e_prime`` is the float64
   check).
2. *Integer reshape twins.*  A piecewise-linear luma polynomial with a1 in
   {1, 2} and a0 = k / (2^b - 1) maps code to code, so (frame, record) equals
   (mapped frame, twin record) in real arithmetic.  The pivots sit on the
   boundary between two codes ((p - 1/2) / (2^b - 1)), so that no code falls
   on a pivot and float32 pivots cannot move a code to the other piece
   (``LUMA_MAPS``, ``luma_map_record``, ``apply_luma_map``).
3. *First-order MMR twins.*  An order-1 MMR with no cross terms is a 3 x 3
   affine map r = m0 + A s; folded into the non-linear matrix and offset (N A,
   A^-1 (off - m0)) it is an identity-reshape record with the same output
   where no clamp acts (``mmr_affine_pair``).
4. *The float64 restatement* of the model of include/h2s.h (``dovi_linear``)
   with the libplacebo branch's tail from linear light (``lp_tail``), taken from
   test_oracle_independent.chain_lp; tests/test_dovi.py pins that copy to
   chain_lp sample for sample on HDR10 content.
5. *A realistic full-order record* (``realistic_record``): luma an 8-piece
   monotone quadratic fit of x^1.15, chroma single-piece order-3 MMR near the
   identity with cross coefficients <= 0.1 in magnitude, seeded; the matrices
   through ``DoviRpu.from_fixed_point``.
"""
import numpy as np

import hdr2sdr
import test_oracle_independent as toi
from hdr2sdr.dovi import DoviCurve, DoviRpu
from hdr2sdr.synth import synth_frames
from subsampling_ref import edge_index, hpass


# ---- the record as the library sees it (float32 fields, read back as float64) -------------
def c_arrays(rpu):
    """The record's numbers after ``to_c()``: what the kernels read."""
    c = rpu.to_c()
    out = dict(off=np.array(list(c.nonlinear_offset), dtype=np.float64),
               nl=np.array(list(c.nonlinear), dtype=np.float64).reshape(3, 3),
               lin=np.array(list(c.linear), dtype=np.float64).reshape(3, 3), comp=[])
    for k in c.comp:
        n = k.num_pivots
        out['comp'].append(dict(
            pivots=np.array(list(k.pivots)[:n], dtype=np.float64), method=list(k.method)[:n - 1],
            poly=np.array([list(p) for p in k.poly], dtype=np.float64)[:n - 1], order=list(k.mmr_order)[:n - 1],
            const=np.array(list(k.mmr_const), dtype=np.float64)[:n - 1],
            mmr=np.array([[list(r) for r in m] for m in k.mmr], dtype=np.float64)[:n - 1]))
    return out


# ---- 4: the float64 restatement -------------------------------------------------------------
def upsample(c, edge='zimg'):
    """The branch's S1 upsampler on one 4:2:0 plane (ch, cw) -> (2 ch, 2 cw):
    left-sited horizontal pass, centre-sited vertical pass (1/4, 3/4), the edge
    rule of params.chroma_edge."""
    h = hpass(np.asarray(c, dtype=np.float64), edge)
    ch = h.shape[-2]
    up = edge_index(np.arange(ch) - 1, ch, edge)
    dn = edge_index(np.arange(ch) + 1, ch, edge)
    v = np.empty((2 * ch, h.shape[-1]))
    v[0::2] = 0.25 * h[up] + 0.75 * h
    v[1::2] = 0.75 * h + 0.25 * h[dn]
    return v


def reshape(s, rpu):
    """Step 2: s [H, W, 3] (code fractions) -> r [H, W, 3]."""
    R = c_arrays(rpu)
    t = np.stack([s[..., 0], s[..., 1], s[..., 2], s[..., 0] * s[..., 1], s[..., 0] * s[..., 2],
                  s[..., 1] * s[..., 2], s[..., 0] * s[..., 1] * s[..., 2]], -1)
    out = np.empty(s.shape)
    for c, K in enumerate(R['comp']):
        x = s[..., c]
        piv = K['pivots']
        k = np.clip(np.searchsorted(piv, x, side='right') - 1, 0, len(piv) - 2)
        r = np.zeros(x.shape)
        for i in range(len(piv) - 1):
            if K['method'][i] == 0:
                a = K['poly'][i]
                ri = a[0] + a[1] * x + a[2] * x * x
            else:
                ri = np.full(x.shape, K['const'][i])
                for o in range(K['order'][i]):
                    ri = ri + (t ** (o + 1)) @ K['mmr'][i][o]
            r = np.where(k == i, ri, r)
        out[..., c] = np.clip(r, piv[0], piv[-1])
    return out


def dovi_lms(y, u, v, bits, rpu, edge='zimg', mask=None):
    """Steps 1-4: integer planes -> (L'M'S' v [H, W, 3], LMS light in nits)."""
    full = float((1 << bits) - 1)
    y, u, v = (np.asarray(p).astype(np.int64) for p in (y, u, v))
    if mask is not None:
        y, u, v = y & mask, u & mask, v & mask
    s = np.clip(np.stack([y / full, upsample(u / full, edge), upsample(v / full, edge)], -1), 0.0, 1.0)
    R = c_arrays(rpu)
    vv = np.clip((reshape(s, rpu) - R['off']) @ R['nl'].T, 0.0, 1.0)
    return vv, toi.pq_eotf(vv) * 1e4


def dovi_linear(y, u, v, bits, rpu, edge='zimg', mask=None):
    """Steps 1-5: linear BT.2020 light in nits, [H, W, 3] (not clamped)."""
    _, lms = dovi_lms(y, u, v, bits, rpu, edge, mask)
    return lms @ c_arrays(rpu)['lin'].T


def hdr10_linear(y, u, v, bits):
    """test_oracle_independent.chain_lp's own stage 1 (PQ input): nits."""
    s = 1 << (bits - 8)
    Y = (np.asarray(y).astype(np.float64) - 16 * s) / (219 * s)
    Cb = toi.upsample((np.asarray(u).astype(np.float64) - 128 * s) / (224 * s))
    Cr = toi.upsample((np.asarray(v).astype(np.float64) - 128 * s) / (224 * s))
    kr, kb = 0.2627, 0.0593
    kg = 1.0 - kr - kb
    E = np.stack([Y + 2 * (1 - kr) * Cr, Y - 2 * kb * (1 - kb) / kg * Cb - 2 * kr * (1 - kr) / kg * Cr,
                  Y + 2 * (1 - kb) * Cb], -1)
    return toi.pq_eotf(E) * 1e4


def lp_tail(L, bits_out, lut_n, white=203.0, ipt=False):
    """The libplacebo branch from linear light L [H, W, 3] (nits) to output
    planes: test_oracle_independent.chain_lp from its ``if ipt:`` on (BT.2390
    against the 1000-nit default peak, BT.1886 encode, 8-bit rgba download,
    lut3d's truncating 8-bit path, BT.709 Y'CbCr at the output depth)."""
    if ipt:
        r2l = toi.rgb_to_lms()
        q = toi.pq_encode(np.minimum(L, 1e8) / 1e4 @ r2l.T)
        I = q @ np.array([0.4, 0.4, 0.2])
        lms = toi.pq_eotf(q + (toi.bt2390(I) - I)[..., None])
        T = lms @ np.linalg.inv(r2l).T * (1e4 / white)
    else:
        sig = np.maximum(L.max(-1), 1e-4)
        out = toi.pq_eotf(toi.bt2390(toi.pq_encode(sig / 1e4))) * 1e4 / white
        T = L * (out / sig)[..., None]
    lb = (1.0 / 1000.0) ** (1 / 2.4)
    enc = np.power(np.maximum(T, 0.0) / (1 - lb) ** 2.4, 1 / 2.4) - lb / (1 - lb)
    q8 = np.floor(np.clip(enc, 0.0, 1.0) * 255.0 + 0.5)
    o = toi.tetrahedral(toi.lattice(lut_n), q8 / 255.0 * (lut_n - 1))
    rgb = np.clip(np.floor(o * 255.0), 0, 255) / 255.0
    Yo = rgb @ np.array([0.2126, 0.7152, 0.0722])
    cb = (rgb[..., 2] - Yo) / 1.8556
    cr = (rgb[..., 0] - Yo) / 1.5748
    qs, qmax = float(1 << (bits_out - 8)), (1 << bits_out) - 1
    yq = np.clip(np.floor((16.0 + 219.0 * Yo) * qs + 0.5), 0, qmax).astype(np.int64)
    quad = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) / 4.0   # noqa: E731
    cq = [np.clip(np.floor((128.0 + 224.0 * quad(p)) * qs + 0.5), 0, qmax).astype(np.int64) for p in (cb, cr)]
    return yq, cq[0], cq[1]


def restated(fb, rpus, bits_out, lut_n, ipt=True, mask=None):
    """The model on a numpy batch (record f for frame f, or one for all):
    [F, W*H*3/2] int64 in the library's frame layout."""
    out = []
    for f in range(fb.nframes):
        r = rpus[f] if isinstance(rpus, (list, tuple)) else rpus
        L = dovi_linear(fb.y[f], fb.u[f], fb.v[f], fb.bits, r, mask=mask)
        out.append(np.concatenate([p.reshape(-1) for p in lp_tail(L, bits_out, lut_n, ipt=ipt)]))
    return np.stack(out)


# ---- 1: the HDR10 twin ------------------------------------------------------------------------
def e_prime(fb):
    """E' of every pixel of a limited-range BT.2020-NCL batch, float64 [F, H, W, 3]."""
    s = 1 << (fb.bits - 8)
    kr, kb = 0.2627, 0.0593
    kg = 1.0 - kr - kb
    out = []
    for f in range(fb.nframes):
        Y = (np.asarray(fb.y[f]).astype(np.float64) - 16 * s) / (219 * s)
        Cb = toi.upsample((np.asarray(fb.u[f]).astype(np.float64) - 128 * s) / (224 * s))
        Cr = toi.upsample((np.asarray(fb.v[f]).astype(np.float64) - 128 * s) / (224 * s))
        out.append(np.stack([Y + 2 * (1 - kr) * Cr, Y - 2 * kb * (1 - kb) / kg * Cb - 2 * kr * (1 - kr) / kg * Cr,
                             Y + 2 * (1 - kb) * Cb], -1))
    return np.stack(out)


def inside(fb, margin=1e-6):
    e = e_prime(fb)
    return bool(e.min() >= margin and e.max() <= 1.0 - margin)


def pull_in(fb, luma=(0.0, 1.0), chroma=1.0):
    """A copy of a numpy batch with luma mapped affinely into the fraction
    ``luma`` of the limited range and chroma scaled toward neutral."""
    s = 1 << (fb.bits - 8)
    out = hdr2sdr.FrameBatch(fb.buf.copy(), fb.width, fb.height, fb.bits)
    yn = (np.asarray(fb.y).astype(np.float64) - 16 * s) / (219 * s)
    out.y[...] = np.rint(16 * s + 219 * s * (luma[0] + (luma[1] - luma[0]) * np.clip(yn, 0, 1))).astype(out.buf.dtype)
    for p, q in ((fb.u, out.u), (fb.v, out.v)):
        q[...] = np.rint(128 * s + chroma * (np.asarray(p).astype(np.float64) - 128 * s)).astype(out.buf.dtype)
    return out


def twin_source(W, H, bits, nframes=3, kind='smooth', seed=13):
    """Content on which the HDR10 twin is exact: E' in [0, 1] at every pixel
    after upsampling, asserted in float64.  'smooth' with seed 13 is inside as
    it is at 128 x 64; anything else is pulled toward neutral until it is."""
    fb = synth_frames(kind, nframes, W, H, bits, device='cpu', seed=seed).to_numpy()
    c = 1.0
    while not inside(fb) and c > 0.05:
        c *= 0.8
        fb = pull_in(synth_frames(kind, nframes, W, H, bits, device='cpu', seed=seed).to_numpy(),
                     (0.5 - 0.5 * c, 0.5 + 0.5 * c), c)
    assert inside(fb), 'the HDR10 twin needs E\' in [0, 1]'
    return fb


# ---- 2: integer reshape twins ---------------------------------------------------------------
# luma maps in 10-bit codes (x 2^(b - 10) at depth b): pieces (first code, a1, k):
# code y >= first maps to a1 y + k
LUMA_MAPS = (
    ((0, 1, 40), (400, 2, -360), (500, 1, 140)),
    ((0, 1, -100), (450, 1, 60)),
    ((0, 2, -300), (350, 1, 50)),
)
LUMA_SRC = (0.27, 0.61)     # the source's luma: codes 300..598 (10-bit), inside every map's range


def apply_luma_map(y, pieces, bits):
    s = 1 << (bits - 10)
    y = np.asarray(y).astype(np.int64)
    out = np.zeros_like(y)
    for first, a1, k in pieces:
        out = np.where(y >= first * s, a1 * y + k * s, out)
    assert out.min() >= 0 and out.max() <= (1 << bits) - 1
    return out


def luma_map_record(pieces, bits, base=None):
    """``base`` (default: the HDR10 twin) with the luma curve of the map: pivots
    0, the half-code boundaries between the pieces, 1."""
    s, full = 1 << (bits - 10), float((1 << bits) - 1)
    base = DoviRpu.hdr10_equivalent(bits) if base is None else base
    piv = [0.0] + [(first * s - 0.5) / full for first, _, _ in pieces[1:]] + [1.0]
    luma = DoviCurve.polynomial(piv, [(k * s / full, float(a1)) for _, a1, k in pieces])
    return base.with_(comp=(luma, base.comp[1], base.comp[2]))


def luma_map_pair(W, H, bits, nframes=3):
    """(source batch, its records, mapped batch): frame f with LUMA_MAPS[f %
    3]; the mapped batch with the HDR10 twin's record is the construction's
    other side, and lies inside the twin's domain (asserted)."""
    src = pull_in(synth_frames('smooth', nframes, W, H, bits, device='cpu', seed=13).to_numpy(), LUMA_SRC, 0.25)
    mapped = hdr2sdr.FrameBatch(src.buf.copy(), W, H, bits)
    recs = []
    for f in range(nframes):
        pieces = LUMA_MAPS[f % len(LUMA_MAPS)]
        mapped.y[f] = apply_luma_map(src.y[f], pieces, bits).astype(mapped.buf.dtype)
        recs.append(luma_map_record(pieces, bits))
        # the identity, float64: the record's reshaped luma is the mapped code's fraction
        full = float((1 << bits) - 1)
        s3 = np.stack([np.asarray(src.y[f]) / full] * 3, -1)
        assert np.abs(reshape(s3, recs[-1])[..., 0] - np.asarray(mapped.y[f]) / full).max() < 1e-7
        assert len(np.unique(np.asarray(mapped.y[f]))) > 8
    assert inside(mapped), 'the mapped frames leave the HDR10 twin\'s domain'
    return src, recs, mapped


# ---- 3: first-order MMR twins -----------------------------------------------------------------
def mmr_affine_pair(bits, seed=3, luma_mmr=True):
    """(record whose components are order-1 MMRs without cross terms, r = m0 +
    A s; the identity-reshape record N A, A^-1 (off - m0)) over the HDR10
    twin's matrices.  A is near the identity, so that r stays inside (0, 1)
    on content inside the twin's domain (checked by the caller).  luma_mmr
    False: the shape the tile kernel takes: luma a polynomial a0 + a1 s0 (row 0
    of A is (a1, 0, 0)), chroma the MMRs."""
    rng = np.random.default_rng(seed)
    A = np.eye(3) + rng.uniform(-0.04, 0.04, size=(3, 3))
    m0 = rng.uniform(0.005, 0.02, size=3)
    base = DoviRpu.hdr10_equivalent(bits)
    comp = [DoviCurve.mmr_single(m0[c], [list(A[c]) + [0.0] * 4]) for c in range(3)]
    if not luma_mmr:
        A[0, 1:] = 0.0
        comp[0] = DoviCurve.polynomial((0.0, 1.0), [(m0[0], A[0, 0])])
    comp = tuple(comp)
    # the folded record from the float32 values the library reads
    R = c_arrays(base.with_(comp=comp))
    A32 = np.array([R['comp'][c]['mmr'][0][0][:3] if R['comp'][c]['method'][0] else [R['comp'][0]['poly'][0][1], 0.0, 0.0]
                    for c in range(3)])
    m32 = np.array([R['comp'][c]['const'][0] if R['comp'][c]['method'][0] else R['comp'][c]['poly'][0][0]
                    for c in range(3)])
    N2 = R['nl'] @ A32
    off2 = np.linalg.solve(A32, R['off'] - m32)
    folded = base.with_(nonlinear=tuple(float(v) for v in N2.reshape(-1)), nonlinear_offset=tuple(float(v) for v in off2))
    return base.with_(comp=comp), folded


def no_clamp_acts(fb, rpu):
    """Neither the reshape's clamp nor the L'M'S' clamp acts on fb under rpu (float64)."""
    R = c_arrays(rpu)
    full = float((1 << fb.bits) - 1)
    for f in range(fb.nframes):
        s = np.stack([np.asarray(fb.y[f]) / full, upsample(np.asarray(fb.u[f]) / full),
                      upsample(np.asarray(fb.v[f]) / full)], -1)
        saved = [K['pivots'].copy() for K in R['comp']]
        r = reshape(s, rpu)
        for c, piv in enumerate(saved):
            if r[..., c].min() <= piv[0] + 1e-6 or r[..., c].max() >= piv[-1] - 1e-6:
                return False
        v = (r - R['off']) @ R['nl'].T
        if v.min() <= 1e-6 or v.max() >= 1.0 - 1e-6:
            return False
    return True


# ---- 5: a realistic full-order record ---------------------------------------------------------
# the colour metadata of a typical profile-5 RPU, as AVDOVIColorMetadata's integers
YCC_TO_RGB = (8192, 799, 1681, 8192, -933, 1091, 8192, 267, -5545)
YCC_OFFSET = (0, 1 << 27, 1 << 27)
RGB_TO_LMS = (5845, 9702, 837, 2568, 12256, 1561, 0, 0, 16383)
COEF_LOG2_DENOM = 23


def realistic_record(bits, seed=7):
    """Luma: 8 quadratic pieces through the ends and the middle of x^1.15 on
    each eighth (monotone: asserted); chroma: one order-3 MMR piece each, the
    own first-order term 1 +- 0.02, every other coefficient <= 0.1 in
    magnitude and shrinking with the order, a constant that keeps neutral
    chroma near neutral.  Everything through from_fixed_point's integers."""
    rng = np.random.default_rng(seed)
    full, den = (1 << bits) - 1, 1 << COEF_LOG2_DENOM
    g = lambda x: x ** 1.15   # noqa: E731
    edges = [round(full * k / 8) for k in range(9)]
    poly = []
    for k in range(8):
        x = np.array([edges[k], 0.5 * (edges[k] + edges[k + 1]), edges[k + 1]]) / full
        a = np.linalg.solve(np.stack([np.ones(3), x, x * x], -1), g(x))
        assert a[1] + 2 * a[2] * x[0] > 0 and a[1] + 2 * a[2] * x[2] > 0      # monotone on the piece
        poly.append([int(round(v * den)) for v in a])
    mmr, const = [], []
    for c in (1, 2):
        coef = rng.uniform(-0.1, 0.1, size=(3, 7)) * np.array([1.0, 0.3, 0.1])[:, None]
        coef[0, c] = 1.0 + rng.uniform(-0.02, 0.02)
        # neutral input (s = (1/2, 1/2, 1/2)) stays at 1/2
        t = np.array([0.5, 0.5, 0.5, 0.25, 0.25, 0.25, 0.125])
        const.append(0.5 - sum((t ** (o + 1)) @ coef[o] for o in range(3)))
        mmr.append(coef)
        assert np.abs(np.delete(coef.reshape(-1), c)).max() <= 0.1
    q = lambda a: np.rint(np.asarray(a) * den).astype(np.int64).tolist()   # noqa: E731
    return DoviRpu.from_fixed_point(
        bits, pivots=[edges, [0, full], [0, full]], methods=[[0] * 8, [1], [1]],
        poly_coef=[poly, [[0, den, 0]], [[0, den, 0]]], mmr_order=[[0] * 8, [3], [3]],
        mmr_constant=[[0] * 8, [q(const[0])], [q(const[1])]], mmr_coef=[[None] * 8, [q(mmr[0])], [q(mmr[1])]],
        coef_log2_denom=COEF_LOG2_DENOM, ycc_to_rgb_matrix=YCC_TO_RGB, ycc_to_rgb_offset=YCC_OFFSET,
        rgb_to_lms_matrix=RGB_TO_LMS)
