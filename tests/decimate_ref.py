"""The 4:2:0 front-end's model (h2s_set_input_decimation) in
float64 numpy, written from its formulas; the tie-aware gate against it; the
float32 evaluation of the model in both pass orders; two mutants; and the
contents the CPU and GPU tests share.

Model: swscale bicubic (B = 0, C = 0.6) chroma decimation.  4:4:4 horizontally
7 taps on source columns 2k-3 .. 2k+3 (left-sited); 4:4:4 and 4:2:2 vertically
8 taps on source rows 2m-3 .. 2m+4 (centred); indices clamped to the plane;
v = floor(acc + 0.5) clamped to [0, 2^b - 1].
"""
import numpy as np

SIZES = [(64, 32), (192, 70), (70, 34), (208, 64)]
CONTENTS = ('noise', 'smooth', 'edges')
# the kernel's edges (tests/test_gpu_decimate.py says which): every width x height, and two more shapes
WIDTHS = (16, 70, 144, 208)
HEIGHTS = (4, 10, 34, 70)
MORE = [(1044, 10), (144, 66)]
SMALL = [(w, h) for w in WIDTHS for h in HEIGHTS] + MORE
TIE_CAP = 0.02        # noise / smooth: at most this share of a plane inside the tie window
CAP_MIN_SAMPLES = 1000   # ... of a plane with at least this many output samples (16 samples: one tie is 6 %)
EDGES_CLEAR = 0.80    # edges: at least this share outside it


def bicubic(x):
    B, C = 0.0, 0.6
    x = abs(x)
    if x < 1.0:
        return ((12 - 9 * B - 6 * C) * x ** 3 + (-18 + 12 * B + 6 * C) * x ** 2 + (6 - 2 * B)) / 6.0
    if x < 2.0:
        return ((-B - 6 * C) * x ** 3 + (6 * B + 30 * C) * x ** 2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) / 6.0
    return 0.0


def taps():
    """(wx7, wy8) in float64, normalised."""
    wx = np.array([bicubic((i - 3) / 2.0) for i in range(7)])
    wy = np.array([bicubic((j - 3.5) / 2.0) for j in range(8)])
    return wx / wx.sum(), wy / wy.sum()


def delta(bits):
    """Half-width of the tie window: at most 17 float32 roundings (15 FMAs and
    the weight roundings) on partial sums of at most (2^b - 1) * 1.15 (sum |wx|)
    * 1.1125 (the positive wy: the largest partial sum of the vertical chain)
    < (2^b - 1) * 1.28."""
    return 17 * 2.0 ** -24 * 1.28 * ((1 << bits) - 1)


def _rows(p, first, n):
    """[H / 2, n]: source rows first + 2 m + t of p, clamped to the plane."""
    H = p.shape[-2]
    return np.clip(first + 2 * np.arange(H // 2)[:, None] + np.arange(n)[None, :], 0, H - 1)


def _vertical(p, wy, fma=None):
    idx = _rows(p, -3, 8)                         # [H/2, 8]
    return _chain(np.moveaxis(p[..., idx, :], -2, 0), wy, fma)     # taps first


def _horizontal(p, wx, fma=None):
    W = p.shape[-1]
    k = np.arange(W // 2)
    idx = np.clip(2 * k[:, None] - 3 + np.arange(7)[None, :], 0, W - 1)   # [W/2, 7]
    return _chain(np.moveaxis(p[..., idx], -1, 0), wx, fma)


def _chain(terms, w, fma):
    """sum_t w[t] * terms[t], ascending from 0: in float64, or with fma(a, b, c)."""
    if fma is None:
        acc = np.zeros(terms.shape[1:], dtype=np.float64)
        for t in range(len(w)):
            acc = acc + w[t] * terms[t].astype(np.float64)
        return acc
    acc = np.zeros(terms.shape[1:], dtype=np.float32)
    for t in range(len(w)):
        acc = fma(np.float32(w[t]), terms[t].astype(np.float32), acc)
    return acc


def _round(u, bits):
    return np.clip(np.floor(u.astype(np.float64) + 0.5), 0, (1 << bits) - 1).astype(np.int64)


def decimate(plane, sub, bits):
    """plane: [..., H, Wc] integer codes of one chroma plane of a 4:2:2 ('422')
    or 4:4:4 ('444') set.  Returns (codes [..., H/2, W/2], the unrounded float64
    values)."""
    wx, wy = taps()
    u = _vertical(np.asarray(plane), wy)
    if sub == '444':
        u = _horizontal(u, wx)
    return _round(u, bits), u


def _fmaf(a, b, c):
    # a * b is exact in float64 (24 + 24 bits); one float64 rounding of the sum, then float32's
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def decimate_f32(plane, sub, bits, order='vh'):
    """The model as the kernel evaluates it: float32 weights and fmaf chains;
    order 'vh' (vertical first) or 'hv'."""
    wx, wy = taps()
    wx, wy = wx.astype(np.float32), wy.astype(np.float32)
    p = np.asarray(plane)
    if sub == '422':
        u = _vertical(p, wy, _fmaf)
    elif order == 'vh':
        u = _horizontal(_vertical(p, wy, _fmaf), wx, _fmaf)
    else:
        u = _vertical(_horizontal(p, wx, _fmaf), wy, _fmaf)
    v = np.floor(u + np.float32(0.5))
    return np.clip(v, 0, (1 << bits) - 1).astype(np.int64)


def mutant_cosited(plane, sub, bits):
    """Vertically co-sited: the 7-tap pass on rows 2m-3 .. 2m+3."""
    wx, _ = taps()
    p = np.asarray(plane)
    idx = _rows(p, -3, 7)
    u = _chain(np.moveaxis(p[..., idx, :], -2, 0), wx, None)
    if sub == '444':
        u = _horizontal(u, wx)
    return _round(u, bits)


def mutant_box(plane, sub, bits):
    """The 2 x 1 (4:2:2) / 2 x 2 (4:4:4) box."""
    p = np.asarray(plane).astype(np.float64)
    u = (p[..., 0::2, :] + p[..., 1::2, :]) / 2
    if sub == '444':
        u = (u[..., 0::2] + u[..., 1::2]) / 2
    return _round(u, bits)


def gate(got, plane, sub, bits):
    """The tie-aware comparison of `got` with the model of `plane`: a sample
    equals the reference's rounded value, except where the unrounded value lies
    within delta(bits) of k + 0.5, where it may differ by one code.  Returns
    (samples that miss, share of samples inside the tie window, samples that
    differ at all)."""
    want, u = decimate(plane, sub, bits)
    got = np.asarray(got).astype(np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    tie = np.abs(u - (np.floor(u) + 0.5)) <= delta(bits)
    d = np.abs(got - want)
    miss = np.where(tie, d > 1, d > 0)
    return int(miss.sum()), float(tie.mean()), int((d > 0).sum())


def beyond_one(got, plane, sub, bits):
    """Share of samples more than one code from the model (the mutants' measure)."""
    want, _ = decimate(plane, sub, bits)
    return float((np.abs(np.asarray(got).astype(np.int64) - want) > 1).mean())


def content(kind, nframes, W, H, sub, bits, seed=5):
    """(y, u, v): [F, H, W] luma and [F, H, Wc] chroma codes (Wc = W / 2 for
    '422', W for '444').  noise: uniform codes; smooth: gradients with a little
    noise; edges: blocks of code 0 and 2^b - 1."""
    rng = np.random.default_rng([seed, W, H, bits, CONTENTS.index(kind), sub == '444'])
    top = (1 << bits) - 1
    Wc = W if sub == '444' else W // 2
    y = rng.integers(64 << (bits - 10), 940 << (bits - 10), (nframes, H, W))
    if kind == 'noise':
        u, v = rng.integers(0, top + 1, (2, nframes, H, Wc))
    elif kind == 'smooth':
        yy, xx = np.mgrid[0:H, 0:Wc]
        base = (xx / max(Wc - 1, 1) * 0.6 + yy / max(H - 1, 1) * 0.3 + 0.05) * top
        u = base[None] + rng.normal(0, top / 256, (nframes, H, Wc))
        v = (top - base)[None] + rng.normal(0, top / 256, (nframes, H, Wc))
        u, v = np.clip(np.rint(u), 0, top), np.clip(np.rint(v), 0, top)
    else:
        bh, bw = 5, 7
        cells = rng.integers(0, 2, (2, nframes, (H + bh - 1) // bh, (Wc + bw - 1) // bw))
        u, v = (np.repeat(np.repeat(c, bh, axis=-2), bw, axis=-1)[..., :H, :Wc] * top for c in cells)
    return y.astype(np.uint16), np.asarray(u).astype(np.uint16), np.asarray(v).astype(np.uint16)
