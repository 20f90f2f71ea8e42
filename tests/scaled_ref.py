"""Expected values for the scaled 4:2:0 output (h2s_process_scaled,
Tonemapper.process_scaled): a numpy restatement of the model in include/h2s.h
and DESIGN.md §4.13, written from those formulas.

The resize is a trailing ``scale=`` stage on the chain's quantised 4:2:0 output:

  codes    the chain's q-bit codes: what h2s_process writes, >> (bits_out - q)
  planes   luma W x H -> ow x oh, each chroma plane W/2 x H/2 -> ow/2 x oh/2
  taps     bicubic B = 0, C = 0.6, centre-aligned, the support widened by the
           ratio when downscaling, normalised, float32 weights, source indices
           clamped at the edges; no chroma-siting correction
  passes   horizontal, then vertical, each an ascending chain from 0
  output   v = floor(acc + 0.5) clamped to [0, 2^q - 1], then S8 to bits_out
           (shift: v << s; replicate: (v << s) | (v >> (8 - s)), s = bits_out - q)

``dtype=np.float64`` is the reference; ``dtype=np.float32`` evaluates the same
chains in float32 with fused multiply-adds, as a kernel does
(tests/test_scaled.py holds it to the GPU gate: the gate is reachable by this
arithmetic alone).
"""
import functools
import math

import numpy as np

MAX_DIFF, MAX_FRACTION = 1, 5e-3   # every sample within 1 code at depth q, at most 0.5 % of a plane differing


def bicubic(x, B=0.0, C=0.6):
    x = np.abs(np.asarray(x, dtype=np.float64))
    near = ((12 - 9 * B - 6 * C) * x ** 3 + (-18 + 12 * B + 6 * C) * x ** 2 + (6 - 2 * B)) / 6
    far = ((-B - 6 * C) * x ** 3 + (6 * B + 30 * C) * x ** 2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) / 6
    return np.where(x < 1, near, np.where(x < 2, far, 0.0))


@functools.lru_cache(maxsize=None)
def taps(src, dst, centre=True, widen=True):
    """(idx [dst, T] clamped source indices, w [dst, T] normalised weights as
    float32 values held in float64).  centre=False samples left-aligned and
    widen=False keeps the 4-tap support when downscaling: the two mutants
    tests/test_scaled.py must tell from the model."""
    scale = src / dst
    fw = max(scale, 1.0) if widen else 1.0
    T = math.ceil(4 * fw) + 1
    idx = np.zeros((dst, T), dtype=np.int64)
    w = np.zeros((dst, T))
    for o in range(dst):
        c = (o + 0.5) * scale - 0.5 if centre else o * scale
        i = math.floor(c - 2 * fw) + 1 + np.arange(T)
        k = bicubic((i - c) / fw)
        idx[o], w[o] = np.clip(i, 0, src - 1), k / k.sum()
    return idx, w.astype(np.float32).astype(np.float64)


def _fma(a, b, c, dtype):
    """a * b + c rounded once to dtype (a float32 product is exact in float64)."""
    return (a * b + c).astype(dtype).astype(np.float64)


def _pass(plane, idx, w, dtype):
    """[rows, src] -> [rows, dst]: out[:, o] = sum_i w[o, i] * plane[:, idx[o, i]], ascending from 0."""
    acc = np.zeros((plane.shape[0], idx.shape[0]))
    for i in range(idx.shape[1]):
        acc = _fma(plane[:, idx[:, i]], w[None, :, i], acc, dtype)
    return acc


def resize_plane(plane, ow, oh, qmax, dtype=np.float64, **how):
    """[h, w] codes -> [oh, ow] codes."""
    h, w = plane.shape
    hor = _pass(plane.astype(np.float64), *taps(w, ow, **how), dtype)
    ver = _pass(hor.T, *taps(h, oh, **how), dtype).T
    return np.clip(np.floor((ver + 0.5).astype(dtype).astype(np.float64)), 0, qmax).astype(np.int64)


def scaled(y, u, v, ow, oh, q, dtype=np.float64, **how):
    """One frame's q-bit code planes -> the scaled frame's q-bit code planes."""
    qmax = (1 << q) - 1
    return (resize_plane(y, ow, oh, qmax, dtype, **how), resize_plane(u, ow // 2, oh // 2, qmax, dtype, **how),
            resize_plane(v, ow // 2, oh // 2, qmax, dtype, **how))


def expand(code, q, bits_out, how='shift'):
    """S8: a q-bit code at bits_out."""
    s = bits_out - q
    if s == 0:
        return code
    return (code << s) | (code >> (8 - s)) if how == 'replicate' else code << s


def planes_of(buf, width, height):
    """A tight planar 4:2:0 batch [F, W * H * 3 / 2] -> (y, u, v) [F, rows, cols] int64."""
    buf = np.asarray(buf).astype(np.int64)
    n, ysz, csz = buf.shape[0], width * height, width * height // 4
    return (buf[:, :ysz].reshape(n, height, width), buf[:, ysz:ysz + csz].reshape(n, height // 2, width // 2),
            buf[:, ysz + csz:].reshape(n, height // 2, width // 2))


def expected(buf, width, height, ow, oh, q, bits_out, how='shift', dtype=np.float64):
    """The scaled batch [F, ow * oh * 3 / 2] (int64, bits_out codes) of a tight
    planar batch of the chain's bits_out output."""
    y, u, v = (p >> (bits_out - q) for p in planes_of(buf, width, height))
    out = []
    for f in range(y.shape[0]):
        out.append(np.concatenate([expand(p, q, bits_out, how).reshape(-1)
                                   for p in scaled(y[f], u[f], v[f], ow, oh, q, dtype)]))
    return np.stack(out)


def gate(got, want, shift=0):
    """The project's integer rule at depth q over one plane or
    batch: (max |diff| in q-bit codes, fraction of samples that differ)."""
    d = np.abs((np.asarray(got).astype(np.int64) >> shift) - (np.asarray(want).astype(np.int64) >> shift))
    return int(d.max()), float((d > 0).mean())


def gate_planes(got, want, ow, oh, shift=0):
    """gate() per plane of two tight planar batches: the worst (max, fraction)."""
    worst = (0, 0.0)
    for g, w in zip(planes_of(got, ow, oh), planes_of(want, ow, oh)):
        mx, frac = gate(g, w, shift)
        worst = (max(worst[0], mx), max(worst[1], frac))
    return worst


# ---- the cases (tests/test_gpu_scaled.py; the CPU suite holds the float32
# evaluation to the same gate on them).  The smallest shapes at which the
# kernel takes another path: (id, W, H, ow, oh)
CASES = (
    ('2to1', 192, 96, 96, 48),          # the 4K -> 1080p ratio; a whole and a ragged strip of luma
    ('nonint', 192, 128, 128, 86),      # 1.5 : 1 across, 1.488 : 1 down; chroma 64 x 43
    ('ratio12', 384, 192, 32, 16),      # the ratio limit: 49 taps on both axes, the LDS worst case
    ('upscale', 64, 64, 128, 128),
    ('ragged', 136, 72, 70, 38),        # source width off the tile path, output width off the 64-column strip
    ('portrait', 96, 192, 50, 100),
    ('tall', 96, 320, 64, 160),         # more output rows than one block owns: several runs of rows
)
# (Not among them: an axis at ratio 1 beside one at 2 : 1, such as 64 x 320 -> 64 x 160.  The identity
# pass leaves integers, a symmetric normalised kernel centred between two rows then lands on k + 0.5
# wherever neighbouring rows differ by an odd count, and on smooth content the float32 evaluation
# alone differs from the float64 one on 8 % of a plane: such a case measures rounding ties, not a kernel)
CONTENTS = ('uniform', 'smooth')
BY_ID = {c[0]: c for c in CASES}
