"""Expected values for the preview's source pane (h2s_preview_source_rgb24,
Previewer.original): a numpy restatement of the model in include/h2s.h and
DESIGN.md §4.4, written from those formulas.

One swscale context from the decoded 10/12-bit Y'CbCr to packed RGB:

  codes    planar: the low bits; semi-planar: word >> (16 - b)
  resize   luma W x H -> ow x oh; each chroma plane cw x ch -> ow2 x oh with
           ow2 = (ow + 1) / 2; pixel (x, y) takes chroma (x >> 1, y).  Bicubic
           B = 0, C = 0.6, centre-aligned, widened by the ratio when
           downscaling, normalised, indices clamped at the edges
  range    limited: Y' = (Y - 16 s) / (219 s), C = (C - 2^(b-1)) / (224 s), s =
           2^(b-8); full: Y' = Y / (2^b - 1), C = (C - 2^(b-1)) / (2^b - 1)
  matrix   R' = Y' + 2 (1 - Kr) Cr, B' = Y' + 2 (1 - Kb) Cb,
           G' = Y' - (2 Kr (1 - Kr) / Kg) Cr - (2 Kb (1 - Kb) / Kg) Cb; clip [0, 1]
  output   trunc16: floor(65535 v + 0.5) >> 8; round8: floor(255 v + 0.5)

Everything is float64 unless ``dtype`` says float32 (tests/test_source_preview.py
holds the float32 evaluation to the GPU gate: the gate is reachable by this
arithmetic alone).
"""
import functools
import math

import numpy as np

KR_KB = {'bt2020nc': (0.2627, 0.0593), 'bt709': (0.2126, 0.0722), 'bt601': (0.299, 0.114)}
MATRICES = tuple(KR_KB)
RGB_MODELS = ('trunc16', 'round8')
_SHIFTS = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}


def bicubic(x, B=0.0, C=0.6):
    x = np.abs(np.asarray(x, dtype=np.float64))
    near = ((12 - 9 * B - 6 * C) * x ** 3 + (-18 + 12 * B + 6 * C) * x ** 2 + (6 - 2 * B)) / 6
    far = ((-B - 6 * C) * x ** 3 + (6 * B + 30 * C) * x ** 2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) / 6
    return np.where(x < 1, near, np.where(x < 2, far, 0.0))


def resize_matrix(src, dst):
    """[dst, src] float64: row o holds output sample o's normalised taps, the
    taps that fall outside the plane added onto its edge sample."""
    scale = src / dst
    fw = max(scale, 1.0)
    T = math.ceil(4 * fw) + 1
    M = np.zeros((dst, src))
    for o in range(dst):
        c = (o + 0.5) * scale - 0.5
        idx = math.floor(c - 2 * fw) + 1 + np.arange(T)
        w = bicubic((idx - c) / fw)
        np.add.at(M[o], np.clip(idx, 0, src - 1), w / w.sum())
    return M


def resize(plane, out_w, out_h, dtype=np.float64):
    """[h, w] -> [out_h, out_w]."""
    h, w = plane.shape
    My, Mx = resize_matrix(h, out_h).astype(dtype), resize_matrix(w, out_w).astype(dtype)
    return My @ (plane.astype(dtype) @ Mx.T)


def matrix_coeffs(matrix):
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    return 2 * (1 - kr), -2 * kb * (1 - kb) / kg, -2 * kr * (1 - kr) / kg, 2 * (1 - kb)   # rcr, gcb, gcr, bcb


def rgb_float(y, u, v, bits, out_w, out_h, matrix='bt2020nc', full=False, dtype=np.float64):
    """One frame's code planes -> [out_h, out_w, 3] R'G'B' in [0, 1]."""
    ow2 = (out_w + 1) // 2
    Y = resize(y, out_w, out_h, dtype)
    Cb, Cr = (resize(c, ow2, out_h, dtype)[:, np.arange(out_w) >> 1] for c in (u, v))
    s, top, mid = 1 << (bits - 8), (1 << bits) - 1, 1 << (bits - 1)
    one = dtype(1)
    if full:
        Y, Cb, Cr = Y / dtype(top), (Cb - dtype(mid)) / dtype(top), (Cr - dtype(mid)) / dtype(top)
    else:
        Y, Cb, Cr = (Y - dtype(16 * s)) / dtype(219 * s), (Cb - dtype(mid)) / dtype(224 * s), \
            (Cr - dtype(mid)) / dtype(224 * s)
    rcr, gcb, gcr, bcb = (dtype(c) for c in matrix_coeffs(matrix))
    rgb = np.stack([Y + rcr * Cr, Y + gcr * Cr + gcb * Cb, Y + bcb * Cb], axis=-1)
    return np.clip(rgb, dtype(0), one)


def quantise16(v):
    """The rgb48 code of v in [0, 1]."""
    return np.floor(v.dtype.type(65535) * v + v.dtype.type(0.5)).astype(np.int64)


def quantise(v, rgb='trunc16'):
    if rgb == 'trunc16':
        return (quantise16(v) >> 8).astype(np.uint8)
    if rgb == 'round8':
        return np.floor(v.dtype.type(255) * v + v.dtype.type(0.5)).astype(np.uint8)
    raise ValueError(rgb)


def codes(fb):
    """A host FrameBatch's (y, u, v) code planes [F, rows, cols] as int64."""
    fb = fb.to_numpy()
    sh = 16 - fb.bits if fb.layout == 'semi' else 0
    mask = (1 << fb.bits) - 1
    return tuple((np.asarray(p).astype(np.int64) >> sh) & mask for p in (fb.y, fb.u, fb.v))


def expected(fb, out_w, out_h, matrix='bt2020nc', rgb='trunc16', dtype=np.float64):
    """[F, out_h, out_w, 3] uint8: the source pane of every frame of fb (its
    layout, subsampling and range tag honoured; the chroma location has no
    effect in this model)."""
    y, u, v = codes(fb)
    cxs, cys = _SHIFTS[fb.subsampling]
    assert u.shape[1:] == (fb.height >> cys, fb.width >> cxs)
    return np.stack([quantise(rgb_float(y[f], u[f], v[f], fb.bits, out_w, out_h, matrix, fb.color_range == 'pc',
                                        dtype), rgb) for f in range(y.shape[0])])


def expected16(fb, out_w, out_h, matrix='bt2020nc'):
    """[F, out_h, out_w, 3] int64: the rgb48 codes before the high-byte read."""
    y, u, v = codes(fb)
    return np.stack([quantise16(rgb_float(y[f], u[f], v[f], fb.bits, out_w, out_h, matrix, fb.color_range == 'pc'))
                     for f in range(y.shape[0])])


def gate(got, want):
    """The project's integer rule: (max |diff|, fraction of bytes that differ)."""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), float((d > 0).mean())


def flat_frame(width, height, bits, y, cb, cr, nframes=1, subsampling='420', color_range='tv'):
    """A host batch of one code per plane."""
    import hdr2sdr
    fb = hdr2sdr.FrameBatch.empty_numpy(nframes, width, height, bits, 'planar', subsampling, color_range)
    fb.y[...] = y
    fb.u[...] = cb
    fb.v[...] = cr
    return fb


@functools.lru_cache(maxsize=None)
def flat_codes(bits, color_range):
    """The first (y, cb, cr) of a fixed list whose rgb48 result lies at least 8
    codes from a multiple of 256 in every channel under every matrix (chosen
    on the restatement alone): where a flat frame's high byte leaves float32
    room, so the kernel is held to it exactly."""
    s = 1 << (bits - 8)
    for k in range(40):    # (all of them legal limited-range codes)
        yuv = ((75 + 3 * k) * s + k % s, (100 + k) * s, (150 - k) * s + k % s)
        rgb48 = [expected16(flat_frame(16, 8, bits, *yuv, color_range=color_range), 16, 8, m)[0, 0, 0]
                 for m in MATRICES]
        if all(8 <= c % 256 <= 247 for v in rgb48 for c in v):
            return yuv
    raise AssertionError('no flat codes with the margin')


def synth_source(kind, nframes, width, height, bits=10, subsampling='420', color_range='tv', seed=0x50A):
    """A host batch of hdr2sdr.synth content: 4:2:0 as synth_frames makes it;
    4:2:2 / 4:4:4 with that luma and, as chroma planes of their own size, the
    chroma planes of a synth frame twice that size."""
    import hdr2sdr
    from hdr2sdr.synth import synth_frames
    base = synth_frames(kind, nframes, width, height, bits, seed=seed).to_numpy()
    if subsampling == '420':
        return hdr2sdr.FrameBatch(base.buf, width, height, bits, 'planar', '420', color_range)
    cxs, cys = _SHIFTS[subsampling]
    big = synth_frames(kind, nframes, 2 * (width >> cxs), 2 * (height >> cys), bits, seed=seed + 1).to_numpy()
    return hdr2sdr.FrameBatch.from_planes(np.asarray(base.y), np.asarray(big.u), np.asarray(big.v), bits, subsampling,
                                          color_range)


# ---- the GPU cases (tests/test_gpu_source_preview.py; the CPU suite holds the
# float32 restatement to the same gate on them).  The smallest shapes at which
# the kernel takes another path: (id, W, H, ('size', ow, oh) | ('box', bw, bh),
# bits, subsampling, color_range)
CASES = (
    ('identity', 64, 32, ('size', 64, 32), 10, '420', 'tv'),       # identity luma; chroma's 2x vertical pass runs
    ('ragged', 66, 34, ('size', 66, 34), 10, '420', 'tv'),         # 33 chroma columns
    ('box48x27', 128, 72, ('box', 48, 27), 10, '420', 'tv'),       # a non-integer downscale
    ('odd47x26', 128, 72, ('size', 47, 26), 10, '420', 'tv'),      # odd out_w: the last pair is half
    ('upscale', 32, 18, ('size', 80, 45), 10, '420', 'tv'),
    ('portrait', 36, 64, ('box', 64, 36), 10, '420', 'tv'),        # sized through h2s_preview_size
    ('ratio12', 384, 16, ('size', 32, 16), 10, '420', 'tv'),       # the widest taps
    ('422', 64, 32, ('size', 40, 20), 10, '422', 'tv'),
    ('444', 64, 32, ('size', 40, 20), 10, '444', 'tv'),
    ('12bit', 64, 32, ('size', 40, 20), 12, '420', 'tv'),
    ('full', 64, 32, ('size', 40, 20), 10, '420', 'pc'),           # codes outside the limited range ('edges')
    ('full12', 66, 34, ('size', 66, 34), 12, '420', 'pc'),
)
CONTENTS = ('smooth', 'edges')
MAX_DIFF, MAX_FRACTION = 1, 5e-3   # every byte within 1, at most 0.5 % of a case's bytes differ at all


def case_size(case):
    """(out_w, out_h) of a case: given, or the aspect fit of its box."""
    _, W, H, (how, a, b) = case[:4]
    if how == 'size':
        return a, b
    import hdr2sdr
    return hdr2sdr.fit_size(W, H, a, b)


def case_frames(case, kind, nframes=1):
    _, W, H, _, bits, sub, rng = case
    return synth_source(kind, nframes, W, H, bits, sub, rng)
