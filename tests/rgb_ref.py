"""Expected values for the RGB tensor output (h2s_process_rgb,
Tonemapper.process_rgb): a numpy restatement of the model in include/h2s.h and
DESIGN.md §4.15, written from those formulas.

  codes    the chain's q-bit 4:2:0 codes y, u, v; s = 2^(q - 8); pixel (x, y)
           takes chroma sample (x >> 1, y >> 1)
  matrix   Y = 1.16438356 (y - 16 s), U = u - 128 s, V = v - 128 s
           cR = 1.79274107 V + Y, cG = -0.53290933 V + (-0.21324861 U + Y),
           cB = 2.11240179 U + Y          (the constants are float32 values)
  uint8    floor(c / s + 0.5) clamped to [0, 255]
  floats   v = min(max(c inv, 0), 1), inv = float32(1 / (255 s));
           out_k = scale[k] v + bias[k]; float16 / bfloat16 round that

``dtype=np.float64`` is the reference; ``dtype=np.float32`` evaluates the same
formulas in float32, every operation rounded on its own (no fused
multiply-adds): tests/test_rgb.py holds it to the gates below, so the gates are
reachable by the arithmetic alone.
"""
import numpy as np

F32 = np.float32
KY, KRV, KGV, KGU, KBU = (float(F32(v)) for v in (1.16438356, 1.79274107, -0.53290933, -0.21324861, 2.11240179))
BT709 = (KY, KRV, KGV, KGU, KBU)
BT601 = tuple(float(F32(v)) for v in (1.16438356, 1.59602678, -0.81296764, -0.39176229, 2.01723214))   # a mutant's
DTYPES = ('uint8', 'float16', 'bfloat16', 'float32')
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalisation(mean=None, std=None):
    """(scale, bias) as the float32 values the library receives, in float64."""
    mean = (0.0,) * 3 if mean is None else mean
    std = (1.0,) * 3 if std is None else std
    scale = [float(F32(1.0 / s)) for s in std]
    bias = [float(F32(-m / s)) for m, s in zip(mean, std)]
    return scale, bias


def prerounding(y, u, v, q, dtype=np.float64, coeffs=BT709, chroma_row='half', luma_offset=True):
    """[H, W] / [H/2, W/2] q-bit code planes -> (cR, cG, cB) [3, H, W] before
    the output rounding, at depth q.  coeffs, chroma_row='same' (chroma row
    min(y, H/2 - 1) instead of y >> 1) and luma_offset=False are the mutants
    tests/test_rgb.py must tell from the model."""
    y, u, v = (np.asarray(p).astype(np.int64) for p in (y, u, v))
    H, W = y.shape
    s = 2.0 ** (q - 8)
    rows = np.arange(H) >> 1 if chroma_row == 'half' else np.minimum(np.arange(H), H // 2 - 1)
    cols = np.arange(W) >> 1
    ky, krv, kgv, kgu, kbu = (dtype(k) for k in coeffs)
    Y = ky * (y.astype(dtype) - dtype(16.0 * s if luma_offset else 0.0))
    U = u[rows][:, cols].astype(dtype) - dtype(128.0 * s)
    V = v[rows][:, cols].astype(dtype) - dtype(128.0 * s)
    out = np.stack([krv * V + Y, kgv * V + (kgu * U + Y), kbu * U + Y])
    assert out.dtype == dtype
    return out


def to_bfloat16(x):
    """float32 values rounded to nearest-even to bfloat16, as float32."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def output(c, q, dtype_name, scale=(1.0,) * 3, bias=(0.0,) * 3, dtype=np.float64):
    """The pre-rounding planes [3, H, W] -> the tensor's values [3, H, W]:
    uint8 as int64; the float dtypes as float64 (dtype=np.float64: unrounded,
    the value a float16 / bfloat16 / float32 element should be nearest to;
    dtype=np.float32: rounded as the element is)."""
    s = 2.0 ** (q - 8)
    c = np.asarray(c, dtype=dtype)
    if dtype_name == 'uint8':
        return np.clip(np.floor(c * dtype(1.0 / s) + dtype(0.5)), 0, 255).astype(np.int64)
    inv = dtype(F32(1.0 / (255.0 * s)))
    v = np.minimum(np.maximum(c * inv, dtype(0.0)), dtype(1.0))
    sc = np.asarray(scale, dtype=dtype).reshape(3, 1, 1)
    bi = np.asarray(bias, dtype=dtype).reshape(3, 1, 1)
    o = sc * v + bi
    if dtype is np.float32:
        if dtype_name == 'float16':
            o = o.astype(np.float16)
        elif dtype_name == 'bfloat16':
            o = to_bfloat16(o)
    return o.astype(np.float64)


def expected(y, u, v, q, dtype_name, scale=(1.0,) * 3, bias=(0.0,) * 3, dtype=np.float64, **mutant):
    """One frame's q-bit code planes -> its expected tensor values [3, H, W] (CHW)."""
    return output(prerounding(y, u, v, q, dtype, **mutant), q, dtype_name, scale, bias, dtype)


# ---- the gates ---------------------------------------------------------------------------
U8_MAX_DIFF, U8_MAX_FRACTION = 1, 1e-3     # every byte within 1, at most 0.1 % of a case's bytes differing


def gate(got, want, dtype_name, scale=(1.0,) * 3, bias=(0.0,) * 3):
    """(passes, a line of figures) for [..., 3, H, W] values against the
    float64 expectation of the same shape."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.shape[-3] == 3, (got.shape, want.shape)
    if dtype_name == 'uint8':
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        mx, frac = int(d.max()), float((d > 0).mean())
        return mx <= U8_MAX_DIFF and frac <= U8_MAX_FRACTION, f'max diff {mx}, {frac:.4%} of the bytes differ'
    d = np.abs(got.astype(np.float64) - want)
    if dtype_name == 'float32':
        k = np.maximum(1.0, np.maximum(np.abs(np.asarray(scale, dtype=np.float64)),
                                       np.abs(np.asarray(bias, dtype=np.float64))))
        bound = np.broadcast_to(2e-6 * k.reshape(3, 1, 1), want.shape)
    elif dtype_name == 'float16':
        bound = 2.0 ** -11 * np.maximum(np.abs(want), 2.0 ** -14) + 2e-6
    else:
        bound = 2.0 ** -8 * np.abs(want) + 2e-6
    worst = float((d - bound).max())
    return bool((d <= bound).all()), f'max |diff| {d.max():.3e}, worst excess over the bound {worst:.3e}'


def planes_of(buf, width, height, shift=0):
    """A tight planar 4:2:0 batch [F, W * H * 3 / 2] -> (y, u, v) [F, rows, cols] int64 codes >> shift."""
    buf = np.asarray(buf).astype(np.int64) >> shift
    n, ysz, csz = buf.shape[0], width * height, width * height // 4
    return (buf[:, :ysz].reshape(n, height, width), buf[:, ysz:ysz + csz].reshape(n, height // 2, width // 2),
            buf[:, ysz + csz:].reshape(n, height // 2, width // 2))


def expected_batch(buf, width, height, q, shift, dtype_name, scale=(1.0,) * 3, bias=(0.0,) * 3):
    """[F, 3, H, W] for a tight planar batch of the chain's bits_out codes."""
    y, u, v = planes_of(buf, width, height, shift)
    return np.stack([expected(y[f], u[f], v[f], q, dtype_name, scale, bias) for f in range(y.shape[0])])
