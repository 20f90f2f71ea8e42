"""The RGB tensor output on the GPU (h2s_process_rgb, Tonemapper.process_rgb)
against the float64 restatement in tests/rgb_ref.py.

Every case takes its source codes from the same context's own h2s_process
(equal size; into a surface whose rows lie 16 bytes apart, as the library's
scratch rows do, so that both conversions take one route) or h2s_process_scaled
(resized) output, >> shift_out: only the new stage is judged.  Gates
(rgb_ref.gate): uint8 every byte within 1 and at most 0.1 % of a case's bytes
differing; float32 |d| <= 2e-6 max(1, |scale_k|, |bias_k|); float16
|d| <= 2^-11 max(|want|, 2^-14) + 2e-6; bfloat16 |d| <= 2^-8 |want| + 2e-6.  The
float32 restatement meets them on the CPU (tests/test_rgb.py).  Twins, pitches,
chunking, the preview at equal size and neutral pixels are exact."""
import ctypes
import functools

import numpy as np
import pytest

import hdr2sdr
import oracle
import rgb_ref as ref
import source_preview_ref as spref
from hdr2sdr import _abi
from hdr2sdr.synth import synth_frames
from padded_frames import RowPadded

pytestmark = pytest.mark.gpu

C2 = dict(tonemapper='hable', gamma=2.2, bits_in=10, bits_out=10)    # compat8: q = 8
LP = dict(tonemapper='bt.2390', maxcll=4000.0)                        # the libplacebo branch at gamma 1: q = 10
CONFIGS = {
    'compat8-8': dict(C2, bits_out=8),
    'compat8-10-shift': C2,
    'compat8-10-replicate': dict(C2, expand='replicate'),
    'native-10': dict(C2, mode='native'),
    'native-12-hlg': dict(C2, bits_in=12, bits_out=12, mode='native', transfer='arib-std-b67'),
    'libplacebo': LP,
    'libplacebo-peak': dict(LP, peak_detect=True),
}
QUANT = {'compat8-8': 8, 'compat8-10-shift': 8, 'compat8-10-replicate': 8, 'native-10': 10, 'native-12-hlg': 12,
         'libplacebo': 10, 'libplacebo-peak': 10}
CONTENTS = ('smooth', 'edges', 'uniform')
SIZES = ((64, 32), (128, 64), (70, 34), (2, 2))            # one tile; several; generic kernel, ragged runs; the smallest
RESIZES = ((128, 64, 64, 32), (128, 64, 86, 48), (64, 32, 96, 48), (2, 2, 2, 2))
LAYOUTS = ('chw', 'hwc')


@functools.lru_cache(maxsize=None)
def _lattice():
    return hdr2sdr.generate_lattice(33)


_contexts = {}


def context(**kw):
    """One context per parameter set for the module."""
    key = tuple(sorted(kw.items()))
    if key not in _contexts:
        _contexts[key] = hdr2sdr.Tonemapper(0, hdr2sdr.TonemapParams(**kw), _lattice())
    return _contexts[key]


@pytest.fixture(scope='module', autouse=True)
def _close_contexts():
    yield
    for t in _contexts.values():
        t.close()
    _contexts.clear()


def quant_bits(tm):
    return oracle.quant_bits(oracle.params_from(tm.params.to_c()))


@functools.lru_cache(maxsize=None)
def _source(kind, nframes, W, H, bits=10):
    return synth_frames(kind, nframes, W, H, bits, seed=0x26B).to_numpy()


def chain_codes(tm, src, ow, oh):
    """The context's own 4:2:0 output of a batch at ow x oh (h2s_process at the
    source's size, else h2s_process_scaled): a tight host buffer of bits_out codes."""
    import torch
    if tm.params.peak_detect:
        tm.reset_peak()
    if (ow, oh) == (src.width, src.height):
        dst = RowPadded(src.nframes, ow, oh, tm.params.bits_out, align=16)
        tm.process(src, dst)
    else:
        dst = hdr2sdr.FrameBatch.empty_torch(src.nframes, ow, oh, tm.params.bits_out, 'cuda:0')
        tm.process_scaled(src, dst)
    torch.cuda.synchronize()
    return dst.to_numpy().buf


def as_chw(t, layout):
    """A result tensor on the host as [F, 3, H, W]: int64 (uint8) or float64."""
    t = t if layout == 'chw' else t.permute(0, 3, 1, 2)
    import torch
    if t.dtype == torch.uint8:
        return t.cpu().numpy().astype(np.int64)
    return t.float().cpu().numpy().astype(np.float64)


def rgb(tm, src, ow, oh, dtype, layout='chw', mean=None, std=None, **kw):
    """process_rgb into a fresh tensor; the tensor (synchronised)."""
    import torch
    if tm.params.peak_detect:
        tm.reset_peak()
    out = tm.process_rgb(src, size=(ow, oh), dtype=dtype, layout=layout, mean=mean, std=std, **kw)
    torch.cuda.synchronize()
    assert tuple(out.shape) == ((src.nframes, 3, oh, ow) if layout == 'chw' else (src.nframes, oh, ow, 3))
    return out


def check(tm, src, ow, oh, dtype, layout, what, mean=None, std=None):
    q, bo = quant_bits(tm), tm.params.bits_out
    scale, bias = ref.normalisation(mean, std)
    want = ref.expected_batch(chain_codes(tm, src, ow, oh), ow, oh, q, bo - q, dtype, scale, bias)
    got = as_chw(rgb(tm, src, ow, oh, dtype, layout, mean, std), layout)
    ok, figures = ref.gate(got, want, dtype, scale, bias)
    print(f'{what} {dtype} {layout} q = {q}: {figures}')
    assert ok, (what, dtype, layout, figures)


def bits_of(t):
    """The tensor's elements as integers (bit for bit)."""
    import torch
    view = {torch.uint8: torch.uint8, torch.float16: torch.int16, torch.bfloat16: torch.int16,
            torch.float32: torch.int32}[t.dtype]
    return t.contiguous().view(view).cpu().numpy()


# ---- 1. the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('size', [(64, 32), (70, 34)], ids=['64x32', '70x34'])
def test_every_dtype_and_layout(size, dtype, layout):
    tm = context(**C2)
    src = _source('smooth', 2, *size).to_torch('cuda:0')
    check(tm, src, *size, dtype, layout, f'{size}')


@pytest.mark.parametrize('kind', CONTENTS)
@pytest.mark.parametrize('dtype', ['uint8', 'float16'])
@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_every_configuration(config, dtype, kind):
    tm = context(**CONFIGS[config])
    assert quant_bits(tm) == QUANT[config]
    src = _source(kind, 2, 70, 34, tm.params.bits_in).to_torch('cuda:0')
    check(tm, src, 70, 34, dtype, 'chw', f'{config} {kind}')


@pytest.mark.parametrize('dtype,layout', [('uint8', 'chw'), ('float32', 'hwc')])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_sizes(size, dtype, layout):
    tm = context(**CONFIGS['native-10'])
    src = _source('edges', 3, *size).to_torch('cuda:0')
    check(tm, src, *size, dtype, layout, f'{size}')


@pytest.mark.parametrize('dtype,layout', [('uint8', 'hwc'), ('float16', 'chw'), ('float32', 'chw')])
@pytest.mark.parametrize('config', ['compat8-10-replicate', 'native-10', 'libplacebo-peak'])
@pytest.mark.parametrize('case', RESIZES, ids=lambda c: f'{c[0]}x{c[1]}-{c[2]}x{c[3]}')
def test_resize_targets(case, config, dtype, layout):
    W, H, ow, oh = case
    tm = context(**CONFIGS[config])
    src = _source('smooth', 2, W, H).to_torch('cuda:0')
    check(tm, src, ow, oh, dtype, layout, f'{config} {W}x{H} -> {ow}x{oh}')


# ---- 2. normalisation ------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float32', 'float16', 'bfloat16'])
@pytest.mark.parametrize('norm', ['imagenet', 'negative'])
def test_normalisation(norm, dtype):
    mean, std = ((ref.IMAGENET_MEAN, ref.IMAGENET_STD) if norm == 'imagenet' else
                 ((0.1, 0.2, 0.3), (-0.5, 0.25, 2.0)))
    tm = context(**CONFIGS['native-10'])
    src = _source('smooth', 2, 70, 34).to_torch('cuda:0')
    check(tm, src, 70, 34, dtype, 'chw', norm, mean, std)
    check(tm, src, 86, 48, dtype, 'hwc', norm, mean, std)


# ---- 3. the two layouts ------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('size', [(64, 32), (70, 34)], ids=['64x32', '70x34'])
def test_hwc_is_chw_permuted(size, dtype):
    tm = context(**CONFIGS['native-10'])
    src = _source('edges', 2, *size).to_torch('cuda:0')
    norm = {} if dtype == 'uint8' else dict(mean=ref.IMAGENET_MEAN, std=ref.IMAGENET_STD)
    chw = rgb(tm, src, *size, dtype, 'chw', **norm)
    hwc = rgb(tm, src, *size, dtype, 'hwc', **norm)
    assert np.array_equal(bits_of(hwc.permute(0, 3, 1, 2)), bits_of(chw))


# ---- 4. the preview yardstick ------------------------------------------------------------------
def preview(tm, src, ow, oh):
    import torch
    out = torch.empty((src.nframes, oh, ow, 3), dtype=torch.uint8, device='cuda:0')
    tm._use_layouts(src)
    d = src.descriptor()
    tm._check(_abi.lib().h2s_preview_rgb24_batch(tm._ctx, ctypes.byref(d), src.nframes, out.data_ptr(), 3 * ow,
                                                 3 * ow * oh, ow, oh, 1.0, _abi.LOC_DEVICE, tm._stream_ptr(None)))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize('kind', CONTENTS)
def test_uint8_hwc_is_the_preview_at_display_gamma_1(kind):
    """k_yuv8_rgb24's arithmetic is the specification at q = 8: byte for byte
    at equal size.  Resized, the preview's planes come from k_resize_u8 and
    this call's from k_scale420: within 1 on at most 0.5 % of the bytes."""
    tm = context(**CONFIGS['compat8-8'])
    src = _source(kind, 2, 64, 32).to_torch('cuda:0')
    assert np.array_equal(rgb(tm, src, 64, 32, 'uint8', 'hwc').cpu().numpy(), preview(tm, src, 64, 32))
    big = _source(kind, 2, 128, 64).to_torch('cuda:0')
    got, want = rgb(tm, big, 86, 48, 'uint8', 'hwc').cpu().numpy().astype(np.int64), preview(tm, big, 86, 48)
    d = np.abs(got - want)
    per_channel = [float((d[..., k] > 0).mean()) for k in range(3)]
    print(f'{kind} 128x64 -> 86x48 against the preview: max diff {d.max()}, {(d > 0).mean():.4%} of the bytes differ '
          f'(R, G, B: {per_channel})')
    assert d.max() <= 1 and (d > 0).mean() <= 5e-3


# ---- 5. pitches --------------------------------------------------------------------------------
def strided(nframes, shape, strides, offset, dtype):
    """A tensor of `shape` (without the frame dimension) over a fresh buffer,
    element strides as given, the first element `offset` elements in."""
    import torch
    extent = offset + sum((n - 1) * s for n, s in zip((nframes,) + shape, strides)) + 1
    base = torch.zeros(extent + 16, dtype=dtype, device='cuda:0')
    return torch.as_strided(base, (nframes,) + shape, strides, offset)


@pytest.mark.parametrize('dtype', ['uint8', 'float16'])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_rows_off_the_16_byte_boundary_equal_the_aligned_run(layout, dtype):
    """uint8: rows at odd byte offsets; float16: at 2-byte, not 16-byte ones.
    Both take the element stores."""
    import torch
    W, H = 70, 34
    tm = context(**CONFIGS['native-10'])
    src = _source('edges', 2, W, H).to_torch('cuda:0')
    aligned = rgb(tm, src, W, H, dtype, layout)
    tdt = getattr(torch, dtype)
    if layout == 'chw':
        row = W + 1
        out = strided(2, (3, H, W), (3 * H * row + 1, H * row, row, 1), 1, tdt)
    else:
        row = 3 * W + 1
        out = strided(2, (H, W, 3), (H * row + 1, row, 3, 1), 1, tdt)
    assert out.data_ptr() % 16 and (row * out.element_size()) % 16
    assert tm.process_rgb(src, out=out, dtype=dtype, layout=layout) is out
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(out), bits_of(aligned))


@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_padded_plane_and_frame_pitches_equal_the_tight_run(dtype):
    """CHW, every row start still on a 16-byte boundary: the 16-byte stores."""
    import torch
    W, H = 64, 32
    tm = context(**CONFIGS['native-10'])
    src = _source('smooth', 3, W, H).to_torch('cuda:0')
    tight = rgb(tm, src, W, H, dtype, 'chw')
    plane = H * W + 32
    out = strided(3, (3, H, W), (3 * plane + 64, plane, W, 1), 0, getattr(torch, dtype))
    base = out.storage_offset()
    assert base == 0
    tm.process_rgb(src, out=out, dtype=dtype)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(out), bits_of(tight))
    # a sliced view of a larger tensor, in place; nothing around it is written
    big = torch.full((3, 3, H + 8, W + 32), 7, dtype=getattr(torch, dtype), device='cuda:0')
    tm.process_rgb(src, out=big[:, :, 4:4 + H, 16:16 + W], dtype=dtype)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(big[:, :, 4:4 + H, 16:16 + W]), bits_of(tight))
    frame = torch.ones_like(big, dtype=torch.bool)
    frame[:, :, 4:4 + H, 16:16 + W] = False
    assert bool((big[frame] == 7).all())


# ---- 6. chunking -------------------------------------------------------------------------------
@pytest.mark.parametrize('config', ['compat8-10-shift', 'libplacebo-peak'])
@pytest.mark.parametrize('target', [(64, 32), (42, 20)], ids=['equal', 'resized'])
def test_a_batch_longer_than_the_scratch_equals_frame_by_frame(target, config):
    """18 frames: one chunk of 16 and one of 2."""
    import torch
    tm = context(**CONFIGS[config])
    src = _source('smooth', 18, 64, 32).to_torch('cuda:0')
    whole = bits_of(rgb(tm, src, *target, 'float16', 'chw'))
    state = tm.peak_state()
    tm.reset_peak()
    single = []
    for f in range(18):                       # (one sequence: the state is not reset in between)
        single.append(tm.process_rgb(src.slice(f, f + 1), size=target, dtype='float16'))
    torch.cuda.synchronize()
    assert np.array_equal(whole, np.concatenate([bits_of(t) for t in single]))
    assert tm.peak_state() == state
    if tm.params.peak_detect:
        assert state['frames'] == 18


# ---- 7. input forms ----------------------------------------------------------------------------
def test_semi_planar_and_422_input():
    tm = context(**C2)
    host = _source('smooth', 2, 70, 34)
    semi = host.to_layout('semi').to_torch('cuda:0')
    check(tm, semi, 70, 34, 'uint8', 'hwc', 'p010 input')
    s422 = spref.synth_source('smooth', 2, 128, 64, 10, '422').to_torch('cuda:0')
    check(tm, s422, 128, 64, 'float32', 'chw', '4:2:2 input')
    check(tm, s422, 86, 48, 'uint8', 'chw', '4:2:2 input, resized')


@pytest.mark.parametrize('target', [(64, 32), (96, 48)], ids=['equal', 'resized'])
def test_host_resident_source_equals_the_device_call(target):
    """The call returns once the frames are staged; the kernel is still queued
    on the stream, and a torch op on that stream sees its result."""
    import torch
    tm = context(**C2)
    host = _source('edges', 3, 64, 32)
    out = tm.process_rgb(host, size=target, dtype='bfloat16', layout='hwc')
    assert out.is_cuda and tuple(out.shape) == (3, target[1], target[0], 3)
    got = bits_of(out)                                           # (.cpu() on the current stream)
    assert np.array_equal(got, bits_of(rgb(tm, host.to_torch('cuda:0'), *target, 'bfloat16', 'hwc')))
    check(tm, host.to_torch('cuda:0'), *target, 'bfloat16', 'hwc', 'device twin of the host source')


# ---- 8. neutral pixels -------------------------------------------------------------------------
@pytest.mark.parametrize('config', ['compat8-8', 'native-10', 'native-12-hlg'])
def test_neutral_chroma_gives_equal_channels(config):
    tm = context(**CONFIGS[config])
    q, bo, bi = quant_bits(tm), tm.params.bits_out, tm.params.bits_in
    W, H = 70, 34
    grey = spref.flat_frame(W, H, bi, 600 << (bi - 10), 512 << (bi - 10), 512 << (bi - 10))
    for host in (grey, _source('smooth', 1, W, H, bi)):
        src = host.to_torch('cuda:0')
        y, u, v = ref.planes_of(chain_codes(tm, src, W, H), W, H, bo - q)
        mid = 128 << (q - 8)
        neutral = ((u == mid) & (v == mid))[0].repeat(2, axis=0).repeat(2, axis=1)
        if host is grey:
            assert neutral.all()
        for dtype in ('uint8', 'float32'):
            got = bits_of(rgb(tm, src, W, H, dtype, 'chw'))[0]
            assert np.array_equal(got[0][neutral], got[1][neutral]), (config, dtype)
            assert np.array_equal(got[0][neutral], got[2][neutral]), (config, dtype)


# ---- 9. stream order ---------------------------------------------------------------------------
def test_a_torch_op_on_the_calls_stream_sees_the_finished_tensor():
    import torch
    tm = context(**C2)
    W, H = 1280, 720                              # (long enough for a missing order to show)
    src = _source('smooth', 4, W, H).to_torch('cuda:0')
    want = rgb(tm, src, 640, 360, 'float32', 'chw').double().sum(dim=(1, 2, 3)).cpu()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = torch.zeros((4, 3, 360, 640), dtype=torch.float32, device='cuda:0')
        tm.process_rgb(src, out=out, dtype='float32')        # the default: torch's current stream, `side`
        total = out.double().sum(dim=(1, 2, 3))
    side.synchronize()
    assert torch.equal(total.cpu(), want)
    # and an explicit stream argument
    out2 = torch.zeros_like(out)
    side.wait_stream(torch.cuda.current_stream())
    tm.process_rgb(src, out=out2, dtype='float32', stream=side)
    with torch.cuda.stream(side):
        total2 = out2.double().sum(dim=(1, 2, 3))
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(total2.cpu(), want)


# ---- 10. timing and the tap cache --------------------------------------------------------------
def timing_records(tm):
    """Entries of the timing record: kernel_ms(k) averages the last k and
    clamps k to what there is, so the average stops changing there."""
    avg = [tm.kernel_ms(k) for k in range(1, 12)]
    return next(k for k in range(1, 10) if avg[k - 1] == avg[k] == avg[k + 1])


def test_timing_records_and_tap_uploads():
    import torch
    tm = hdr2sdr.Tonemapper(0, hdr2sdr.TonemapParams(**C2), _lattice())
    try:
        def uploads():
            return next(n for n in range(16)
                        if _abi.lib().h2s_set_option(tm._ctx, _abi.OPT_TEST_SCALE_UPLOADS, n) == 0)

        W, H = 640, 360
        one = _source('smooth', 1, W, H).to_torch('cuda:0')
        many = hdr2sdr.FrameBatch(one.buf.repeat(18, 1), W, H, 10)
        tm.set_timing(True)
        for src, target, want in ((one, (W, H), 2), (one, (320, 180), 3), (many, (W, H), 4), (many, (320, 180), 6)):
            tm.kernel_ms(0)
            tm.process_rgb(src, size=target, dtype='float16')
            torch.cuda.synchronize()
            assert timing_records(tm) == want, (src.nframes, target)
            assert tm.kernel_ms(1) > 0.0
        tm.set_timing(False)
        assert uploads() == 1                                   # 320 x 180, once for both calls
        a = bits_of(tm.process_rgb(one, size=(320, 180), dtype='float16'))
        assert uploads() == 1
        tm.process_rgb(one, size=(426, 240), dtype='float16')
        assert uploads() == 2
        tm.process_rgb(one, size=(W, H), dtype='float16')      # the equal size never touches them
        assert uploads() == 2
        dst = hdr2sdr.FrameBatch.empty_torch(1, 426, 240, 10, 'cuda:0')
        tm.process_scaled(one, dst)                              # the scaled output shares the cache
        assert uploads() == 2
        b = bits_of(tm.process_rgb(one, size=(320, 180), dtype='float16'))
        assert uploads() == 3 and np.array_equal(a, b)
    finally:
        tm.close()


# ---- 11. errors --------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    import torch
    tm = context(**CONFIGS['native-10'])
    W, H = 192, 96
    src = _source('uniform', 1, W, H).to_torch('cuda:0')
    buf = torch.zeros(4 * 3 * W * H + 64, dtype=torch.uint8, device='cuda:0')     # room for any target below
    L = _abi.lib()

    def call(ow=W, oh=H, dtype=_abi.RGB_U8, layout=_abi.RGB_CHW, row=None, plane=None, frame=None, data=0,
             scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0), n=1, ctx=True, inp=True, out=True):
        E = _abi.RGB_ELEM_BYTES.get(dtype, 1)
        d = _abi.H2SRgbFrames()
        d.data = None if data is None else buf.data_ptr() + data
        d.width, d.height, d.dtype, d.layout = ow, oh, dtype, layout
        d.row_pitch = (ow * E * (1 if layout == _abi.RGB_CHW else 3)) if row is None else row
        d.plane_pitch = d.row_pitch * oh if plane is None else plane
        d.frame_pitch = (3 * d.plane_pitch if layout == _abi.RGB_CHW else d.row_pitch * oh) if frame is None else frame
        for k in range(3):
            d.scale[k], d.bias[k] = scale[k], bias[k]
        tm._use_layouts(src)
        di = src.descriptor()
        return L.h2s_process_rgb(tm._ctx if ctx else None, ctypes.byref(di) if inp else None,
                                 ctypes.byref(d) if out else None, n, tm._stream_ptr(None))

    INV, UNS = _abi.H2S_E_INVALID_ARG, _abi.H2S_E_UNSUPPORTED
    assert call() == 0
    assert call(ctx=False) == INV and call(inp=False) == INV and call(out=False) == INV and call(data=None) == INV
    assert call(n=-1) == INV and call(n=0) == 0
    for ow, oh in ((95, 48), (96, 47), (0, 48), (96, -2)):
        assert call(ow, oh) == INV, (ow, oh)
    assert call(dtype=4) == INV and call(dtype=-1) == INV and call(layout=2) == INV
    assert call(scale=(1.0, 2.0, 1.0)) == INV and call(bias=(0.0, 0.0, 0.5)) == INV          # uint8 is not normalised
    F32 = _abi.RGB_F32
    assert call(dtype=F32, scale=(1.0, 2.0, 1.0), bias=(0.0, 0.0, 0.5)) == 0
    assert call(dtype=F32, scale=(1.0, float('nan'), 1.0)) == INV and call(dtype=F32, bias=(float('inf'), 0, 0)) == INV
    assert call(dtype=F32, row=W * 4 + 2) == INV and call(dtype=_abi.RGB_F16, plane=W * 2 * H + 1) == INV
    assert call(dtype=F32, frame=3 * W * 4 * H + 6) == INV                                  # not multiples of the element
    assert call(row=W - 1) == INV and call(layout=_abi.RGB_HWC, row=3 * W - 1) == INV       # smaller than a row
    assert call(plane=W * H - 1) == INV and call(frame=3 * W * H - 1) == INV
    assert call(layout=_abi.RGB_HWC, frame=3 * W * H - 1) == INV
    assert call(dtype=_abi.RGB_F16, data=1) == INV and call(dtype=F32, data=2) == INV      # data off the element size
    assert call(data=1) == 0                                                                # (uint8: any address)
    assert call(14, 48) == UNS and call(96, 6) == UNS                                       # 13.7 : 1 and 16 : 1
    assert call(16, 8) == 0                                                                 # 12 on both axes is inside
    # through Python: ValueError, and the next good call succeeds
    with pytest.raises(ValueError, match='ratio'):
        tm.process_rgb(src, size=(14, 48))
    big = _source('uniform', 1, 3840, 2160).to_torch('cuda:0')
    with pytest.raises(ValueError, match='ratio'):
        tm.process_rgb(big, size=(224, 224))                                                # 17 : 1 across
    unset = hdr2sdr.Tonemapper(0)
    try:
        with pytest.raises(ValueError, match='set_params'):
            unset.process_rgb(src)
    finally:
        unset.close()
    torch.cuda.synchronize()
    check(tm, src, W, H, 'uint8', 'chw', 'after the errors')
