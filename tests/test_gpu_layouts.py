"""GPU: semi-planar frame sets (nv12 / p010le / p012le, h2s_set_frame_layout)
against the planar path, which the rest of the suite holds to the oracle.

Same codes in, same arithmetic, same codes out: every comparison here is exact
equality.  With in_semi = to_layout(in_planar), every layout combination's
result equals the repacked planar -> planar result.

Sizes: 64x32 one tile, all edges; 192x96 3x3 tiles (the centre one on the
interior scalar-origin loads); 192x70 a bottom tile with 6 live rows; 200x64
the tile kernel plus 8 columns on the generic kernel; 70x34 the generic kernel
with a ragged group.  Three frames, so the frame pitches matter.

The alignment of each side's rows decides the path, as it always has.  A
tight 200-wide planar batch has 200-byte (16-bit) or 100-byte (8-bit) chroma
rows, which miss the tile kernel's 16 / 8-byte row alignment: it is on the
generic kernel with or without this feature, and the generic kernel's exact
arithmetic is not the tile kernel's float32 arithmetic bit for bit.  So that
200x64 exercises TILE_TAIL in all four combinations, and planar and
semi-planar results come from the same kernels, a planar side of that size is
a surface with 16-byte aligned rows (RowAlignedPlanar: chroma rows 208 bytes
apart); the semi-planar side is tight (400 / 200-byte rows).  Every other
size uses tight batches on both sides."""
import numpy as np
import pytest

import hdr2sdr
from hdr2sdr import _abi
from hdr2sdr.frames import FrameBatch
from hdr2sdr.synth import synth_frames

pytestmark = pytest.mark.gpu

F = 3
SIZES = [(64, 32), (192, 96), (192, 70), (200, 64), (70, 34)]
BASE_PATH = {(64, 32): _abi.PATH_TILE, (192, 96): _abi.PATH_TILE, (192, 70): _abi.PATH_TILE,
             (200, 64): _abi.PATH_TILE_TAIL, (70, 34): _abi.PATH_GENERIC}
CHAINS = {
    'hable_lut_g22': dict(tonemapper='hable', gamma=2.2),
    'lp_bt2390_peak_detect': dict(tonemapper='bt.2390', peak_detect=True, maxcll=4000.0),
    'mobius_hlg12': dict(tonemapper='mobius', transfer='arib-std-b67', bits_in=12, bits_out=12),
    'reinhard_nv12': dict(tonemapper='reinhard', bits_out=8),
    'native10': dict(tonemapper='hable', mode='native'),
    'lp_bt2390_12to10_truncate': dict(tonemapper='bt.2390', bits_in=12, bits_out=10, lp_p010='truncate'),
}
BICUBIC = dict(tonemapper='hable', gamma=2.2, chroma_filter='bicubic')
KIND = {'hable_lut_g22': 'edges'}    # codes outside the legal range too (the tile kernel's exact-capable body)
LUT_N = 17
COMBOS = [('semi', 'semi'), ('semi', 'planar'), ('planar', 'semi')]

_lattice = {}
_sources = {}
_results = {}


def lattice():
    if LUT_N not in _lattice:
        _lattice[LUT_N] = hdr2sdr.generate_lattice(LUT_N)
    return _lattice[LUT_N]


@pytest.fixture(scope='module')
def tm():
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.close()


def configure(tm, kw):
    params = hdr2sdr.TonemapParams(**kw)
    tm.set_params(params)
    tm.set_lut(lattice())
    return params


def source(name, kw, size):
    """The seeded planar source of a case, on the host (made once)."""
    key = (name, size)
    if key not in _sources:
        bits = kw.get('bits_in', 10)
        _sources[key] = synth_frames(KIND.get(name, 'smooth'), F, size[0], size[1], bits, device='cpu',
                                     seed=1000 + 7 * size[0] + size[1]).to_numpy()
    return _sources[key]


class RowAlignedPlanar:
    """Planar frames over a byte buffer with every row a multiple of 16 bytes
    apart (what FrameBatch is to Tonemapper: nframes, layout, descriptor())."""
    layout = 'planar'

    def __init__(self, nframes, width, height, bits, fill=0x55):
        import torch
        self.nframes, self.width, self.height, self.bits = nframes, width, height, bits
        self.bps = 1 if bits == 8 else 2
        al = lambda n: (n + 15) // 16 * 16
        self.ls = (al(width * self.bps), al(width // 2 * self.bps))
        self.off = (0, self.ls[0] * height, self.ls[0] * height + self.ls[1] * (height // 2))
        self.fp = self.off[2] + self.ls[1] * (height // 2)
        self.buf = torch.full((nframes * self.fp,), fill, dtype=torch.uint8, device='cuda')

    def descriptor(self):
        d = _abi.H2SFrames()
        for p in range(3):
            d.data[p] = self.buf.data_ptr() + self.off[p]
            d.linesize[p] = self.ls[0 if p == 0 else 1]
            d.frame_pitch[p] = self.fp
        d.width, d.height, d.bits, d.location = self.width, self.height, self.bits, _abi.LOC_DEVICE
        return d

    def _rows(self, raw):
        """(view of this surface's bytes, view of a tight batch's bytes) per plane and frame."""
        w, h, b = self.width, self.height, self.bps
        tight = (0, w * h * b, w * h * b + (w // 2) * (h // 2) * b)
        for f in range(self.nframes):
            for p in range(3):
                rows, rowb = (h, w * b) if p == 0 else (h // 2, w // 2 * b)
                ls = self.ls[0 if p == 0 else 1]
                mine = raw[f * self.fp + self.off[p]:][:rows * ls].reshape(rows, ls)[:, :rowb]
                yield f, mine, tight[p], rows, rowb

    def load(self, fb):
        import torch
        raw = np.full(self.nframes * self.fp, 0x55, dtype=np.uint8)
        src = np.ascontiguousarray(fb.buf).view(np.uint8).reshape(self.nframes, -1)
        for f, mine, o, rows, rowb in self._rows(raw):
            mine[...] = src[f, o:o + rows * rowb].reshape(rows, rowb)
        self.buf.copy_(torch.from_numpy(raw))
        return self

    def to_numpy(self):
        raw = self.buf.cpu().numpy()
        out = FrameBatch.empty_numpy(self.nframes, self.width, self.height, self.bits)
        dst = out.buf.view(np.uint8).reshape(self.nframes, -1)
        for f, mine, o, rows, rowb in self._rows(raw):
            dst[f, o:o + rows * rowb] = mine.reshape(-1)
        return out


def row_aligned(size):
    return size[0] == 200     # tight planar chroma rows of this width miss the tile kernel's alignment


def device_source(fb, layout='planar', aligned=False):
    """A host planar batch on the device in `layout` (aligned: a planar one
    with 16-byte aligned rows whatever the width)."""
    if layout == 'semi':
        return fb.to_layout('semi').to_torch('cuda')
    if aligned or row_aligned((fb.width, fb.height)):
        return RowAlignedPlanar(fb.nframes, fb.width, fb.height, fb.bits).load(fb)
    return fb.to_torch('cuda')


def device_dest(n, size, bits, layout, aligned=False):
    if layout == 'planar' and (aligned or row_aligned(size)):
        return RowAlignedPlanar(n, size[0], size[1], bits)
    dst = FrameBatch.empty_torch(n, size[0], size[1], bits, 'cuda', layout)
    dst.buf.fill_(0x55 if bits == 8 else 0x5555)    # a pattern no repacked result has everywhere
    return dst


def run(tm, params, src, dst):
    import torch
    if params.peak_detect:
        tm.reset_peak()
    tm.process(src, dst)
    torch.cuda.synchronize()
    return dst


def convert(tm, params, src, out_layout, aligned=False):
    dst = device_dest(src.nframes, (src.width, src.height), params.bits_out, out_layout, aligned)
    return run(tm, params, src, dst).to_numpy()


def reference(tm, params, name, kw, size, kind='tight'):
    """planar -> planar of a case (computed once, kept unchanged).  kind:
    'tight' batches (row-aligned surfaces at 200 wide, see above); 'aligned':
    planar surfaces with 16-byte aligned rows on both sides, the planar
    counterpart of a decoder's padded surface (the tile kernel from 64 pixels
    of width up); 'generic': the generic kernel only (H2S_OPT_FAST_PATH 0);
    any other name: tight batches again, kept apart for a caller whose `tm`
    runs the chain under other parameters (a Previewer's)."""
    key = (name, size, kind)
    if key not in _results:
        if kind == 'generic':
            tm.set_option(_abi.OPT_FAST_PATH, 0)
        try:
            al = kind == 'aligned'
            out = convert(tm, params, device_source(source(name, kw, size), aligned=al), 'planar', aligned=al)
        finally:
            tm.set_option(_abi.OPT_FAST_PATH, 1)
        out.buf.setflags(write=False)
        _results[key] = out
    return _results[key]


CASES = [(n, s) for n in sorted(CHAINS) for s in SIZES]


@pytest.mark.parametrize('name,size', CASES, ids=[f'{n}-{s[0]}x{s[1]}' for n, s in CASES])
def test_layout_combinations_equal_planar(tm, name, size):
    kw = CHAINS[name]
    params = configure(tm, kw)
    want = reference(tm, params, name, kw, size)
    src = {l: device_source(source(name, kw, size), l) for l in ('planar', 'semi')}
    assert src['semi'].layout == 'semi'
    for il, ol in COMBOS:
        got = convert(tm, params, src[il], ol)
        assert got.layout == ol
        assert np.array_equal(got.buf, want.to_layout(ol).buf), (il, ol)
        if ol == 'semi' and params.bits_out != 8:
            assert not (got.buf & ((1 << (16 - params.bits_out)) - 1)).any(), 'low bits of a semi word'


def test_bicubic_two_pass_layouts(tm):
    size = (192, 96)
    params = configure(tm, BICUBIC)
    want = reference(tm, params, 'bicubic', BICUBIC, size)
    planar = source('bicubic', BICUBIC, size).to_torch('cuda')
    semi = planar.to_layout('semi')
    for il, ol in COMBOS:
        src = semi if il == 'semi' else planar
        dst = FrameBatch.empty_torch(F, size[0], size[1], params.bits_out, 'cuda', ol)
        assert tm.query_path(src, dst) == _abi.PATH_TILE
        assert np.array_equal(convert(tm, params, src, ol).buf, want.to_layout(ol).buf), (il, ol)
    # the generic two-pass kernels too
    tm.set_option(_abi.OPT_FAST_PATH, 0)
    try:
        slow = convert(tm, params, planar, 'planar')
        dst = FrameBatch.empty_torch(F, size[0], size[1], params.bits_out, 'cuda', 'semi')
        assert tm.query_path(semi, dst) == _abi.PATH_TWO_PASS
        assert np.array_equal(convert(tm, params, semi, 'semi').buf, slow.to_layout('semi').buf)
    finally:
        tm.set_option(_abi.OPT_FAST_PATH, 1)


@pytest.mark.parametrize('size', SIZES, ids=[f'{s[0]}x{s[1]}' for s in SIZES])
@pytest.mark.parametrize('name', ['hable_lut_g22', 'reinhard_nv12', 'lp_bt2390_peak_detect'])
def test_semi_stays_on_the_tile_kernel(tm, name, size):
    params = configure(tm, CHAINS[name])
    for il in ('planar', 'semi'):
        for ol in ('planar', 'semi'):
            src = device_dest(F, size, params.bits_in, il)
            dst = device_dest(F, size, params.bits_out, ol)
            assert tm.query_path(src, dst) == BASE_PATH[size], (il, ol)
    if row_aligned(size):
        # the tight planar batch of this width: its own rows keep it off the
        # tile kernel, on either side, as they did before the layouts existed
        tight = {b: FrameBatch.empty_torch(F, size[0], size[1], b, 'cuda') for b in (params.bits_in, params.bits_out)}
        semi = {b: FrameBatch.empty_torch(F, size[0], size[1], b, 'cuda', 'semi') for b in tight}
        assert tm.query_path(tight[params.bits_in], tight[params.bits_out]) == _abi.PATH_GENERIC
        assert tm.query_path(tight[params.bits_in], semi[params.bits_out]) == _abi.PATH_GENERIC
        assert tm.query_path(semi[params.bits_in], tight[params.bits_out]) == _abi.PATH_GENERIC


@pytest.mark.parametrize('size', SIZES, ids=[f'{s[0]}x{s[1]}' for s in SIZES])
@pytest.mark.parametrize('name', ['hable_lut_g22', 'lp_bt2390_12to10_truncate', 'mobius_hlg12'])
def test_low_bits_of_semi_input_are_ignored(tm, name, size):
    kw = CHAINS[name]
    params = configure(tm, kw)
    want = reference(tm, params, name, kw, size)
    semi = source(name, kw, size).to_layout('semi')
    sh = 16 - params.bits_in
    junk = np.random.default_rng(size[0] * 131 + size[1]).integers(0, 1 << sh, size=semi.buf.shape, dtype=np.uint16)
    assert junk.any()
    dirty = FrameBatch(semi.buf | junk, size[0], size[1], params.bits_in, 'semi')
    for ol in ('semi', 'planar'):
        got = convert(tm, params, dirty.to_torch('cuda'), ol)
        assert np.array_equal(got.buf, want.to_layout(ol).buf), ol


class Surface:
    """A hand-built frame set over a larger byte buffer: what FrameBatch is to
    Tonemapper (nframes, layout, descriptor()), with padded pitches."""

    def __init__(self, buf, width, height, bits, layout, planes):
        self.buf, self.width, self.height, self.bits, self.layout = buf, width, height, bits, layout
        self.planes = planes      # per plane: (byte offset, linesize, frame pitch)
        self.nframes = F

    def descriptor(self):
        d = _abi.H2SFrames()
        for p, (off, ls, fp) in enumerate(self.planes):
            d.data[p] = self.buf.data_ptr() + off
            d.linesize[p] = ls
            d.frame_pitch[p] = fp
        d.width, d.height, d.bits, d.location = self.width, self.height, self.bits, _abi.LOC_DEVICE
        return d


SENTINEL = 0xA5
GUARD = 4096
PITCH = 512


def padded_surface(w, h, bits, uv_shift=0):
    """Semi-planar surface as a decoder lays it out: Y rows then UV rows, all
    PITCH bytes apart, frames a padded pitch apart, guards around the whole."""
    import torch
    fp = PITCH * (h + h // 2) + 1024
    total = GUARD + F * fp + GUARD
    buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device='cuda')
    planes = [(GUARD, PITCH, fp), (GUARD + PITCH * h + uv_shift, PITCH, fp)]
    return Surface(buf, w, h, bits, 'semi', planes), fp


def surface_image(fb, w, h, fp, uv_shift=0):
    """The bytes a padded surface must hold when it carries the tight semi
    batch fb: its rows where the samples are, the sentinel everywhere else."""
    bps = 1 if fb.bits == 8 else 2
    img = np.full(GUARD + F * fp + GUARD, SENTINEL, dtype=np.uint8)
    raw = np.ascontiguousarray(fb.buf).view(np.uint8).reshape(F, -1)
    rowb = w * bps
    for f in range(F):
        for r in range(h + h // 2):
            o = GUARD + f * fp + r * PITCH + (uv_shift if r >= h else 0)
            img[o:o + rowb] = raw[f, r * rowb:(r + 1) * rowb]
    return img


@pytest.mark.parametrize('size', SIZES, ids=[f'{s[0]}x{s[1]}' for s in SIZES])
@pytest.mark.parametrize('name', ['hable_lut_g22', 'reinhard_nv12', 'lp_bt2390_peak_detect'])
def test_padded_surfaces(tm, name, size):
    import torch
    kw = CHAINS[name]
    params = configure(tm, kw)
    w, h = size
    # (rows 512 bytes apart are aligned at any width, so 70x34 is on the tile
    # kernel here, as its row-aligned planar counterpart is)
    want = reference(tm, params, name, kw, size, 'aligned').to_layout('semi')
    semi = source(name, kw, size).to_layout('semi')
    src, fp_in = padded_surface(w, h, params.bits_in)
    src_img = surface_image(semi, w, h, fp_in)
    src.buf.copy_(torch.from_numpy(src_img))
    dst, fp_out = padded_surface(w, h, params.bits_out)
    assert tm.query_path(src, dst) == (_abi.PATH_TILE if w % 64 == 0 else _abi.PATH_TILE_TAIL)
    planar = [device_dest(F, size, b, 'planar', aligned=True) for b in (params.bits_in, params.bits_out)]
    assert tm.query_path(planar[0], planar[1]) == tm.query_path(src, dst)
    run(tm, params, src, dst)
    assert np.array_equal(dst.buf.cpu().numpy(), surface_image(want, w, h, fp_out))
    assert np.array_equal(src.buf.cpu().numpy(), src_img)


@pytest.mark.parametrize('size', SIZES, ids=[f'{s[0]}x{s[1]}' for s in SIZES])
def test_peak_stats_identical(tm, size):
    for name in ('lp_bt2390_peak_detect', 'lp_bt2390_12to10_truncate'):
        kw = CHAINS[name]
        configure(tm, kw)
        planar = source(name, kw, size).to_torch('cuda')
        a = tm.peak_stats(planar)
        b = tm.peak_stats(planar.to_layout('semi'))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
        assert (a[0] > 0).all()
    # HLG input (the chunked form where the rows allow it), and the percentile off
    kw = dict(tonemapper='bt.2390', transfer='arib-std-b67', peak_detect=True, pd_percentile=100.0)
    configure(tm, kw)
    planar = source('hlg_peak', kw, size).to_torch('cuda')
    a, b = tm.peak_stats(planar), tm.peak_stats(planar.to_layout('semi'))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('size', [(192, 96), (200, 64), (70, 34)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', ['hable_lut_g22', 'lp_bt2390_12to10_truncate'])
def test_debug_float_identical(tm, name, size):
    kw = CHAINS[name]
    configure(tm, kw)
    planar, semi = (device_source(source(name, kw, size), l) for l in ('planar', 'semi'))
    for stage in (1, 2, 3, 4, 5):
        a, b = tm.debug_float(planar, stage), tm.debug_float(semi, stage)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), stage


@pytest.mark.parametrize('size', [(192, 96), (70, 34)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('use_gpu', [False, True])
def test_preview_identical(size, use_gpu):
    name, kw = 'hable_lut_g22', CHAINS['hable_lut_g22']
    planar = source(name, kw, size).to_torch('cuda')
    semi = planar.to_layout('semi')
    with hdr2sdr.preview.Previewer(0, tonemapper='hable', lattice=lattice(), use_gpu=use_gpu) as pv:
        for box in (('iw', 'ih'), (96, 54)):
            a = pv.convert(planar, box[0], box[1], gamma=1.2)
            b = pv.convert(semi, box[0], box[1], gamma=1.2)
            assert a.shape == b.shape and np.array_equal(a, b), box
        many = pv.convert_batch(semi, 'iw', 'ih')
        for got, want in zip(many, pv.convert_batch(planar, 'iw', 'ih')):
            assert np.array_equal(got, want)


@pytest.mark.parametrize('size', [(192, 96), (70, 34)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('use_gpu', [False, True])
def test_preview_on_semi_output_context(size, use_gpu):
    """A preview's chain output is the call's own planar scratch whatever
    layout the context writes its callers' frames in: the images equal those
    of a context whose output layout was never changed, and that layout is
    still the context's afterwards."""
    name, kw = 'hable_lut_g22', CHAINS['hable_lut_g22']
    planar = source(name, kw, size).to_torch('cuda')
    with hdr2sdr.preview.Previewer(0, tonemapper='hable', lattice=lattice(), use_gpu=use_gpu) as fresh:
        one = fresh.convert(planar, 96, 54, gamma=1.2)
        many = fresh.convert_batch(planar, 'iw', 'ih')
        want = reference(fresh._tm, fresh.params, name, kw, size, f'preview{int(use_gpu)}').to_layout('semi')
    with hdr2sdr.preview.Previewer(0, tonemapper='hable', lattice=lattice(), use_gpu=use_gpu) as pv:
        pv._tm.set_frame_layout('planar', 'semi')
        assert np.array_equal(pv.convert(planar, 96, 54, gamma=1.2), one)
        got = pv.convert_batch(planar, 'iw', 'ih')
        assert len(got) == len(many) == F
        for a, b in zip(got, many):
            assert np.array_equal(a, b)
        assert pv._tm._layouts == ('planar', 'semi')     # so process below sends the context no new layout
        dst = device_dest(F, size, pv.params.bits_out, 'semi')
        assert np.array_equal(run(pv._tm, pv.params, planar, dst).to_numpy().buf, want.buf)


@pytest.mark.parametrize('size', [(192, 96), (200, 64), (70, 34)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', ['hable_lut_g22', 'reinhard_nv12', 'lp_bt2390_peak_detect'])
def test_host_semi_batches(tm, name, size):
    """Host frames (staged by h2s_process: the chunk pipeline for 3 frames, the
    serial path for 1) in both layouts on both sides."""
    kw = CHAINS[name]
    params = configure(tm, kw)
    want = reference(tm, params, name, kw, size)
    planar = source(name, kw, size)
    semi = planar.to_layout('semi')
    # (a host set is staged into a tight device copy, so a 200-wide planar side
    # would be on the generic kernel: semi on both sides there)
    for il, ol in COMBOS[:1] if row_aligned(size) else COMBOS:
        src = semi if il == 'semi' else planar
        dst = FrameBatch.empty_numpy(F, size[0], size[1], params.bits_out, ol)
        run(tm, params, src, dst)
        assert np.array_equal(dst.buf, want.to_layout(ol).buf), (il, ol)
    # one frame: no chunk pipeline; and a device destination for a host source
    one = FrameBatch.empty_numpy(1, size[0], size[1], params.bits_out, 'semi')
    run(tm, params, semi.slice(0, 1), one)
    assert np.array_equal(one.buf, want.to_layout('semi').buf[:1])
    got = convert(tm, params, semi, 'semi')
    assert np.array_equal(got.buf, want.to_layout('semi').buf)


def test_semi_descriptor_validation(tm):
    import torch
    name, kw, size = 'hable_lut_g22', CHAINS['hable_lut_g22'], (192, 96)
    params = configure(tm, kw)
    w, h = size
    # (off the alignment the generic kernel runs: its planar result is the yardstick)
    want = reference(tm, params, name, kw, size, 'generic').to_layout('semi')
    semi = source(name, kw, size).to_layout('semi')
    # a UV linesize below a row of pairs; odd pitches of 16-bit words
    for plane, ls, fp_add in ((1, w * 2 - 2, 0), (1, PITCH + 1, 0), (0, PITCH, 1)):
        src, fp = padded_surface(w, h, 10)
        dst, _ = padded_surface(w, h, 10)
        pl = list(src.planes[plane])
        pl[1], pl[2] = ls if plane == 1 else pl[1], fp + fp_add
        src.planes[plane] = tuple(pl)
        with pytest.raises(ValueError):
            tm.process(src, dst)
    # an unknown layout value, and a planar set's plane 2 is still required
    assert tm._L.h2s_set_frame_layout(tm._ctx, 2, 0) == _abi.H2S_E_INVALID_ARG
    assert tm._L.h2s_set_frame_layout(tm._ctx, 0, -1) == _abi.H2S_E_INVALID_ARG
    src, _ = padded_surface(w, h, 10)
    dst, _ = padded_surface(w, h, 10)
    src.layout = dst.layout = 'planar'
    with pytest.raises(ValueError):
        tm.process(src, dst)
    # UV data two bytes off the alignment: the generic kernel, same result
    src, fp_in = padded_surface(w, h, 10, uv_shift=2)
    src_img = surface_image(semi, w, h, fp_in, uv_shift=2)
    src.buf.copy_(torch.from_numpy(src_img))
    dst, fp_out = padded_surface(w, h, 10, uv_shift=2)
    assert tm.query_path(src, dst) == _abi.PATH_GENERIC
    run(tm, params, src, dst)
    assert np.array_equal(dst.buf.cpu().numpy(), surface_image(want, w, h, fp_out, uv_shift=2))
    # only the source off alignment: still generic, into an aligned surface
    dst, fp_out = padded_surface(w, h, 10)
    assert tm.query_path(src, dst) == _abi.PATH_GENERIC
    run(tm, params, src, dst)
    assert np.array_equal(dst.buf.cpu().numpy(), surface_image(want, w, h, fp_out))
