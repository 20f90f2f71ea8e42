"""4:2:0 frame batches: planar (yuv420p / yuv420p10le / yuv420p12le) and
semi-planar (nv12 / p010le / p012le).

The reference never holds frames itself: ffmpeg owns every buffer
(SURVEY.md §8b "Ownership").  Here the caller owns them, in device memory
(torch tensors on a HIP device) or host memory (numpy), and describes them to
libh2s with an ``h2s_frames`` record: one base pointer, linesize and
frame pitch per plane.

Layout in HBM: one contiguous allocation per batch, frames back to back, each
frame = Y plane (H x W) then U (H/2 x W/2) then V, rows packed (linesize =
width * bytes-per-sample).  A 3840x2160 10-bit frame is 24,883,200 B, so a
288 GB MI355X holds >10,000 such frames; batches of 16-64 frames per launch
keep the grid far above the 256-CU fill point.

Semi-planar batches (``layout='semi'``: what hardware decoders produce and
hardware encoders take) hold, per frame, the Y plane then one plane of
interleaved (Cb, Cr) pairs (H/2 rows of W samples), the same number of bytes;
10/12-bit samples carry the value in the high bits of their 16-bit word.  The
kernels read and write both layouts in place (h2s_set_frame_layout);
``to_layout`` is the host-side repack for tests and callers.

Source batches may also be planar 4:2:2 or 4:4:4 (``subsampling='422'`` /
``'444'``: yuv422p10le / yuv444p10le and their 12-bit forms), with U and V
planes of H x W/2 or H x W samples: W * H * 2 or W * H * 3 samples per frame.
The kernels read them at their own chroma resolution
(h2s_set_input_subsampling); the output side is always 4:2:0.

Semi-planar 4:2:2 / 4:4:4 source batches (p210le / p212le / p410le / p412le:
what a hardware decoder hands out for such streams) exist only behind the
explicit ``allow_semi_sub=True``: the Y plane, then one plane of (Cb, Cr) pairs
with H rows of W/2 (4:2:2) or W (4:4:4) pairs, the code in the high bits of
each word.  Only the 4:2:0 front-end reads them
(Tonemapper.set_input_decimation('bicubic'), h2s_set_input_decimation).

A source batch also carries two tags of its stream (``color_range`` 'tv' |
'pc', ``chroma_location`` 'left' | 'topleft': ffprobe's fields of those names),
which the kernels honour when they read it (h2s_set_input_tags): full-range
codes, and 4:2:0 chroma rows co-sited with the even luma rows.  They describe
how the samples are to be read and change nothing about the buffer; on a
destination batch they are ignored (the output is limited range, left-sited).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _abi


LAYOUTS = ('planar', 'semi')
SUBSAMPLINGS = ('420', '422', '444')
COLOR_RANGES = ('tv', 'pc')
CHROMA_LOCATIONS = ('left', 'topleft')
# chroma plane = (width >> cxs) x (height >> cys) samples
_CHROMA_SHIFTS = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}


def sample_bytes(bits: int) -> int:
    return 1 if bits == 8 else 2


def frame_samples(width: int, height: int, subsampling: str = '420') -> int:
    """Samples of one frame: W * H * {3/2, 2, 3}."""
    cxs, cys = _CHROMA_SHIFTS[subsampling]
    return width * height + 2 * ((width >> cxs) * (height >> cys))


def frame_bytes(width: int, height: int, bits: int, subsampling: str = '420') -> int:
    return frame_samples(width, height, subsampling) * sample_bytes(bits)


@dataclass
class FrameBatch:
    """``nframes`` planar 4:2:0 frames in one contiguous buffer.

    ``buf`` is a 2-D array/tensor [nframes, frame_bytes/sample_bytes] of
    uint8 (8-bit) or int16 (10/12-bit samples stored little-endian in 16
    bits, the *le formats).  Plane views are exposed as y / u / v."""
    buf: Any
    width: int
    height: int
    bits: int
    layout: str = 'planar'
    subsampling: str = '420'
    color_range: str = 'tv'
    chroma_location: str = 'left'
    # admits layout='semi' with subsampling '422' / '444' (p210le / p212le / p410le / p412le)
    allow_semi_sub: bool = False

    def __post_init__(self):
        if self.color_range not in COLOR_RANGES:
            raise ValueError(f"color_range must be 'tv' or 'pc', got {self.color_range!r}")
        if self.chroma_location not in CHROMA_LOCATIONS:
            raise ValueError(f"chroma_location must be 'left' or 'topleft', got {self.chroma_location!r} "
                             '(other chroma locations are not modelled)')
        if self.layout not in LAYOUTS:
            raise ValueError(f"layout must be 'planar' or 'semi', got {self.layout!r}")
        if self.subsampling not in SUBSAMPLINGS:
            raise ValueError(f"subsampling must be '420', '422' or '444', got {self.subsampling!r}")
        if self.subsampling != '420' and self.layout == 'semi' and not self.allow_semi_sub:
            raise ValueError('4:2:2 / 4:4:4 batches are planar only (no p210 / p410) unless allow_semi_sub=True '
                             '(read through the 4:2:0 front-end alone)')

    def _like(self, buf: Any, layout: 'str | None' = None) -> 'FrameBatch':
        """A batch over ``buf`` with this batch's geometry, form and tags."""
        return FrameBatch(buf, self.width, self.height, self.bits, self.layout if layout is None else layout,
                          self.subsampling, self.color_range, self.chroma_location, self.allow_semi_sub)

    # ---- constructors ---------------------------------------------------
    @staticmethod
    def _shape(nframes: int, width: int, height: int, bits: int, subsampling: str = '420') -> 'tuple[int, int]':
        # (4:2:2 / 4:4:4 sources too: the output they convert to is 4:2:0)
        if width <= 0 or height <= 0 or width % 2 or height % 2:
            raise ValueError(f'4:2:0 frames need positive even dimensions, got {width}x{height}')
        if bits not in (8, 10, 12):
            raise ValueError(f'bits must be 8, 10 or 12, got {bits}')
        if subsampling not in SUBSAMPLINGS:
            raise ValueError(f"subsampling must be '420', '422' or '444', got {subsampling!r}")
        return nframes, frame_samples(width, height, subsampling)

    @classmethod
    def empty_torch(cls, nframes: int, width: int, height: int, bits: int, device: Any,
                    layout: str = 'planar', subsampling: str = '420', color_range: str = 'tv',
                    chroma_location: str = 'left', allow_semi_sub: bool = False) -> 'FrameBatch':
        """``allow_semi_sub=True`` admits ``layout='semi'`` with ``subsampling``
        '422' / '444' (p210le / p212le / p410le / p412le: the Y plane, then H
        rows of W/2 or W (Cb, Cr) pairs, codes in the high bits); so do
        empty_numpy and empty_pinned."""
        import torch
        dt = torch.uint8 if bits == 8 else torch.int16
        return cls(torch.empty(cls._shape(nframes, width, height, bits, subsampling), dtype=dt, device=device),
                   width, height, bits, layout, subsampling, color_range, chroma_location, allow_semi_sub)

    @classmethod
    def empty_numpy(cls, nframes: int, width: int, height: int, bits: int,
                    layout: str = 'planar', subsampling: str = '420', color_range: str = 'tv',
                    chroma_location: str = 'left', allow_semi_sub: bool = False) -> 'FrameBatch':
        dt = np.uint8 if bits == 8 else np.uint16
        return cls(np.zeros(cls._shape(nframes, width, height, bits, subsampling), dtype=dt), width, height, bits,
                   layout, subsampling, color_range, chroma_location, allow_semi_sub)

    @classmethod
    def empty_pinned(cls, nframes: int, width: int, height: int, bits: int,
                     layout: str = 'planar', subsampling: str = '420', color_range: str = 'tv',
                     chroma_location: str = 'left', allow_semi_sub: bool = False) -> 'FrameBatch':
        """Host batch in page-locked memory (DMA-able without a bounce copy:
        the host-buffer path of h2s_process then runs at PCIe speed). Falls
        back to pageable numpy memory when no GPU runtime is present."""
        try:
            import torch
            if torch.cuda.is_available():
                dt = torch.uint8 if bits == 8 else torch.int16
                t = torch.empty(cls._shape(nframes, width, height, bits, subsampling), dtype=dt, pin_memory=True)
                a = t.numpy() if bits == 8 else t.numpy().view(np.uint16)
                fb = cls(a, width, height, bits, layout, subsampling, color_range, chroma_location, allow_semi_sub)
                fb._pin = t          # keep the pinned allocation alive
                return fb
        except (ImportError, RuntimeError):
            pass
        return cls.empty_numpy(nframes, width, height, bits, layout, subsampling, color_range, chroma_location,
                               allow_semi_sub)

    @classmethod
    def from_planes(cls, y: np.ndarray, u: np.ndarray, v: np.ndarray, bits: int,
                    subsampling: str = '420', color_range: str = 'tv', chroma_location: str = 'left') -> 'FrameBatch':
        """Pack [F,H,W] / [F,H/2,W/2] numpy planes into a batch (4:2:2: U, V
        [F,H,W/2]; 4:4:4: [F,H,W])."""
        f, h, w = y.shape
        fb = cls.empty_numpy(f, w, h, bits, 'planar', subsampling, color_range, chroma_location)
        fb.y[...] = y
        fb.u[...] = u
        fb.v[...] = v
        return fb

    # ---- plane views ------------------------------------------------------
    @property
    def nframes(self) -> int:
        return int(self.buf.shape[0])

    @property
    def is_torch(self) -> bool:
        return not isinstance(self.buf, np.ndarray)

    def _plane(self, p: int):
        w, h = self.width, self.height
        ysz = w * h
        cxs, cys = _CHROMA_SHIFTS[self.subsampling]
        csz = (w >> cxs) * (h >> cys)
        if p == 0:
            return self.buf[:, :ysz].reshape(self.nframes, h, w)
        if self.layout == 'semi':
            return self.uv[..., p - 1]
        off = ysz + (p - 1) * csz
        return self.buf[:, off:off + csz].reshape(self.nframes, h >> cys, w >> cxs)

    @property
    def uv(self):
        """The interleaved plane of a semi-planar batch as [F, H/2, W/2, 2]
        ((Cb, Cr) last; a 4:2:2 / 4:4:4 batch: [F, H, W/2, 2] / [F, H, W, 2]);
        ``u`` / ``v`` of such a batch are strided views of it."""
        if self.layout != 'semi':
            raise ValueError('uv is the interleaved plane of a semi-planar batch')
        w, h = self.width, self.height
        cxs, cys = _CHROMA_SHIFTS[self.subsampling]
        return self.buf[:, w * h:].reshape(self.nframes, h >> cys, w >> cxs, 2)

    @property
    def y(self):
        return self._plane(0)

    @property
    def u(self):
        return self._plane(1)

    @property
    def v(self):
        return self._plane(2)

    def to_numpy(self) -> 'FrameBatch':
        if not self.is_torch:
            return self
        a = self.buf.detach().cpu().numpy()
        if self.bits != 8:
            a = a.view(np.uint16)
        return self._like(a)

    def to_torch(self, device: Any) -> 'FrameBatch':
        import torch
        if self.is_torch:
            return self._like(self.buf.to(device))
        a = self.buf if self.bits == 8 else self.buf.view(np.int16)
        return self._like(torch.from_numpy(np.ascontiguousarray(a)).to(device))

    def slice(self, start: int, stop: int) -> 'FrameBatch':
        return self._like(self.buf[start:stop])

    def to_layout(self, layout: str) -> 'FrameBatch':
        """A copy of the batch in ``layout`` (the batch itself when it already
        is): planes interleaved or split, 10/12-bit codes moved to the high
        bits of their words (semi) or back to the low bits (planar; whatever
        the low bits of a semi word held is dropped).  A host / torch repack
        for tests and callers: the product path reads and writes both layouts
        in place and never calls it."""
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be 'planar' or 'semi', got {layout!r}")
        if self.subsampling != '420':
            raise ValueError('to_layout repacks 4:2:0 batches only (4:2:2 / 4:4:4 batches are planar)')
        if layout == self.layout:
            return self
        sh = 0 if self.bits == 8 else 16 - self.bits
        if self.is_torch:
            import torch
            dst = self._like(torch.empty_like(self.buf), layout)
            # (int16 storage: the codes move as unsigned 16-bit words)
            def up(x):
                if not sh:
                    return x
                v = (x.to(torch.int32) << sh) & 0xFFFF
                return (v - ((v & 0x8000) << 1)).to(torch.int16)   # the word's bits as int16

            def down(x):
                return ((x.to(torch.int32) & 0xFFFF) >> sh).to(torch.int16) if sh else x
        else:
            dst = self._like(np.empty_like(self.buf), layout)

            def up(x):
                return (x.astype(np.uint32) << sh).astype(self.buf.dtype) if sh else x

            def down(x):
                return x >> sh if sh else x
        conv = up if layout == 'semi' else down
        dst.y[...] = conv(self.y)
        if layout == 'semi':
            dst.uv[..., 0] = conv(self.u)
            dst.uv[..., 1] = conv(self.v)
        else:
            dst.u[...] = conv(self.u)
            dst.v[...] = conv(self.v)
        return dst

    # ---- C-ABI descriptor ---------------------------------------------------
    def descriptor(self) -> _abi.H2SFrames:
        d = _abi.H2SFrames()
        sb = sample_bytes(self.bits)
        w, h = self.width, self.height
        if self.is_torch:
            if not self.buf.is_contiguous():
                raise ValueError('frame buffer must be contiguous')
            base = self.buf.data_ptr()
            loc = _abi.LOC_DEVICE if self.buf.is_cuda else _abi.LOC_HOST
        else:
            if not self.buf.flags['C_CONTIGUOUS']:
                raise ValueError('frame buffer must be C-contiguous')
            base = self.buf.ctypes.data
            loc = _abi.LOC_HOST
        ysz = w * h * sb
        cxs, cys = _CHROMA_SHIFTS[self.subsampling]
        csz = (w >> cxs) * (h >> cys) * sb
        fpitch = ysz + 2 * csz
        d.data[0] = base
        d.data[1] = base + ysz
        d.linesize[0] = w * sb
        if self.layout == 'semi':
            # plane 1: the interleaved plane, a row of W samples (4:4:4: 2 W); plane 2 unused (zero)
            d.linesize[1] = 2 * (w >> cxs) * sb
            d.frame_pitch[0] = d.frame_pitch[1] = fpitch
        else:
            d.data[2] = base + ysz + csz
            d.linesize[1] = d.linesize[2] = (w >> cxs) * sb
            for p in range(3):
                d.frame_pitch[p] = fpitch
        d.width, d.height, d.bits, d.location = w, h, self.bits, loc
        return d


def descriptor_ptr(fb: FrameBatch):
    d = fb.descriptor()
    return d, ctypes.byref(d)
