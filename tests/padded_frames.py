"""Device frame sets with padded rows, in every form the library reads or
writes: what FrameBatch is to Tonemapper (nframes, width, height, bits, layout,
subsampling, descriptor()), over a byte buffer whose rows lie a multiple of
``align`` bytes apart.  Rows 16 bytes apart send a frame of any width through
the tile kernel (and k_process for the W % 64 columns), where a tight batch of
that width would run on the generic kernel."""
import numpy as np

from hdr2sdr import _abi
from hdr2sdr.frames import _CHROMA_SHIFTS, FrameBatch, sample_bytes

FILL = 0x55     # what the padding holds, before and after a run


class RowPadded:
    def __init__(self, nframes, width, height, bits, layout='planar', subsampling='420', align=16):
        import torch
        self.nframes, self.width, self.height, self.bits = nframes, width, height, bits
        self.layout, self.subsampling = layout, subsampling
        b = sample_bytes(bits)
        cxs, cys = _CHROMA_SHIFTS[subsampling]
        if layout == 'semi':      # Y, then one plane of (Cb, Cr) pairs
            geo = [(height, width * b), (height // 2, width * b)]
        else:
            geo = [(height, width * b)] + [(height >> cys, (width >> cxs) * b)] * 2
        self.planes, off = [], 0       # per plane: (byte offset in the frame, linesize, rows, bytes of a row)
        for rows, rowb in geo:
            ls = (rowb + align - 1) // align * align
            self.planes.append((off, ls, rows, rowb))
            off += rows * ls
        self.fp = off
        self.buf = torch.full((nframes * self.fp,), FILL, dtype=torch.uint8, device='cuda')

    def descriptor(self):
        d = _abi.H2SFrames()
        for p, (off, ls, _, _) in enumerate(self.planes):
            d.data[p] = self.buf.data_ptr() + off
            d.linesize[p], d.frame_pitch[p] = ls, self.fp
        d.width, d.height, d.bits, d.location = self.width, self.height, self.bits, _abi.LOC_DEVICE
        return d

    def _rows(self, raw):
        """(frame, this surface's rows of a plane, the plane's offset in a tight frame) per plane and frame."""
        for f in range(self.nframes):
            tight = 0
            for off, ls, rows, rowb in self.planes:
                yield f, raw[f * self.fp + off:][:rows * ls].reshape(rows, ls)[:, :rowb], tight
                tight += rows * rowb

    def load(self, fb):
        """Fill from a host batch of the same form; returns self."""
        import torch
        assert (fb.layout, fb.subsampling, fb.bits) == (self.layout, self.subsampling, self.bits)
        raw = np.full(self.nframes * self.fp, FILL, dtype=np.uint8)
        src = np.ascontiguousarray(fb.buf).view(np.uint8).reshape(self.nframes, -1)
        for f, mine, o in self._rows(raw):
            mine[...] = src[f, o:o + mine.size].reshape(mine.shape)
        self.buf.copy_(torch.from_numpy(raw))
        return self

    def raw(self):
        """Every byte of the surface, padding included (numpy)."""
        return self.buf.cpu().numpy()

    def to_numpy(self):
        """The frames as a tight host batch."""
        raw = self.raw()
        out = FrameBatch.empty_numpy(self.nframes, self.width, self.height, self.bits, self.layout, self.subsampling)
        dst = out.buf.view(np.uint8).reshape(self.nframes, -1)
        for f, mine, o in self._rows(raw):
            dst[f, o:o + mine.size] = mine.reshape(-1)
        return out
