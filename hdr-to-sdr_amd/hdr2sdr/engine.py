"""Tonemapper: one libh2s context on one GPU.

Replaces what the reference does per conversion — spawn ffmpeg with the chain
(src/conversion.py:209-224) and let it run filter_frame per frame — with a
context that holds the LUT lattice and resolved parameters in HBM and launches
the fused HIP kernel over whole batches of device-resident frames.
"""
from __future__ import annotations

import ctypes
from typing import Any, Sequence

import numpy as np

from . import _abi
from .chain import TonemapParams, parse_filter_chain
from .frames import FrameBatch
from . import lut as _lut


# ---- the RGB tensor output's argument checks (Tonemapper.process_rgb) --------
def rgb_dtype(dtype: Any) -> 'tuple[int, Any]':
    """(enum h2s_rgb_dtype, torch dtype) of 'uint8' | 'float16' | 'bfloat16' |
    'float32' or the torch dtype of that name."""
    import torch
    name = dtype if isinstance(dtype, str) else str(dtype).replace('torch.', '')
    if name not in _abi.RGB_DTYPES:
        raise ValueError(f"dtype must be one of {sorted(_abi.RGB_DTYPES)} (or the torch dtype), got {dtype!r}")
    return _abi.RGB_DTYPES[name], getattr(torch, name)


def rgb_normalisation(code: int, mean: Any, std: Any) -> 'tuple[list[float], list[float]]':
    """(scale, bias) with out = scale * v + bias for (v - mean) / std."""
    if mean is None and std is None:
        return [1.0] * 3, [0.0] * 3
    if code == _abi.RGB_U8:
        raise ValueError('mean / std normalisation is for the float dtypes (uint8 holds the 0..255 picture)')
    m = [0.0] * 3 if mean is None else [float(v) for v in mean]
    s = [1.0] * 3 if std is None else [float(v) for v in std]
    if len(m) != 3 or len(s) != 3:
        raise ValueError('mean and std are three floats each (R, G, B)')
    if not all(np.isfinite(m + s)) or any(v == 0.0 for v in s):
        raise ValueError('mean and std must be finite, and std non-zero')
    return [1.0 / v for v in s], [-a / v for a, v in zip(m, s)]


def check_rgb_size(w: int, h: int) -> None:
    if w < 2 or h < 2 or w % 2 or h % 2:
        raise ValueError(f'the RGB target needs even width and height >= 2, got {w}x{h}')


def rgb_tensor_size(out: Any, layout: str) -> 'tuple[int, int]':
    """(width, height) of an N x 3 x H x W ('chw') or N x H x W x 3 ('hwc') tensor."""
    if out.dim() != 4 or out.shape[1 if layout == 'chw' else 3] != 3:
        want = 'N x 3 x H x W' if layout == 'chw' else 'N x H x W x 3'
        raise ValueError(f'out must be {want} for layout {layout!r}, got {tuple(out.shape)}')
    return (int(out.shape[3]), int(out.shape[2])) if layout == 'chw' else (int(out.shape[2]), int(out.shape[1]))


def rgb_frames(out: Any, code: int, layout: str, scale: Any, bias: Any, nframes: int) -> _abi.H2SRgbFrames:
    """The h2s_rgb_frames record of a torch tensor, pitches from its strides.
    Raises ValueError for a tensor the library cannot write in place."""
    _, tdtype = rgb_dtype({v: k for k, v in _abi.RGB_DTYPES.items()}[code])
    w, h = rgb_tensor_size(out, layout)
    check_rgb_size(w, h)
    if out.dtype != tdtype:
        raise ValueError(f'out has dtype {out.dtype}, the call asks for {tdtype}')
    if out.shape[0] < nframes:
        raise ValueError(f'out holds {out.shape[0]} frames, the call converts {nframes}')
    E = _abi.RGB_ELEM_BYTES[code]
    st = [int(v) for v in out.stride()]
    if st[3] != 1:
        raise ValueError(f'out needs an innermost stride of 1, got {st[3]}')
    d = _abi.H2SRgbFrames()
    if layout == 'chw':
        frame, plane, row = st[0], st[1], st[2]
        if row < w or plane < row * h:
            raise ValueError(f'out has overlapping rows or planes (strides {st})')
        extent = 3 * plane
    else:
        if st[2] != 3:
            raise ValueError(f"layout 'hwc' needs stride(-2) == 3 (packed pixels), got {st[2]}")
        frame, plane, row = st[0], 0, st[1]
        if row < 3 * w:
            raise ValueError(f'out has overlapping rows (strides {st})')
        extent = row * h
    if out.shape[0] == 1:
        frame = max(frame, extent)      # (the stride of a dimension of size 1 says nothing)
    if frame < extent:
        raise ValueError(f'out has overlapping frames (strides {st})')
    d.data = out.data_ptr()
    d.width, d.height, d.dtype, d.layout = w, h, code, _abi.RGB_LAYOUTS[layout]
    d.row_pitch, d.plane_pitch, d.frame_pitch = row * E, plane * E, frame * E
    for k in range(3):
        d.scale[k], d.bias[k] = scale[k], bias[k]
    return d


def _residence(batch: Any) -> str:
    """'host', or the torch device of a batch's buffer (Tonemapper.process_ladder)."""
    buf = getattr(batch, 'buf', None)
    dev = getattr(buf, 'device', None)
    return 'host' if dev is None or getattr(dev, 'type', 'cpu') == 'cpu' else str(dev)


class Tonemapper:
    """One context per GPU / worker (contexts share no state)."""

    def __init__(self, device: int = 0, params: 'TonemapParams | None' = None,
                 lut: 'np.ndarray | None' = None):
        L = _abi.lib()
        self._L = L
        ctx = ctypes.c_void_p()
        rc = L.h2s_create(int(device), ctypes.byref(ctx))
        if rc != 0:
            _abi.raise_for(rc, L.h2s_last_error(None).decode())
        self._ctx = ctx
        self.device = device
        self.params: 'TonemapParams | None' = None
        self.lut_size = 0
        self._layouts = ('planar', 'planar')   # what the context last got (h2s_set_frame_layout)
        self._subsampling = '420'              # ... (h2s_set_input_subsampling)
        self._tags = ('tv', 'left')            # ... (h2s_set_input_tags)
        self._decimation = 'off'               # ... (h2s_set_input_decimation)
        self.dovi_records = 0                  # Dolby Vision records set (set_dovi; 0: off)
        if params is not None:
            self.set_params(params)
        if lut is not None:
            self.set_lut(lut)

    # ---- lifecycle --------------------------------------------------------
    def close(self) -> None:
        if getattr(self, '_ctx', None) and self._ctx.value:
            self._L.h2s_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self) -> 'Tonemapper':
        return self

    def __exit__(self, *exc: Any) -> None:
        self.close()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != 0:
            _abi.raise_for(rc, self._L.h2s_last_error(self._ctx).decode())

    # ---- configuration ------------------------------------------------------
    def set_params(self, params: TonemapParams) -> None:
        c = params.to_c()
        self._check(self._L.h2s_set_params(self._ctx, ctypes.byref(c)))
        self.params = params

    def set_lut(self, lattice: Any) -> None:
        """lattice: float32 [n^3, 3] (.cube order) as numpy, or a torch
        tensor (copied to host first)."""
        if not isinstance(lattice, np.ndarray):
            lattice = lattice.detach().cpu().numpy()
        a = np.ascontiguousarray(lattice, dtype=np.float32).reshape(-1, 3)
        n = round(a.shape[0] ** (1 / 3))
        if n ** 3 != a.shape[0]:
            raise ValueError(f'LUT has {a.shape[0]} entries, not a cube')
        self._check(self._L.h2s_set_lut(self._ctx, a.ctypes.data, n))
        self.lut_size = n

    def load_cube(self, path: str) -> None:
        self.set_lut(_lut.load_cube(path))

    def configure_from_chain(self, chain: str, **kw: Any) -> TonemapParams:
        """Drop-in: configure from a reference chain string (src/utils.py:38-42)."""
        params, path = parse_filter_chain(chain, **kw)
        self.set_params(params)
        if params.lut_enabled:
            if path is None or path == '<LUT>':
                self.set_lut(_lut.generate_lattice(_lut.LUT_SIZE))
            else:
                self.load_cube(_lut.unescape_filter_path(path))
        return params

    # ---- execution ----------------------------------------------------------
    def set_frame_layout(self, in_layout: str = 'planar', out_layout: str = 'planar') -> None:
        """How later calls read their source batch and write their
        destination batch ('planar' | 'semi'; h2s_set_frame_layout).  process,
        query_path, debug_float and peak_stats set it from their batches'
        ``layout``, so callers of those never need to."""
        for name in (in_layout, out_layout):
            if name not in _abi.LAYOUTS:
                raise ValueError(f"layout must be 'planar' or 'semi', got {name!r}")
        if (in_layout, out_layout) != self._layouts:
            self._check(self._L.h2s_set_frame_layout(self._ctx, _abi.LAYOUTS[in_layout], _abi.LAYOUTS[out_layout]))
            self._layouts = (in_layout, out_layout)

    def set_input_subsampling(self, subsampling: str = '420') -> None:
        """The chroma subsampling later calls read their source batch with
        ('420' | '422' | '444'; h2s_set_input_subsampling).  process,
        query_path, debug_float and peak_stats set it from their source
        batch's ``subsampling``, so callers of those never need to."""
        if subsampling not in _abi.SUBSAMPLINGS:
            raise ValueError(f"subsampling must be '420', '422' or '444', got {subsampling!r}")
        if subsampling != self._subsampling:
            self._check(self._L.h2s_set_input_subsampling(self._ctx, _abi.SUBSAMPLINGS[subsampling]))
            self._subsampling = subsampling

    def set_input_tags(self, color_range: str = 'tv', chroma_location: str = 'left') -> None:
        """The source tags later calls read their source batch with
        (color_range 'tv' | 'pc', chroma_location 'left' | 'topleft';
        h2s_set_input_tags).  process, query_path, debug_float and peak_stats
        set them from their source batch, so a tag never sticks from one batch
        to the next and callers of those never need to."""
        if color_range not in _abi.COLOR_RANGES:
            raise ValueError(f"color_range must be 'tv' or 'pc', got {color_range!r}")
        if chroma_location not in _abi.CHROMA_LOCATIONS:
            raise ValueError(f"chroma_location must be 'left' or 'topleft', got {chroma_location!r}")
        if (color_range, chroma_location) != self._tags:
            self._check(self._L.h2s_set_input_tags(self._ctx, _abi.COLOR_RANGES[color_range],
                                                   _abi.CHROMA_LOCATIONS[chroma_location]))
            self._tags = (color_range, chroma_location)

    def set_input_decimation(self, mode: str = 'off') -> None:
        """The 4:2:0 front-end of a 4:2:2 / 4:4:4 source batch ('off' |
        'bicubic'; h2s_set_input_decimation).  'bicubic': every later call that
        converts such a batch sees the 4:2:0 frames a swscale-bicubic chroma
        decimation on the device makes of it, on either pipeline, with
        peak_detect, and for semi-planar batches
        (``FrameBatch(..., allow_semi_sub=True)``) too.  Unlike the layout,
        subsampling and tags it is a setting of the context, not of a batch:
        it stays until it is set again."""
        if mode not in _abi.DECIMATIONS:
            raise ValueError(f"input decimation must be 'off' or 'bicubic', got {mode!r}")
        if mode != self._decimation:
            self._check(self._L.h2s_set_input_decimation(self._ctx, _abi.DECIMATIONS[mode]))
            self._decimation = mode

    def set_dovi(self, rpus: Any = None) -> None:
        """Dolby Vision profile 5 (h2s_set_dovi): None (or an empty sequence)
        switches the front-end off; one ``dovi.DoviRpu`` serves every frame; a
        sequence gives record f to frame f of each later call (a later call
        with more frames than records raises ValueError).  The records are
        copied; the call first waits for the context's queued launches, so
        per-frame metadata costs one wait per batch."""
        from .dovi import records_to_c
        if rpus is None:
            self._check(self._L.h2s_set_dovi(self._ctx, None, 0))
            self.dovi_records = 0
            return
        arr = records_to_c(rpus)
        self._check(self._L.h2s_set_dovi(self._ctx, ctypes.addressof(arr) if len(arr) else None, len(arr)))
        self.dovi_records = len(arr)

    def _use_layouts(self, src: FrameBatch, dst: 'FrameBatch | None' = None) -> None:
        # (a call without a destination batch leaves the output side as it is)
        self.set_frame_layout(getattr(src, 'layout', 'planar'),
                              self._layouts[1] if dst is None else getattr(dst, 'layout', 'planar'))
        self.set_input_subsampling(getattr(src, 'subsampling', '420'))
        self.set_input_tags(getattr(src, 'color_range', 'tv'), getattr(src, 'chroma_location', 'left'))
        if dst is not None and getattr(dst, 'subsampling', '420') != '420':
            raise ValueError('the output side is 4:2:0 (destination batch subsampling must be 420)')

    @staticmethod
    def _stream_ptr(stream: Any) -> 'int | None':
        if stream is None:
            try:
                import torch
                if torch.cuda.is_available():
                    return torch.cuda.current_stream().cuda_stream
            except ImportError:
                pass
            return None
        return getattr(stream, 'cuda_stream', stream)

    def process(self, src: FrameBatch, dst: FrameBatch, stream: Any = None,
                nframes: 'int | None' = None) -> None:
        """Tone-map src into dst (asynchronous when both are on the device)."""
        n = src.nframes if nframes is None else nframes
        if n > src.nframes or n > dst.nframes:
            raise ValueError(f'nframes {n} exceeds the batch ({src.nframes} in, {dst.nframes} out)')
        self._use_layouts(src, dst)
        di, do = src.descriptor(), dst.descriptor()
        self._check(self._L.h2s_process(self._ctx, ctypes.byref(di), ctypes.byref(do), int(n),
                                        self._stream_ptr(stream)))

    def process_scaled(self, src: FrameBatch, dst: FrameBatch, stream: Any = None,
                       nframes: 'int | None' = None) -> None:
        """Tone-map src and resize it to dst's width x height in one call
        (h2s_process_scaled: the chain's quantised 4:2:0 output through a
        trailing bicubic ``scale=``; asynchronous when both batches are on the
        device).  With dst of src's size this is ``process``."""
        n = src.nframes if nframes is None else nframes
        if n > src.nframes or n > dst.nframes:
            raise ValueError(f'nframes {n} exceeds the batch ({src.nframes} in, {dst.nframes} out)')
        self._use_layouts(src, dst)
        di, do = src.descriptor(), dst.descriptor()
        self._check(self._L.h2s_process_scaled(self._ctx, ctypes.byref(di), ctypes.byref(do), int(n),
                                               self._stream_ptr(stream)))

    def process_ladder(self, src: FrameBatch, dsts: 'Sequence[FrameBatch]', nframes: 'int | None' = None,
                       stream: Any = None) -> None:
        """Tone-map src once and write every rung of a rendition ladder
        (h2s_process_ladder): ``dsts`` is one to ``_abi.LADDER_MAX``
        destination batches, each of its own width x height (the source's size
        is a rung too), all of one layout, bit depth and residence (all numpy,
        or all torch tensors on one device).  Each rung's bytes are those of
        ``process_scaled`` (``process`` for a rung of the source's size) on an
        equal context, but every frame is converted, and counted by the dynamic
        peak, once.  Asynchronous when every batch is on the device.  The
        arguments are checked here (ValueError) before the library is called."""
        dsts = list(dsts)
        if not 1 <= len(dsts) <= _abi.LADDER_MAX:
            raise ValueError(f'a ladder has 1 to {_abi.LADDER_MAX} rungs, got {len(dsts)}')
        n = src.nframes if nframes is None else int(nframes)
        if n < 0:
            raise ValueError(f'nframes {n} is negative')
        for i, d in enumerate(dsts):
            if n > src.nframes or n > d.nframes:
                raise ValueError(f'rung {i}: nframes {n} exceeds the batch ({src.nframes} in, {d.nframes} out)')
            if d.width < 2 or d.height < 2 or d.width % 2 or d.height % 2:
                raise ValueError(f'rung {i}: the target needs even width and height >= 2, got {d.width}x{d.height}')
            if getattr(d, 'subsampling', '420') != '420':
                raise ValueError(f'rung {i}: the output side is 4:2:0 (destination batch subsampling must be 420)')
            for what in ('layout', 'bits'):
                a, b = getattr(d, what, None), getattr(dsts[0], what, None)
                if a != b:
                    raise ValueError(f'rung {i}: {what} {a!r} differs from rung 0 ({b!r})')
            if _residence(d) != _residence(dsts[0]):
                raise ValueError(f'rung {i}: every rung must live where rung 0 does '
                                 f'({_residence(d)} != {_residence(dsts[0])})')
        self._use_layouts(src, dsts[0])
        di = src.descriptor()
        outs = (_abi.H2SFrames * len(dsts))(*[d.descriptor() for d in dsts])
        self._check(self._L.h2s_process_ladder(self._ctx, ctypes.byref(di), outs, len(dsts), n,
                                               self._stream_ptr(stream)))

    def ladder(self, src: FrameBatch, sizes: 'Sequence[tuple[int, int]]', stream: Any = None,
               out_layout: str = 'planar') -> 'list[FrameBatch]':
        """The converted batch at every ``(w, h)`` of ``sizes``, each allocated
        beside src as ``tm(src, size=(w, h))`` allocates it, from one conversion
        (process_ladder)."""
        if self.params is None:
            raise ValueError('set_params first')
        dsts = []
        for w, h in sizes:
            if src.is_torch:
                dsts.append(FrameBatch.empty_torch(src.nframes, int(w), int(h), self.params.bits_out,
                                                   src.buf.device, out_layout))
            else:
                dsts.append(FrameBatch.empty_numpy(src.nframes, int(w), int(h), self.params.bits_out, out_layout))
        self.process_ladder(src, dsts, stream=stream)
        return dsts

    def process_rgb(self, src: FrameBatch, out: Any = None, size: 'tuple[int, int] | None' = None,
                    dtype: Any = 'uint8', layout: str = 'chw', mean: Any = None, std: Any = None,
                    stream: Any = None, nframes: 'int | None' = None) -> Any:
        """Tone-map src and deliver the SDR picture as an R'G'B' torch tensor
        on the device (h2s_process_rgb): ``layout`` 'chw' gives N x 3 x H x W,
        'hwc' N x H x W x 3, in ``dtype`` 'uint8' | 'float16' | 'bfloat16' |
        'float32' (or the torch dtype).  uint8 holds 0..255; the float dtypes
        hold 0..1, or ``(x - mean) / std`` per channel with ``mean`` / ``std``
        (three floats each).  ``size=(w, h)`` resizes as process_scaled does
        (even sizes, at most 12 : 1 per axis: a 4K source cannot go straight to
        224 x 224).  ``out`` is written in place through its strides (innermost
        stride 1, 'hwc' also stride(-2) == 3: a padded or sliced view works);
        without it a tensor is allocated on the context's device.  The call is
        queued on ``stream`` (default: torch's current stream), so the tensor
        is safe for the next torch op on that stream."""
        import torch
        n = src.nframes if nframes is None else int(nframes)
        if n > src.nframes:
            raise ValueError(f'nframes {n} exceeds the batch ({src.nframes} in)')
        code, tdtype = rgb_dtype(dtype)
        if layout not in _abi.RGB_LAYOUTS:
            raise ValueError(f"layout must be 'chw' or 'hwc', got {layout!r}")
        scale, bias = rgb_normalisation(code, mean, std)
        if out is None:
            w, h = (src.width, src.height) if size is None else (int(size[0]), int(size[1]))
            check_rgb_size(w, h)
            device = src.buf.device if src.is_torch and src.buf.is_cuda else f'cuda:{self.device}'
            out = torch.empty((n, 3, h, w) if layout == 'chw' else (n, h, w, 3), dtype=tdtype, device=device)
        elif size is not None and tuple(int(v) for v in size) != rgb_tensor_size(out, layout):
            raise ValueError(f'size {tuple(size)} is not the size of out {rgb_tensor_size(out, layout)}')
        d = rgb_frames(out, code, layout, scale, bias, n)
        if not out.is_cuda:
            raise ValueError('out must be a tensor on the device (h2s_process_rgb writes device memory only)')
        self._use_layouts(src)
        di = src.descriptor()
        self._check(self._L.h2s_process_rgb(self._ctx, ctypes.byref(di), ctypes.byref(d), n,
                                            self._stream_ptr(stream)))
        return out

    def __call__(self, src: FrameBatch, stream: Any = None, out_layout: str = 'planar',
                 size: 'tuple[int, int] | None' = None) -> FrameBatch:
        """The converted batch, allocated beside src in ``out_layout``; with
        ``size=(w, h)`` at that size (process_scaled)."""
        if self.params is None:
            raise ValueError('set_params first')
        w, h = (src.width, src.height) if size is None else (int(size[0]), int(size[1]))
        if src.is_torch:
            dst = FrameBatch.empty_torch(src.nframes, w, h, self.params.bits_out, src.buf.device, out_layout)
        else:
            dst = FrameBatch.empty_numpy(src.nframes, w, h, self.params.bits_out, out_layout)
        if size is None:
            self.process(src, dst, stream)
        else:
            self.process_scaled(src, dst, stream)
        return dst

    def set_option(self, key: int, value: int) -> None:
        """h2s_set_option (_abi.OPT_FAST_PATH / OPT_TILES_PER_BLOCK / OPT_HOST_SERIAL / OPT_LP_EXACT)."""
        self._check(self._L.h2s_set_option(self._ctx, int(key), int(value)))

    def query_path(self, src: FrameBatch, dst: FrameBatch) -> int:
        """The kernel path (_abi.PATH_*) h2s_process would take for src -> dst."""
        self._use_layouts(src, dst)
        di, do = src.descriptor(), dst.descriptor()
        rc = self._L.h2s_query_path(self._ctx, ctypes.byref(di), ctypes.byref(do))
        if rc < 0:
            self._check(rc)
        return rc

    def debug_float(self, src: FrameBatch, stage: int) -> np.ndarray:
        """float32 [3, H, W] of frame 0 after ``stage``: R, G, B for 1..4,
        the quantiser inputs (Y code, Cb, Cr in code units) for 5; computed by
        the kernel h2s_process would use (the tile kernel's debug instance on
        the tile path)."""
        out = np.empty((3, src.height, src.width), dtype=np.float32)
        self._use_layouts(src)
        d = src.descriptor()
        self._check(self._L.h2s_debug_float(self._ctx, ctypes.byref(d), int(stage), out.ctypes.data,
                                            _abi.LOC_HOST, self._stream_ptr(None)))
        return out

    # ---- dynamic peak (BT.2390 peak_detect) ----------------------------------
    def reset_peak(self) -> None:
        """Start a new sequence: forget the smoothed peak state."""
        self._check(self._L.h2s_peak_reset(self._ctx))

    def peak_stats(self, src: FrameBatch, stream: Any = None) -> 'tuple[np.ndarray, np.ndarray]':
        """Per-frame (max, mean) of PQ(max R,G,B) of a device batch: the
        statistics process() folds into the smoothing (h2s_peak_stats)."""
        n = src.nframes
        fmax, favg = np.zeros(n), np.zeros(n)
        self._use_layouts(src)
        di = src.descriptor()
        self._check(self._L.h2s_peak_stats(self._ctx, ctypes.byref(di), n, fmax.ctypes.data, favg.ctypes.data,
                                           self._stream_ptr(stream)))
        return fmax, favg

    def feed_peak(self, fmax: Any, favg: Any) -> None:
        """Fold frames' statistics into the smoothing state in order, without
        converting them (h2s_peak_feed): a frame-sharded rank replays the
        frames before its range."""
        fmax = np.ascontiguousarray(fmax, dtype=np.float64)
        favg = np.ascontiguousarray(favg, dtype=np.float64)
        if fmax.shape != favg.shape or fmax.ndim != 1:
            raise ValueError('fmax and favg must be 1-D arrays of one length')
        self._check(self._L.h2s_peak_feed(self._ctx, fmax.ctypes.data, favg.ctypes.data, int(fmax.size)))

    def peak_state(self) -> 'dict[str, float]':
        mx, avg, pk = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n = ctypes.c_int64()
        self._check(self._L.h2s_peak_state(self._ctx, ctypes.byref(mx), ctypes.byref(avg), ctypes.byref(pk),
                                           ctypes.byref(n)))
        return {'max_pq': mx.value, 'avg_pq': avg.value, 'peak': pk.value, 'frames': n.value}

    # ---- timing (bench) -----------------------------------------------------
    def set_timing(self, enabled: bool) -> None:
        self._check(self._L.h2s_set_timing(self._ctx, 1 if enabled else 0))

    def kernel_ms(self, count: int) -> float:
        return float(self._L.h2s_kernel_ms(self._ctx, int(count)))
