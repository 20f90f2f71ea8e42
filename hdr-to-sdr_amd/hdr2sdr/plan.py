"""Drop-in I/O planner and executor around libh2s.

The reference runs one ffmpeg child per conversion:
``build()`` (src/ffmpeg_command.py:455-514) emits
``ffmpeg … -i IN -filter_complex "[0:v:0]{chain}[vout]" -map [vout] …``.
``ConversionManager.start`` launches it (src/conversion.py:209-224), and
``monitor_progress`` (:225-272) reads ``time=`` lines from its stderr.
ffmpeg has no external-filter ABI, so here ffmpeg keeps demux, decode,
encode and mux. The tone-map chain moves onto the GPU between two pipes:

    decode:  ffmpeg -i IN -map 0:v:0 -f rawvideo -pix_fmt yuv420p1Xle -
             (or p010le / p012le, and nv12 / p010le / p012le on the encode
             pipe: the semi-planar layouts, ``in_layout`` / ``out_layout``;
             or yuv422p1Xle / yuv444p1Xle for such a source on the CPU chain,
             ``in_subsampling``; the source's own family either way, so a
             full-range or top-left source's codes cross the pipe untouched and
             the kernels honour the tags, ``in_range`` / ``in_chroma_location``)
    libh2s:  h2s_process() on batches of frames (h2s_process_scaled() when the
             plan asks for a smaller deliverable, ``scale=``)
    encode:  ffmpeg -f rawvideo … -i - -i IN <every non-filter option build() chose>

``plan_from_argv`` takes the argv the reference's own ``build()`` produced.
Streams, encoder, rate control, tags, ``-r``, ``-pix_fmt``, metadata and
faststart therefore stay exactly the reference's choice. Only the filter
graph leaves ffmpeg. ``H2SProcess`` is Popen-shaped (``stderr``, ``wait``,
``poll``, ``returncode``, ``terminate``, ``kill``), so ``monitor_progress``
and its ``time=`` parsing work on it unchanged.
"""
from __future__ import annotations

import io
import queue
import subprocess
import threading
from dataclasses import dataclass, field
from typing import Any, Callable, Optional, Tuple

import numpy as np

from .chain import DOVI_P5_ERROR, TonemapParams, is_dovi_profile5, parse_filter_chain

# planar 4:2:0 formats the pipe carries, by bit depth
PIPE_PIX_FMT = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le'}
# the semi-planar formats (hardware decoder / encoder surfaces), by bit depth
PIPE_PIX_FMT_SEMI = {8: 'nv12', 10: 'p010le', 12: 'p012le'}
# planar 4:2:2 / 4:4:4 sources the decode pipe can carry as they are (CPU chain)
PIPE_PIX_FMT_SUB = {'422': {10: 'yuv422p10le', 12: 'yuv422p12le'}, '444': {10: 'yuv444p10le', 12: 'yuv444p12le'}}
# ffprobe pix_fmt -> in_subsampling='auto'
SOURCE_SUBSAMPLING = {'yuv422p10le': '422', 'yuv422p12le': '422', 'yuv444p10le': '444', 'yuv444p12le': '444'}
# encoder -pix_fmt values build() emits (src/ffmpeg_command.py:355-368) -> bits
OUT_PIX_FMT_BITS = {'yuv420p': 8, 'yuv420p10le': 10, 'p010le': 10, 'yuv420p12le': 12}
# setparams=color_primaries=bt709:color_trc=bt709:colorspace=bt709 (src/utils.py:40)
# on frames that leave zscale r=tv: as output tags on the encode side
BT709_TAGS = ['-color_primaries', 'bt709', '-color_trc', 'bt709', '-colorspace', 'bt709', '-color_range', 'tv']
# ffprobe color_range / chroma_location -> in_range / in_chroma_location 'auto'
# (absent, 'unknown' and 'unspecified' are the defaults: tv, left)
SOURCE_RANGE = {'': 'tv', 'unknown': 'tv', 'unspecified': 'tv', 'tv': 'tv', 'pc': 'pc'}
SOURCE_CHROMA_LOCATION = {'': 'left', 'unknown': 'left', 'unspecified': 'left', 'left': 'left', 'topleft': 'topleft'}
TRANSFERS = {'smpte2084': 'smpte2084', 'arib-std-b67': 'arib-std-b67', '': 'smpte2084'}


def scaled_size(in_w: int, in_h: int, box_w: int, box_h: int) -> Tuple[int, int]:
    """The size of a scaled 4:2:0 deliverable (h2s_scaled_size, which this
    restates so that planning needs no library): the aspect fit of
    ``scale=box_w:box_h:force_original_aspect_ratio=decrease`` (libavfilter
    scale_eval: av_rescale, then min with the box), each dimension then rounded
    down to even and not below 2 (``force_divisible_by=2``)."""
    in_w, in_h, box_w, box_h = int(in_w), int(in_h), int(box_w), int(box_h)
    if min(in_w, in_h, box_w, box_h) <= 0:
        raise ValueError('scaled sizes must be positive')
    tw = (box_h * in_w + in_h // 2) // in_h
    th = (box_w * in_h + in_w // 2) // in_w
    w, h = max(min(tw, box_w), 1), max(min(th, box_h), 1)
    return max(w & ~1, 2), max(h & ~1, 2)


@dataclass
class PipePlan:
    decode: 'list[str]'
    encode: 'list[str]'
    params: TonemapParams
    lut_path: 'str | None'
    width: int
    height: int
    input_path: str
    output_path: str
    reference_argv: 'list[str]' = field(default_factory=list)
    # frame layouts on the two pipes ('planar' | 'semi'): what the decode side
    # emits and what the encode side is fed
    in_layout: str = 'planar'
    layout: str = 'planar'
    # chroma subsampling on the decode pipe ('420' | '422' | '444')
    in_subsampling: str = '420'
    # the source's tags, handed to every source batch ('tv' | 'pc', 'left' | 'topleft')
    in_range: str = 'tv'
    in_chroma_location: str = 'left'
    # Dolby Vision profile 5: a DoviRpu for every frame, or a callable
    # dovi(first_frame, count) -> list[DoviRpu]; None: not such a source
    dovi: Any = None
    # the deliverable's size (``scale=``); None: the source's
    out_width: 'int | None' = None
    out_height: 'int | None' = None
    # where a libplacebo plan's 4:2:2 / 4:4:4 source becomes 4:2:0: 'cpu' (the
    # decode side's swscale; the pipe is 4:2:0) or 'gpu' (the pipe carries the
    # source's own subsampling and the context decimates: set_input_decimation)
    decimate: str = 'cpu'

    def __post_init__(self):
        if self.out_width is None:
            self.out_width = self.width
        if self.out_height is None:
            self.out_height = self.height

    @property
    def scaled(self) -> bool:
        return (self.out_width, self.out_height) != (self.width, self.height)

    @property
    def frame_bytes_in(self) -> int:
        from .frames import frame_bytes
        return frame_bytes(self.width, self.height, self.params.bits_in, self.in_subsampling)

    @property
    def frame_bytes_out(self) -> int:
        return self.out_width * self.out_height * 3 // 2 * (1 if self.params.bits_out == 8 else 2)


def _remap_input(spec: str) -> str:
    """'0:a?' -> '1:a?': the original file is input 1 of the encode side."""
    if spec.startswith('0:') or spec == '0':
        return '1' + spec[1:]
    return spec


def plan_from_argv(argv: 'list[str]', properties: 'dict[str, Any]', hdr: 'dict[str, Any] | None' = None,
                   mode: str = 'compat8', in_layout: str = 'planar', out_layout: str = 'planar',
                   in_subsampling: str = '420', in_range: str = 'tv',
                   in_chroma_location: str = 'left', dovi: Any = None,
                   scale: 'Tuple[int, int] | None' = None, decimate: str = 'cpu') -> PipePlan:
    """Split a reference ``build()`` argv into decode/encode argvs + params.

    in_layout / out_layout ('planar' | 'semi' | 'auto'): the frame layout on
    the decode and encode pipes.  'semi' carries nv12 / p010le / p012le, which
    libh2s reads and writes in place.  out_layout='auto' is semi exactly when
    the reference's ``-pix_fmt`` is ``p010le`` (its hardware HEVC encoders,
    src/ffmpeg_command.py:365-368): the encoder then takes the pipe's frames
    as they are instead of repacking each one on the CPU.  in_layout='auto'
    is planar (a software decoder's native output).

    in_subsampling ('420' | '422' | '444' | 'auto'): the chroma subsampling on
    the decode pipe.  With '422' / '444' a CPU-chain plan asks the decoder for
    yuv422p1Xle / yuv444p1Xle, so a ProRes 422 / 4444 or HEVC 4:2:2 / 4:4:4
    source reaches the kernels at its own chroma resolution, as it reaches
    zscale in the reference's chain (no swscale chroma pass in front).
    'auto' reads ``properties.get('pix_fmt')`` (ffprobe's stream field; the
    reference's ``get_video_properties`` dict does not carry it, and without
    it the answer is '420'): yuv422p10le / 12le and yuv444p10le / 12le map to
    themselves, anything else is '420'.  A libplacebo chain always pipes 4:2:0
    whatever is asked: the reference uploads ``format=p010`` there
    (src/utils.py:430-431), so swscale's 4:2:0 is what libplacebo sees.
    Planar input only.

    in_range ('tv' | 'pc' | 'auto') and in_chroma_location ('left' | 'topleft'
    | 'auto'): the source's colour range and 4:2:0 chroma siting, which the
    reference's chains take from the decoded frame (zscale has no ``rin=``,
    vf_libplacebo reads the AVFrame) and the kernels honour
    (h2s_set_input_tags); both apply to both pipelines.  The defaults are the
    untagged behaviour.  'auto' reads ``properties.get('color_range')`` /
    ``properties.get('chroma_location')`` (ffprobe's stream fields; the
    reference's ``get_video_properties`` dict does not carry them): absent,
    'unknown' or 'unspecified' is 'tv' / 'left'; a chroma location other than
    left / topleft (center, top, bottomleft, bottom) is not modelled and raises
    ValueError.  The decode argv does not change: the pipe's ``-pix_fmt`` is
    the source's own family, so the codes pass through as they are.

    properties: the reference's ``get_video_properties`` dict
    (src/utils.py:1040-1058): width, height, bit_depth, color_transfer.
    hdr: ``_probe_hdr_metadata`` output (src/utils.py:329-372). Inside
    ffmpeg, vf_tonemap reads MaxCLL from frame side data. Raw pipes drop side
    data, so it is passed to libh2s explicitly here.
    dovi: for a Dolby Vision profile 5 source, the RPU's numbers from
    elsewhere (ffprobe frame side data, an RPU tool): one ``dovi.DoviRpu`` for
    every frame, or a callable ``dovi(first_frame, count) -> list[DoviRpu]``
    that the run loop asks per batch (``Tonemapper.set_dovi``).  The
    reference's argv for such a source is always a libplacebo chain
    (src/ffmpeg_command.py:96-144); any other chain raises ValueError.  The
    unspecified ``color_transfer`` such streams carry is not an error: the
    kernels ignore the transfer once records are set.

    scale: None, or the (box_w, box_h) box of a smaller deliverable (a 4K
    master as 1080p: ``scale=(1920, 1080)``).  The out size is ``scaled_size``
    of the source in that box; the encode pipe carries frames of that size
    (``-s``, ``frame_bytes_out``) and the run loop converts and resizes each
    batch in one call (``Tonemapper.process_scaled``), with no second pass on
    the CPU.  With None every argv and every byte is as without the argument.

    decimate ('cpu' | 'gpu'): where a libplacebo plan's 4:2:2 / 4:4:4 source
    (``in_subsampling`` given, or 'auto' from ffprobe's ``pix_fmt``) becomes the
    4:2:0 that the branch tone-maps.  'cpu' (the default: every argv and byte as
    without the argument): the decode side's swscale, per frame, as above.
    'gpu': the decode pipe keeps the source's own ``-pix_fmt`` (yuv422p1Xle /
    yuv444p1Xle), the plan carries ``decimate='gpu'`` and the run loop sets the
    context's 4:2:0 front-end (``Tonemapper.set_input_decimation('bicubic')``;
    'off' for every other plan), so the chroma decimation runs on the device in
    front of the conversion.  A
    CPU-chain plan ignores it (it reads the source natively); a 4:2:0 source
    needs none.  A semi-planar 4:2:2 / 4:4:4 decode pipe stays refused: the
    software decode pipe is planar.

    Raises ValueError for an argv without a tone-map filter graph, and for a
    Dolby Vision profile 5 source without ``dovi`` (its RPU cannot cross the
    pipe)."""
    argv = list(argv)
    p5 = is_dovi_profile5(properties)
    if p5 and dovi is None:
        # src/ffmpeg_command.py:100-106: profile 5 needs the RPU libplacebo
        # applies; the rawvideo decode pipe drops it
        raise ValueError(DOVI_P5_ERROR)
    if dovi is not None and not p5:
        raise ValueError('dovi= is for a Dolby Vision profile 5 source (properties: is_dolby_vision, dovi_profile 5)')
    if '-i' not in argv or '-filter_complex' not in argv:
        raise ValueError('argv has no -i / -filter_complex: not a build() conversion command')
    exe = argv[0]
    i_in = argv.index('-i')
    input_path = argv[i_in + 1]
    i_fc = argv.index('-filter_complex')
    chain = argv[i_fc + 1]
    rest = argv[i_fc + 2:]
    # drop '-map [vout]' (the filter graph's output pad)
    out: 'list[str]' = []
    k = 0
    while k < len(rest):
        tok = rest[k]
        if tok == '-map' and k + 1 < len(rest) and rest[k + 1].startswith('['):
            k += 2
            continue
        if tok == '-map' and k + 1 < len(rest):
            out += [tok, _remap_input(rest[k + 1])]
            k += 2
            continue
        if tok == '-map_metadata' and k + 1 < len(rest):
            out += [tok, _remap_input(rest[k + 1])]
            k += 2
            continue
        out.append(tok)
        k += 1
    if '-pix_fmt' not in out:
        raise ValueError('argv has no -pix_fmt for the output')
    enc_pix_fmt = out[out.index('-pix_fmt') + 1]
    if enc_pix_fmt not in OUT_PIX_FMT_BITS:
        raise ValueError(f'unsupported output pix_fmt {enc_pix_fmt!r}')
    bits_out = OUT_PIX_FMT_BITS[enc_pix_fmt]
    bits_in = int(properties.get('bit_depth') or 10)
    if bits_in not in (10, 12):
        raise ValueError(f'{bits_in}-bit sources are not HDR10/HLG inputs')
    trc = properties.get('color_transfer', '') or ''
    if p5 and trc not in TRANSFERS:
        trc = ''      # profile 5 streams are tagged unspecified / unknown; the records define the decode
    if trc not in TRANSFERS:
        raise ValueError(f'unsupported source transfer {trc!r} (expected smpte2084 or arib-std-b67)')
    extra: 'dict[str, Any]' = {}
    if hdr:
        if hdr.get('maxcll'):
            extra['maxcll'] = float(hdr['maxcll'])
        if hdr.get('mastering_max'):
            extra['mastering_max'] = float(hdr['mastering_max'])
    params, lut_path = parse_filter_chain(chain, bits_in=bits_in, bits_out=bits_out,
                                          transfer=TRANSFERS[trc], mode=mode, **extra)
    if p5 and params.resolved_pipeline() != 'libplacebo':
        raise ValueError('a Dolby Vision profile 5 source converts on the libplacebo branch only; '
                         'this argv carries the CPU chain (the reference shows wrong colours there)')
    W, H = int(properties['width']), int(properties['height'])
    fps = out[out.index('-r') + 1] if '-r' in out else str(properties.get('frame_rate', 24.0))
    # output path = last positional before the optional trailing -y
    o_idx = len(out) - 2 if out and out[-1] == '-y' else len(out) - 1
    output_path = out[o_idx]
    encode_opts = out[:o_idx] + BT709_TAGS + out[o_idx:]
    for name in (in_layout, out_layout):
        if name not in ('planar', 'semi', 'auto'):
            raise ValueError(f"layout must be 'planar', 'semi' or 'auto', got {name!r}")
    if in_layout == 'auto':
        in_layout = 'planar'
    if in_subsampling not in ('420', '422', '444', 'auto'):
        raise ValueError(f"in_subsampling must be '420', '422', '444' or 'auto', got {in_subsampling!r}")
    if in_subsampling == 'auto':
        in_subsampling = SOURCE_SUBSAMPLING.get(str(properties.get('pix_fmt') or ''), '420')
    if decimate not in ('cpu', 'gpu'):
        raise ValueError(f"decimate must be 'cpu' or 'gpu', got {decimate!r}")
    if params.resolved_pipeline() != 'libplacebo' or in_subsampling == '420':
        decimate = 'cpu'           # nothing to decimate in front of the chain
    if params.resolved_pipeline() == 'libplacebo' and decimate == 'cpu':
        in_subsampling = '420'     # format=p010,hwupload: the reference's own 4:2:0
    if in_subsampling != '420' and in_layout == 'semi':
        raise ValueError('4:2:2 / 4:4:4 decode pipes are planar only (no p210 / p410)')
    if in_range not in ('tv', 'pc', 'auto'):
        raise ValueError(f"in_range must be 'tv', 'pc' or 'auto', got {in_range!r}")
    if in_chroma_location not in ('left', 'topleft', 'auto'):
        raise ValueError(f"in_chroma_location must be 'left', 'topleft' or 'auto', got {in_chroma_location!r}")
    if in_range == 'auto':
        tag = str(properties.get('color_range') or '')
        if tag not in SOURCE_RANGE:
            raise ValueError(f'unsupported source color_range {tag!r} (expected tv or pc)')
        in_range = SOURCE_RANGE[tag]
    if in_chroma_location == 'auto':
        tag = str(properties.get('chroma_location') or '')
        if tag not in SOURCE_CHROMA_LOCATION:
            raise ValueError(f'source chroma_location {tag!r} is not modelled (left and topleft are)')
        in_chroma_location = SOURCE_CHROMA_LOCATION[tag]
    if out_layout == 'auto':
        out_layout = 'semi' if enc_pix_fmt == 'p010le' else 'planar'
    pipe_in = (PIPE_PIX_FMT_SEMI if in_layout == 'semi' else PIPE_PIX_FMT)[bits_in]
    if in_subsampling != '420':
        pipe_in = PIPE_PIX_FMT_SUB[in_subsampling][bits_in]
    pipe_out = (PIPE_PIX_FMT_SEMI if out_layout == 'semi' else PIPE_PIX_FMT)[bits_out]
    decode = [exe, '-loglevel', 'error', '-nostdin', '-i', input_path, '-map', '0:v:0',
              '-f', 'rawvideo', '-pix_fmt', pipe_in, '-']
    OW, OH = (W, H) if scale is None else scaled_size(W, H, scale[0], scale[1])
    encode = [exe, '-loglevel', 'info', '-f', 'rawvideo', '-pix_fmt', pipe_out, '-s', f'{OW}x{OH}',
              '-r', fps, '-i', '-', '-i', input_path, '-map', '0:v:0'] + encode_opts
    return PipePlan(decode=decode, encode=encode, params=params, lut_path=lut_path, width=W, height=H,
                    input_path=input_path, output_path=output_path, reference_argv=argv,
                    in_layout=in_layout, layout=out_layout, in_subsampling=in_subsampling,
                    in_range=in_range, in_chroma_location=in_chroma_location, dovi=dovi,
                    out_width=OW, out_height=OH, decimate=decimate)


def _read_full(stream: Any, buf: memoryview) -> int:
    """Fill buf from a pipe; returns bytes read (short only at EOF)."""
    got = 0
    while got < len(buf):
        n = stream.readinto(buf[got:])
        if not n:
            break
        got += n
    return got


class H2SProcess:
    """Popen-shaped handle of a decode -> libh2s -> encode conversion.

    ``stderr`` is the encoder's stderr as text lines. ffmpeg prints its
    ``time=`` progress there, as it does for the reference's single process
    (src/conversion.py:225-240). ``returncode`` is the encoder's, or the
    decoder's when that failed, or 1 when the GPU stage raised (``error``
    holds the exception)."""

    def __init__(self, plan: PipePlan, tonemapper: Any, batch: int = 8,
                 popen: Callable[..., Any] = subprocess.Popen, depth: int = 2):
        from .frames import FrameBatch
        self.plan = plan
        self.error: Optional[BaseException] = None
        self._tm = tonemapper
        self._batch = max(1, int(batch))
        self.dec = popen(plan.decode, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, stdin=subprocess.DEVNULL)
        self.enc = popen(plan.encode, stdin=subprocess.PIPE, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
        self.stderr = io.TextIOWrapper(self.enc.stderr, encoding='utf-8', errors='replace')
        p = plan.params
        # the 4:2:0 front-end of the libplacebo branch, on the device; off for every other plan, so a context
        # that served such a plan reads a later plan's 4:2:2 / 4:4:4 source natively again
        # (a tonemapper object without the setting has nothing to switch off)
        if plan.decimate == 'gpu':
            tonemapper.set_input_decimation('bicubic')
        elif hasattr(tonemapper, 'set_input_decimation'):
            tonemapper.set_input_decimation('off')
        # page-locked staging: the pipe bytes go straight to / from HBM by DMA.
        # `depth` input slots let the decoder run ahead while the GPU stage
        # and the encoder work on earlier batches.
        self._src = [FrameBatch.empty_pinned(self._batch, plan.width, plan.height, p.bits_in, plan.in_layout,
                                             plan.in_subsampling, plan.in_range, plan.in_chroma_location)
                     for _ in range(max(1, int(depth)))]
        self._dst = FrameBatch.empty_pinned(self._batch, plan.out_width, plan.out_height, p.bits_out, plan.layout)
        self._free: 'queue.Queue[Optional[int]]' = queue.Queue()
        self._filled: 'queue.Queue[Optional[Tuple[int, int]]]' = queue.Queue()
        for i in range(len(self._src)):
            self._free.put(i)
        self.frames = 0
        self._reader = threading.Thread(target=self._read, name='h2s-read', daemon=True)
        self._thread = threading.Thread(target=self._pump, name='h2s-pump', daemon=True)
        self._reader.start()
        self._thread.start()

    def _fail(self, e: BaseException) -> None:
        """GPU / pipe failure: record the first error and stop both ends."""
        if self.error is None:
            self.error = e
        for p in (self.dec, self.enc):
            try:
                p.kill()
            except Exception:
                pass

    def _read(self) -> None:
        """Decoder pipe -> free input slots, in order (one batch per slot)."""
        fin = self.plan.frame_bytes_in
        try:
            while True:
                slot = self._free.get()
                if slot is None:          # the pump stopped
                    return
                mv = memoryview(self._src[slot].buf).cast('B')
                got = _read_full(self.dec.stdout, mv)
                if got // fin:
                    self._filled.put((slot, got // fin))
                if got < len(mv):
                    return
        except BaseException as e:
            self._fail(e)
        finally:
            self._filled.put(None)

    def _pump(self) -> None:
        """Filled slots -> libh2s -> encoder pipe, in decode order."""
        fout = self.plan.frame_bytes_out
        dst_mv = memoryview(self._dst.buf).cast('B')
        try:
            while True:
                item = self._filled.get()
                if item is None:
                    break
                slot, n = item
                if self.plan.dovi is not None:   # this batch's records (frames self.frames .. + n)
                    from .dovi import resolve_records
                    self._tm.set_dovi(resolve_records(self.plan.dovi, self.frames, n))
                if self.plan.scaled:             # convert and resize in one call
                    self._tm.process_scaled(self._src[slot], self._dst, nframes=n)
                else:
                    self._tm.process(self._src[slot], self._dst, nframes=n)   # synchronous for host frames
                self._free.put(slot)
                self.enc.stdin.write(dst_mv[:n * fout])
                self.frames += n
        except BaseException as e:
            self._fail(e)
        finally:
            self._free.put(None)          # release a reader waiting for a slot
            try:
                self.enc.stdin.close()
            except Exception:
                pass

    # ---- Popen surface -----------------------------------------------------
    @property
    def returncode(self) -> 'int | None':
        rc = self.enc.poll()
        if rc is None or self._thread.is_alive():
            return None
        if self.error is not None:
            return 1
        drc = self.dec.poll()
        if drc not in (None, 0):
            return drc
        return rc

    def poll(self) -> 'int | None':
        return self.returncode

    def wait(self, timeout: 'float | None' = None) -> int:
        self._thread.join(timeout)
        self._reader.join(timeout)
        self.enc.wait(timeout)
        self.dec.wait(timeout)
        rc = self.returncode
        assert rc is not None
        return rc

    def terminate(self) -> None:
        for p in (self.dec, self.enc):
            p.terminate()

    def kill(self) -> None:
        for p in (self.dec, self.enc):
            p.kill()


class RgbReader:
    """Iterator over a planned source as R'G'B' tensors on the device: it runs
    only the plan's decode pipe and yields ``tonemapper.process_rgb(...)`` of
    each batch of decoded frames (the last one short), in decode order.  For a
    torch pipeline on the same card, a thumbnail or storyboard writer, a QC
    tool: no encoder, no second pass on the CPU.

    ``rgb_kw`` goes to ``Tonemapper.process_rgb`` (dtype, layout, mean, std,
    size, stream); a plan with a ``scale=`` box delivers that size unless
    ``size`` says otherwise.  Each yielded tensor is a fresh allocation unless
    ``out`` is given, in which case the consumer must be done with it before
    asking for the next batch.  The decode-side reader and its ``depth`` pinned
    input slots are H2SProcess's: the decoder runs ahead while the consumer
    works.  A slot is free again when process_rgb returns (a host batch is
    staged before it does).

    A decode failure (the child's non-zero exit) or a GPU error ends the
    iteration with the error raised; the child is reaped on ``close()`` and on
    exhaustion.  Also a context manager."""

    def __init__(self, plan: PipePlan, tonemapper: Any, batch: int = 8, depth: int = 2,
                 popen: Callable[..., Any] = subprocess.Popen, **rgb_kw: Any):
        from .frames import FrameBatch
        self.plan = plan
        self.error: Optional[BaseException] = None
        self.frames = 0
        self._tm = tonemapper
        self._batch = max(1, int(batch))
        self._kw = dict(rgb_kw)
        if plan.scaled and 'size' not in self._kw and 'out' not in self._kw:
            self._kw['size'] = (plan.out_width, plan.out_height)
        self._closed = False
        self.dec = popen(plan.decode, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, stdin=subprocess.DEVNULL)
        # (as H2SProcess: the libplacebo branch's 4:2:0 front-end, off for every other plan)
        if plan.decimate == 'gpu':
            tonemapper.set_input_decimation('bicubic')
        elif hasattr(tonemapper, 'set_input_decimation'):
            tonemapper.set_input_decimation('off')
        p = plan.params
        self._src = [FrameBatch.empty_pinned(self._batch, plan.width, plan.height, p.bits_in, plan.in_layout,
                                             plan.in_subsampling, plan.in_range, plan.in_chroma_location)
                     for _ in range(max(1, int(depth)))]
        self._free: 'queue.Queue[Optional[int]]' = queue.Queue()
        self._filled: 'queue.Queue[Optional[Tuple[int, int]]]' = queue.Queue()
        for i in range(len(self._src)):
            self._free.put(i)
        self._reader = threading.Thread(target=self._read, name='h2s-rgb-read', daemon=True)
        self._reader.start()

    _read = H2SProcess._read      # decoder pipe -> free input slots, in order

    def _fail(self, e: BaseException) -> None:
        if self.error is None:
            self.error = e
        try:
            self.dec.kill()
        except Exception:
            pass

    def __iter__(self) -> 'RgbReader':
        return self

    def __next__(self) -> Any:
        if self._closed:
            raise StopIteration
        item = self._filled.get()
        if item is None:               # the decoder's pipe ended (or the reader failed)
            self._shutdown(kill=False)
            if self.error is not None:
                raise self.error
            if self.dec.returncode not in (0, None):
                self.error = RuntimeError(f'the decode pipe failed with exit code {self.dec.returncode}')
                raise self.error
            raise StopIteration
        slot, n = item
        try:
            if self.plan.dovi is not None:   # this batch's records (frames self.frames .. + n)
                from .dovi import resolve_records
                self._tm.set_dovi(resolve_records(self.plan.dovi, self.frames, n))
            out = self._tm.process_rgb(self._src[slot], nframes=n, **self._kw)
        except BaseException as e:
            self._fail(e)
            self.close()
            raise
        self._free.put(slot)
        self.frames += n
        return out

    def close(self) -> None:
        """Stop the reader and reap the decode child (idempotent)."""
        self._shutdown(kill=True)

    def _shutdown(self, kill: bool) -> None:
        if self._closed:
            return
        self._closed = True
        self._free.put(None)           # release a reader waiting for a slot
        if kill and self.dec.poll() is None:
            try:
                self.dec.kill()        # (closed early: the reader may be blocked on the pipe)
            except Exception:
                pass
        self._reader.join()
        self.dec.wait()
        try:
            self.dec.stdout.close()
        except Exception:
            pass

    def __enter__(self) -> 'RgbReader':
        return self

    def __exit__(self, *exc: Any) -> None:
        self.close()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


@dataclass
class LadderPlan:
    """A rendition ladder from one source: ``rungs[i]`` is the PipePlan of
    rung i (its own encode argv, output path and size), ``decode`` the one
    decode argv they share."""
    rungs: 'list[PipePlan]'
    decode: 'list[str]'

    @property
    def params(self) -> TonemapParams:
        return self.rungs[0].params

    @property
    def lut_path(self) -> 'str | None':
        return self.rungs[0].lut_path

    @property
    def frame_bytes_in(self) -> int:
        return self.rungs[0].frame_bytes_in

    @property
    def sizes(self) -> 'list[Tuple[int, int]]':
        return [(r.out_width, r.out_height) for r in self.rungs]


# what every rung of a ladder must agree on: one decoder, one conversion
_LADDER_SHARED = ('input_path', 'decode', 'params', 'lut_path', 'width', 'height', 'in_layout', 'layout',
                  'in_subsampling', 'in_range', 'in_chroma_location', 'decimate')


def plan_ladder(argvs: 'list[list[str]]', properties: 'dict[str, Any]',
                boxes: 'list[Tuple[int, int] | None]', **kw: Any) -> LadderPlan:
    """The plans of a rendition ladder (a 4K master as 2160p, 1080p, 720p and
    360p SDR files) that one decoder and one conversion per frame serve.

    ``argvs[i]`` is the reference's own ``build()`` argv for rung i (its own
    output path and rate arguments), ``boxes[i]`` that rung's ``scale=`` box,
    or None for the source's size; ``kw`` goes to ``plan_from_argv``
    unchanged.  ``rungs[i]`` is ``plan_from_argv(argvs[i], properties,
    scale=boxes[i], **kw)`` field for field.  The rungs must agree on the input
    path, the decode argv, the parameters, the LUT path, the layouts and the
    source's form (what one decode pipe and one ``Tonemapper.process_ladder``
    call per batch can serve): a ValueError names the first rung and field
    that differ from rung 0."""
    argvs, boxes = list(argvs), list(boxes)
    if not argvs:
        raise ValueError('a ladder needs at least one rung')
    if len(argvs) != len(boxes):
        raise ValueError(f'{len(argvs)} argvs but {len(boxes)} boxes: one box (or None) per rung')
    from . import _abi
    if len(argvs) > _abi.LADDER_MAX:
        raise ValueError(f'a ladder has at most {_abi.LADDER_MAX} rungs, got {len(argvs)}')
    if 'scale' in kw:
        raise ValueError('scale= is per rung: pass boxes')
    rungs = [plan_from_argv(a, properties, scale=b, **kw) for a, b in zip(argvs, boxes)]
    for i, r in enumerate(rungs[1:], 1):
        for name in _LADDER_SHARED:
            a, b = getattr(r, name), getattr(rungs[0], name)
            if (repr(a) != repr(b)) if name == 'params' else (a != b):    # (params holds NaN defaults)
                raise ValueError(f'rung {i}: {name} differs from rung 0 ({a!r} != {b!r})')
    return LadderPlan(rungs=rungs, decode=list(rungs[0].decode))


class H2SLadderProcess:
    """Popen-shaped handle of a decode -> libh2s -> one encoder per rung
    conversion: H2SProcess with several encode pipes.  One decoder feeds the
    pinned input slots, each batch takes one ``process_ladder`` call, and each
    rung's pinned batch is then written to its encoder's stdin, in rung order
    (one writer thread per encoder is not built: a slow encoder holds the
    others back).

    ``stderr`` is rung 0's encoder's stderr as text lines (the others' are
    discarded).  ``returncode`` is None while anything runs, then 1 when the
    GPU stage raised (``error`` holds the exception), else the first non-zero
    code among the encoders, in rung order, and the decoder, else 0."""

    def __init__(self, plan: LadderPlan, tonemapper: Any, batch: int = 8,
                 popen: Callable[..., Any] = subprocess.Popen, depth: int = 2):
        from .frames import FrameBatch
        self.plan = plan
        self.error: Optional[BaseException] = None
        self._tm = tonemapper
        self._batch = max(1, int(batch))
        first = plan.rungs[0]
        self.dec = popen(plan.decode, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, stdin=subprocess.DEVNULL)
        self.encs = [popen(r.encode, stdin=subprocess.PIPE, stdout=subprocess.DEVNULL,
                           stderr=subprocess.PIPE if i == 0 else subprocess.DEVNULL)
                     for i, r in enumerate(plan.rungs)]
        self.stderr = io.TextIOWrapper(self.encs[0].stderr, encoding='utf-8', errors='replace')
        p = plan.params
        # (as H2SProcess: the libplacebo branch's 4:2:0 front-end, off for every other plan)
        if first.decimate == 'gpu':
            tonemapper.set_input_decimation('bicubic')
        elif hasattr(tonemapper, 'set_input_decimation'):
            tonemapper.set_input_decimation('off')
        self._src = [FrameBatch.empty_pinned(self._batch, first.width, first.height, p.bits_in, first.in_layout,
                                             first.in_subsampling, first.in_range, first.in_chroma_location)
                     for _ in range(max(1, int(depth)))]
        self._dsts = [FrameBatch.empty_pinned(self._batch, r.out_width, r.out_height, p.bits_out, r.layout)
                      for r in plan.rungs]
        self._free: 'queue.Queue[Optional[int]]' = queue.Queue()
        self._filled: 'queue.Queue[Optional[Tuple[int, int]]]' = queue.Queue()
        for i in range(len(self._src)):
            self._free.put(i)
        self.frames = 0
        self._reader = threading.Thread(target=self._read, name='h2s-ladder-read', daemon=True)
        self._thread = threading.Thread(target=self._pump, name='h2s-ladder-pump', daemon=True)
        self._reader.start()
        self._thread.start()

    _read = H2SProcess._read      # decoder pipe -> free input slots, in order

    def _fail(self, e: BaseException) -> None:
        """GPU / pipe failure: record the first error and stop every process."""
        if self.error is None:
            self.error = e
        for p in [self.dec] + self.encs:
            try:
                p.kill()
            except Exception:
                pass

    def _pump(self) -> None:
        """Filled slots -> libh2s -> every encoder pipe, in decode order."""
        fouts = [r.frame_bytes_out for r in self.plan.rungs]
        mvs = [memoryview(d.buf).cast('B') for d in self._dsts]
        dovi = self.plan.rungs[0].dovi
        try:
            while True:
                item = self._filled.get()
                if item is None:
                    break
                slot, n = item
                if dovi is not None:             # this batch's records (frames self.frames .. + n)
                    from .dovi import resolve_records
                    self._tm.set_dovi(resolve_records(dovi, self.frames, n))
                self._tm.process_ladder(self._src[slot], self._dsts, nframes=n)   # synchronous for host frames
                self._free.put(slot)
                for enc, mv, fout in zip(self.encs, mvs, fouts):
                    enc.stdin.write(mv[:n * fout])
                self.frames += n
        except BaseException as e:
            self._fail(e)
        finally:
            self._free.put(None)          # release a reader waiting for a slot
            for enc in self.encs:
                try:
                    enc.stdin.close()
                except Exception:
                    pass

    # ---- Popen surface -----------------------------------------------------
    @property
    def returncode(self) -> 'int | None':
        codes = [enc.poll() for enc in self.encs]
        if any(rc is None for rc in codes) or self._thread.is_alive():
            return None
        if self.error is not None:
            return 1
        for rc in codes + [self.dec.poll()]:
            if rc not in (None, 0):
                return rc
        return 0

    def poll(self) -> 'int | None':
        return self.returncode

    def wait(self, timeout: 'float | None' = None) -> int:
        self._thread.join(timeout)
        self._reader.join(timeout)
        for p in self.encs + [self.dec]:
            p.wait(timeout)
        rc = self.returncode
        assert rc is not None
        return rc

    def terminate(self) -> None:
        for p in [self.dec] + self.encs:
            p.terminate()

    def kill(self) -> None:
        for p in [self.dec] + self.encs:
            p.kill()


def start(plan: PipePlan, device: int = 0, batch: int = 8, lattice: 'np.ndarray | None' = None,
          popen: Callable[..., Any] = subprocess.Popen) -> H2SProcess:
    """Launch a planned conversion on ``device`` (the GPU replacement of
    ``start_ffmpeg_process(cmd)``, src/conversion.py:209-224)."""
    from . import lut as _lut
    from .engine import Tonemapper
    tm = Tonemapper(device, plan.params)
    if plan.params.lut_enabled:
        if lattice is not None:
            tm.set_lut(lattice)
        elif plan.lut_path and plan.lut_path != '<LUT>':
            tm.load_cube(_lut.unescape_filter_path(plan.lut_path))
        else:
            tm.set_lut(_lut.generate_lattice(_lut.LUT_SIZE))
    return H2SProcess(plan, tm, batch=batch, popen=popen)
