#!/usr/bin/env python3
"""Time of the RGB tensor output (h2s_process_rgb) for a batch of
device-resident 3840x2160 10-bit frames on C2's parameters (hable, gamma 2.2,
65^3 LUT), at 3840x2160, 1920x1080 and 640x360 (--sizes picks others):

  process            h2s_process alone (full-size 4:2:0 output), 10-bit output
  rgb DTYPE/LAYOUT   h2s_process_rgb, uint8 / hwc and float16 / chw, per size
  copy               a device-to-device copy of k_rgb420's read-plus-write
                     byte count (half of it copied: read once, written once)
  preview            h2s_preview_rgb24_batch to device RGB at display gamma 1,
                     on a second context with bits_out 8 (the preview's depth),
                     and `rgb8 uint8/hwc`: h2s_process_rgb on that context, so
                     the two are compared on the same frames and sizes
  process again      h2s_process once more: the run-to-run spread of unchanged code
  kernel             per size and form, from the timing record
                     (h2s_set_timing): k_rgb420 alone, as a multiple of the copy

Every variant is warmed up (--warmup calls), then --rounds rounds visit the
variants in turn; a round times --calls calls between two HIP events on the
stream.  The preview is synchronous by itself; the others are queued.

--process-only times h2s_process alone (for a tree or a library without the
feature: H2S_LIB=<the parent commit's libh2s.so> gives the parent's number).

Writes a markdown table to stdout (and to --out).

  python scripts/time_rgb.py [--rounds 5] [--calls 20] [--warmup 20] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'hdr-to-sdr_amd'))

SIZES = ((3840, 2160), (1920, 1080), (640, 360))
FORMS = (('uint8', 'hwc'), ('float16', 'chw'))
ELEM = {'uint8': 1, 'float16': 2, 'bfloat16': 2, 'float32': 4}


def rgb_traffic(ow, oh, dtype, scratch_bps, n):
    """Bytes k_rgb420 reads (the planar 4:2:0 scratch at the target size) and writes (the tensor)."""
    return (ow * oh * 3 // 2 * scratch_bps + ow * oh * 3 * ELEM[dtype]) * n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20, help='timed calls per variant and round')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--width', type=int, default=3840)
    ap.add_argument('--height', type=int, default=2160)
    ap.add_argument('--tonemapper', default='hable')
    ap.add_argument('--sizes', default=','.join(f'{w}x{h}' for w, h in SIZES), help='WxH,WxH,...')
    ap.add_argument('--process-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in b.split('x')) for b in args.sizes.split(',')]
    if args.rounds * args.calls < 100 or args.warmup < 20:
        ap.error('at least 20 warm-up and 100 timed calls per variant')

    import torch

    import hdr2sdr
    from hdr2sdr import _abi
    from hdr2sdr.synth import synth_frames

    if not torch.cuda.is_available():
        raise RuntimeError('the timing needs a GPU (no fallback)')
    W, H, n = args.width, args.height, args.frames
    if n > 16:
        ap.error('at most 16 frames: one chunk, so that the timing record has one k_rgb420 entry per call')
    lattice = hdr2sdr.generate_lattice(65)

    def params(bits_out):
        return hdr2sdr.TonemapParams(tonemapper=args.tonemapper, gamma=2.2, bits_in=10, bits_out=bits_out)

    tm = hdr2sdr.Tonemapper(0, params(10), lattice)
    one = synth_frames('smooth', 1, W, H, 10, device='cuda:0', seed=0x5EED)
    src = hdr2sdr.FrameBatch(one.buf.repeat(n, 1), W, H, 10)
    full = hdr2sdr.FrameBatch.empty_torch(n, W, H, 10, 'cuda:0')
    variants = [('process', lambda: tm.process(src, full))]
    kernel_of = {}            # variant name -> (context, call, traffic bytes)
    tm8 = None
    if not args.process_only:
        tm8 = hdr2sdr.Tonemapper(0, params(8), lattice)
        L = _abi.lib()
        d = src.descriptor()

        def shape(ow, oh, layout):
            return (n, 3, oh, ow) if layout == 'chw' else (n, oh, ow, 3)

        for ow, oh in sizes:
            for dtype, layout in FORMS:
                out = torch.empty(shape(ow, oh, layout), dtype=getattr(torch, dtype), device='cuda:0')
                name = f'rgb {dtype}/{layout} {ow}x{oh}'
                fn = (lambda o=out, dt=dtype, lo=layout: tm.process_rgb(src, out=o, dtype=dt, layout=lo))
                variants.append((name, fn))
                by = rgb_traffic(ow, oh, dtype, 2, n)
                kernel_of[name] = (tm, fn, by)
                a, b = (torch.empty(by // 2, dtype=torch.uint8, device='cuda:0') for _ in range(2))
                variants.append((f'copy of {name}', lambda a=a, b=b: b.copy_(a)))
            rgb8 = torch.empty(shape(ow, oh, 'hwc'), dtype=torch.uint8, device='cuda:0')
            prev = torch.empty_like(rgb8)

            def preview(o=prev, ow=ow, oh=oh):
                tm8._use_layouts(src)
                tm8._check(L.h2s_preview_rgb24_batch(tm8._ctx, ctypes.byref(d), n, o.data_ptr(), 3 * ow, 3 * ow * oh,
                                                     ow, oh, 1.0, _abi.LOC_DEVICE, tm8._stream_ptr(None)))
            name8 = f'rgb8 uint8/hwc {ow}x{oh}'
            fn8 = (lambda o=rgb8: tm8.process_rgb(src, out=o, dtype='uint8', layout='hwc'))
            variants.append((f'preview {ow}x{oh}', preview))
            variants.append((name8, fn8))
            kernel_of[name8] = (tm8, fn8, rgb_traffic(ow, oh, 'uint8', 1, n))
            # the two agree: byte for byte at the source's size, within 1 where the planes were resized
            preview()
            fn8()
            torch.cuda.synchronize()
            diff = (prev.int() - rgb8.int()).abs()
            if int(diff.max()) > (0 if (ow, oh) == (W, H) else 1):
                raise AssertionError(f'h2s_process_rgb differs from the preview at {ow}x{oh}: max {int(diff.max())}')
    variants.append(('process again', lambda: tm.process(src, full)))

    for _, fn in variants:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
    per_round = {name: [] for name, _ in variants}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.rounds):
        for name, fn in variants:
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(args.calls):
                fn()
            ev1.record()
            ev1.synchronize()
            per_round[name].append(ev0.elapsed_time(ev1) / args.calls)

    # the timing record: the last entry of an h2s_process_rgb call is its k_rgb420 launch
    kernels = {}
    for name, (ctx, fn, by) in kernel_of.items():
        ctx.set_timing(True)
        ms = []
        for _ in range(args.calls):
            ctx.kernel_ms(0)
            fn()
            ms.append(ctx.kernel_ms(1))
        ctx.set_timing(False)
        kernels[name] = (ms, by)
    tm.close()
    if tm8 is not None:
        tm8.close()

    nt = args.rounds * args.calls
    lines = [f'{n} device-resident {W}x{H} 10-bit frames per call ({args.tonemapper}, gamma 2.2, 65^3 LUT; 10-bit '
             f'output, `preview` and `rgb8` on a second context with 8-bit output), {args.warmup} warm-up and {nt} '
             f'timed calls per variant ({args.rounds} rounds of {args.calls}, variants alternated, HIP events around '
             'each round); ms per call: median, minimum and maximum of the round means.', '',
             '| call | median ms | min | max | ms per frame |', '|---|---|---|---|---|']
    for name, _ in variants:
        v = per_round[name]
        lines.append(f'| {name} | {statistics.median(v):.3f} | {min(v):.3f} | {max(v):.3f} | '
                     f'{statistics.median(v) / n:.4f} |')
    if kernels:
        lines += ['', f'k_rgb420 alone, from the timing record, {args.calls} calls per form; ms per call (median, '
                  'minimum, maximum).  Bytes: the planar 4:2:0 scratch at the target size read once, the tensor '
                  'written once.  `x copy`: against the device-to-device copy of the same read-plus-write byte '
                  'count above (`rgb8`: against the copy of its byte count scaled from the uint8/hwc one).', '',
                  '| form | k_rgb420 ms | min | max | bytes per call | TB/s | x copy |', '|---|---|---|---|---|---|---|']
        for name, (ms, by) in kernels.items():
            med = statistics.median(ms)
            ref_name = name if name.startswith('rgb ') else name.replace('rgb8 ', 'rgb ')
            copy_ms = statistics.median(per_round[f'copy of {ref_name}'])
            copy_ms *= by / kernel_of[ref_name][2]
            lines.append(f'| {name} | {med:.4f} | {min(ms):.4f} | {max(ms):.4f} | {by} | '
                         f'{by / (med * 1e-3) / 1e12:.2f} | {med / copy_ms:.2f} |')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
