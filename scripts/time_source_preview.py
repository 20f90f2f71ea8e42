#!/usr/bin/env python3
"""Latency of the preview's two panes for one 3840x2160 10-bit frame, at the
boxes 3840x2160, 1280x720 and 960x540 (--boxes picks others), from a host
(pinned) frame and from a device frame:

  original()   the source pane, h2s_preview_source_rgb24_batch (one kernel)
  convert()    the converted pane, h2s_preview_rgb24_batch (at 1280x720: 4K -> 720p)
  pair()       both, from one upload of the frame
  kernel       k_source_rgb24 alone (HIP events around the launch: h2s_set_timing)

Every call is synchronous and returns host RGB, so a host clock around it is
the call's latency.  Each variant is warmed up (--warmup calls), then --rounds
rounds visit the variants in turn, --calls timed calls each; convert() is
visited twice per round ("convert", "convert again"), which shows the
run-to-run spread of unchanged code within the session.  Before anything is
timed, pair() is compared with original() and convert() byte for byte.

Writes a markdown table to stdout (and to --out).

  python scripts/time_source_preview.py [--rounds 5] [--calls 20] [--warmup 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'hdr-to-sdr_amd'))

BOXES = ((3840, 2160), (1280, 720), (960, 540))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20, help='timed calls per variant and round')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--width', type=int, default=3840)
    ap.add_argument('--height', type=int, default=2160)
    ap.add_argument('--tonemapper', default='hable')
    ap.add_argument('--boxes', default=','.join(f'{w}x{h}' for w, h in BOXES), help='WxH,WxH,...')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.rounds * args.calls < 100 or args.warmup < 20:
        ap.error('at least 20 warm-up and 100 timed calls per variant')

    import numpy as np
    import torch

    import hdr2sdr
    from hdr2sdr.synth import synth_frames

    if not torch.cuda.is_available():
        raise RuntimeError('the timing needs a GPU (no fallback)')
    W, H = args.width, args.height
    src = synth_frames('smooth', 1, W, H, 10, seed=0x5EED).to_numpy()
    host = hdr2sdr.FrameBatch.empty_pinned(1, W, H, 10)
    host.buf[...] = src.buf
    dev = host.to_torch('cuda:0')
    pv = hdr2sdr.Previewer(0, tonemapper=args.tonemapper)
    rows = []
    for box in [tuple(int(v) for v in b.split('x')) for b in args.boxes.split(',')]:
        for where, fb in (('host', host), ('device', dev)):
            o, c = pv.original(fb, *box), pv.convert(fb, *box)
            po, pc = pv.pair(fb, *box)
            if not (np.array_equal(o, po) and np.array_equal(c, pc)):
                raise AssertionError('pair() differs from original() + convert()')
            variants = (('original', lambda: pv.original(fb, *box)), ('convert', lambda: pv.convert(fb, *box)),
                        ('pair', lambda: pv.pair(fb, *box)), ('convert again', lambda: pv.convert(fb, *box)))
            for _, fn in variants:
                for _ in range(args.warmup):
                    fn()
            per_round = {name: [] for name, _ in variants}
            kernel = []
            for _ in range(args.rounds):
                for name, fn in variants:
                    if name == 'original':
                        pv._tm.set_timing(True)
                        pv._tm.kernel_ms(0)
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn()
                    per_round[name].append((time.perf_counter() - t0) / args.calls * 1e3)
                    if name == 'original':
                        kernel.append(pv._tm.kernel_ms(args.calls))
                        pv._tm.set_timing(False)
            per_round['kernel'] = kernel
            for name in ('original', 'convert', 'convert again', 'pair', 'kernel'):
                v = per_round[name]
                rows.append((f'{box[0]}x{box[1]}', where, name, statistics.median(v), min(v), max(v)))
            med = {name: statistics.median(v) for name, v in per_round.items()}
            rows.append((f'{box[0]}x{box[1]}', where, 'original + convert', med['original'] + med['convert'], None, None))
    pv.close()
    n = args.rounds * args.calls
    lines = [f'One {W}x{H} 10-bit frame ({args.tonemapper} + 65^3 LUT for the converted pane), {args.warmup} warm-up and '
             f'{n} timed calls per variant ({args.rounds} rounds of {args.calls}, variants alternated); ms per call: '
             'median, minimum and maximum of the round means.', '',
             '| box | frame | call | median ms | min | max |', '|---|---|---|---|---|---|']
    for box, where, name, med, lo, hi in rows:
        lines.append(f'| {box} | {where} | {name} | {med:.3f} | ' +
                     (f'{lo:.3f} | {hi:.3f} |' if lo is not None else 'sum of the medians | |'))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
