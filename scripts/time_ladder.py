#!/usr/bin/env python3
"""Time of a rendition ladder for a batch of device-resident 3840x2160 10-bit
frames on C2's parameters (hable, gamma 2.2, 65^3 LUT, 10-bit output), rungs
3840x2160, 1920x1080, 1280x720 and 640x360 (--sizes picks others; the first
must be the source's size):

  ladder           one h2s_process_ladder call
  separate         the calls it replaces, on the same frames: h2s_process and
                   one h2s_process_scaled per smaller rung
  process          h2s_process alone
  scaled WxH       h2s_process_scaled to the second rung alone
  process again    h2s_process once more: the run-to-run spread of unchanged code
  kernel           from the timing record (h2s_set_timing) of the ladder calls:
                   the conversion entry and one entry per rung
  repack           k_repack420 alone (the ladder's source-size rung), planar ->
                   planar and planar -> p010le, beside a device-to-device
                   hipMemcpyAsync of half the bytes it reads plus writes (the
                   same traffic), timed with HIP events in the same run

Every call is asynchronous on the device; a host clock runs around --calls
calls and one synchronisation.  Each variant is warmed up (--warmup calls),
then --rounds rounds visit the variants in turn.  Before anything is timed,
every rung of the ladder is compared with its separate call, byte for byte.

The decodes and uploads a ladder call saves a transcode box are not part of
this: every variant reads the same device-resident frames.

Writes a markdown table to stdout (and to --out).

  python scripts/time_ladder.py [--rounds 5] [--calls 20] [--warmup 20] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'hdr-to-sdr_amd'))
sys.path.insert(0, os.path.join(REPO, 'tests'))       # padded_frames.RowPadded: the source-size rung's reference

SIZES = ((3840, 2160), (1920, 1080), (1280, 720), (640, 360))


def row(name, v, n=None):
    per = '' if n is None else f' {statistics.median(v) / n:.4f} |'
    return f'| {name} | {statistics.median(v):.3f} | {min(v):.3f} | {max(v):.3f} |{per}'


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20, help='timed calls per variant and round')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--tonemapper', default='hable')
    ap.add_argument('--sizes', default=','.join(f'{w}x{h}' for w, h in SIZES), help='WxH,WxH,... (the source size first)')
    ap.add_argument('--hbm', type=float, default=6.29, help='measured HBM rate, TB/s')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in b.split('x')) for b in args.sizes.split(',')]
    if args.rounds * args.calls < 100 or args.warmup < 20:
        ap.error('at least 20 warm-up and 100 timed calls per variant')
    if len(sizes) < 2 or args.frames > 16:
        ap.error('at least two rungs, and one chunk: at most 16 frames')

    import numpy as np
    import torch

    import hdr2sdr
    from hdr2sdr.synth import synth_frames
    from padded_frames import RowPadded

    if not torch.cuda.is_available():
        raise RuntimeError('the timing needs a GPU (no fallback)')
    (W, H), n = sizes[0], args.frames
    params = hdr2sdr.TonemapParams(tonemapper=args.tonemapper, gamma=2.2, bits_in=10, bits_out=10)
    lattice = hdr2sdr.generate_lattice(65)
    tm = hdr2sdr.Tonemapper(0, params, lattice)       # the ladder's context
    sep = hdr2sdr.Tonemapper(0, params, lattice)      # the separate calls'
    one = synth_frames('smooth', 1, W, H, 10, device='cuda:0', seed=0x5EED)
    src = hdr2sdr.FrameBatch(one.buf.repeat(n, 1), W, H, 10)
    rungs = [hdr2sdr.FrameBatch.empty_torch(n, w, h, 10, 'cuda:0') for w, h in sizes]
    outs = [hdr2sdr.FrameBatch.empty_torch(n, w, h, 10, 'cuda:0') for w, h in sizes]

    def separate():
        sep.process(src, outs[0])
        for d in outs[1:]:
            sep.process_scaled(src, d)

    # every rung is its separate call's bytes (the source-size rung: h2s_process into rows 16 bytes apart, as the
    # scratch's are; a tight 3840-wide batch has such rows)
    tm.process_ladder(src, rungs)
    separate()
    padded = RowPadded(n, W, H, 10, align=16)
    sep.process(src, padded)
    torch.cuda.synchronize()
    if not np.array_equal(rungs[0].to_numpy().buf, padded.to_numpy().buf):
        raise AssertionError('the source-size rung differs from h2s_process')
    del padded
    for r, o, size in zip(rungs[1:], outs[1:], sizes[1:]):
        if not np.array_equal(r.to_numpy().buf, o.to_numpy().buf):
            raise AssertionError(f'rung {size} differs from h2s_process_scaled')

    second = f'scaled {sizes[1][0]}x{sizes[1][1]}'
    variants = [('ladder', lambda: tm.process_ladder(src, rungs)),
                ('separate', separate),
                ('process', lambda: sep.process(src, outs[0])),
                (second, lambda: sep.process_scaled(src, outs[1])),
                ('process again', lambda: sep.process(src, outs[0]))]
    for _, fn in variants:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
    per_round = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            per_round[name].append((time.perf_counter() - t0) / args.calls * 1e3)

    # the timing record of a ladder call: the conversion entry, then one entry per rung in rung order
    nt = args.rounds * args.calls
    entries = [[] for _ in range(1 + len(sizes))]
    tm.set_timing(True)
    for _ in range(nt):
        tm.kernel_ms(0)
        tm.process_ladder(src, rungs)
        total = [tm.kernel_ms(k) * k for k in range(1, len(entries) + 1)]        # the newest k entries
        newest_first = [total[0]] + [total[k] - total[k - 1] for k in range(1, len(total))]
        for e, v in zip(entries, newest_first[::-1]):
            e.append(v)
    tm.set_timing(False)

    # k_repack420 alone: a two-rung ladder of the source's size twice is one conversion and two repack launches
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream()
    frame = W * H * 3 // 2 * 2
    a = torch.empty(frame * n, dtype=torch.uint8, device='cuda:0')
    b = torch.empty(frame * n, dtype=torch.uint8, device='cuda:0')
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kern, copy = {}, {}
    tm.set_timing(True)
    for layout in ('planar', 'semi'):
        twice = [hdr2sdr.FrameBatch.empty_torch(n, W, H, 10, 'cuda:0', layout) for _ in range(2)]
        kern[layout], copy[layout] = [], []
        for i in range(args.warmup + nt):
            tm.kernel_ms(0)
            tm.process_ladder(src, twice)
            k = tm.kernel_ms(1)
            ev0.record(stream)
            rc = hip.hipMemcpyAsync(b.data_ptr(), a.data_ptr(), frame * n, 3, stream.cuda_stream)    # device to device
            ev1.record(stream)
            if rc:
                raise RuntimeError(f'hipMemcpyAsync: {rc}')
            ev1.synchronize()
            if i >= args.warmup:
                kern[layout].append(k), copy[layout].append(ev0.elapsed_time(ev1))
        del twice
    tm.set_timing(False)
    tm.close()
    sep.close()

    med = {name: statistics.median(v) for name, v in per_round.items()}
    sizes_s = ', '.join(f'{w}x{h}' for w, h in sizes)
    lines = [f'{n} device-resident {W}x{H} 10-bit frames per call ({args.tonemapper}, gamma 2.2, 65^3 LUT, 10-bit '
             f'output), rungs {sizes_s}; {args.warmup} warm-up and {nt} timed calls per variant ({args.rounds} rounds '
             f'of {args.calls}, variants alternated); ms per call: median, minimum and maximum of the round means.', '',
             '| call | median ms | min | max | ms per frame |', '|---|---|---|---|---|']
    for name, _ in variants:
        lines.append(row(name, per_round[name], n))
    saved = med['separate'] - med['ladder']
    lines += ['', f'ladder / separate = {med["ladder"] / med["separate"]:.3f}; the ladder saves {saved:.3f} ms of the '
              f'{(len(sizes) - 1) * med["process"]:.3f} ms that {len(sizes) - 1} x h2s_process take '
              f'({saved / ((len(sizes) - 1) * med["process"]):.0%}).', '',
              f'From the timing record of {nt} ladder calls (HIP events around each launch group); ms (median, minimum, '
              'maximum).', '', '| entry | median ms | min | max |', '|---|---|---|---|']
    names = ['conversion'] + [f'rung {i} {w}x{h} ({"k_repack420" if (w, h) == (W, H) else "k_scale420"})'
                              for i, (w, h) in enumerate(sizes)]
    for name, e in zip(names, entries):
        lines.append(row(name, e))
    lines.append(f'| sum of the entries | {sum(statistics.median(e) for e in entries):.3f} | | |')
    lines += ['', f'k_repack420 alone, from the timing record, and a device-to-device hipMemcpyAsync of the same traffic '
              f'({frame * n} bytes read and as many written), from HIP events; {args.warmup} warm-up and {nt} timed '
              f'launches each, alternated; ms (median, minimum, maximum).  HBM {args.hbm} TB/s.', '',
              '| rung layout | k_repack420 ms | min | max | bytes read + written | TB/s | of HBM | copy ms | min | max | '
              'kernel / copy |', '|---|---|---|---|---|---|---|---|---|---|---|']
    for layout, label in (('planar', 'planar -> planar'), ('semi', 'planar -> p010le')):
        mk, mc = statistics.median(kern[layout]), statistics.median(copy[layout])
        tbs = 2 * frame * n / (mk * 1e-3) / 1e12
        lines.append(f'| {label} | {mk:.3f} | {min(kern[layout]):.3f} | {max(kern[layout]):.3f} | {2 * frame * n} | '
                     f'{tbs:.2f} | {tbs / args.hbm:.0%} | {mc:.3f} | {min(copy[layout]):.3f} | {max(copy[layout]):.3f} | '
                     f'{mk / mc:.2f} |')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
