#!/usr/bin/env python3
"""Time of the 4:2:0 front-end (h2s_set_input_decimation) for a batch of
device-resident 3840x2160 10-bit frames:

  kernel       k_decimate420 alone, 4:2:2 and 4:4:4, planar and semi-planar, from
               the timing record (h2s_set_timing: HIP events around the launch),
               beside a device-to-device hipMemcpyAsync of half the bytes the
               kernel reads plus writes (the same traffic), timed with HIP
               events in the same run
  whole call   h2s_process on C3's parameters with peak_detect (BT.2390 on the
               libplacebo branch, 65^3 LUT, 10-bit output) with a 4:2:0 source,
               and with 4:2:2 and 4:4:4 sources through the front-end

Every whole call is asynchronous on the device; a host clock runs around
--calls calls and one synchronisation.  Each variant is warmed up (--warmup
calls), then --rounds rounds visit the variants in turn.

--process-only times the 4:2:0 whole call alone (for a tree without the
feature: --tree names a built checkout of the parent commit).

Writes a markdown table to stdout (and to --out).

  python scripts/time_decimate.py [--rounds 5] [--calls 20] [--warmup 20] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORMS = (('422', 'planar'), ('422', 'semi'), ('444', 'planar'), ('444', 'semi'))


def chroma_bytes(W, H, sub):
    """(bytes the front-end reads, bytes it writes) per frame."""
    return 2 * (W if sub == '444' else W // 2) * H * 2, 2 * (W // 2) * (H // 2) * 2


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20, help='timed calls per variant and round')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--width', type=int, default=3840)
    ap.add_argument('--height', type=int, default=2160)
    ap.add_argument('--hbm', type=float, default=6.29, help='measured HBM rate, TB/s')
    ap.add_argument('--process-only', action='store_true')
    ap.add_argument('--tree', default=REPO, help='the checkout whose built package is timed (with --process-only: '
                                                 'the parent commit\'s)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.rounds * args.calls < 100 or args.warmup < 20:
        ap.error('at least 20 warm-up and 100 timed calls per variant')

    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), 'hdr-to-sdr_amd'))
    import numpy as np
    import torch

    import hdr2sdr
    from hdr2sdr.synth import synth_frames

    if not torch.cuda.is_available():
        raise RuntimeError('the timing needs a GPU (no fallback)')
    W, H, n = args.width, args.height, args.frames
    if n > 16:
        ap.error('one chunk: at most 16 frames')
    params = hdr2sdr.TonemapParams(tonemapper='bt.2390', gamma=1.0, bits_in=10, bits_out=10, peak_detect=True,
                                   maxcll=4000.0)
    tm = hdr2sdr.Tonemapper(0, params, hdr2sdr.generate_lattice(65))
    one = synth_frames('smooth', 1, W, H, 10, device='cuda:0', seed=0x5EED)
    src420 = hdr2sdr.FrameBatch(one.buf.repeat(n, 1), W, H, 10)
    dst = hdr2sdr.FrameBatch.empty_torch(n, W, H, 10, 'cuda:0')
    variants = [('4:2:0', lambda: tm.process(src420, dst))]
    sources = {}
    if not args.process_only:
        tm.set_input_decimation('bicubic')
        base = one.to_numpy()
        for sub, layout in FORMS:
            fb = hdr2sdr.FrameBatch.empty_numpy(1, W, H, 10, layout, sub, allow_semi_sub=True)
            sh = 6 if layout == 'semi' else 0
            fb.y[...] = base.y << sh
            # the 4:2:0 frame's chroma, each sample repeated: the conversion behind the front-end sees about
            # the colours of the 4:2:0 call (its lut3d table reads depend on them)
            u, v = (np.repeat(np.repeat(p, 2, axis=1), 1 if sub == '422' else 2, axis=2) for p in (base.u, base.v))
            if layout == 'semi':
                fb.uv[..., 0], fb.uv[..., 1] = u << sh, v << sh
            else:
                fb.u[...], fb.v[...] = u, v
            dev = fb.to_torch('cuda:0')
            sources[(sub, layout)] = hdr2sdr.FrameBatch(dev.buf.repeat(n, 1), W, H, 10, layout, sub, allow_semi_sub=True)
        for sub in ('422', '444'):
            variants.append((f'4:{sub[1]}:{sub[2]} planar, front-end on',
                             lambda s=sources[(sub, 'planar')]: tm.process(s, dst)))
        variants.append(('4:2:0 again', lambda: tm.process(src420, dst)))
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

    nt = args.rounds * args.calls
    lines = [f'{n} device-resident {W}x{H} 10-bit frames per call (BT.2390 on the libplacebo branch, peak_detect, 65^3 '
             f'LUT, 10-bit output), {args.warmup} warm-up and {nt} timed calls per variant ({args.rounds} rounds of '
             f'{args.calls}, variants alternated); ms per call: median, minimum and maximum of the round means.', '',
             '| h2s_process, source | median ms | min | max | ms per frame |', '|---|---|---|---|---|']
    for name, _ in variants:
        v = per_round[name]
        lines.append(f'| {name} | {statistics.median(v):.3f} | {min(v):.3f} | {max(v):.3f} | '
                     f'{statistics.median(v) / n:.4f} |')

    if not args.process_only:
        # the kernel alone (the entry in front of the conversion's) and the copy of the same traffic, alternated
        hip = ctypes.CDLL('libamdhip64.so')
        hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        stream = torch.cuda.current_stream()
        kern = {f: [] for f in FORMS}
        copy = {f: [] for f in FORMS}
        bufs = {}
        for sub, _ in FORMS:
            rd, wr = chroma_bytes(W, H, sub)
            half = (rd + wr) * n // 2
            bufs[sub] = (torch.empty(half, dtype=torch.uint8, device='cuda:0'),
                         torch.empty(half, dtype=torch.uint8, device='cuda:0'), half)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def one_kernel(form):
            """(the front-end's entry, the conversion's entry behind it) of one call."""
            tm.kernel_ms(0)
            tm.process(sources[form], dst)
            conv = tm.kernel_ms(1)
            return tm.kernel_ms(2) * 2 - conv, conv

        def conversion_420():
            tm.kernel_ms(0)
            tm.process(src420, dst)
            return tm.kernel_ms(1)

        def one_copy(form):
            a, b, half = bufs[form[0]]
            ev0.record(stream)
            rc = hip.hipMemcpyAsync(b.data_ptr(), a.data_ptr(), half, 3, stream.cuda_stream)      # device to device
            ev1.record(stream)
            if rc:
                raise RuntimeError(f'hipMemcpyAsync: {rc}')
            ev1.synchronize()
            return ev0.elapsed_time(ev1)

        conv = {f: [] for f in FORMS + ('420',)}
        tm.set_timing(True)
        for i in range(args.warmup + nt):
            c420 = conversion_420()
            if i >= args.warmup:
                conv['420'].append(c420)
            for form in FORMS:
                (k, cv), c = one_kernel(form), one_copy(form)
                if i >= args.warmup:
                    kern[form].append(k), copy[form].append(c), conv[form].append(cv)
        tm.set_timing(False)
        lines += ['', f'k_decimate420 alone, from the timing record, and a device-to-device hipMemcpyAsync of half the '
                  f'bytes it reads plus writes, from HIP events; {args.warmup} warm-up and {nt} timed launches each, '
                  f'alternated; ms (median, minimum, maximum).  HBM {args.hbm} TB/s.', '',
                  '| source | k_decimate420 ms | min | max | bytes read + written | TB/s | of HBM | copy ms | min | max | '
                  'kernel / copy |', '|---|---|---|---|---|---|---|---|---|---|---|']
        for form in FORMS:
            rd, wr = chroma_bytes(W, H, form[0])
            by = (rd + wr) * n
            mk, mc = statistics.median(kern[form]), statistics.median(copy[form])
            tbs = by / (mk * 1e-3) / 1e12
            lines.append(f'| 4:{form[0][1]}:{form[0][2]} {form[1]} | {mk:.3f} | {min(kern[form]):.3f} | {max(kern[form]):.3f} | '
                         f'{by} | {tbs:.2f} | {tbs / args.hbm:.0%} | {mc:.3f} | {min(copy[form]):.3f} | '
                         f'{max(copy[form]):.3f} | {mk / mc:.2f} |')
        lines += ['', 'The conversion behind the front-end, from the same calls\' timing record (the entry of the statistics, '
                  'finish and tile launches), beside that of a 4:2:0 source; ms (median, minimum, maximum).', '',
                  '| source | conversion entry ms | min | max |', '|---|---|---|---|']
        for form in ('420',) + FORMS:
            name = '4:2:0' if form == '420' else f'4:{form[0][1]}:{form[0][2]} {form[1]}'
            v = conv[form]
            lines.append(f'| {name} | {statistics.median(v):.3f} | {min(v):.3f} | {max(v):.3f} |')
    tm.close()
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
