#!/usr/bin/env python3
"""Kernel time of the four frame-layout combinations (planar / semi-planar on
each side, h2s_set_frame_layout) on the bench workloads, alternated within
one process so that they share the box's state:

  C2      3840x2160, 64 device-resident frames, hable + 65^3 LUT + gamma 2.2, 10 -> 10
  C3_dyn  3840x2160, 16 frames, BT.2390 on the libplacebo branch with peak_detect

Per workload: every combination is warmed up, then ROUNDS rounds visit the
combinations in turn, LAUNCHES timed launches each (h2s_kernel_ms: HIP events
around the call's launches on its stream).  One JSON line per combination:
the median over rounds, the per-round values and their min / max.  The semi
rows' yardstick is the planar row of the same run (the algorithmic bytes are
the same 6 B/px); outputs are checked equal to the repacked planar result
before anything is timed.

  python scripts/bench_layouts.py [--rounds 4] [--launches 5] [--workloads C2,C3_dyn]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'hdr-to-sdr_amd'))

WORKLOADS = {
    'C2': (dict(tonemapper='hable', gamma=2.2, bits_in=10, bits_out=10), 64),
    'C3_dyn': (dict(tonemapper='bt.2390', gamma=1.0, bits_in=10, bits_out=10, peak_detect=True, maxcll=4000.0), 16),
}
COMBOS = [('planar', 'planar'), ('semi', 'semi'), ('planar', 'semi'), ('semi', 'planar')]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--launches', type=int, default=5, help='timed launches per combination and round')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--width', type=int, default=3840)
    ap.add_argument('--height', type=int, default=2160)
    ap.add_argument('--lut', type=int, default=65)
    ap.add_argument('--workloads', default='C2,C3_dyn')
    ap.add_argument('--frames', type=int, default=0, help='override the workloads\' frame counts')
    args = ap.parse_args()
    if args.rounds * args.launches < 20:
        ap.error('at least 20 timed launches per combination (rounds x launches)')

    import torch

    import hdr2sdr
    from hdr2sdr.synth import synth_frames

    dev = torch.device('cuda', 0)
    lattice = hdr2sdr.generate_lattice(args.lut)
    W, H = args.width, args.height
    for name in args.workloads.split(','):
        kw, nframes = WORKLOADS[name]
        nframes = args.frames or nframes
        params = hdr2sdr.TonemapParams(**kw)
        tm = hdr2sdr.Tonemapper(0, params, lattice)
        stream = torch.cuda.current_stream(dev)
        src = {'planar': synth_frames('smooth', nframes, W, H, params.bits_in, device=dev, seed=0x5EED)}
        src['semi'] = src['planar'].to_layout('semi')
        dst = {l: hdr2sdr.FrameBatch.empty_torch(nframes, W, H, params.bits_out, dev, l) for l in ('planar', 'semi')}

        def launch(il, ol):
            if params.peak_detect:
                tm.reset_peak()
            tm.process(src[il], dst[ol], stream)

        want = None
        for il, ol in COMBOS:       # warm-up, and the outputs against planar -> planar
            dst[ol].buf.zero_()
            for _ in range(args.warmup):
                launch(il, ol)
            torch.cuda.synchronize(dev)
            got = dst[ol].to_layout('planar').buf
            if want is None:
                want = got.clone()
            elif not torch.equal(got, want):
                raise SystemExit(f'{name} {il}->{ol}: output differs from planar->planar')
        series = {c: [] for c in COMBOS}
        tm.set_timing(True)
        for _ in range(args.rounds):
            for il, ol in COMBOS:
                tm.kernel_ms(0)
                for _ in range(args.launches):
                    launch(il, ol)
                torch.cuda.synchronize(dev)
                series[(il, ol)].append(tm.kernel_ms(args.launches))
        tm.set_timing(False)
        base = statistics.median(series[COMBOS[0]])
        for (il, ol), v in series.items():
            med = statistics.median(v)
            print(json.dumps({'workload': name, 'in': il, 'out': ol, 'frames': nframes, 'size': f'{W}x{H}',
                              'kernel_ms_median': round(med, 4), 'kernel_ms_min': round(min(v), 4),
                              'kernel_ms_max': round(max(v), 4), 'vs_planar': round(med / base, 4),
                              'mpx_s': round(nframes * W * H / med / 1e3, 1),
                              'launches': args.rounds * args.launches,
                              'kernel_ms_rounds': [round(x, 4) for x in v]}), flush=True)
        tm.close()
        del src, dst
        torch.cuda.empty_cache()
    return 0


if __name__ == '__main__':
    sys.exit(main())
