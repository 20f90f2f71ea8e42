#!/usr/bin/env python3
"""Kernel time of the C2 workload with 4:2:0, 4:2:2 and 4:4:4 input
(h2s_set_input_subsampling), alternated within one process so that the three
share the box's state:

  C2   3840x2160, 64 device-resident frames, hable + 65^3 LUT + gamma 2.2, 10 -> 10

The 4:2:2 and 4:4:4 sources are the exact upsamples of the 4:2:0 one (chroma
codes rounded to multiples of 8, then the S1 passes in integers), so all three
convert the same picture and their outputs are compared before anything is
timed: the tile kernel stages exact integers in every form.  Every input is
warmed up, then ROUNDS rounds visit the inputs in turn, LAUNCHES timed
launches each (h2s_kernel_ms: HIP events around the call's launches on its
stream).  One JSON line per input: the median over rounds, the per-round
values, their min / max, the ratio to the 4:2:0 row and the algorithmic bytes
per pixel (6, 7, 9 at 10 -> 10).

  python scripts/bench_subsampling.py [--rounds 4] [--launches 5]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'hdr-to-sdr_amd'))

SUBS = ('420', '422', '444')
BYTES_PER_PX = {'420': 6, '422': 7, '444': 9}     # 16-bit samples in, 4:2:0 16-bit samples out


def upsampled(src, sub, dev):
    """The exact 4:2:2 / 4:4:4 upsample of a 4:2:0 torch batch whose chroma
    codes are multiples of 8 (zimg edge rule), built on the device."""
    import torch

    import hdr2sdr
    out = hdr2sdr.FrameBatch.empty_torch(src.nframes, src.width, src.height, src.bits, dev, 'planar', sub)
    out.y.copy_(src.y)
    for name in ('u', 'v'):
        c = getattr(src, name).to(torch.int32)
        ch, cw = c.shape[1], c.shape[2]
        m = torch.arange(ch, device=dev)
        v = torch.empty((c.shape[0], 2 * ch, cw), dtype=torch.int32, device=dev)
        v[:, 0::2] = (c[:, (m - 1).abs()] + 3 * c) // 4
        v[:, 1::2] = (3 * c + c[:, (m + 1).clamp(max=ch - 1)]) // 4
        if sub == '444':
            k = torch.arange(cw, device=dev)
            h = torch.empty((c.shape[0], 2 * ch, 2 * cw), dtype=torch.int32, device=dev)
            h[:, :, 0::2] = v
            h[:, :, 1::2] = (v + v[:, :, (k + 1).clamp(max=cw - 1)]) // 2
            v = h
        getattr(out, name).copy_(v.to(out.buf.dtype))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--launches', type=int, default=5, help='timed launches per input and round')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--width', type=int, default=3840)
    ap.add_argument('--height', type=int, default=2160)
    ap.add_argument('--lut', type=int, default=65)
    ap.add_argument('--frames', type=int, default=64)
    args = ap.parse_args()
    if args.rounds * args.launches < 20:
        ap.error('at least 20 timed launches per input (rounds x launches)')

    import torch

    import hdr2sdr
    from hdr2sdr.synth import synth_frames

    dev = torch.device('cuda', 0)
    W, H, nframes = args.width, args.height, args.frames
    params = hdr2sdr.TonemapParams(tonemapper='hable', gamma=2.2, bits_in=10, bits_out=10)
    tm = hdr2sdr.Tonemapper(0, params, hdr2sdr.generate_lattice(args.lut))
    stream = torch.cuda.current_stream(dev)
    base = synth_frames('smooth', nframes, W, H, params.bits_in, device=dev, seed=0x5EED)
    for p in (base.u, base.v):      # chroma to multiples of 8: the upsamples below are exact
        p.copy_(((p.to(torch.int32) + 4) // 8 * 8).to(p.dtype))
    src = {'420': base, '422': upsampled(base, '422', dev), '444': upsampled(base, '444', dev)}
    dst = hdr2sdr.FrameBatch.empty_torch(nframes, W, H, params.bits_out, dev)
    paths = {s: tm.query_path(src[s], dst) for s in SUBS}

    want, equal = None, {}
    for s in SUBS:                  # warm-up, and the outputs against the 4:2:0 input's
        dst.buf.zero_()
        for _ in range(args.warmup):
            tm.process(src[s], dst, stream)
        torch.cuda.synchronize(dev)
        if want is None:
            want = dst.buf.clone()
        equal[s] = bool(torch.equal(dst.buf, want))
    series = {s: [] for s in SUBS}
    tm.set_timing(True)
    for _ in range(args.rounds):
        for s in SUBS:
            tm.kernel_ms(0)
            for _ in range(args.launches):
                tm.process(src[s], dst, stream)
            torch.cuda.synchronize(dev)
            series[s].append(tm.kernel_ms(args.launches))
    tm.set_timing(False)
    ref = statistics.median(series['420'])
    for s, v in series.items():
        med = statistics.median(v)
        print(json.dumps({'workload': 'C2', 'in_subsampling': s, 'path': paths[s], 'frames': nframes,
                          'size': f'{W}x{H}', 'kernel_ms_median': round(med, 4), 'kernel_ms_min': round(min(v), 4),
                          'kernel_ms_max': round(max(v), 4), 'vs_420': round(med / ref, 4),
                          'bytes_per_px': BYTES_PER_PX[s], 'bytes_vs_420': round(BYTES_PER_PX[s] / 6, 4),
                          'gb_s': round(nframes * W * H * BYTES_PER_PX[s] / med / 1e6, 1),
                          'output_equals_420': equal[s], 'launches': args.rounds * args.launches,
                          'kernel_ms_rounds': [round(x, 4) for x in v]}), flush=True)
    tm.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
