#!/usr/bin/env python3
"""Kernel time of the C2 and C3 workloads with untagged, full-range and
top-left input (h2s_set_input_tags), alternated within one process so that the
three share the box's state:

  C2   3840x2160, 64 device-resident frames, hable + 65^3 LUT + gamma 2.2, 10 -> 10
  C3   3840x2160, 16 frames, BT.2390 on the libplacebo branch, 10 -> 10

The inputs are one buffer read three ways, (tv, left), (pc, left) and (tv,
topleft), and three controls.  The tags change how the samples are read, so
the outputs are different pictures; what is compared before anything is timed
is that each tagged output differs from the untagged one (the tag reached the
kernel) and that the route is the untagged one's.  Full range runs the same
kernels with other constants; the share of tiles that lose the tile kernel's
branch-free body is reported for both ranges (tiles holding a luma code above
the bound or a chroma code beyond it).  Its control is "twin":
the limited-range buffer that normalises to the full-range reading's values
(codes 64 + 876 y / 1023 and 512 + 896 (c - 512) / 1023, rounded), read (tv,
left): the same picture through the same kernel, so what is left between the
(pc, left) row and it is the constants, and what is left between it and the
(tv, left) row is the picture.  Top-left runs the SUB 3 instances: the same
loads and staging, another vertical combine; they are SEMI instances (either
side may be semi-planar), where a planar (tv, left) launch runs the planar
ones, so its controls are both sitings on the semi-planar repack of the
buffer, which run the SEMI instances of either siting.

Every input is warmed up, then ROUNDS rounds visit the inputs in turn,
LAUNCHES timed launches each (h2s_kernel_ms: HIP events around the call's
launches on its stream).  One JSON line per workload and input: the median over
rounds, the per-round values, their min / max and the ratio to the (tv, left)
row.

  python scripts/bench_source_tags.py [--rounds 4] [--launches 5] [--workloads C2,C3]
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
    'C3': (dict(tonemapper='bt.2390', gamma=1.0, bits_in=10, bits_out=10), 16),
}
# (color_range, chroma_location, layout, source buffer)
INPUTS = (('tv', 'left', 'planar', 'base'), ('pc', 'left', 'planar', 'base'), ('tv', 'left', 'planar', 'twin'),
          ('tv', 'topleft', 'planar', 'base'), ('tv', 'left', 'semi', 'base'), ('tv', 'topleft', 'semi', 'base'))


def limited_twin(base):
    """The limited-range batch whose normalised values are the full-range reading's of base (10 bit)."""
    import torch

    import hdr2sdr
    out = hdr2sdr.FrameBatch(torch.empty_like(base.buf), base.width, base.height, base.bits)
    out.y.copy_(torch.round(64 + base.y.double() * (876 / 1023)).to(out.buf.dtype))
    for name in ('u', 'v'):
        getattr(out, name).copy_(torch.round(512 + (getattr(base, name).double() - 512) * (896 / 1023)).to(out.buf.dtype))
    return out


def slow_tile_share(src, full):
    """Share of the 64 x 32 tiles (chroma halo included) that hold a sample
    outside the branch-free body's bound for 10-bit input: limited range
    |c - 512| <= 448 and Y' <= 0.933 (code 881); full range |c - 512| <= 475,
    any luma code."""
    import torch
    y = src.y.to(torch.int32)
    c = torch.maximum((src.u.to(torch.int32) - 512).abs(), (src.v.to(torch.int32) - 512).abs())
    F, H, W = y.shape
    ty = torch.nn.functional.max_pool2d(y.float()[:, None], (32, 64), ceil_mode=True)[:, 0]
    # a tile's chroma window: rows cy0 - 1 .. cy0 + 16, columns cx0 .. cx0 + 32
    cp = torch.nn.functional.pad(c.float()[:, None], (0, 1, 1, 1), mode='replicate')
    tc = torch.nn.functional.max_pool2d(cp, (18, 33), stride=(16, 32), ceil_mode=True)[:, 0][:, :ty.shape[1], :ty.shape[2]]
    slow = (tc > 475) if full else ((tc > 448) | (ty > 881))
    return float(slow.float().mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--launches', type=int, default=5, help='timed launches per input and round')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--width', type=int, default=3840)
    ap.add_argument('--height', type=int, default=2160)
    ap.add_argument('--lut', type=int, default=65)
    ap.add_argument('--workloads', default='C2,C3')
    ap.add_argument('--frames', type=int, default=0, help='override the workloads\' frame counts')
    args = ap.parse_args()
    if args.rounds * args.launches < 20:
        ap.error('at least 20 timed launches per input (rounds x launches)')

    import torch

    import hdr2sdr
    from hdr2sdr.synth import synth_frames

    dev = torch.device('cuda', 0)
    W, H = args.width, args.height
    lattice = hdr2sdr.generate_lattice(args.lut)
    stream = torch.cuda.current_stream(dev)
    for name in args.workloads.split(','):
        kw, nframes = WORKLOADS[name]
        nframes = args.frames or nframes
        params = hdr2sdr.TonemapParams(**kw)
        tm = hdr2sdr.Tonemapper(0, params, lattice)
        base = synth_frames('smooth', nframes, W, H, params.bits_in, device=dev, seed=0x5EED)
        bufs = {'base': base, 'twin': limited_twin(base)}
        semi = {k: b.to_layout('semi') for k, b in bufs.items()}
        src = {t: hdr2sdr.FrameBatch((semi if t[2] == 'semi' else bufs)[t[3]].buf, W, H, params.bits_in, t[2], '420', t[0], t[1])
               for t in INPUTS}
        dst = hdr2sdr.FrameBatch.empty_torch(nframes, W, H, params.bits_out, dev)
        paths = {t: tm.query_path(src[t], dst) for t in INPUTS}
        slow = {t: slow_tile_share(bufs[t[3]], t[0] == 'pc') for t in INPUTS}

        want, differs = None, {}
        for t in INPUTS:                # warm-up, and the outputs against the untagged input's
            dst.buf.zero_()
            for _ in range(args.warmup):
                tm.process(src[t], dst, stream)
            torch.cuda.synchronize(dev)
            if want is None:
                want = dst.buf.clone()
            differs[t] = not bool(torch.equal(dst.buf, want))
        series = {t: [] for t in INPUTS}
        tm.set_timing(True)
        for _ in range(args.rounds):
            for t in INPUTS:
                tm.kernel_ms(0)
                for _ in range(args.launches):
                    tm.process(src[t], dst, stream)
                torch.cuda.synchronize(dev)
                series[t].append(tm.kernel_ms(args.launches))
        tm.set_timing(False)
        ref = statistics.median(series[INPUTS[0]])
        for t, v in series.items():
            med = statistics.median(v)
            print(json.dumps({'workload': name, 'color_range': t[0], 'chroma_location': t[1], 'layout': t[2],
                              'buffer': t[3], 'path': paths[t],
                              'frames': nframes, 'size': f'{W}x{H}', 'kernel_ms_median': round(med, 4),
                              'kernel_ms_min': round(min(v), 4), 'kernel_ms_max': round(max(v), 4),
                              'vs_tv_left': round(med / ref, 4), 'mpx_s': round(nframes * W * H / med / 1e3, 1),
                              'tiles_off_the_fast_body': round(slow[t], 4), 'output_differs_from_untagged': differs[t],
                              'launches': args.rounds * args.launches,
                              'kernel_ms_rounds': [round(x, 4) for x in v]}), flush=True)
        tm.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
