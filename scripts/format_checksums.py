#!/usr/bin/env python3
"""SHA-256 of the output bytes of every frame form the kernels read or write,
for the library H2S_LIB names (default: the tree's): two builds whose lines
are equal convert every form identically.  The suite holds 4:2:2 / 4:4:4 input
to the oracle within a tolerance only, so a change that must not alter a
single output code is held to this instead.  GPU box.

Every case: 3 frames, seed 11, a 17^3 LUT, device sets.  4:2:0 input in all
four layout combinations, 4:2:2 / 4:4:4 input (the exact upsamples of the
4:2:0 source, tests/subsampling_ref.py) into both output layouts.  Sizes: one
tile, 3 x 3 tiles, a bottom tile with 6 live rows, tile + k_process columns,
the generic kernel, and 130x98 / 194x66 with rows padded to 16 bytes (the tile
kernel's interior / border equalities; the hash covers the padding too).
Tagged 4:2:0 input (h2s_set_input_tags: pc / left, tv / topleft, pc / topleft),
planar and semi-planar, into planar output, on TAGGED_CHAINS at the same sizes
(sub field "420-RANGE-LOCATION").
One JSON line: {"chain/kind/WxH/sub/in->out": sha256, ...}, keys sorted.

  [H2S_LIB=/path/to/libh2s.so] python scripts/format_checksums.py [OUT.json]

--debug-planes OUT.npz instead saves the h2s_debug_float planes of stages 1-5
(the tile kernel's debug instances), so that two builds' planes can be compared
value by value: every tests/float_gate.py FLOAT_CFGS entry x edges / smooth,
one frame, planar and semi-planar input, at 64x32, 192x70 and 208x64; keys
"cfg/kind/WxH/layout/stage".

  [H2S_LIB=...] python scripts/format_checksums.py --debug-planes OUT.npz

--preview OUT.json instead hashes the RGB bytes of both preview panes (the
engine-level calls, so that any output size can be asked for), one JSON line
like the first mode's.  Converted pane ("chain/..."): reinhard and bt.2390
with peak detection, a 128x64 source to 128x64 (identity), 64x32, 50x50 and
200x40 (the last two: unequal tap widths on the two axes, either way round),
one frame and a batch of 3, host and device RGB (device: also rows padded by
5 bytes, the hash covers the padding), display gamma 1.0 and 2.2.  Source pane
("source/..."): 10-bit planar 4:2:0 / 4:2:2 / 4:4:4, semi-planar 4:2:0 and
12-bit planar 4:2:0, tv and pc, host and device input, 3 frames; the three
matrices x both RGB models at 128x64 -> 51x25 (odd width: the half pair),
identity and 2x up for bt2020nc / trunc16.

  [H2S_LIB=...] python scripts/format_checksums.py --preview OUT.json

--peak OUT.json instead hashes the dynamic peak's own results, one JSON line:
the raw bytes of h2s_peak_stats's per-frame (measurement, average) of a
3-frame batch ("stats/...") and of peak_state() after reset_peak and one
3-frame process ("state/...").  PQ 10-bit and HLG 12-bit, planar and
semi-planar input, pd_percentile default (histograms) and 100 (none), at one
width per statistics form and heights chosen from the launch geometry: the
default PEAK_BLOCKS = 128 blocks of 256 threads give a thread stride of 32768
units.
  208 wide, PQ: the quad form, 13 units per row pair, 2 in flight.  22688 rows
    are 147472 units, 4.5 strides: every thread runs two in-flight groups (the
    loop's own step is taken), and the threads of the first half stride then
    one unit in the remainder loop, the rest none.
  208 wide, HLG (never quad) and 200 wide (8 | W, not 16): the 8-pixel
    row-chunk form, 26 / 25 chunks per row, 4 in flight.  11142 rows are 289692
    / 278550 chunks, 8.84 / 8.5 strides: every thread runs two groups of four,
    then the threads below 0.84 / 0.5 stride one chunk in the remainder loop.
  204 wide: the 2-byte row form, one row per block and step; 258 rows give
    blocks 0 and 1 a third row.
  64 rows at every width: 416 / 1664 / 1600 units, under one stride, so only
    the remainder loop runs (and half the row form's blocks idle).
A Dolby Vision record set (three luma maps, tests/dovi_ref.py) goes through
the row form at 208x64, planar PQ 10-bit.

  [H2S_LIB=...] python scripts/format_checksums.py --peak OUT.json

--tile-sets OUT.json instead makes one launch per instance of the tile kernel
(tests/tile_sets_ref.py ROWS: each set x its transfers x operators x desat
settings; the Dolby Vision sets with a full-order record): 192x96, 2 frames,
device sets, {"set/transfer/operator/desat": [h2s_query_path, sha256]}; a debug
set's hash is of its stage-5 planes.  Two builds whose lines are equal route
every launch to the same instance: one that took a neighbouring instance
changes bytes or path.

  [H2S_LIB=...] python scripts/format_checksums.py --tile-sets OUT.json
"""
import ctypes
import dataclasses
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'hdr-to-sdr_amd'), REPO, os.path.join(REPO, 'tests')]

NF, SEED, LUT_N = 3, 11, 17
TIGHT = [(64, 32), (192, 96), (192, 70), (208, 64), (70, 34)]
PADDED = [(130, 98), (194, 66)]
# name -> (parameters, content kinds, 4:2:2 / 4:4:4 input too)
CHAINS = {
    'hable_lut_g22': (dict(tonemapper='hable', gamma=2.2, bits_in=10, bits_out=10), ('edges', 'smooth'), True),
    'reinhard_8_dither': (dict(tonemapper='reinhard', bits_out=8, dither='ordered'), ('smooth',), True),
    'mobius_hlg12': (dict(tonemapper='mobius', transfer='arib-std-b67', bits_in=12, bits_out=12), ('smooth',), True),
    'lp_bt2390_peak_detect': (dict(tonemapper='bt.2390', peak_detect=True, maxcll=4000.0), ('smooth',), False),
    'hable_bicubic': (dict(tonemapper='hable', gamma=2.2, chroma_filter='bicubic'), ('smooth',), True),
}
FORMS = [('420', il, ol) for il in ('planar', 'semi') for ol in ('planar', 'semi')] + \
        [(sub, 'planar', ol) for sub in ('422', '444') for ol in ('planar', 'semi')]
TAGGED_CHAINS = ('hable_lut_g22', 'lp_bt2390_peak_detect')
TAGS = [('pc', 'left'), ('tv', 'topleft'), ('pc', 'topleft')]

PREVIEW_SRC = (128, 64)
PREVIEW_SIZES = [(128, 64), (64, 32), (50, 50), (200, 40)]
PREVIEW_CHAINS = {'reinhard': dict(tonemapper='reinhard'), 'bt2390_peak_detect': dict(tonemapper='bt.2390')}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _write(res, path):
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(line + '\n')


def debug_planes(path):
    import hdr2sdr
    from float_gate import FLOAT_CFGS
    from hdr2sdr.synth import synth_frames

    lattice = hdr2sdr.generate_lattice(LUT_N)
    res = {}
    tm = hdr2sdr.Tonemapper(0)
    for name, kw in sorted(FLOAT_CFGS.items()):
        params = hdr2sdr.TonemapParams(**kw)
        tm.set_params(params)
        tm.set_lut(lattice)
        for kind in ('edges', 'smooth'):
            for W, H in [(64, 32), (192, 70), (208, 64)]:
                planar = synth_frames(kind, 1, W, H, params.bits_in, device='cpu', seed=SEED).to_torch('cuda')
                for layout, src in (('planar', planar), ('semi', planar.to_layout('semi'))):
                    for stage in (1, 2, 3, 4, 5):
                        res[f'{name}/{kind}/{W}x{H}/{layout}/{stage}'] = tm.debug_float(src, stage)
    tm.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **res)
    print(f'{len(res)} plane sets -> {path}')
    return 0


def _rgb_hash(call, tm, fb, ow, oh, extra, where, pad=0):
    """One engine-level preview call (h2s_preview_rgb24_batch /
    h2s_preview_source_rgb24_batch) on every frame of fb: the hash of the whole
    RGB buffer, host or device, rows `pad` bytes longer than a row of pixels."""
    import torch
    from hdr2sdr import _abi

    n, ls = fb.nframes, 3 * ow + pad
    fp = ls * oh
    if where == 'host':
        out = np.full(n * fp, 0x55, np.uint8)
        ptr, loc = out.ctypes.data, _abi.LOC_HOST
    else:
        out = torch.full((n * fp,), 0x55, dtype=torch.uint8, device='cuda')
        ptr, loc = out.data_ptr(), _abi.LOC_DEVICE
    tm._use_layouts(fb)
    d = fb.descriptor()
    L = _abi.lib()
    rc = getattr(L, call)(tm._ctx, ctypes.byref(d), n, ptr, ls, fp, ow, oh, *extra, loc, tm._stream_ptr(None))
    if rc:
        _abi.raise_for(rc, L.h2s_last_error(tm._ctx).decode())
    torch.cuda.synchronize()
    return _sha(out if where == 'host' else out.cpu().numpy())


def preview(path):
    import hdr2sdr
    import subsampling_ref as SR
    from hdr2sdr import _abi
    from hdr2sdr.preview import preview_params
    from hdr2sdr.synth import synth_frames

    lattice = hdr2sdr.generate_lattice(LUT_N)
    W, H = PREVIEW_SRC
    res = {}
    tm = hdr2sdr.Tonemapper(0)
    # the converted pane
    src3 = synth_frames('smooth', NF, W, H, 10, device='cpu', seed=SEED).to_numpy()
    for name, kw in PREVIEW_CHAINS.items():
        tm.set_params(preview_params(**kw))
        tm.set_lut(lattice)
        for ow, oh in PREVIEW_SIZES:
            for n in (1, NF):
                fb = src3.slice(0, n).to_torch('cuda')
                for gamma in (1.0, 2.2):
                    for where, pad in (('host', 0), ('device', 0), ('device', 5)):
                        if pad and (n, gamma) != (NF, 1.0):
                            continue
                        res[f'chain/{name}/{W}x{H}->{ow}x{oh}/n{n}/g{gamma}/{where}' + (f'+{pad}' if pad else '')] = \
                            _rgb_hash('h2s_preview_rgb24_batch', tm, fb, ow, oh, (gamma,), where, pad)
    # the source pane
    forms = {}
    fb10 = SR.round8(synth_frames('smooth', NF, W, H, 10, device='cpu', seed=SEED).to_numpy())
    forms['10/420/planar'] = fb10
    forms['10/420/semi'] = fb10.to_layout('semi')
    forms.update({f'10/{s}/planar': b for s, b in SR.exact_inputs(fb10).items()})
    forms['12/420/planar'] = synth_frames('smooth', NF, W, H, 12, device='cpu', seed=SEED).to_numpy()
    cases = [((51, 25), m, r) for m in sorted(_abi.SRC_MATRICES) for r in sorted(_abi.SRC_RGB_MODELS)] + \
            [((W, H), 'bt2020nc', 'trunc16'), ((2 * W, 2 * H), 'bt2020nc', 'trunc16')]
    for form, host in sorted(forms.items()):
        for rng in ('tv', 'pc'):
            tagged = dataclasses.replace(host, color_range=rng)
            for where, fb in (('host', tagged), ('device', tagged.to_torch('cuda'))):
                for (ow, oh), matrix, model in cases:
                    res[f'source/{form}/{rng}/{where}-in/{W}x{H}->{ow}x{oh}/{matrix}/{model}'] = \
                        _rgb_hash('h2s_preview_source_rgb24_batch', tm, fb, ow, oh,
                                  (_abi.SRC_MATRICES[matrix], _abi.SRC_RGB_MODELS[model]), 'host')
    tm.close()
    _write(res, path)
    return 0


PEAK_SOURCES = {'pq10': dict(bits_in=10), 'hlg12': dict(transfer='arib-std-b67', bits_in=12, bits_out=12)}
# (width, source) -> heights: both loops of the form, then the remainder loop alone (the docstring)
PEAK_SIZES = {(208, 'pq10'): (22688, 64), (208, 'hlg12'): (11142, 64), (200, 'pq10'): (11142, 64),
              (200, 'hlg12'): (11142, 64), (204, 'pq10'): (258, 64), (204, 'hlg12'): (258, 64)}


def peak(path):
    import struct

    import dovi_ref as DR
    import torch

    import hdr2sdr
    from hdr2sdr.frames import FrameBatch
    from hdr2sdr.synth import synth_frames

    lattice = hdr2sdr.generate_lattice(LUT_N)
    res = {}
    tm = hdr2sdr.Tonemapper(0)

    def case(key, params, src):
        fmax, favg = tm.peak_stats(src)
        res[f'stats/{key}'] = _sha(np.stack([fmax, favg]))
        dst = FrameBatch.empty_torch(NF, src.width, src.height, params.bits_out, 'cuda', 'planar')
        tm.reset_peak()
        tm.process(src, dst)
        torch.cuda.synchronize()
        st = tm.peak_state()
        res[f'state/{key}'] = hashlib.sha256(struct.pack('<dddq', st['max_pq'], st['avg_pq'], st['peak'],
                                                         st['frames'])).hexdigest()

    for (W, name), heights in sorted(PEAK_SIZES.items()):
        for H in heights:
            planar = synth_frames('smooth', NF, W, H, PEAK_SOURCES[name]['bits_in'], device='cpu', seed=SEED).to_numpy()
            for pct in (None, 100.0):
                kw = dict(PEAK_SOURCES[name], **({} if pct is None else dict(pd_percentile=pct)))
                params = hdr2sdr.TonemapParams(tonemapper='bt.2390', peak_detect=True, maxcll=4000.0, **kw)
                tm.set_params(params)
                tm.set_lut(lattice)
                for layout in ('planar', 'semi'):
                    case(f'{name}/{W}x{H}/{layout}/pct-{"default" if pct is None else pct}', params,
                         planar.to_layout(layout).to_torch('cuda'))
    W, H = 208, 64
    src, recs, _ = DR.luma_map_pair(W, H, 10, NF)
    for pct in (None, 100.0):
        params = hdr2sdr.TonemapParams(tonemapper='bt.2390', peak_detect=True, maxcll=4000.0,
                                       **({} if pct is None else dict(pd_percentile=pct)))
        tm.set_params(params)
        tm.set_lut(lattice)
        tm.set_dovi(recs)
        case(f'dovi-maps/{W}x{H}/planar/pct-{"default" if pct is None else pct}', params, src.to_torch('cuda'))
        tm.set_dovi(None)
    tm.close()
    _write(res, path)
    return 0


def tile_sets(path):
    import tile_sets_ref as TS
    import torch

    import hdr2sdr
    from hdr2sdr.frames import FrameBatch

    lattice = hdr2sdr.generate_lattice(TS.LUT_N)
    record = TS.dovi_record()
    srcs = {name: src.to_torch('cuda') for name, (src, _) in TS.sources(TS.base_source()).items()}
    res = {}
    tm = hdr2sdr.Tonemapper(0)
    for row in TS.ROWS:
        s = row[0]
        tm.set_params(TS.params(row))
        tm.set_lut(lattice)
        tm.set_dovi(record if s.chain == 'dv' else None)
        src = srcs[s.name]
        dst = FrameBatch.empty_torch(TS.NF, TS.W, TS.H, TS.BITS, 'cuda', 'planar' if s.debug else s.layout)
        dst.buf.fill_(0x5555)
        route = tm.query_path(src, dst)
        if s.debug:
            out = tm.debug_float(src, TS.DEBUG_STAGE)
        else:
            tm.process(src, dst)
            torch.cuda.synchronize()
            out = dst.to_numpy().buf
        res[TS.row_id(row)] = [route, _sha(out)]
    tm.set_dovi(None)
    tm.close()
    _write(res, path)
    return 0


def main():
    if len(sys.argv) == 3 and sys.argv[1] == '--peak':
        return peak(sys.argv[2])
    if len(sys.argv) == 3 and sys.argv[1] == '--tile-sets':
        return tile_sets(sys.argv[2])
    if len(sys.argv) == 3 and sys.argv[1] == '--debug-planes':
        return debug_planes(sys.argv[2])
    if len(sys.argv) == 3 and sys.argv[1] == '--preview':
        return preview(sys.argv[2])
    import torch

    import hdr2sdr
    import subsampling_ref as SR
    from hdr2sdr.frames import FrameBatch
    from hdr2sdr.synth import synth_frames
    from padded_frames import RowPadded

    lattice = hdr2sdr.generate_lattice(LUT_N)
    res = {}
    tm = hdr2sdr.Tonemapper(0)
    for name, (kw, kinds, subs) in CHAINS.items():
        params = hdr2sdr.TonemapParams(**kw)
        tm.set_params(params)
        tm.set_lut(lattice)
        for kind in kinds:
            for W, H in TIGHT + PADDED:
                pad = (W, H) in PADDED
                fb = SR.round8(synth_frames(kind, NF, W, H, params.bits_in, device='cpu', seed=SEED).to_numpy())
                host = {('420', 'planar'): fb, ('420', 'semi'): fb.to_layout('semi')}
                if subs:
                    host.update({(s, 'planar'): b for s, b in SR.exact_inputs(fb).items()})
                forms = [(sub, il, ol, 'tv', 'left') for sub, il, ol in FORMS]
                if name in TAGGED_CHAINS:
                    forms += [('420', il, 'planar', rng, loc) for il in ('planar', 'semi') for rng, loc in TAGS]
                for sub, il, ol, rng, loc in forms:
                    if (sub, il) not in host:
                        continue
                    h = host[(sub, il)]
                    if pad:
                        src = RowPadded(NF, W, H, params.bits_in, il, sub).load(h)
                        src.color_range, src.chroma_location = rng, loc
                        dst = RowPadded(NF, W, H, params.bits_out, ol)
                    else:
                        src = dataclasses.replace(h.to_torch('cuda'), color_range=rng, chroma_location=loc)
                        dst = FrameBatch.empty_torch(NF, W, H, params.bits_out, 'cuda', ol)
                        dst.buf.fill_(0x55 if params.bits_out == 8 else 0x5555)
                    if params.peak_detect:
                        tm.reset_peak()
                    tm.process(src, dst)
                    torch.cuda.synchronize()
                    out = dst.raw() if pad else dst.to_numpy().buf
                    tag = sub if (rng, loc) == ('tv', 'left') else f'{sub}-{rng}-{loc}'
                    res[f'{name}/{kind}/{W}x{H}/{tag}/{il}->{ol}'] = _sha(out)
    tm.close()
    if len(sys.argv) > 1:
        _write(res, sys.argv[1])
    else:
        print(json.dumps(res, sort_keys=True))
    return 0


if __name__ == '__main__':
    sys.exit(main())
