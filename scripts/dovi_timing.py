#!/usr/bin/env python3
"""Device time of the Dolby Vision profile-5 front-end beside the HDR10 launch
(profiles/dovi/timing.md).  One process on one box, h2s_kernel_ms around each
launch; the content is C3_dyn's: 16 4K 'smooth' frames, BT.2390, the 65^3 LUT,
peak_detect on.  Measured, round by round so that drift shows:

  * the HDR10 launch of another build of the library (--parent-lib: the parent
    commit's libh2s.so), when given;
  * the HDR10 launch of this tree's library (equal to the parent's within the
    run-to-run spread: the front-end is off by default);
  * the Dolby Vision launch on the tile kernel with the identity record (the
    floor of the front-end's cost: no luma pieces to select, no MMR) and with
    the realistic full-order record of tests/dovi_ref.py (the meaningful one);
  * for scale, the exact path (the generic kernel, H2S_OPT_FAST_PATH 0): the
    HDR10 launch and the realistic record's.

Both libraries are driven through the same few C-ABI calls (ctypes, each
handle with its own symbols), so neither goes through a different host layer.

  python scripts/dovi_timing.py [--parent-lib PATH] [--rounds 3] [--json OUT]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, 'hdr-to-sdr_amd'), os.path.join(REPO, 'tests'), REPO]

W, H, NF, LUT_N = 3840, 2160, 16, 65


class Ctx:
    """One context of one loaded libh2s, through the C-ABI alone."""

    def __init__(self, path, params, lattice):
        from hdr2sdr import _abi
        self.L = L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        L.h2s_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.h2s_destroy.argtypes = [vp]
        L.h2s_last_error.restype, L.h2s_last_error.argtypes = ctypes.c_char_p, [vp]
        L.h2s_set_params.argtypes = [vp, ctypes.POINTER(_abi.H2SParams)]
        L.h2s_set_lut.argtypes = [vp, vp, ctypes.c_int]
        L.h2s_set_option.argtypes = [vp, ctypes.c_int, ctypes.c_int64]
        L.h2s_set_timing.argtypes = [vp, ctypes.c_int]
        L.h2s_kernel_ms.restype, L.h2s_kernel_ms.argtypes = ctypes.c_double, [vp, ctypes.c_int]
        L.h2s_process.argtypes = [vp, ctypes.POINTER(_abi.H2SFrames), ctypes.POINTER(_abi.H2SFrames), ctypes.c_int, vp]
        self.has_dovi = hasattr(L, 'h2s_set_dovi')
        if self.has_dovi:
            L.h2s_set_dovi.argtypes = [vp, vp, ctypes.c_int]
        self.ctx = vp()
        self.check(L.h2s_create(0, ctypes.byref(self.ctx)))
        c = params.to_c()
        self.check(L.h2s_set_params(self.ctx, ctypes.byref(c)))
        self.check(L.h2s_set_lut(self.ctx, lattice.ctypes.data, LUT_N))

    def check(self, rc):
        if rc:
            raise RuntimeError(f'libh2s error {rc}: {self.L.h2s_last_error(self.ctx).decode()}')

    def set_dovi(self, rpu):
        from hdr2sdr.dovi import records_to_c
        if rpu is None:
            self.check(self.L.h2s_set_dovi(self.ctx, None, 0))
        else:
            arr = records_to_c(rpu)
            self.check(self.L.h2s_set_dovi(self.ctx, ctypes.addressof(arr), len(arr)))

    def timed(self, src, dst, stream, warm, reps):
        import torch
        di, do = src.descriptor(), dst.descriptor()
        for _ in range(warm):
            self.check(self.L.h2s_process(self.ctx, ctypes.byref(di), ctypes.byref(do), NF, stream))
        torch.cuda.synchronize()
        self.check(self.L.h2s_set_timing(self.ctx, 1))
        for _ in range(reps):
            self.check(self.L.h2s_process(self.ctx, ctypes.byref(di), ctypes.byref(do), NF, stream))
        torch.cuda.synchronize()
        ms = self.L.h2s_kernel_ms(self.ctx, reps)
        self.check(self.L.h2s_set_timing(self.ctx, 0))
        return ms

    def close(self):
        self.L.h2s_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import hdr2sdr
    from hdr2sdr import _abi
    from hdr2sdr.dovi import DoviRpu
    from hdr2sdr.synth import synth_frames
    import dovi_ref

    params = hdr2sdr.TonemapParams(tonemapper='bt.2390', gamma=1.0, bits_out=10, peak_detect=True, maxcll=4000.0)
    lattice = np.ascontiguousarray(hdr2sdr.generate_lattice(LUT_N), dtype=np.float32)
    dev = torch.device('cuda', 0)
    src = synth_frames('smooth', NF, W, H, 10, device=dev, seed=0x5EED)
    dst = hdr2sdr.FrameBatch.empty_torch(NF, W, H, 10, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    this = Ctx(_abi.LIB_PATH, params, lattice)
    parent = Ctx(args.parent_lib, params, lattice) if args.parent_lib else None
    rows = {k: [] for k in ('hdr10_parent', 'hdr10_this', 'dovi_identity', 'dovi_realistic', 'hdr10_generic',
                        'dovi_realistic_generic')}
    for _ in range(args.rounds):
        if parent:
            rows['hdr10_parent'].append(parent.timed(src, dst, stream, 3, 20))
        rows['hdr10_this'].append(this.timed(src, dst, stream, 3, 20))
    for _ in range(args.rounds):
        this.set_dovi(DoviRpu.identity(10))
        rows['dovi_identity'].append(this.timed(src, dst, stream, 3, 20))
        this.set_dovi(dovi_ref.realistic_record(10))
        rows['dovi_realistic'].append(this.timed(src, dst, stream, 3, 20))
        this.check(this.L.h2s_set_option(this.ctx, _abi.OPT_FAST_PATH, 0))
        rows['dovi_realistic_generic'].append(this.timed(src, dst, stream, 1, 3))
        this.set_dovi(None)
        rows['hdr10_generic'].append(this.timed(src, dst, stream, 1, 3))
        this.check(this.L.h2s_set_option(this.ctx, _abi.OPT_FAST_PATH, 1))
    out = {'device': torch.cuda.get_device_name(0), 'frames': NF, 'size': f'{W}x{H}', 'rounds': args.rounds,
           'kernel_ms': {k: [round(v, 4) for v in vs] for k, vs in rows.items() if vs},
           'median_ms': {k: round(statistics.median(vs), 4) for k, vs in rows.items() if vs}}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)
    this.close()
    if parent:
        parent.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
