#!/usr/bin/env python3
"""SHA-256 of every device source's gfx950 assembly listing, for comparing two
trees' machine code without a GPU (a refactor that must not move one
instruction).  Every .hip of _build.SOURCES is cross-compiled, device side
only, with that file's own flags (_build.CFLAGS + SOURCE_FLAGS) and one fixed
compilation-unit id, so equal code gives equal listings; the lines that name
the __hip_cuid_ symbol are left out of the digest as well.  Whole listings are
hashed; the instruction stream is never searched.

  python scripts/listing_digests.py OUT.txt [--tree DIR] [--keep DIR] [--jobs 8]

--tree: the checkout to compile (default: this one); OUT.txt gets one
"digest  lines  source" row per unit.  --keep: also leave the listings there.
"""
import argparse
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(text):
    lines = [l for l in text.splitlines() if '__hip_cuid_' not in l]
    return hashlib.sha256('\n'.join(lines).encode()).hexdigest(), len(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('out')
    ap.add_argument('--tree', default=REPO)
    ap.add_argument('--keep')
    ap.add_argument('--jobs', type=int, default=8)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location(
        '_h2s_build', os.path.join(args.tree, 'hdr-to-sdr_amd', 'hdr2sdr', '_build.py'))
    _build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(_build)
    if args.keep:
        os.makedirs(args.keep, exist_ok=True)

    def one(src):
        with tempfile.TemporaryDirectory() as tmp:
            s = os.path.join(args.keep or tmp, src + '.s')
            cmd = [_build._hipcc(), f'--offload-arch={_build.ARCH}'] + _build.CFLAGS + _build.SOURCE_FLAGS.get(src, []) + \
                  ['-cuid=h2s', '--cuda-device-only', '-S', '-o', s, os.path.join(_build.CSRC, src)]
            subprocess.run(cmd, check=True)
            with open(s) as fh:
                return (src,) + digest(fh.read())

    with ThreadPoolExecutor(max_workers=args.jobs) as ex:
        rows = list(ex.map(one, [s for s in _build.SOURCES if s.endswith('.hip')]))
    with open(args.out, 'w') as fh:
        for src, d, n in sorted(rows):
            fh.write(f'{d}  {n:7d}  {src}\n')
    print(f'{len(rows)} units -> {args.out}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
