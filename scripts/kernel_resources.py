#!/usr/bin/env python3
"""Register, LDS, scratch and code-size figures of every kernel in libh2s, from
the compiler's own metadata.  Needs no GPU: every device source of
_build.SOURCES is cross-compiled (device side only) to assembly with that
file's own flags (_build.CFLAGS + SOURCE_FLAGS), and the figures are read from
the assembly's .amdgpu_metadata record of each kernel and from the "Kernel
info" comment block the compiler writes after it (occupancy, code bytes).
Only those fields are read; the instruction stream is never searched.

JSON, one line per kernel so that two commits' files diff symbol by symbol (as
long as k_tile's template parameter list stands): {"fields": FIELDS, "kernels":
{source file: {mangled kernel symbol: [the fields' values]}}}; lds_bytes is the
static part (the eq table's dynamic part is the launch's), occupancy in waves
per SIMD.  load() gives {symbol: {field: value, 'source': file}} back.

  python scripts/kernel_resources.py OUT.json [--jobs 8]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'hdr-to-sdr_amd'))

META = {'.vgpr_count': 'vgprs', '.sgpr_count': 'sgprs', '.sgpr_spill_count': 'sgpr_spills',
        '.vgpr_spill_count': 'vgpr_spills', '.group_segment_fixed_size': 'lds_bytes',
        '.private_segment_fixed_size': 'private_bytes'}
INFO = {'codeLenInByte': 'code_bytes', 'Occupancy': 'occupancy'}
FIELDS = ['vgprs', 'sgprs', 'sgpr_spills', 'vgpr_spills', 'lds_bytes', 'private_bytes', 'occupancy', 'code_bytes']


def dump(res, path):
    by_src = {}
    for name, rec in res.items():
        by_src.setdefault(rec['source'], {})[name] = [rec.get(f) for f in FIELDS]
    out = ['{"fields": ' + json.dumps(FIELDS) + ',', '"kernels": {']
    for i, src in enumerate(sorted(by_src)):
        rows = [f' {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in sorted(by_src[src].items())]
        out.append(f'{json.dumps(src)}: {{\n' + ',\n'.join(rows) + '\n}' + (',' if i + 1 < len(by_src) else ''))
    with open(path, 'w') as fh:
        fh.write('\n'.join(out) + '\n}}\n')


def load(path):
    with open(path) as fh:
        d = json.load(fh)
    return {k: dict(zip(d['fields'], v), source=src) for src, ks in d['kernels'].items() for k, v in ks.items()}


def parse(asm, source):
    """The kernels of one assembly listing: the metadata's records (a YAML
    list under amdhsa.kernels, one `- .key: value` / `  .key: value` entry per
    line) and the comment blocks that follow each `.amdhsa_kernel NAME`."""
    out, info, cur, rec, in_meta = {}, {}, None, None, False
    for line in asm.splitlines():
        s = line.strip()
        if s.startswith('.amdgpu_metadata'):
            in_meta = True
        elif s.startswith('.end_amdgpu_metadata'):
            in_meta = False
        elif in_meta:
            m = re.match(r'^(- )?\s*(\.[a-z_]+):\s*(.*)$', s)
            if not m or not line.startswith('  ') or line.startswith('      '):
                continue     # (nested lists: the kernels' .args records)
            if m.group(1):
                rec = {}
            if rec is None:
                continue
            if m.group(2) == '.name':
                out[m.group(3).strip("'\"")] = rec
            elif m.group(2) in META:
                rec[META[m.group(2)]] = int(m.group(3))
        elif s.startswith('.amdhsa_kernel '):
            cur = s.split()[1]
            info[cur] = {}
        elif cur and s.startswith(';'):
            m = re.match(r'^;\s*(codeLenInByte|Occupancy)\s*[:=]\s*(\d+)', s)
            if m:
                info[cur][INFO[m.group(1)]] = int(m.group(2))
    for name, rec in out.items():
        rec.update(info.get(name, {}))
        rec['source'] = source
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('out')
    ap.add_argument('--jobs', type=int, default=8)
    args = ap.parse_args()
    from hdr2sdr import _build

    def one(src):
        with tempfile.TemporaryDirectory() as tmp:
            s = os.path.join(tmp, src + '.s')
            cmd = [_build._hipcc(), f'--offload-arch={_build.ARCH}'] + _build.CFLAGS + _build.SOURCE_FLAGS.get(src, []) + \
                  ['--cuda-device-only', '-S', '-o', s, os.path.join(_build.CSRC, src)]
            subprocess.run(cmd, check=True)
            with open(s) as fh:
                return parse(fh.read(), src)

    res = {}
    with ThreadPoolExecutor(max_workers=args.jobs) as ex:
        for part in ex.map(one, [s for s in _build.SOURCES if s.endswith('.hip')]):
            res.update(part)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dump(res, args.out)
    print(f'{len(res)} kernels -> {args.out}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
