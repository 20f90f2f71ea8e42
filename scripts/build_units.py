#!/usr/bin/env python3
"""The library's translation units and their flags as shell assignments, for
the variant builds (build_ablation.sh, build_variants.sh: `eval "$(python3
scripts/build_units.py)"` after `declare -A UNIT_FLAGS`).  hdr2sdr/_build.py is
the one list; _build.py is loaded on its own, without importing the package."""
import importlib.util
import os
import shlex

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location(
    '_build', os.path.join(os.path.dirname(HERE), 'hdr-to-sdr_amd', 'hdr2sdr', '_build.py'))
b = importlib.util.module_from_spec(spec)
spec.loader.exec_module(b)

print('SOURCES=' + shlex.quote(' '.join(b.SOURCES)))
print('CFLAGS=' + shlex.quote(' '.join(b.CFLAGS)))
for unit, flags in b.SOURCE_FLAGS.items():
    print(f'UNIT_FLAGS[{shlex.quote(unit)}]=' + shlex.quote(' '.join(flags)))
