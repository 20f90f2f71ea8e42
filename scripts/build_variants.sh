#!/bin/bash
# Build libh2s variants for scripts/time_variants.py.
# Usage: bash scripts/build_variants.sh NAME:"-DFLAG ..." NAME2:"..."
# (The flags reach the product source as it is.  The tile kernel's decided
# switches -- H2S_TAGSEL, H2S_EQMAGIC, H2S_YST*, H2S_NT_*, H2S_TILE_WPE* -- are
# no longer in it: build those variants with scripts/build_ablation.sh and
# profiles/tile_split/ab_patches/tile_switches.patch.)
# Only the product tile instances (h2s_fast.hip, h2s_fast_lp.hip) are rebuilt
# with the flags;
# every other object comes from the in-tree build (hdr-to-sdr_amd/build/obj,
# run `python -c "import __graft_entry__ as g; g.build()"` first).  The
# translation units, the common flags and the per-unit flags are
# hdr2sdr/_build.py's (SOURCES, CFLAGS, SOURCE_FLAGS).
# Outputs scripts/variants/libh2s_NAME.so (git-ignored, travels with gpurun).
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
C=$ROOT/hdr-to-sdr_amd/csrc
O=$ROOT/hdr-to-sdr_amd/build/obj
V=$ROOT/scripts/variants
mkdir -p "$V"
# SOURCES, CFLAGS and UNIT_FLAGS[unit] from _build.py
declare -A UNIT_FLAGS
eval "$(python3 "$ROOT/scripts/build_units.py")"
MMC=${MMC-""}   # extra flags for h2s_fast.hip (env MMC)
pids=()
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  [ "$flags" = "$spec" ] && flags=""
  (
    objs=(); built=()
    for s in $SOURCES; do
      rebuild=0; extra=${UNIT_FLAGS[$s]:-}
      case $s in
        h2s_fast.hip) rebuild=1; extra="$extra $MMC";;
        h2s_fast_lp.hip) rebuild=1;;
        # DBG=1: the debug instances (h2s_debug_float) get the flags too
        h2s_debug.hip|h2s_debug_lp.hip) rebuild=${DBG:-0};;
        # KERN=1: h2s_kernels.hip (generic kernel) and h2s_peak.hip (peak statistics) get the flags too
        h2s_kernels.hip|h2s_peak.hip) rebuild=${KERN:-0};;
      esac
      if [ "$rebuild" = 1 ]; then
        o="$V/${s%.*}_$name.o"
        /opt/rocm/bin/hipcc --offload-arch=gfx950 $CFLAGS $extra $flags -c -o "$o" "$C/$s" || exit 1
        built+=("$o")
      else
        o="$O/$s.o"
      fi
      objs+=("$o")
    done
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$V/libh2s_$name.so" "${objs[@]}" && rm -f "${built[@]}"
  ) &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
ls -la "$V"
