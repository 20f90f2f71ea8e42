"""In-tree build of libh2s.so (hipcc, gfx950) and of the test oracle.

The .so files land next to their loaders (hdr2sdr/libh2s.so,
oracle/build/liboracle.so): git-ignored, but they travel to the GPU box with
the gpurun snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
PROJ_DIR = os.path.dirname(PKG_DIR)            # hdr-to-sdr_amd/
REPO_DIR = os.path.dirname(PROJ_DIR)
CSRC = os.path.join(PROJ_DIR, 'csrc')
INCLUDE = os.path.join(REPO_DIR, 'include')
LIB = os.path.join(PKG_DIR, 'libh2s.so')
ORACLE_DIR = os.path.join(REPO_DIR, 'oracle')
ORACLE_LIB = os.path.join(ORACLE_DIR, 'build', 'liboracle.so')

ARCH = os.environ.get('H2S_OFFLOAD_ARCH', 'gfx950')
# (the longest compiles first, so that the parallel build does not end on one)
SOURCES = ['h2s_kernels.hip', 'h2s_debug_lp_dv_semi.hip', 'h2s_debug_lp_dv.hip', 'h2s_fast_lp_dv_semi.hip',
           'h2s_fast_lp_dv.hip', 'h2s_fast_lp.hip', 'h2s_fast_lp_semi.hip', 'h2s_fast_lp_tl.hip', 'h2s_debug_semi.hip',
           'h2s_debug.hip', 'h2s_debug_lp_semi.hip', 'h2s_debug_lp.hip', 'h2s_fast_semi.hip', 'h2s_fast_tl.hip',
           'h2s_fast_sub422.hip', 'h2s_fast.hip', 'h2s_fast_sub444.hip', 'h2s_peak.hip', 'h2s_api.hip',
           'h2s_resolve.hip', 'h2s_api_peak.hip', 'h2s_api_preview.hip', 'h2s_api_dovi.hip', 'h2s_preview.hip',
           'h2s_scale.hip', 'h2s_api_scale.hip', 'h2s_decimate.hip', 'h2s_api_decimate.hip',
           'h2s_rgb.hip', 'h2s_api_rgb.hip', 'h2s_repack.hip', 'h2s_api_ladder.hip', 'h2s_testhooks.hip', 'h2s_cube.cpp']
HEADERS = ['h2s_params.h', 'h2s_math.h', 'h2s_chain.h', 'h2s_tile.h', 'h2s_tile_tone.h', 'h2s_tile_px.h', 'h2s_tile_io.h', 'h2s_tile_sets.h',
           'h2s_peak.h', 'h2s_libm.h', 'h2s_lpx.h', 'h2s_dovi.h', 'h2s_srcprev.h', 'h2s_scale.h', 'h2s_decimate.h', 'h2s_rgb.h', 'h2s_repack.h', 'h2s_launch.h', 'h2s_host.h']


def _hipcc() -> str:
    for cand in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError('hipcc not found (ROCm toolchain required to build libh2s)')


def _stale(target: str, deps: 'list[str]') -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


OBJ_DIR = os.path.join(PROJ_DIR, 'build', 'obj')
# -fno-slp-vectorize: packing scalar f32 pairs into v_pk_* costs register
# moves that outweigh the packed issue on this kernel (measured static VALU
# slots per pixel 207 -> 199)
CFLAGS = ['-O3', '-std=c++17', '-fno-slp-vectorize', '-fPIC', '-Wno-unused-value', '-Wno-unused-result',
          '-Wno-pass-failed']
# the product tile kernel's scheduler: round 2 measured LLVM's
# max-memory-clause 2 % faster than the default; after round 4's changes the
# default is the faster one (C2 -0.7 % smooth, -3 % uniform noise; Mobius
# alike; identical output: profiles/r04/ablations/sched_strategy.log), so the
# tile TU builds with the default again (iterative-minreg stays 13 % slower)
SOURCE_FLAGS = {
    # the generic kernel is the chain's exact restatement (the libplacebo
    # branch's exact path): no FMA contraction, so its float arithmetic rounds
    # where the oracle's does
    'h2s_kernels.hip': ['-ffp-contract=off'],
    # the peak statistics' per-pixel sums (peak_px) round where they are written
    'h2s_peak.hip': ['-ffp-contract=off'],
}


def build_lib(force: bool = False, verbose: bool = False) -> str:
    """One object per source, compiled in parallel (each .hip holds its own
    kernels and their launchers), then one shared link."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(INCLUDE, 'h2s.h')]
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs = [os.path.join(OBJ_DIR, os.path.basename(s) + '.o') for s in srcs]

    def flags(s):
        return [f'--offload-arch={ARCH}'] + CFLAGS + SOURCE_FLAGS.get(os.path.basename(s), [])

    def cmd_stale(s, o):
        # an object built with other flags (an ablation build, a changed
        # CFLAGS / SOURCE_FLAGS entry) is stale whatever its mtime says
        try:
            with open(o + '.cmd') as fh:
                return fh.read() != ' '.join(flags(s))
        except OSError:
            return True

    # the gpurun snapshot carries libh2s.so but not build/obj: a library newer
    # than every source and header, linked from objects built with today's
    # flags (its .cmd stamp), is current without its objects
    stamp = '\n'.join(f'{os.path.basename(s)}: ' + ' '.join(flags(s)) for s in srcs)
    try:
        with open(LIB + '.cmd') as fh:
            lib_cmd = fh.read()
    except OSError:
        lib_cmd = None
    if not force and lib_cmd == stamp and not _stale(LIB, srcs + hdrs):
        return LIB

    todo = [(s, o) for s, o in zip(srcs, objs) if force or _stale(o, [s] + hdrs) or cmd_stale(s, o)]

    def compile_one(so):
        s, o = so
        tmp = o + f'.tmp{os.getpid()}'
        cmd = [_hipcc()] + flags(s) + ['-c', '-o', tmp, s]
        if verbose:
            print(' '.join(cmd))
        subprocess.run(cmd, check=True)
        os.replace(tmp, o)
        with open(o + '.cmd', 'w') as fh:
            fh.write(' '.join(flags(s)))

    with ThreadPoolExecutor(max_workers=max(1, min(len(todo), int(os.environ.get('MAX_JOBS', '8'))))) as ex:
        list(ex.map(compile_one, todo))
    if force or todo or _stale(LIB, objs):
        tmp = LIB + f'.tmp{os.getpid()}'
        cmd = [_hipcc(), f'--offload-arch={ARCH}', '-shared', '-fPIC', '-o', tmp] + objs
        if verbose:
            print(' '.join(cmd))
        subprocess.run(cmd, check=True)
        os.replace(tmp, LIB)
    with open(LIB + '.cmd', 'w') as fh:
        fh.write(stamp)
    return LIB


def build_oracle(force: bool = False, verbose: bool = False) -> str:
    src = os.path.join(ORACLE_DIR, 'h2s_oracle.c')
    deps = [src, os.path.join(INCLUDE, 'h2s.h')]
    if not force and not _stale(ORACLE_LIB, deps):
        return ORACLE_LIB
    os.makedirs(os.path.dirname(ORACLE_LIB), exist_ok=True)
    tmp = ORACLE_LIB + f'.tmp{os.getpid()}'
    cmd = ['gcc', '-O2', '-std=c11', '-fopenmp', '-shared', '-fPIC', '-o', tmp, src, '-lm']
    if verbose:
        print(' '.join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(tmp, ORACLE_LIB)
    return ORACLE_LIB


def build_all(force: bool = False, verbose: bool = False) -> None:
    build_lib(force, verbose)
    build_oracle(force, verbose)
