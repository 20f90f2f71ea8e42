#!/usr/bin/env python3
"""SHA-256 of everything the C-ABI's host arithmetic (h2s_resolve.hip) makes,
for comparing two trees' host constants without a GPU (a refactor that must
not move one bit of a table or of a parameter block).  h2s_resolve.hip makes
no HIP call, so a small stand-alone program (its own main, its own
h2s::host::fail / hip_fail) is compiled together with the tree's
h2s_resolve.hip, host side under AddressSanitizer and UBSan, and run on the
CPU.  It writes named records; this script hashes them per name:

  the three cubic tables (build_pq_table at two scales, build_pqi_table,
  build_hlg_table), chroma_taps, resize_taps for a few ratios, source_consts
  for both depths, both ranges and the three matrices, and, per transfer and
  operator over a fixed grid of parameter sets (pipelines where valid, depths,
  LUT on / off, modes, the lp_* options, non-default tm_param / targets /
  knee), the KParams bytes, the eq table, the FastParams bytes of resolve_fast
  (both range tags) and the peak_model fields.

Structs their writers zero-fill first (KParams, FastParams) are hashed as
bytes; the others (PeakModel, SourceConsts) field by field, never padding.

  python scripts/host_digests.py OUT.json [--tree DIR]

--tree: the checkout whose h2s_resolve.hip is compiled (default: this one).
A sanitizer report fails the run.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import struct
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <stdio.h>

#include "h2s_host.h"

namespace h2s {
namespace host {
int fail(h2s_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}
int hip_fail(h2s_ctx* c, hipError_t, const char* what) { return fail(c, H2S_E_HIP, what); }
}  // namespace host
}  // namespace h2s

using namespace h2s::host;

static FILE* g_out;

// one record: name, byte count, bytes (the script keeps one hash per name)
static void put(const std::string& name, const void* p, size_t n) {
  const unsigned long long len = n;
  fprintf(g_out, "%s\n", name.c_str());
  fwrite(&len, sizeof(len), 1, g_out);
  fwrite(p, 1, n, g_out);
}
template <class T>
static void put_vec(const std::string& name, const std::vector<T>& v) {
  put(name, v.data(), v.size() * sizeof(T));
}

struct Fields {
  std::vector<unsigned char> b;
  template <class T>
  void add(const T& v) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
    b.insert(b.end(), p, p + sizeof(T));
  }
};

static void put_peak_model(const std::string& name, const h2s::PeakModel& m) {
  Fields f;
  f.add(m.t_white), f.add(m.t_black), f.add(m.knee_off), f.add(m.contrast), f.add(m.tm_param), f.add(m.static_peak);
  f.add(m.smoothing), f.add(m.scene_low), f.add(m.scene_high), f.add(m.percentile), f.add(m.min_peak), f.add(m.iir_a);
  f.add(m.npx), f.add(m.nblocks), f.add(m.pct), f.add(m.family), f.add(m.pq.smin), f.add(m.pq.white), f.add(m.pq.black);
  put(name, f.b.data(), f.b.size());
}

static void put_source_consts(const std::string& name, const SourceConsts& s) {
  Fields f;
  f.add(s.y_scale), f.add(s.y_off), f.add(s.y_black), f.add(s.c_scale), f.add(s.c_off), f.add(s.mid);
  f.add(s.m_rcr), f.add(s.m_gcb), f.add(s.m_gcr), f.add(s.m_bcb);
  put(name, f.b.data(), f.b.size());
}

int main(int argc, char** argv) {
  if (argc != 2 || !(g_out = fopen(argv[1], "wb"))) return 2;
  std::vector<float4> tab;
  build_pq_table(100.0, &tab), put_vec("table/pq_100", tab);
  build_pq_table(10000.0 / 203.0, &tab), put_vec("table/pq_203", tab);
  build_pqi_table(&tab), put_vec("table/pqi", tab);
  build_hlg_table(&tab), put_vec("table/hlg", tab);

  float wx7[7], wy8[8];
  chroma_taps(wx7, wy8);
  put("chroma_taps", wx7, sizeof(wx7)), put("chroma_taps", wy8, sizeof(wy8));

  // up-scaling, identity, down-scaling, an odd ratio and the 12x limit
  const int ratios[][2] = {{960, 1920}, {1280, 1280}, {3840, 1920}, {1919, 642}, {3840, 320}};
  for (const auto& r : ratios) {
    std::vector<float> w;
    std::vector<int> start;
    const int T = resize_taps(r[0], r[1], &w, &start);
    const std::string name = "resize_taps/" + std::to_string(r[0]) + "_" + std::to_string(r[1]);
    put(name, &T, sizeof(T)), put_vec(name, w), put_vec(name, start);
  }

  for (int bits = 10; bits <= 12; bits += 2)
    for (int full = 0; full < 2; full++)
      for (int matrix = 0; matrix < 3; matrix++) put_source_consts("source_consts", source_consts(bits, full != 0, matrix));

  h2s_ctx* c = new h2s_ctx;
  c->lut_n = 33;
  long long sets = 0, refused = 0;
  const double nan = NAN;
  for (int trc = H2S_TRC_PQ; trc <= H2S_TRC_HLG; trc++)
    for (int tm = H2S_TM_NONE; tm <= H2S_TM_SPLINE; tm++) {
      const std::string key = "/trc" + std::to_string(trc) + "/tm" + std::to_string(tm);
      for (int pipe = H2S_PIPE_CPU_CHAIN; pipe <= H2S_PIPE_LIBPLACEBO; pipe++)
        for (int bits_in = 10; bits_in <= 12; bits_in += 2)
          for (int bits_out = 8; bits_out <= 12; bits_out += 2)
            for (int lut = 1; lut >= 0; lut--)
              for (int mode = H2S_MODE_COMPAT8; mode <= H2S_MODE_NATIVE; mode++)
                for (int var = 0; var < 3; var++) {
                  h2s_params p;
                  memset(&p, 0, sizeof(p));
                  p.transfer_in = trc, p.bits_in = bits_in, p.bits_out = bits_out, p.tonemap = tm;
                  p.tm_param = nan, p.desat = 2.0, p.peak = 0.0, p.npl = 100.0, p.gamma = 1.0;
                  p.lut_enabled = lut, p.mode = mode, p.pipeline = pipe;
                  p.knee_offset = nan, p.target_black = nan, p.target_white = nan;
                  p.lp_p010 = H2S_LP_P010_TRUNCATE;
                  p.pd_smoothing = nan, p.pd_scene_low = nan, p.pd_scene_high = nan, p.pd_percentile = nan;
                  p.pd_min_peak = nan;
                  if (var == 1) {   // the lp_* options and the [EXT] switches off their defaults
                    p.lp_tone = H2S_LP_TONE_MAX_RGB, p.lp_range = H2S_LP_RANGE_LIMITED;
                    p.lp_dither = H2S_LP_DITHER_ORDERED, p.lp_p010 = H2S_LP_P010_KEEP;
                    p.dither = H2S_DITHER_ORDERED, p.expand = H2S_EXPAND_REPLICATE, p.lut_input = H2S_LUT_IN_RGB48;
                    p.chroma_edge = H2S_EDGE_MIRROR, p.desat_luma = H2S_DESAT_LUMA_BT2020, p.maxcll = 1000.0;
                  }
                  if (var == 2) {   // non-default tm_param, target black / white, knee offset, gamma, peak model
                    p.tm_param = 0.4, p.target_black = 0.1, p.target_white = 150.0, p.knee_offset = 0.75;
                    p.gamma = 1.2, p.npl = 203.0, p.desat = 0.0, p.peak = 40.0, p.peak_detect = 1;
                    p.desat_luma = H2S_DESAT_LUMA_BT709, p.mastering_max = 4000.0;
                    p.pd_smoothing = 20.0, p.pd_scene_low = 3.0, p.pd_scene_high = 8.0, p.pd_percentile = 100.0;
                    p.pd_min_peak = 2.0;
                  }
                  sets++;
                  if (validate_params(c, &p) != 0) {
                    refused++;
                    continue;
                  }
                  c->params = p;
                  h2s::KParams k;
                  std::vector<uint16_t> eq;
                  resolve(&p, &k, &eq);
                  put("kparams" + key, &k, sizeof(k));
                  put_vec("eq" + key, eq);
                  k.W = 1920, k.H = 1080;   // (fill_geometry's; peak_model reads them)
                  for (int full = 0; full < 2; full++) {
                    h2s::FastParams F;
                    k.full = full;
                    resolve_fast(c, k, &F);
                    put("fastparams" + key, &F, sizeof(F));
                  }
                  put_peak_model("peak_model" + key, peak_model(c, k));
                }
    }
  delete c;
  const long long counts[4] = {sets, refused, (long long)sizeof(h2s::KParams), (long long)sizeof(h2s::FastParams)};
  put("counts", counts, sizeof(counts));
  if (fclose(g_out) != 0) return 3;
  printf("%lld parameter sets, %lld refused by validate_params; sizeof(KParams) %lld, sizeof(FastParams) %lld\n", sets,
         refused, counts[2], counts[3]);
  return 0;
}
'''


def load_build(tree):
    spec = importlib.util.spec_from_file_location(
        '_h2s_build', os.path.join(tree, 'hdr-to-sdr_amd', 'hdr2sdr', '_build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def records(path):
    """{name: [sha256 of the name's records in order, their byte count]}"""
    out = {}
    with open(path, 'rb') as fh:
        while True:
            name = fh.readline()
            if not name:
                return {k: [h.hexdigest(), n] for k, (h, n) in out.items()}
            (n,) = struct.unpack('<Q', fh.read(8))
            rec = out.setdefault(name.decode().rstrip('\n'), [hashlib.sha256(), 0])
            rec[0].update(fh.read(n))
            rec[1] += n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('out')
    ap.add_argument('--tree', default=REPO)
    args = ap.parse_args()
    _build = load_build(args.tree)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, rec = (os.path.join(tmp, n) for n in ('host_digests.hip', 'host_digests', 'records.bin'))
        with open(src, 'w') as fh:
            fh.write(PROGRAM)
        # host code only is of interest; the resolve unit's own flags otherwise
        cmd = [_build._hipcc(), f'--offload-arch={_build.ARCH}'] + _build.CFLAGS + \
              _build.SOURCE_FLAGS.get('h2s_resolve.hip', []) + \
              ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
               '-I', _build.CSRC, '-o', exe, src, os.path.join(_build.CSRC, 'h2s_resolve.hip')]
        subprocess.run(cmd, check=True)
        # (leaks: the HIP runtime the program links, but never calls, keeps its own start-up allocations)
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0', UBSAN_OPTIONS='print_stacktrace=1')
        run = subprocess.run([exe, rec], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        sys.stdout.write(run.stdout)
        if run.returncode != 0 or 'Sanitizer' in run.stderr or 'runtime error' in run.stderr:
            sys.stderr.write(run.stderr)
            print(f'host_digests: the program failed or a sanitizer reported (exit {run.returncode})', file=sys.stderr)
            return 1
        res = records(rec)
    with open(args.out, 'w') as fh:
        fh.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v)}' for k, v in sorted(res.items())) + '\n}\n')
    print(f'{len(res)} digests -> {args.out}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
