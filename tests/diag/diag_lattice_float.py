"""Survey (GPU box, no assertion): the stage-4 float gate's floor-only share
(values beyond 1e-3 relative that pass through the lattice-slope conditioning
term alone) per lattice, noise amplitude, configuration and content, on both
kernels.  The figures in tests/test_gpu_lattices.py's docstring and
profiles/lattices/float_stage4_survey.txt come from it."""
import os
import sys

os.environ['H2S_FLOOR_ONLY_MAX'] = '1.0'      # report the share, do not cap it
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, 'tests'), os.path.join(REPO, 'hdr-to-sdr_amd'), REPO]
import hdr2sdr  # noqa: E402
import lattices_ref as LR  # noqa: E402
from float_gate import lattice  # noqa: E402
from test_gpu_parity import check_float_stage  # noqa: E402

tm = hdr2sdr.Tonemapper(0)
lats = {'bundled65': None, 'bundled17': lattice(17), 'bumpy17@0.01': LR.bumpy(17, 0.01), 'bumpy17@0.02': LR.bumpy(17, 0.02),
        'bumpy33@0.01': LR.bumpy(33, 0.01), 'bumpy33@0.02': LR.bumpy(33, 0.02)}
for cfg, kind in [('C3_bt2390_pq10_cpu', 'smooth'), ('C3_bt2390_pq10_cpu', 'uniform'), ('C2_hable_pq10', 'uniform'),
                  ('C4_mobius_native', 'smooth'), ('C4_mobius_native', 'uniform')]:
    for name, lat in lats.items():
        for kernel in ('k_tile', 'k_debug'):
            try:
                rep = check_float_stage(tm, kernel, cfg, kind, 4, lat=lat)
                print(f'SURVEY {cfg} {kind} {name} {kernel}: floor_only {rep["floor_only_frac"]:.4f} '
                      f'excluded {rep["excluded_frac"]:.4f} max_rel_rest {rep["max_rel_err_rest"]:.2e}', flush=True)
            except AssertionError as e:
                print(f'SURVEY {cfg} {kind} {name} {kernel}: FAIL {str(e)[:160]}', flush=True)
tm.close()
