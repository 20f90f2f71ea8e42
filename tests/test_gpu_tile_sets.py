"""Every instance set of the tile kernel, walked from the library's interface
(tests/tile_sets_ref.py states the rows; the C table in csrc/h2s_tile_sets.h is
what this checks): one launch per (set, transfer, operator, desat) at 192 x 96,
2 frames, a 17^3 LUT.

Every row is routed to the tile kernel (H2S_PATH_TILE) and runs without error:
a row whose instance the table, the dispatch or the predicate lacked would be
refused at the launch or routed elsewhere.  Rows with an exact twin are held to
it sample for sample, so a launch that took a neighbouring instance shows:
  semi-planar sets == the planar run, repacked;
  4:2:2 / 4:4:4 sets, fed the exact upsamples of the 4:2:0 frame == the 4:2:0 run;
  top-left sets == the left-sited run on chroma that is constant down every
    column (both vertical passes then give 4 h exactly).
The planar and Dolby Vision sets' values are the parity tests' (test_gpu_parity,
test_gpu_dovi); the debug sets' planes are test_float_gate's.
"""
import numpy as np
import pytest

import hdr2sdr
import tile_sets_ref as TS
from hdr2sdr import _abi
from hdr2sdr.frames import FrameBatch

pytestmark = pytest.mark.gpu

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope='module')
def tm():
    t = hdr2sdr.Tonemapper(0)
    yield t
    t.set_dovi(None)
    t.close()


def sources():
    return cached('sources', lambda: TS.sources(TS.base_source()))


def run(tm, src, layout):
    """(path, output as a planar int64 array) of src -> a device set of the layout."""
    import torch
    dev = src.to_torch('cuda')
    dst = FrameBatch.empty_torch(src.nframes, src.width, src.height, TS.BITS, 'cuda', layout)
    path = tm.query_path(dev, dst)
    tm.process(dev, dst)
    torch.cuda.synchronize()
    return path, dst.to_numpy().to_layout('planar').buf.astype(np.int64)


@pytest.mark.parametrize('row', TS.ROWS, ids=TS.row_id)
def test_every_row_runs_on_its_tile_instance(tm, row):
    s, t, op, d = row
    params = TS.params(row)
    tm.set_params(params)
    tm.set_lut(cached('lattice', lambda: hdr2sdr.generate_lattice(TS.LUT_N)))
    tm.set_dovi(cached('record', TS.dovi_record) if s.chain == 'dv' else None)
    src, twin = sources()[s.name]
    if s.debug:
        dev = src.to_torch('cuda')
        assert tm.query_path(dev, FrameBatch.empty_torch(TS.NF, TS.W, TS.H, TS.BITS, 'cuda')) == _abi.PATH_TILE
        planes = tm.debug_float(dev, TS.DEBUG_STAGE)
        assert planes.shape[-2:] == (TS.H, TS.W) and np.isfinite(planes).all()
        return
    path, got = run(tm, src, s.layout)
    assert path == _abi.PATH_TILE
    if twin is None:
        return
    # (the twin's run: the same parameters on the planar left-sited 4:2:0 set, once per case)
    tpath, want = cached(('twin', s.chain, t, op, d, id(twin)), lambda: run(tm, twin, 'planar'))
    assert tpath == _abi.PATH_TILE
    differ = int((got != want).sum())
    print(f'TILE-SETS {TS.row_id(row)}: differ={differ}')
    assert differ == 0
