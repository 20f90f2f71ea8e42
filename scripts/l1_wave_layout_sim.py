"""L1 reuse of wave -> sub-block layouts for the tile kernel's lattice gathers
("Wave layout").  A layout says which 8x8 sub-block of the
64 x 32 tile wave w works on in step s.  For each layout, an LRU model of one
CU's vector L1 (LINES lines of 128 B) is run over the gathers of BLOCKS
resident blocks that sit on unrelated tiles and each walk TILES consecutive
tiles: per step 4 waves x 4 tetrahedral corner gathers of 12-byte records in
.cube order, plus the tile's streamed frame lines (FRAME_LINES per tile, each
touched once, at the tile's start).  Wave order inside a step is either
lockstep (blocks and waves in index order) or shuffled (a random order of all
BLOCKS x 4 waves per step).  Also printed: the static union of distinct lines
that the four waves of one step touch (no cache model).  Lattice coordinates
come from the oracle's stage-3 output (C2 params, geom_sim.coords).  Test
infrastructure only (imports the oracle).
Usage: python scripts/l1_wave_layout_sim.py [--kinds smooth real uniform]
       [--lines 256] [--blocks 5] [--tiles 2] [--trials 300] [--seed 0]"""
import argparse
import os
import sys
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # geom_sim (which itself runs from the repository root)
from geom_sim import coords, corner_offsets, W, H   # noqa: E402

TBW, TBH = 64, 32
LINE = 128
# lines a tile streams through the L1 besides its gathers, each touched once (they only evict): the 10-bit
# tile's frame loads, 64 x 32 luma = 32 lines and 2 x 18 chroma rows of 66 bytes, which lie in 1 or 2 lines
# each, are 68-104 lines; 144 (0.070 per px) is the larger figure the strips' counters leave (0.211 L1->L2
# read requests per px less the modelled gather misses), so the sum agrees with them by construction
FRAME_LINES = 144


# layouts: (step 0..7, wave 0..3) -> (x-block 0..7, y-block 0..3) of the tile
def strips(s, w):            # the 16-px column strips k_tile had
    return 2 * w + (s & 1), s >> 1


def macro2x2(s, w):          # the four waves tile one 16x16 macro-block per step
    return 2 * (s & 3) + (w & 1), 2 * (s >> 2) + (w >> 1)


def macro2x2_serp(s, w):     # the same, macro-row 1 walked right to left
    mc = (s & 3) if s < 4 else 3 - (s & 3)
    return 2 * mc + (w & 1), 2 * (s >> 2) + (w >> 1)


def column1x4(s, w):         # the four waves are one 8 x 32 column per step
    return s, w


def row4x1(s, w):            # the four waves are one 32 x 8 row per step
    return 4 * (s & 1) + w, s >> 1


LAYOUTS = [('today: 16-px column strips', strips), ('2x2 macro-block', macro2x2),
           ('2x2, serpentine macro walk', macro2x2_serp), ('1x4 column', column1x4), ('4x1 row', row4x1)]


def check(layout):
    seen = {layout(s, w) for s in range(8) for w in range(4)}
    assert seen == {(x, y) for x in range(8) for y in range(4)}, 'a layout covers each sub-block once'


def block_lines(offs, px0, py0, xb, yb):
    """distinct 128-B lines of each of the 4 corner gathers of one 8x8 block"""
    ys, xs = slice(py0 + 8 * yb, py0 + 8 * yb + 8), slice(px0 + 8 * xb, px0 + 8 * xb + 8)
    out = []
    for o in offs:
        v = o[ys, xs].ravel()
        out.append(np.unique(np.concatenate([v // LINE, (v + 11) // LINE])))
    return out


def simulate(offs, layout, lines, blocks, tiles, trials, shuffled, seed):
    rng = np.random.default_rng(seed)
    nbx, nby = W // TBW, H // TBH
    miss = px = 0
    union = []
    for _ in range(trials):
        lru = OrderedDict()
        # unrelated tiles: each block's walk starts at a random tile (walks stay in one tile row)
        starts = [(int(rng.integers(0, nbx - tiles + 1)), int(rng.integers(0, nby))) for _ in range(blocks)]
        for ti in range(tiles):
            for b in range(blocks):   # the tile's streamed frame lines: touched once, never reused
                for k in range(FRAME_LINES):
                    lru[('f', b, ti, k)] = None
                    if len(lru) > lines:
                        lru.popitem(last=False)
            for s in range(8):
                order = [(b, w) for b in range(blocks) for w in range(4)]
                if shuffled:
                    order = [order[i] for i in rng.permutation(len(order))]
                per_block = {}
                for b, w in order:
                    bx, by = starts[b]
                    xb, yb = layout(s, w)
                    g = block_lines(offs, (bx + ti) * TBW, by * TBH, xb, yb)
                    per_block.setdefault(b, []).append(np.concatenate(g))
                    for corner in g:
                        for ln in corner.tolist():
                            if ln in lru:
                                lru.move_to_end(ln)
                            else:
                                miss += 1
                                lru[ln] = None
                                if len(lru) > lines:
                                    lru.popitem(last=False)
                    px += 64
                union += [len(np.unique(np.concatenate(v))) for v in per_block.values()]
    return miss / px, float(np.mean(union))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kinds', nargs='+', default=['smooth', 'real', 'uniform'])
    ap.add_argument('--lines', type=int, default=256)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--tiles', type=int, default=2)
    ap.add_argument('--trials', type=int, default=300)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    for _, f in LAYOUTS:
        check(f)
    print(f'L1 {a.lines} lines x {LINE} B, {a.blocks} blocks x {a.tiles} tiles, {a.trials} trials, seed {a.seed};'
          f' frame lines {FRAME_LINES} per tile = {FRAME_LINES / (TBW * TBH):.3f} per px (not in the gather misses below)')
    for kind in a.kinds:
        offs = corner_offsets(coords(kind))
        print(f'== {kind}')
        base = None
        for name, f in LAYOUTS:
            m0, u = simulate(offs, f, a.lines, a.blocks, a.tiles, a.trials, False, a.seed)
            m1, _ = simulate(offs, f, a.lines, a.blocks, a.tiles, a.trials, True, a.seed)
            base = base or (m0, m1)
            print(f'  {name:30s} gather misses/px lockstep {m0:.4f} ({100 * (m0 / base[0] - 1):+5.1f} %)'
                  f'  shuffled {m1:.4f} ({100 * (m1 / base[1] - 1):+5.1f} %)  lines per block-step (union of 4 waves) {u:6.1f}')


if __name__ == '__main__':
    main()
