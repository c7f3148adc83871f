#!/usr/bin/env python3
"""Every host-side answer of the library about what a call would run on and how much scratch it needs, as text.  No GPU needed.

    PERCNN_PI_LIB=/path/to/libpercnn_pi.so python tools/dump_plans.py > plans.txt

One line per tuple over a seeded set of shapes (2D and 3D, ragged and power-of-two extents 8 ... 4096, plus the edges), hc in
{-1, 0, 2, 4, 8, 16}, both element sizes, batch 1 / 2 / 64 and the option strings below:

    plan       percnn_pi_debug_plan           (15 ints)
    batchplan  percnn_pi_debug_batch_plan     (4 ints)
    blockmap   percnn_pi_debug_blockmap       (6 ints)
    ws         the six *_workspace_bytes exports

Two builds that plan alike give byte-identical output; `diff` names the rows that do not.  Run each build in a process of its
own.  Without a device the resident bits of `plan` are all 0 (the library cannot ask for the CU count): repeat on the GPU.
`--options-only STRING` restricts the option strings to those containing STRING (a quick look at one combination)."""
import argparse
import ctypes
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from percnn_amd import _lib  # noqa: E402

EXTENTS = [8, 12, 16, 24, 31, 32, 33, 40, 48, 64, 72, 96, 100, 112, 127, 128, 130, 144, 160, 192, 200, 224, 256, 260, 288, 300,
           320, 352, 384, 400, 448, 500, 512, 544, 640, 768, 1000, 1024, 1280, 1536, 2048, 3072, 4096]
HCS = [-1, 0, 2, 4, 8, 16]
BATCHES = [1, 2, 64]
OPTIONS = [
    "", "tile=0", "tile=2", "tile_k=2", "tile_k=8", "tile_nt=256", "tile_nt=1024", "tile_by=8", "tile_by=16", "tile_by=32",
    "tile_wide=0", "tile_wide=1", "tile_wide=2", "tile_fuse=0", "fuse_wgrad=0", "fuse_wgrad=1", "skip_wgrad=1", "vec=1", "rz=2",
    "stream3d=0", "stream3d=2", "brick3d=0", "brick3d=2", "brick_rz=4", "brick_nt=512", "brick_wide=0", "res3d=0", "res3d=2",
    "tile_persist=0", "persist_small=2", "fwd_persist=0", "fwd_small_half=0", "fwd_persist_per_cu=2", "adj_persist_f64=0",
    # the combinations where the plan query and the launchers once disagreed (docs/NOTEBOOK.md section 25)
    "res3d=2,brick3d=0", "res3d=0,brick3d=0", "tile_k=2,tile_by=8", "tile_k=2,tile_by=16", "tile_k=8,tile_by=16",
    "tile_k=8,tile_by=8", "tile_nt=1024,tile_by=8", "tile_nt=1024,tile_by=16", "tile_nt=256,tile_by=16", "tile=2,tile_k=2,tile_by=8",
]


def shapes():
    rng = random.Random(20251021)
    out = [(n, n) for n in EXTENTS]                                            # squares
    out += [(8, 4096), (4096, 8), (32, 32), (32, 64), (64, 32), (256, 512), (384, 320), (300, 320), (100, 104)]
    out += [tuple(rng.choice(EXTENTS) for _ in range(2)) for _ in range(120)]
    cubes = [n for n in EXTENTS if n <= 512]
    out += [(n, n, n) for n in cubes]
    out += [(32, 32, 64), (16, 256, 256), (24, 256, 256), (32, 256, 256), (64, 256, 256), (64, 384, 384), (192, 192, 512),
            (130, 126, 128), (8, 8, 4096), (4096, 8, 8), (2, 2, 8), (128, 128, 260)]
    out += [tuple(rng.choice(cubes) for _ in range(3)) for _ in range(120)]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--options-only", default=None, help="only the option strings that contain this text")
    ap.add_argument("--max-shapes", type=int, default=0, help="only the first N shapes of each dimension (0: all)")
    a = ap.parse_args()
    L = _lib.lib()
    opts = [o for o in OPTIONS if a.options_only is None or a.options_only in o]
    all_shapes = shapes()
    if a.max_shapes:
        all_shapes = [s for d in (2, 3) for s in [t for t in all_shapes if len(t) == d][:a.max_shapes]]
    w = sys.stdout.write
    plan, bplan, bmap = (ctypes.c_int * 15)(), (ctypes.c_int * 4)(), (ctypes.c_int * 6)()

    def ints(rc, buf):
        return " ".join(str(v) for v in buf) if rc == 0 else f"rc={rc}"

    for shape in all_shapes:
        sa, nd, name = _lib.shape_arg(shape), len(shape), "x".join(map(str, shape))
        for es in (4, 8):
            for hc in HCS:
                ws = [L.percnn_pi_bwd_workspace_bytes(hc, nd, sa, es)]
                ws += [L.percnn_pi_rollout_bwd_workspace_bytes(hc, nd, sa, T, es) for T in (1, 17, 200)]
                for b in BATCHES:
                    ws += [L.percnn_pi_batch_bwd_workspace_bytes(hc, nd, sa, b, es), L.percnn_pi_ensemble_bwd_workspace_bytes(hc, nd, sa, b, es)]
                    ws += [f(hc, nd, sa, b, T, es) for T in (1, 17) for f in (L.percnn_pi_batch_rollout_bwd_workspace_bytes,
                                                                             L.percnn_pi_ensemble_rollout_bwd_workspace_bytes)]
                w(f"ws {name} es={es} hc={hc}: {' '.join(map(str, ws))}\n")
            for o in opts:
                ob = o.encode() if o else None
                for i in range(6):
                    bmap[i] = 0
                w(f"blockmap {name} es={es} [{o}]: {ints(L.percnn_pi_debug_blockmap(nd, sa, es, ob, bmap), bmap)}\n")
                for hc in HCS:
                    for i in range(15):
                        plan[i] = 0
                    w(f"plan {name} es={es} hc={hc} [{o}]: {ints(L.percnn_pi_debug_plan(hc, nd, sa, es, ob, plan), plan)}\n")
                    for b in BATCHES:
                        for i in range(4):
                            bplan[i] = 0
                        w(f"batchplan {name} es={es} hc={hc} B={b} [{o}]: "
                          f"{ints(L.percnn_pi_debug_batch_plan(hc, nd, sa, es, b, ob, bplan), bplan)}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
