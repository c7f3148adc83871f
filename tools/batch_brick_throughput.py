"""Batched 3D rollouts on the brick kernels against the direct kernels: forward + backward sample-steps/s of ONE batched call
(torch.ops.percnn.pi_rollout_batched + pi_rollout_batched_backward) under brick3d=2 and under brick3d=0, both routes alternating in
one process.  brick3d=0 is timed as two separate routes ("direct", "direct_again"): their difference is the spread a gain has to
beat before the default rule (batch_brick_default, csrc/pi_abi.hip) sends a class of batches to the bricks.

Shapes: the 3D batch shapes of tools/batch_throughput.py (48^3 x 300, B = 8 and 64) and 128^3 x 32, B = 4; blocks: the
reference's Hc = 2 cell as the factored block (--hc 2) and as its pre-contracted polynomial (--hc 0, the cells' default).  Timed with HIP events over regions of at least
--seconds after warm-up, best of --repeats per route.  Prints ONE JSON line and, with --out, writes it to that file.

    python tools/batch_brick_throughput.py [--cases 48x48x48:300:8,48x48x48:300:64,128x128x128:32:4] [--hc 2,0] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import percnn_amd as pa  # noqa: E402
from percnn_amd import _lib, ops  # noqa: E402
from batch_throughput import timed  # noqa: E402

ROUTES = (("brick", "brick3d=2"), ("direct", "brick3d=0"), ("direct_again", "brick3d=0"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="48x48x48:300:8,48x48x48:300:64,128x128x128:32:4")
    ap.add_argument("--hc", default="2,0")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ops.load_native()
    dev = torch.device("cuda:0")
    R = torch.ops.percnn
    out = {"metric": "fwd+bwd sample-steps/s of one batched call, best of %d regions of >= %g s" % (args.repeats, args.seconds),
           "routes": dict(ROUTES), "rows": []}
    for hc in (int(h) for h in args.hc.split(",")):
        torch.manual_seed(0)
        cell = pa.gs3d_cell(2, reaction="poly" if hc == 0 else "factored").to(dev)
        P = cell.param_block().detach()
        assert P.numel() == (36 if hc == 0 else 16 + 2 * (10 * hc + 1)), P.shape
        for spec in args.cases.split(","):
            s, T, B = spec.split(":")
            shape, T, B = tuple(int(x) for x in s.split("x")), int(T), int(B)
            plan = _lib.batch_plan(hc, shape, 4, B, "brick3d=2")
            h0 = (0.5 + 0.3 * torch.rand((B, 2) + shape, device=dev)).contiguous()
            g = torch.randn((T + 1, B, 2) + shape, device=dev)
            best = {}
            for _ in range(args.repeats):
                for name, opt in ROUTES:
                    def call():
                        tr = R.pi_rollout_batched(h0, P, T, opt)
                        R.pi_rollout_batched_backward(tr, P, g, opt)
                    best[name] = max(best.get(name, 0.0), timed(call, args.seconds) * B * T)
            spread = abs(best["direct"] - best["direct_again"]) / min(best["direct"], best["direct_again"])
            direct = max(best["direct"], best["direct_again"])
            row = {"shape": list(shape), "hc": hc, "T": T, "B": B, "points_per_sample": int(torch.tensor(shape).prod()),
                   "plan_brick3d_2": plan, "brick": round(best["brick"]), "direct": round(best["direct"]),
                   "direct_again": round(best["direct_again"]), "spread": round(spread, 4), "gain": round(best["brick"] / direct - 1, 4),
                   "default_now": _lib.batch_plan(hc, shape, 4, B, None)}
            out["rows"].append(row)
            print("# " + json.dumps(row), file=sys.stderr, flush=True)
            del g, h0
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
