"""Batched rollouts: forward + backward sample-steps/s of ONE batched call against B sequential unbatched calls.

For the reference's own grids -- gs2d_100 (100^2, Hc = 8, float32, T = 200) and gs3d_48 (48^3, Hc = 2, float32, T = 300) --
and B in {1, 2, 4, 8, 16, 32, 64}: torch.ops.percnn.pi_rollout_batched + pi_rollout_batched_backward on [B,2,*S] against
B x (pi_rollout + pi_rollout_backward) on [1,2,*S] in the same process.  Timed with HIP events over a region of at least
--seconds after warm-up.  Prints ONE JSON line.

    python tools/batch_throughput.py [--workloads gs2d_100,gs3d_48] [--batches 1,2,4,8,16,32,64] [--seconds 1.0]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import percnn_amd as pa  # noqa: E402
from percnn_amd import ops  # noqa: E402

WORKLOADS = {"gs2d_100": (pa.gs2d_cell, 8, (100, 100), 200), "gs3d_48": (pa.gs3d_cell, 2, (48, 48, 48), 300)}


def timed(fn, seconds):
    """sample-step throughput: calls per second of fn, over a region of >= `seconds` (HIP events)"""
    fn()
    torch.cuda.synchronize()
    n, elapsed = 1, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        elapsed = a.elapsed_time(b) / 1e3
        if elapsed >= seconds:
            return n / elapsed
        n = max(n + 1, int(n * 1.2 * seconds / max(elapsed, 1e-4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="gs2d_100,gs3d_48")
    ap.add_argument("--batches", default="1,2,4,8,16,32,64")
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    ops.load_native()
    dev = torch.device("cuda:0")
    R = torch.ops.percnn
    out = {"metric": "fwd+bwd sample-steps/s", "results": {}}
    for name in args.workloads.split(","):
        mk, hc, shape, T = WORKLOADS[name]
        torch.manual_seed(0)
        cell = mk(hc).to(dev)
        P = cell.param_block().detach()
        rows = []
        for B in (int(b) for b in args.batches.split(",")):
            h0 = (0.5 + 0.3 * torch.rand((B, 2) + shape, device=dev)).contiguous()
            g = torch.randn((T + 1, B, 2) + shape, device=dev)
            traj = R.pi_rollout_batched(h0, P, T)

            def batched():
                tr = R.pi_rollout_batched(h0, P, T)
                R.pi_rollout_batched_backward(tr, P, g)

            singles = [(h0[b:b + 1].contiguous(), g[:, b].contiguous()) for b in range(B)]

            def sequential():
                for hb, gb in singles:
                    tr = R.pi_rollout(hb, P, T)
                    R.pi_rollout_backward(tr, P, gb)

            rb = timed(batched, args.seconds) * B * T
            rs = timed(sequential, args.seconds) * B * T
            rows.append({"B": B, "batched": round(rb), "sequential": round(rs), "speedup": round(rb / rs, 3)})
            print(f"# {name} B={B}: batched {rb:.4g} sequential {rs:.4g} sample-steps/s", file=sys.stderr, flush=True)
            del traj, g, h0, singles
            torch.cuda.empty_cache()
        out["results"][name] = {"shape": list(shape), "hc": hc, "T": T, "rows": rows}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
