"""Ensemble rollouts: forward + backward sample-steps/s of ONE ensemble call (one parameter block per sample) against B
sequential unbatched calls.

For the reference's own grids -- gs2d_100 (100^2, Hc = 8, float32, T = 200) and gs3d_48 (48^3, Hc = 2, float32, T = 300) --
and B in {1, 2, 4, 8, 16, 32, 64}: torch.ops.percnn.pi_rollout_ensemble + pi_rollout_ensemble_backward on [B,2,*S] with B
distinct blocks (B seeds of the workload's cell) against B x (pi_rollout + pi_rollout_backward) on [1,2,*S], each sample with
its own block, in the same process.  Timed with HIP events over a region of at least --seconds after warm-up (the timing of
tools/batch_throughput.py).  Prints ONE JSON line.

    python tools/ensemble_throughput.py [--workloads gs2d_100,gs3d_48] [--batches 1,2,4,8,16,32,64] [--seconds 1.0]
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
    """calls per second of fn, over a region of >= `seconds` (HIP events)"""
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
        batches = [int(b) for b in args.batches.split(",")]
        blocks = []
        for s in range(max(batches)):                      # one cell per seed: B distinct blocks, the dt of the cell
            torch.manual_seed(s)
            blocks.append(mk(hc).to(dev).param_block().detach())
        rows = []
        for B in batches:
            P = torch.stack(blocks[:B]).contiguous()
            h0 = (0.5 + 0.3 * torch.rand((B, 2) + shape, device=dev)).contiguous()
            g = torch.randn((T + 1, B, 2) + shape, device=dev)

            def ensemble():
                tr = R.pi_rollout_ensemble(h0, P, T)
                R.pi_rollout_ensemble_backward(tr, P, g)

            singles = [(h0[b:b + 1].contiguous(), P[b].contiguous(), g[:, b].contiguous()) for b in range(B)]

            def sequential():
                for hb, pb, gb in singles:
                    tr = R.pi_rollout(hb, pb, T)
                    R.pi_rollout_backward(tr, pb, gb)

            re = timed(ensemble, args.seconds) * B * T
            rs = timed(sequential, args.seconds) * B * T
            rows.append({"B": B, "ensemble": round(re), "sequential": round(rs), "speedup": round(re / rs, 3)})
            print(f"# {name} B={B}: ensemble {re:.4g} sequential {rs:.4g} sample-steps/s", file=sys.stderr, flush=True)
            del g, h0, singles
            torch.cuda.empty_cache()
        out["results"][name] = {"shape": list(shape), "hc": hc, "T": T, "rows": rows}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
