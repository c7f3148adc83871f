"""Per-sample squared-error loss of a batch / an ensemble: forward + backward sample-steps/s and peak memory of the ONE-node
loss (pa.pi_rollout_sqerr_batched / pa.pi_rollout_sqerr_ensemble, loss.mean().backward(): the loss gradient is formed inside
the sweep) against the materialised route (pa.pi_rollout_batched / pa.pi_rollout_ensemble, F.mse_loss, backward(): autograd
writes a dL/dtraj [T+1,B,2,*S] that the sweep reads back).

The project's batch shapes: gs2d_100 (100^2, Hc = 8, float32, T = 200) with B = 16 and 64, gs3d_48 (48^3, Hc = 2, float32,
T = 300) with B = 8.  Timed with HIP events over a region of at least --seconds after warm-up; peak memory is
torch.cuda.max_memory_allocated over the timed region, minus what the inputs hold.  Prints ONE JSON line.

    python tools/batch_loss_throughput.py [--routes one_node,materialised] [--kinds batch,ensemble] [--seconds 1.0]
                                          [--package-root DIR]

--package-root: import percnn_amd from another checkout (a build of the parent commit has only the materialised route)."""
import argparse
import json
import os
import sys

import torch

CASES = [("gs2d_100", 16), ("gs2d_100", 64), ("gs3d_48", 8)]


def timed(fn, seconds):
    """calls per second of fn over a region of >= `seconds` (HIP events), and the peak of allocated memory in it"""
    fn()
    torch.cuda.synchronize()
    n, elapsed = 1, 0.0
    while True:
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        elapsed = a.elapsed_time(b) / 1e3
        if elapsed >= seconds:
            return n / elapsed, torch.cuda.max_memory_allocated()
        n = max(n + 1, int(n * 1.2 * seconds / max(elapsed, 1e-4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--routes", default="one_node,materialised")
    ap.add_argument("--kinds", default="batch,ensemble")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import percnn_amd as pa
    from percnn_amd import ops
    ops.load_native()
    workloads = {"gs2d_100": (pa.gs2d_cell, 8, (100, 100), 200), "gs3d_48": (pa.gs3d_cell, 2, (48, 48, 48), 300)}
    dev = torch.device("cuda:0")
    out = {"metric": "fwd+bwd sample-steps/s; peak_mib = max_memory_allocated over the timed region minus the inputs",
           "package_root": os.path.relpath(args.package_root), "rows": []}
    for name, B in CASES:
        mk, hc, shape, T = workloads[name]
        torch.manual_seed(0)
        cell = mk(hc).to(dev)
        block = cell.param_block().detach()
        for kind in args.kinds.split(","):
            P = (block if kind == "batch" else block.repeat(B, 1).contiguous()).requires_grad_(True)
            h0 = (0.5 + 0.3 * torch.rand((B, 2) + shape, device=dev)).requires_grad_(True)
            target = torch.rand((T + 1, B, 2) + shape, device=dev)
            rollout = pa.pi_rollout_batched if kind == "batch" else pa.pi_rollout_ensemble

            def materialised():
                h0.grad = P.grad = None
                torch.nn.functional.mse_loss(rollout(h0, P, T), target).backward()

            def one_node():
                h0.grad = P.grad = None
                op = pa.pi_rollout_sqerr_batched if kind == "batch" else pa.pi_rollout_sqerr_ensemble
                op(h0, P, T, target)[0].mean().backward()

            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            for route in args.routes.split(","):
                rate, peak = timed({"materialised": materialised, "one_node": one_node}[route], args.seconds)
                row = {"workload": name, "B": B, "kind": kind, "route": route, "sample_steps_per_s": round(rate * B * T),
                       "peak_mib": round((peak - base) / 2 ** 20, 1), "trajectory_mib": round(target.numel() * 4 / 2 ** 20, 1)}
                out["rows"].append(row)
                print(f"# {row}", file=sys.stderr, flush=True)
            del h0, P, target
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
