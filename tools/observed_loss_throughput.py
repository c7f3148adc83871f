"""Per-sample loss on sparse observations of a batch / an ensemble: forward + backward sample-steps/s and peak memory of
RCNN.sample_losses(space_stride=...) (the loss gradient is formed inside the sweep at the lattice points, no dL/dtraj) against
the materialised route (pa.pi_rollout_batched / pa.pi_rollout_ensemble, the strided slice, F.mse_loss, backward(): autograd
writes a dense, almost entirely zero dL/dtraj [T+1,B,2,*S] that the sweep reads back).

The project's batch shapes with the reference's observation patterns: gs2d_100 (100^2, Hc = 8, float32, T = 200), frames
[0:-1:20], stride 4, B = 16 and 64; gs3d_48 (48^3, Hc = 2, float32, T = 300), frames [:-1:15], stride 2, B = 8.  Timed with HIP
events over a region of at least --seconds after warm-up; peak memory is torch.cuda.max_memory_allocated over the timed region,
minus what the inputs hold.  Prints ONE JSON line.

    python tools/observed_loss_throughput.py [--routes in_sweep,materialised] [--kinds batch,ensemble] [--seconds 1.0]
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
    ap.add_argument("--routes", default="in_sweep,materialised")
    ap.add_argument("--kinds", default="batch,ensemble")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import percnn_amd as pa
    from percnn_amd import ops
    ops.load_native()
    # (cell constructor, Hc, grid, T, observed frames, space stride)
    workloads = {"gs2d_100": (pa.gs2d_cell, 8, (100, 100), 200, slice(0, -1, 20), 4),
                 "gs3d_48": (pa.gs3d_cell, 2, (48, 48, 48), 300, slice(None, -1, 15), 2)}
    dev = torch.device("cuda:0")
    out = {"metric": "fwd+bwd sample-steps/s; peak_mib = max_memory_allocated over the timed region minus the inputs",
           "package_root": os.path.relpath(args.package_root), "rows": []}
    for name, B in CASES:
        mk, hc, shape, T, tsl, s = workloads[name]
        sub = (slice(None),) * 3 + (slice(None, None, s),) * len(shape)
        torch.manual_seed(0)
        cells = [mk(hc).to(dev) for _ in range(B)]
        for kind in args.kinds.split(","):
            cell = cells[0] if kind == "batch" else pa.CellEnsemble(cells)
            h0 = 0.5 + 0.3 * torch.rand((B, 2) + shape, device=dev)
            model = pa.RCNN(cell, step=T, effective_step=list(range(T)), init_state=h0)
            with torch.no_grad():
                target = torch.rand_like(model.trajectory()[tsl][sub])

            def materialised():
                cell.zero_grad(set_to_none=True)
                torch.nn.functional.mse_loss(model.trajectory()[tsl][sub], target).backward()

            def in_sweep():
                cell.zero_grad(set_to_none=True)
                model.sample_losses(target, tsl, space_stride=s).mean().backward()

            torch.cuda.synchronize()
            model.last_trajectory = None
            base = torch.cuda.memory_allocated()
            for route in args.routes.split(","):
                rate, peak = timed({"materialised": materialised, "in_sweep": in_sweep}[route], args.seconds)
                model.last_trajectory = None
                row = {"workload": name, "B": B, "kind": kind, "route": route, "frames": len(range(T + 1)[tsl]), "stride": s,
                       "sample_steps_per_s": round(rate * B * T), "peak_mib": round((peak - base) / 2 ** 20, 1),
                       "trajectory_mib": round((T + 1) * h0.numel() * 4 / 2 ** 20, 1)}
                out["rows"].append(row)
                print(f"# {row}", file=sys.stderr, flush=True)
            del h0, target, model
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
