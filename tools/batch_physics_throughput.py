"""Physics-residual loss per sample: forward + backward of ONE physics_loss_batched call against B sequential unbatched
physics_loss calls on the same data.

For the reference's own grids -- gs2d_100 (100^2, float32, 200 residual frames) at B = 16 and 64, gs3d_48 (48^3, float32, 300
frames) at B = 8: ``physics.physics_loss_batched(traj, Q).sum().backward()`` on a frame-major trajectory [F+2, B, 2, *S] against
B x ``physics.physics_loss(traj[:, b].contiguous(), Q).backward()`` in the same process -- the ``contiguous()`` copies that route
needs are inside its timed region.  Timed with HIP events over a region of at least --seconds after warm-up; the two routes
alternate --repeats times and every time is kept.  ``torch.cuda.max_memory_allocated`` is read after each route's first timed
region, from a reset counter.  The outputs of the two routes are compared before anything is timed.  Prints ONE JSON line.

    python tools/batch_physics_throughput.py [--cases gs2d_100:16,gs2d_100:64,gs3d_48:8] [--seconds 1.0] [--repeats 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import percnn_amd as pa  # noqa: E402
from percnn_amd import physics  # noqa: E402

WORKLOADS = {"gs2d_100": (pa.gs2d_cell, (100, 100), 200, (2e-5, 5e-6, 1 / 25, 3 / 50)),
             "gs3d_48": (pa.gs3d_cell, (48, 48, 48), 300, (0.2, 0.1, 0.025, 0.055))}


def timed(fn, seconds):
    """milliseconds per call of fn, over a region of >= `seconds` (HIP events)"""
    fn()
    torch.cuda.synchronize()
    n = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        elapsed = a.elapsed_time(b) / 1e3
        if elapsed >= seconds:
            return 1e3 * elapsed / n
        n = max(n + 1, int(n * 1.2 * seconds / max(elapsed, 1e-4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="gs2d_100:16,gs2d_100:64,gs3d_48:8")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("batch_physics_throughput.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    out = {"metric": "ms per forward + backward of the residual loss of B trajectories", "rows": []}
    for case in args.cases.split(","):
        name, B = case.split(":")
        B = int(B)
        mk, shape, F, coef = WORKLOADS[name]
        cell = mk().to(dev)
        Q = physics.gray_scott_block(cell, *coef)
        traj = torch.rand((F + 2, B, 2) + shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0)).requires_grad_(True)

        def batched():
            traj.grad = None
            physics.physics_loss_batched(traj, Q).sum().backward()
            return traj.grad

        def sequential():
            gs = []
            for b in range(B):
                o = traj.detach()[:, b].contiguous().requires_grad_(True)
                physics.physics_loss(o, Q).backward()
                gs.append(o.grad)
            return gs

        # same results first: gradients bit for bit, values to the order of the float64 sums
        gb, gs = batched(), sequential()
        lb = physics.physics_loss_batched(traj.detach(), Q)
        ls = torch.stack([physics.physics_loss(traj.detach()[:, b].contiguous(), Q) for b in range(B)])
        same_grad = all(torch.equal(gb[:, b], gs[b]) for b in range(B))
        loss_err = float(((lb - ls).abs() / ls.abs()).max())
        del gb, gs
        times, mem = {"batched": [], "sequential": []}, {}
        for r in range(args.repeats):
            for key, fn in (("batched", batched), ("sequential", sequential)):
                if r == 0:
                    traj.grad = None
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                times[key].append(round(timed(fn, args.seconds), 4))
                if r == 0:
                    mem[key] = torch.cuda.max_memory_allocated()
        tb, ts = min(times["batched"]), min(times["sequential"])
        row = {"workload": name, "shape": list(shape), "frames": F, "B": B, "dtype": "float32", "batched_ms": times["batched"],
               "sequential_ms": times["sequential"], "speedup_best_of": round(ts / tb, 3),
               "max_memory_allocated_batched": mem["batched"], "max_memory_allocated_sequential": mem["sequential"],
               "gradients_bit_identical": same_grad, "loss_max_rel_diff": loss_err}
        out["rows"].append(row)
        print("# " + json.dumps(row), file=sys.stderr, flush=True)
        del traj
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
