"""Stage-2 library moments: ONE ``library_moments`` call against the stock-torch route on the same device.

Workload: 100 frames x 100^2, float32, interior region, the reference's split (keep 20 %, train 80 % of those) -- the size of
the reference's own Stage-2 run.  The stock-torch route builds the 70 columns in float64 with torch ops (rolls for the stencils,
products for the library), keeps the rows of each class by the same hash (evaluated once, outside the timed region: the stock
route gets its row indices for free) and forms ``Theta^T Theta``, ``Theta^T y`` and ``y^T y`` per class with matmuls.  Both
routes are compared before anything is timed.  Timed with HIP events over a region of at least --seconds after warm-up; the
two routes alternate --repeats times and every time is kept.  The spread of a route is (max - min) / min of its own repeats.

    python tools/stage2_moments_bench.py [--seconds 1.0] [--repeats 5] [--out profiles/stage2_library_moments.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import percnn_amd as pa  # noqa: E402
from percnn_amd.discovery import REFERENCE_SPLIT, row_class, split_thresholds  # noqa: E402

N, H, W, DX, DT = 100, 100, 100, 1.0 / 100, 2.5e-4


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


def stock_route(traj, idx):
    """the reference's library with stock torch ops in float64, interior points, rows of class c = idx[c]"""
    h = traj.double()
    u, v = h[:N - 2, 0], h[:N - 2, 1]
    ut, vt = (h[1:N - 1, 0] - u) / DT, (h[1:N - 1, 1] - v) / DT

    def d1(f, ax):
        return (torch.roll(f, 2, ax) - 8 * torch.roll(f, 1, ax) + 8 * torch.roll(f, -1, ax) - torch.roll(f, -2, ax)) / (12 * DX)

    def lap(f):
        s = -5.0 * f
        for ax in (1, 2):
            s = s + (-1 / 12) * (torch.roll(f, 2, ax) + torch.roll(f, -2, ax)) + (4 / 3) * (torch.roll(f, 1, ax) + torch.roll(f, -1, ax))
        return s / DX ** 2

    Bs = [torch.ones_like(u), d1(u, 1), d1(u, 2), d1(v, 1), d1(v, 2), lap(u), lap(v)]
    As = [torch.ones_like(u), u, v, u * u, u * v, v * v, u ** 3, u * u * v, u * v * v, v ** 3]
    sl = (slice(None), slice(2, H - 2), slice(2, W - 2))
    theta = torch.stack([(a * b)[sl].reshape(-1) for a in As for b in Bs], dim=1)
    y = torch.stack([ut[sl].reshape(-1), vt[sl].reshape(-1)], dim=1)
    out = []
    for c in (0, 1):
        X, Y = theta[idx[c]], y[idx[c]]
        out.append((X.T @ X, X.T @ Y, (Y * Y).sum(0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage2_library_moments.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stage2_moments_bench.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    traj = (0.5 * torch.randn((N, 2, H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(0))).float()
    seed, t_train, t_keep = split_thresholds(REFERENCE_SPLIT)
    r = np.arange((N - 2) * H * W, dtype=np.int64).reshape(N - 2, H, W)[:, 2:H - 2, 2:W - 2].reshape(-1)
    cls = row_class(r, seed, t_train, t_keep)
    idx = [torch.from_numpy(np.flatnonzero(cls == c)).to(dev) for c in (0, 1)]

    def ours():
        return pa.library_moments(traj, DX, DT, region="interior", split=REFERENCE_SPLIT)

    def stock():
        return stock_route(traj, idx)

    # same results first (the project's float64 reduction bar, relative to the diagonals)
    m, s = ours(), stock()
    worst = 0.0
    for c in (0, 1):
        dg = torch.sqrt(torch.diagonal(s[c][0]))
        worst = max(worst, float(((m.G[c] - s[c][0]).abs() / (dg[:, None] * dg[None, :])).max()))
        worst = max(worst, float(((m.b[c] - s[c][1]).abs() / (dg[:, None] * torch.sqrt(s[c][2])[None, :])).max()))
    rows_ok = [int(m.n[c]) == int(idx[c].numel()) for c in (0, 1)]
    del m, s
    times = {"library_moments": [], "stock_torch": []}
    for _ in range(args.repeats):
        for key, fn in (("library_moments", ours), ("stock_torch", stock)):
            times[key].append(round(timed(fn, args.seconds), 4))
    spread = {k: round((max(v) - min(v)) / min(v), 4) for k, v in times.items()}
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"metric": "ms per call: second moments of the 70-term library, both row classes",
           "workload": {"frames": N, "shape": [H, W], "dtype": "float32", "region": "interior", "split": list(REFERENCE_SPLIT),
                        "rows_kept": [int(i.numel()) for i in idx]},
           "device": torch.cuda.get_device_name(0), "seconds_per_region": args.seconds,
           "library_moments_ms": times["library_moments"], "stock_torch_ms": times["stock_torch"], "spread": spread,
           "ratio_stock_over_library_moments_median": round(med["stock_torch"] / med["library_moments"], 2),
           "not_slower_beyond_spread": med["library_moments"] <= med["stock_torch"] * (1 + max(spread.values())),
           "max_scaled_difference_between_routes": worst, "row_counts_equal": all(rows_ok)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
