"""Library cell: one Stage-3 fine-tuning iteration (rollout forward + backward) of the Burgers equation on three routes.

Workload: 100^2, float64, 200 explicit Euler steps, the reference's Stage-3 Burgers parameters, loss = mean(traj^2).
  (a) library_cell    ``LibraryCell.from_cell(Stage3BurgersCell())``: csrc/pi_lib.h, one launch per step and per adjoint step
  (b) stage3_burgers  ``Stage3BurgersCell`` on the advective kernels (csrc/pi_adv.h): this one equation's hand-written path
  (c) stock_torch     the same step on stock tensor operations (rolls for the stencils, the equation's six terms only) with
                      stock autograd: what a user whose Stage-2 run returned any OTHER equation had before the library cell
  (d) library_cell_dense  (a) with 140 random coefficients on the same state: no column is skipped
The routes are compared before anything is timed.  Timed with HIP events over a region of at least --seconds after warm-up;
the routes alternate --repeats times and every time is kept.  The spread of a route is (max - min) / min of its own repeats.

    python tools/library_cell_bench.py [--seconds 1.0] [--repeats 5] [--out profiles/library_cell.json]

``--integrator rk4``: the same workload with the classical Runge-Kutta step, 200 steps, on two routes
  (e) library_cell_rk4  ``LibraryCell.from_cell(Stage3BurgersCell(), integrator="rk4")``: one fused launch per step forward, one
                        recompute launch and four stage launches per step backward
  (f) stock_torch_rk4   a ``Stage3BurgersCell.forward_rk4`` loop with stock autograd
next to (a), whose Euler step times four is the yardstick.  Forward only (no tape) and forward + backward of every route; the
result goes to profiles/library_cell_rk4.json.

``--ensemble B[,B...]`` (e.g. ``1,2,4,8,16``): the same workload with one Burgers equation per member (the Stage-3 parameters
scaled by 1 + b / 100, the state shifted by 7 b columns), both integrators, forward only and forward + backward, on two routes
  (g) ensemble    ONE ``LibraryEnsemble`` rollout: B members in the launches of one (the sample index on blockIdx.z)
  (h) sequential  B ``LibraryCell`` rollouts one after the other, what a user had before the ensemble
compared bit for bit before anything is timed, alternating; microseconds per step of the whole ensemble.  Where B x tiles crosses
``rk4_tile``'s 256 workgroups the Runge-Kutta forward launch switches to its 16-wide tile: route (g)'s Runge-Kutta timings are
repeated in child processes on two builds with the tile pinned (``-DPERCNN_PI_LIB_RK4_TILE=8`` / ``=16``, built once into
tools/scratch/; ``--rebuild-tiles`` builds them again).  The result goes to profiles/library_cell_ensemble.json.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import percnn_amd as pa  # noqa: E402
from percnn_amd import _lib  # noqa: E402

H = W = 100
STEPS = 200


def timed(fn, seconds):
    """microseconds per call of fn, over a region of >= `seconds` (HIP events)"""
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
            return 1e6 * elapsed / n
        n = max(n + 1, int(n * 1.2 * seconds / max(elapsed, 1e-4)))


def stock_rollout(h0, terms, dx, dt, steps):
    """terms: per species a list of (coefficient tensor, monomial index, factor index); -> [steps+1,2,H,W]"""
    def d1(f, ax):
        return ((torch.roll(f, 2, ax) - torch.roll(f, -2, ax)) + 8.0 * (torch.roll(f, -1, ax) - torch.roll(f, 1, ax))) * (1.0 / (12.0 * dx))

    def lap(f):
        return ((-1.0 / 12.0) * ((torch.roll(f, 2, 0) + torch.roll(f, -2, 0)) + (torch.roll(f, 2, 1) + torch.roll(f, -2, 1)))
                + (4.0 / 3.0) * ((torch.roll(f, 1, 0) + torch.roll(f, -1, 0)) + (torch.roll(f, 1, 1) + torch.roll(f, -1, 1)))
                - 5.0 * f) * (1.0 / (dx * dx))

    mono = [lambda u, v: None, lambda u, v: u, lambda u, v: v, lambda u, v: u * u, lambda u, v: u * v, lambda u, v: v * v,
            lambda u, v: u * u * u, lambda u, v: u * u * v, lambda u, v: u * v * v, lambda u, v: v * v * v]
    fact = [lambda u, v: None, lambda u, v: d1(u, 0), lambda u, v: d1(u, 1), lambda u, v: d1(v, 0), lambda u, v: d1(v, 1),
            lambda u, v: lap(u), lambda u, v: lap(v)]
    frames = [h0[0]]
    for _ in range(steps):
        u, v = frames[-1][0], frames[-1][1]
        nxt = []
        for s, h in enumerate((u, v)):
            rhs = 0.0
            for c, m, k in terms[s]:
                a, b = mono[m](u, v), fact[k](u, v)
                t = c if a is None and b is None else (c * b if a is None else (c * a if b is None else c * a * b))
                rhs = rhs + t
            nxt.append(h + dt * rhs)
        frames.append(torch.stack(nxt))
    return torch.stack(frames)


def resource_usage():
    """registers / scratch / LDS of the library cell's kernels, from a compile of its translation unit (no GPU work)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + _lib.HIPCC_FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                                       os.path.join(_lib.CSRC, "pi_lib_abi.hip")]
    try:
        err = subprocess.run(cmd, cwd=_lib.CSRC, capture_output=True, text=True, check=True).stderr
    except (OSError, subprocess.CalledProcessError) as e:
        return {"error": str(e)}
    out, cur = {}, None
    for line in err.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
            m = re.search(r"rk4_kernelILi(\d+)ELb([01])E", name)      # rk4_kernel<FT, STAGES>
            if m:
                name = f"rk4_kernel<{m.group(1)}, {'stages' if m.group(2) == '1' else 'step'}>"
            cur = out.setdefault(next((k for k in ("step_kernel", "adjoint_kernel", "finish_kernel", "rk4_stage_kernel") if k in name),
                                      name), {})
        elif cur is not None:
            for key in ("VGPRs:", "AGPRs:", "TotalSGPRs:", "ScratchSize [bytes/lane]:", "LDS Size [bytes/block]:", "Occupancy [waves/SIMD]:"):
                if " " + key in line:
                    cur[key.rstrip(":")] = int(line.split(key)[1].split()[0])
    return out


def burgers_state(dev):
    ys = torch.arange(H, dtype=torch.float64) / H
    yy, xx = torch.meshgrid(ys, ys, indexing="ij")
    tp = 2 * np.pi
    u = torch.sin(tp * xx) * torch.cos(tp * yy) + 0.3 * torch.cos(2 * tp * xx + 0.5)
    v = torch.cos(tp * xx) * torch.sin(tp * yy) - 0.2 * torch.sin(tp * (xx + 2 * yy))
    return torch.stack((u, v))[None].to(dev).requires_grad_(True)


def main_rk4(args, dev):
    stage3 = pa.Stage3BurgersCell().to(dev)
    euler = pa.LibraryCell.from_cell(stage3)
    cell = pa.LibraryCell.from_cell(stage3, integrator="rk4")
    h0 = burgers_state(dev)
    names = list(pa.Stage3BurgersCell.INIT)
    where = {"nu_u": (0, 0, 5), "C1_u": (0, 1, 1), "C2_u": (0, 2, 2), "nu_v": (1, 0, 6), "C1_v": (1, 1, 3), "C2_v": (1, 2, 4)}

    def stock(h):
        frames = [h]
        for _ in range(STEPS):
            frames.append(stage3.forward_rk4(frames[-1])[0])
        return torch.cat(frames, 0)

    def fwd_only(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def grads_of(traj, params):
        return torch.autograd.grad((traj ** 2).mean(), params + [h0])

    forward = {"library_cell": lambda: euler.rollout(h0, STEPS), "library_cell_rk4": lambda: cell.rollout(h0, STEPS),
               "stock_torch_rk4": lambda: stock(h0)}
    params = {"library_cell": [euler.coef], "library_cell_rk4": [cell.coef], "stock_torch_rk4": [getattr(stage3, n) for n in names]}
    routes = {}
    for key, fn in forward.items():
        routes[key + "/fwd"] = fwd_only(fn)
        routes[key + "/fwd_bwd"] = (lambda fn=fn, key=key: grads_of(fn(), params[key]))

    # same results first: the trajectory, the six scalar gradients and dL/dh0 of the two Runge-Kutta routes
    ta, tb = routes["library_cell_rk4/fwd"](), routes["stock_torch_rk4/fwd"]()
    ga, gb = routes["library_cell_rk4/fwd_bwd"](), routes["stock_torch_rk4/fwd_bwd"]()
    a6 = torch.stack([ga[0][where[n]] for n in names])
    diff = {"trajectory_rel_l2": float((ta - tb).norm() / tb.norm()),
            "six_gradients_max_relative": float(((a6 - torch.stack(gb[:6])).abs() / torch.stack(gb[:6]).abs()).max()),
            "dLdh0_rel_l2": float((ga[1] - gb[6]).norm() / gb[6].norm()),
            "rk4_vs_euler_trajectory_rel_l2": float((ta - routes["library_cell/fwd"]()).norm() / ta.norm())}
    if not (diff["trajectory_rel_l2"] < 1e-12 and diff["six_gradients_max_relative"] < 1e-9 and diff["dLdh0_rel_l2"] < 1e-11):
        sys.exit(f"library_cell_bench.py: the Runge-Kutta routes disagree: {diff}")
    del ta, tb, ga, gb

    times = {k: [] for k in routes}
    for _ in range(args.repeats):
        for key, fn in routes.items():
            times[key].append(round(timed(fn, args.seconds) / STEPS, 3))
    spread = {k: round((max(v) - min(v)) / min(v), 4) for k, v in times.items()}
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"metric": "microseconds per step: rollout forward only (no tape) and forward + backward (one fine-tuning iteration / steps)",
           "workload": {"shape": [H, W], "dtype": "float64", "steps": STEPS, "equation": "Burgers (Stage3BurgersCell.INIT)",
                        "loss": "mean(traj^2)", "step": "classical Runge-Kutta; library_cell: explicit Euler, the yardstick"},
           "device": torch.cuda.get_device_name(0), "seconds_per_region": args.seconds, "library": os.path.basename(_lib.LIB_PATH),
           "us_per_step": times, "median": med, "spread": spread,
           "four_euler_steps": {"fwd": round(4 * med["library_cell/fwd"], 3), "fwd_bwd": round(4 * med["library_cell/fwd_bwd"], 3)},
           "rk4_fwd_below_four_euler_fwd": med["library_cell_rk4/fwd"] < 4 * med["library_cell/fwd"],
           "rk4_fwd_bwd_below_four_euler_fwd_bwd": med["library_cell_rk4/fwd_bwd"] < 4 * med["library_cell/fwd_bwd"],
           "library_cell_rk4_median_below_stock_torch_rk4_min":
               med["library_cell_rk4/fwd_bwd"] < min(times["stock_torch_rk4/fwd_bwd"]),
           "ratio_library_cell_rk4_over_stock_torch_rk4": {k: round(med["library_cell_rk4/" + k] / med["stock_torch_rk4/" + k], 5)
                                                           for k in ("fwd", "fwd_bwd")},
           "max_relative_difference_between_routes": diff, "kernel_resources": resource_usage()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    if not out["library_cell_rk4_median_below_stock_torch_rk4_min"]:
        sys.exit("library_cell_bench.py: the Runge-Kutta library cell's median is not below the stock route's minimum")


def tile_library(tile, rebuild=False):
    """libpercnn_pi.so with the Runge-Kutta forward tile pinned: csrc/pi_lib_abi.hip compiled with -DPERCNN_PI_LIB_RK4_TILE,
    linked with the committed build's other objects"""
    scratch = os.path.join(ROOT, "tools", "scratch")
    out = os.path.join(scratch, f"libpercnn_pi_rk4tile{tile}.so")
    if os.path.exists(out) and not rebuild:
        return out
    os.makedirs(scratch, exist_ok=True)
    _lib.build()                                            # the objects of the other translation units
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = os.path.join(scratch, f"pi_lib_abi_rk4tile{tile}.o")
    subprocess.check_call([hipcc] + _lib.HIPCC_FLAGS + [f"-DPERCNN_PI_LIB_RK4_TILE={tile}", "-c", "-o", obj,
                                                         os.path.join(_lib.CSRC, "pi_lib_abi.hip")], cwd=_lib.CSRC)
    objs = [os.path.join(_lib.CSRC, src.replace(".hip", ".o")) for src in _lib.SOURCES if src != "pi_lib_abi.hip"] + [obj]
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out] + objs, cwd=_lib.CSRC)
    return out


def ensemble_routes(B, integrator, dev):
    """{"fwd/ensemble", "fwd/sequential", "fwd_bwd/ensemble", "fwd_bwd/sequential"} of B Burgers members"""
    cells = []
    for b in range(B):
        stage3 = pa.Stage3BurgersCell().to(dev)
        with torch.no_grad():
            for p in stage3.parameters():
                p.mul_(1.0 + b / 100.0)
        cells.append(pa.LibraryCell.from_cell(stage3, integrator=integrator))
    ens = pa.LibraryEnsemble(cells)
    base = burgers_state(dev).detach()
    h0 = torch.cat([torch.roll(base, 7 * b, -1) for b in range(B)]).requires_grad_(True)
    singles = [h0.detach()[b:b + 1].clone().requires_grad_(True) for b in range(B)]
    coefs = [c.coef for c in cells]

    def ensemble():
        return ens.rollout(h0, STEPS)

    def sequential():
        return [c.rollout(h, STEPS) for c, h in zip(cells, singles)]

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def ensemble_grads():
        t = ensemble()
        return torch.autograd.grad((t ** 2).sum() / t.numel(), coefs + [h0])

    def sequential_grads():
        # the ensemble's loss: the mean over all B trajectories
        return [torch.autograd.grad((t ** 2).sum() / (B * t.numel()), [c.coef, h]) for t, c, h in zip(sequential(), cells, singles)]

    routes = {"fwd/ensemble": no_grad(ensemble), "fwd/sequential": no_grad(sequential), "fwd_bwd/ensemble": ensemble_grads,
              "fwd_bwd/sequential": sequential_grads}
    # the same bits first: trajectories, coefficient gradients, dL/dh0
    te, ts = routes["fwd/ensemble"](), routes["fwd/sequential"]()
    ge, gs = ensemble_grads(), sequential_grads()
    same = all(torch.equal(te[:, b], ts[b]) and torch.equal(ge[b], gs[b][0]) and torch.equal(ge[B][b:b + 1], gs[b][1])
               for b in range(B))
    if not same:
        sys.exit(f"library_cell_bench.py: the ensemble and the sequential route differ at B = {B}, {integrator}")
    return routes


def time_routes(routes, args):
    """{route: [microseconds per step of the whole ensemble, one per repeat]}, the routes alternating"""
    times = {k: [] for k in routes}
    for _ in range(args.repeats):
        for key, fn in routes.items():
            times[key].append(round(timed(fn, args.seconds) / STEPS, 3))
    return times


def summary(times):
    return {"us_per_step": times, "median": {k: float(np.median(v)) for k, v in times.items()},
            "spread": {k: round((max(v) - min(v)) / min(v), 4) for k, v in times.items()}}


def main_ensemble_child(args, dev):
    """route (g) with the Runge-Kutta step only, on the library PERCNN_PI_LIB names: one JSON line"""
    out = {}
    for B in args.ensemble:
        routes = ensemble_routes(B, "rk4", dev)
        out[str(B)] = summary(time_routes({k: v for k, v in routes.items() if k.endswith("/ensemble")}, args))
    print("TILE_CHILD " + json.dumps(out))


def main_ensemble(args, dev):
    results = {}
    for B in args.ensemble:
        for integrator in ("euler", "rk4"):
            res = summary(time_routes(ensemble_routes(B, integrator, dev), args))
            med, t = res["median"], res["us_per_step"]
            res["sequential_over_ensemble"] = {m: round(med[m + "/sequential"] / med[m + "/ensemble"], 4) for m in ("fwd", "fwd_bwd")}
            # faster by more than the spread of both routes: the slowest ensemble repeat below the fastest sequential repeat
            res["every_ensemble_repeat_below_every_sequential_repeat"] = {
                m: max(t[m + "/ensemble"]) < min(t[m + "/sequential"]) for m in ("fwd", "fwd_bwd")}
            results.setdefault(str(B), {})[integrator] = res
            print(B, integrator, json.dumps(res["median"]), file=sys.stderr)
    tiles = {}
    for tile in (8, 16):
        env = dict(os.environ, PERCNN_PI_LIB=tile_library(tile, args.rebuild_tiles))
        cmd = [sys.executable, os.path.abspath(__file__), "--ensemble", ",".join(map(str, args.ensemble)), "--tile-child",
               "--seconds", str(args.seconds), "--repeats", str(args.repeats)]
        line = [ln for ln in subprocess.run(cmd, env=env, capture_output=True, text=True, check=True).stdout.splitlines()
                if ln.startswith("TILE_CHILD ")][-1]
        tiles[str(tile)] = json.loads(line[len("TILE_CHILD "):])
    def tile_rule(B):                                       # csrc/pi_lib.h: rk4_tile
        n8, n16 = B * ((H + 7) // 8) * ((W + 7) // 8), B * ((H + 15) // 16) * ((W + 15) // 16)
        if B == 1:
            return 8 if n8 <= 256 else 16
        return 8 if -(-n8 // 1280) * 5 < -(-n16 // 768) * 10 else 16

    rule = {str(B): tile_rule(B) for B in args.ensemble}
    out = {"metric": "microseconds per step of the whole ensemble (B members advance one step): rollout forward only (no tape) and "
                     "forward + backward (one fine-tuning iteration / steps)",
           "workload": {"shape": [H, W], "dtype": "float64", "steps": STEPS, "members": args.ensemble,
                        "equation": "Burgers (Stage3BurgersCell.INIT scaled by 1 + b / 100 per member)", "loss": "mean(traj^2)"},
           "routes": {"ensemble": "one LibraryEnsemble rollout", "sequential": "B LibraryCell rollouts one after the other"},
           "device": torch.cuda.get_device_name(0), "seconds_per_region": args.seconds, "repeats": args.repeats,
           "results": results,
           "rk4_tile": {"rule": rule, "ensemble_route_with_the_tile_pinned": tiles,
                        "note": "own processes on builds with -DPERCNN_PI_LIB_RK4_TILE; the tile changes no bit"}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    if 4 in args.ensemble:
        lost = [(i, m) for i in ("euler", "rk4") for m in ("fwd", "fwd_bwd")
                if not results["4"][i]["every_ensemble_repeat_below_every_sequential_repeat"][m]]
        if lost:
            sys.exit(f"library_cell_bench.py: at B = 4 the ensemble route is not faster than the sequential route beyond the "
                     f"spread of their repeats: {lost}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--integrator", choices=("euler", "rk4"), default="euler")
    ap.add_argument("--ensemble", default=None, type=lambda s: [int(b) for b in s.split(",")], metavar="B[,B...]")
    ap.add_argument("--rebuild-tiles", action="store_true")
    ap.add_argument("--tile-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "library_cell_ensemble.json" if args.ensemble else
                                "library_cell.json" if args.integrator == "euler" else "library_cell_rk4.json")
    if not torch.cuda.is_available():
        sys.exit("library_cell_bench.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    if args.ensemble:
        return main_ensemble_child(args, dev) if args.tile_child else main_ensemble(args, dev)
    if args.integrator == "rk4":
        return main_rk4(args, dev)
    stage3 = pa.Stage3BurgersCell().to(dev)
    dx, dt = stage3.dx, stage3.dt
    cell = pa.LibraryCell.from_cell(stage3)
    rng = np.random.default_rng(0)
    dense = pa.LibraryCell(0.1 * rng.standard_normal((2, 10, 7)) * np.array([1, 1, 1, 1, 1, 1e-4, 1e-4]), dx, dt,
                           support="dense").to(dev)            # diffusion-like columns scaled to dx^2: the rollout stays bounded
    h0 = burgers_state(dev)
    rcnn = pa.RCNN(stage3, step=STEPS, effective_step=list(range(STEPS)), init_state=h0)
    names = list(pa.Stage3BurgersCell.INIT)
    where = {"nu_u": (0, 0, 5), "C1_u": (0, 1, 1), "C2_u": (0, 2, 2), "nu_v": (1, 0, 6), "C1_v": (1, 1, 3), "C2_v": (1, 2, 4)}
    terms = [[(getattr(stage3, n), where[n][1], where[n][2]) for n in names if where[n][0] == s] for s in (0, 1)]

    def grads_of(traj, params):
        return torch.autograd.grad((traj ** 2).mean(), params + [h0])

    routes = {"library_cell": lambda: grads_of(cell.rollout(h0, STEPS), [cell.coef]),
              "stage3_burgers": lambda: grads_of(rcnn.trajectory(), [getattr(stage3, n) for n in names]),
              "stock_torch": lambda: grads_of(stock_rollout(h0, terms, dx, dt, STEPS), [getattr(stage3, n) for n in names]),
              "library_cell_dense": lambda: grads_of(dense.rollout(h0, STEPS), [dense.coef])}

    # same results first: the six scalar gradients and dL/dh0 of the three Burgers routes
    ga, gb, gc = routes["library_cell"](), routes["stage3_burgers"](), routes["stock_torch"]()
    a6 = torch.stack([ga[0][where[n]] for n in names])
    diff = {"library_cell_vs_stage3_burgers": float(((a6 - torch.stack(gb[:6])).abs() / torch.stack(gb[:6]).abs()).max()),
            "library_cell_vs_stock_torch": float(((a6 - torch.stack(gc[:6])).abs() / torch.stack(gc[:6]).abs()).max()),
            "dLdh0_vs_stage3_burgers_rel_l2": float((ga[1] - gb[6]).norm() / gb[6].norm()),
            "dLdh0_vs_stock_torch_rel_l2": float((ga[1] - gc[6]).norm() / gc[6].norm())}
    dense_finite = bool(torch.isfinite(routes["library_cell_dense"]()[0]).all())
    del ga, gb, gc

    times = {k: [] for k in routes}
    for _ in range(args.repeats):
        for key, fn in routes.items():
            times[key].append(round(timed(fn, args.seconds) / STEPS, 3))
    spread = {k: round((max(v) - min(v)) / min(v), 4) for k, v in times.items()}
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"metric": "microseconds per step, rollout forward + backward (one fine-tuning iteration / steps)",
           "workload": {"shape": [H, W], "dtype": "float64", "steps": STEPS, "equation": "Burgers (Stage3BurgersCell.INIT)",
                        "loss": "mean(traj^2)"},
           "device": torch.cuda.get_device_name(0), "seconds_per_region": args.seconds,
           "us_per_step": times, "median": med, "spread": spread,
           "library_cell_median_below_stock_torch_min": med["library_cell"] < min(times["stock_torch"]),
           "ratio_library_cell_over_stock_torch": round(med["library_cell"] / med["stock_torch"], 4),
           "ratio_library_cell_over_stage3_burgers": round(med["library_cell"] / med["stage3_burgers"], 4),
           "ratio_dense_over_library_cell": round(med["library_cell_dense"] / med["library_cell"], 4),
           "max_relative_difference_between_routes": diff, "dense_gradient_finite": dense_finite,
           "kernel_resources": resource_usage()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    if not out["library_cell_median_below_stock_torch_min"]:
        sys.exit("library_cell_bench.py: the library cell's median is not below the stock route's minimum")


if __name__ == "__main__":
    main()
