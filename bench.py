#!/usr/bin/env python3
"""Benchmark of the Pi-block rollout hot path.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload gs2d_512|gs3d_128|lo2d_512] [--T T]
                    [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times exactly K steps and prints one JSON line (metric, value, unit, higher_is_better, dtype,
ms_per_step, ...).  --full adds everything else the line used to carry: the per-kernel roofline (the sweep timed alone), the
CPU baselines, the module-path / loss / physics add-ons, the 3D-GS 128^3 half of the metric and the slab-sharded series.
--dump-outputs DIR writes what the timed path returned in its last step (the trajectory's final frame plus a fixed, seeded
sample of the whole trajectory, dL/dh0, the parameter-block gradient) as DIR/<name>.npy; the inputs are the same in every run.

One "step" (the unit of --steps) is ONE full rollout pass of the hot path over one synthetic
problem: T Pi-block time steps forward + the T-step reverse sweep with a dense dL/dtraj already
resident in HBM.  The headline `value` is Pi-block time steps per second (forward+backward),
whole job.  Default workload = BASELINE.json configs[1]: 2D Gray-Scott 512^2, 2 species, Hc=8,
fp32, T=1000, with the parameter magnitudes of the shipped checkpoint (values from
tests/golden, the checkpoint file itself does not travel).

N>1 (launched by torch.distributed.run, one rank per GPU, RCCL): the 512^2 problem does not shard
profitably (8 KB halos) so ranks run independent replicas -- weak scaling, no data-path
collective; a barrier + synchronize brackets the timed region and the MAX over ranks is taken.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (family, shape, hc, dtype, default T, golden file holding checkpoint-magnitude parameters)
    "gs2d_512": ("gs2d", (512, 512), 8, torch.float32, 1000, "gs2d_big_512x512.npz"),
    "gs2d_100": ("gs2d", (100, 100), 8, torch.float32, 200, "gs2d_big_512x512.npz"),   # BASELINE configs[0]: the reference's own grid / horizon
    "gs3d_128": ("gs3d", (128, 128, 128), 2, torch.float32, 500, "gs3d_big_128x128x128.npz"),
    "gs3d_48": ("gs3d", (48, 48, 48), 2, torch.float32, 300, "gs3d_big_128x128x128.npz"),   # the reference's own 3D grid / horizon (3dgs:497-536)
    "lo2d_512": ("lo2d", (512, 512), 4, torch.float64, 400, "lo2d_big_512x512.npz"),
}
# Stage-1 Pi-block (5x5 conv branches 2 -> 16 on the matrix cores): name -> (family, shape, T, golden)
STAGE1 = {
    "bur1_100": ("burgers", (100, 100), 200, "bur1_stage1_32x32.npz"),      # the reference's Stage-1 grid and horizon (bur1:914-935)
    "lo1_100": ("lo", (100, 100), 200, "lo1_stage1_32x32.npz"),
    "bur1_512": ("burgers", (512, 512), 50, "bur1_stage1_32x32.npz"),
}
MFMA_F32_PEAK_TFS = 157.3    # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense, 2.4 GHz
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy ceiling)
HBM_COPY_CEILING_GBS = 6290.0    # the same table's measured float4-copy ceiling
# what the SQ / TCP / TCC counters say limits each kernel (shares of a resident wave's life: issuing / stalled at issue / parked at
# barriers, polls and waitcnts).  The roofline the path is priced against stays HBM; this is the honest "why not".
LIMITERS = {
    "pi_adj2d_persist_split_kernel": "VALU instruction issue: a strip is ~450 VALU instructions at the single-wave rate; since round 6 the thin passes "
                                     "(P0, P3-P5) run on two-point half-strips so both waves of every SIMD issue (7.9 -> 7.1 us per group of 4 steps); "
                                     "237 / 253 VGPRs (profiles/r06_granule_pairs.txt; round-5 counters: issue 0.29 / stall 0.28 / parked 0.44)",
    "pi_adj2d_persist_kernel": "hand-over waits (profiles/r04_persistent_split_timelines.txt)",
    "pi_fwd2d_persist_kernel": "LDS latency at low occupancy: a pass is ONE 128-instruction strip per wave (0.19 us of VALU issue) that takes "
                               "0.45 us alone on its CU and 0.8 us next to three others (VALU active 22 %, waiting 67 %); six passes + a 0.4 us "
                               "ring wait per 4 steps (profiles/r06_granule_pairs.txt)",
    "pi_fwd2d_persist_small_kernel": "the un-hidden hand-over: 1.6 us round trip per 4 steps (profiles/r05_small_tile_resident_forward.txt)",
    "pi_adj2d_persist_small_kernel": "hand-over + one wave per SIMD (profiles/r05_counters_summary.txt)",
    "pi_fwd2d_tile_kernel": "launch boundary 2.0 us + cold window 1.4 us per 4 steps: parked 0.60 (profiles/r05_counters_summary.txt)",
    "pi_adj2d_tile_kernel": "launch boundary + window + sub-steps: parked 0.47 (profiles/r05_counters_summary.txt)",
    "pi_fwd3d_brick_kernel": "L1 request volume + launch boundary (~1.9 of 8.3 us): issue 0.24-0.28 / issue stalls 0.36 / waits 0.36-0.42, more "
                             "SALU than VALU; within 6-8 % of its own access pattern (profiles/r05_access_pattern_floors.txt)",
    "pi_adj3d_brick_kernel": "L1 request volume + launch boundary; 256^3: instruction issue over the 3-reads-1-write floor "
                             "(profiles/r05_access_pattern_floors.txt, r05_counters_summary.txt)",
    "pi_adj3d_resident_kernel": "instruction issue at two waves per SIMD (418 VALU per 4-point strip) + one granule round trip per step: "
                                "issue 0.30 / stall 0.13 / parked 0.58; 11.75 of 16.4 us per step without the hand-over "
                                "(profiles/r06_resident3d_ab.txt)",
    "pi_stream3d_kernel": "memory side: 5.1 TB/s of real traffic at 1.28-1.48x the algorithmic reads (profiles/r05_counters_summary.txt)",
    "pi_moments_kernel": "HBM (6.2 TB/s)",
}


def flush_c_stdio():
    """librccl prints a version banner through C stdio; when stdout is a pipe it would be flushed at process exit,
    i.e. AFTER the JSON line.  Flush it first so the JSON line stays the last line of stdout."""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


def load_params(golden):
    z = np.load(os.path.join(ROOT, "tests", "golden", golden))
    return {k[6:]: torch.tensor(z[k]) for k in z.files if k.startswith("param/")}


def make_cell(family, sd, device, reaction="poly"):
    import percnn_amd as pa
    cell = {"gs2d": pa.gs2d_cell, "gs3d": pa.gs3d_cell, "lo2d": pa.lo2d_cell}[family](reaction=reaction)
    cell.load_state_dict(sd)
    return cell.to(device)


def initial_state(family, shape):
    from percnn_amd import synthetic as S     # synthetic ICs of SURVEY 8(d)
    return S.lo_initial_state(shape[0]) if family == "lo2d" else S.gs_initial_state(shape, seed=0)


def cpu_baseline(family, sd, shape, budget_s=15.0, threads=None, extra_counts=True):
    """The oracle's torch restatement (stock F.conv + cat padding + autograd; proven bit-identical to the imported
    reference in the build container) timed on this box's host cores -- SURVEY 8(d): thread count stated, the all-cores
    and the single-thread figures reported next to the best one, medians of repeated runs."""
    from oracle import restatement as R
    cell = {"gs2d": R.gs2d_cell, "gs3d": R.gs3d_cell, "lo2d": R.lo2d_cell}[family]()
    cell.load_state_dict(sd)
    h0 = initial_state(family, shape)

    def run(n):
        t0 = time.perf_counter()
        traj = R.rollout(cell, h0, n)
        (traj ** 2).mean().backward()
        return time.perf_counter() - t0

    ncpu = os.cpu_count() or 1
    probes = {}
    if threads is None:
        # the thread count that is actually fastest on this host (all cores is NOT: oneDNN's small single-image
        # convolutions oversubscribe badly on 100+ core boxes)
        best = None
        for th in sorted({min(ncpu, c) for c in (8, 16, 32, 64)}):
            torch.set_num_threads(th)
            run(1)                                # warm-up (oneDNN primitive creation)
            t1 = run(2) / 2
            probes[th] = 1.0 / t1
            if best is None or t1 < best[1]:
                best = (th, t1)
            if t1 > 4 * best[1]:
                break
        threads, t_probe = best
    else:
        torch.set_num_threads(threads)
        run(1)
        t_probe = run(1)
    torch.set_num_threads(threads)
    reps = 5
    n = int(max(2, min(40, budget_s / reps / max(t_probe, 1e-6))))
    times = sorted(run(n) for _ in range(reps))
    med = times[reps // 2]
    out = {"value": n / med, "unit": "steps/s", "cores": threads, "kind": "port", "host_cpus": ncpu,
           "statistic": f"median of {reps} runs", "min_max": [n / times[-1], n / times[0]],
           "sample": f"{reps} x {n}-step fwd+bwd rollouts of the same {'x'.join(map(str, shape))} problem, "
                     f"torch {torch.__version__} CPU ({threads} threads), loss=mean(traj^2)",
           "probe_steps_per_s_by_threads": probes}

    def bounded(th, label):
        # one warm-up step; if that alone is slow the single cold step IS the figure (keeps the bench within minutes)
        torch.set_num_threads(th)
        t_w = run(1)
        if t_w > 8.0:
            return {"value": 1.0 / t_w, "threads": th, "sample": "1 cold fwd+bwd step (no warm-up: > 8 s per step)"}
        k = int(max(1, min(10, 3.0 / max(t_w, 1e-6))))
        ts = sorted(run(k) for _ in range(3))
        return {"value": k / ts[1], "threads": th, "sample": f"median of 3 x {k}-step fwd+bwd rollouts"}

    if extra_counts:
        out["threads_1"] = bounded(1, "1")
        out["threads_all"] = bounded(ncpu, "all") if ncpu != threads else {"value": out["value"], "threads": ncpu,
                                                                         "sample": "same as the headline figure"}
        torch.set_num_threads(threads)
    return out


def ensure_library(local_rank):
    """The built libpercnn_pi.so normally travels with the tree.  A source-only tree is compiled once per node (local
    rank 0, hipcc, ~80 s) while the other ranks wait for the file; the package itself never builds or falls back."""
    from percnn_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        return
    if local_rank == 0:
        tmp = _lib.LIB_PATH + ".building"
        _lib.build(out=tmp)
        os.replace(tmp, _lib.LIB_PATH)                  # atomic: waiters never load a half-written file
        return
    deadline = time.time() + 600
    while not os.path.exists(_lib.LIB_PATH):
        if time.time() > deadline:
            raise SystemExit("bench.py: timed out waiting for local rank 0 to build libpercnn_pi.so")
        time.sleep(1.0)


def measure_workload(pa, dev, dist, rank, world, name, steps, warmup, reaction, opts, T=0, full=True):
    """Time `steps` rollout passes (T Pi-block time steps forward + the full backward each) of workload `name`.
    Returns the measurement as a dict (value, ms_per_step, with `full` the per-kernel roofline, ...) and the live tensors
    for add-ons and --dump-outputs."""
    family, shape, hc, dtype, T_def, golden = WORKLOADS[name]
    T = T or T_def
    sd = load_params(golden)
    cell = make_cell(family, sd, dev, reaction)
    with torch.no_grad():
        P = cell.param_block().contiguous()
    npts = int(np.prod(shape))
    esz = dtype.itemsize
    traj = torch.empty((T + 1, 2) + shape, dtype=dtype, device=dev)
    traj[0] = initial_state(family, shape)[0].to(dev)
    # dense synthetic loss gradient, resident before the timed region (what autograd hands the op
    # for L = mean(traj^2) has this shape and density)
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    gtraj = torch.randn(traj.shape, dtype=dtype, device=dev, generator=gen) * (2.0 / traj.numel())

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]

    def one_pass(e=None):
        if e: e[0].record()
        with torch.no_grad():
            Pc = cell.param_block().contiguous()     # parameter packing / contraction is part of every pass
        pa.rollout_fwd_(traj, Pc)
        if e: e[1].record()
        g0, pg = pa.rollout_bwd(traj, gtraj, Pc)
        if e: e[2].record()
        return g0, pg

    for _ in range(warmup):
        one_pass()
    barrier()
    t0 = time.perf_counter()
    for k in range(steps):
        g0, pg = one_pass(ev[k])
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = tt.item()
    assert torch.isfinite(g0).all() and torch.isfinite(pg).all() and torch.isfinite(traj[-1]).all()

    fwd_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))
    bwd_ms = float(np.mean([e[1].elapsed_time(e[2]) for e in ev]))
    value = world * steps * T / elapsed

    # which kernel families ran, asked from the library itself (percnn_pi_debug_plan: its own dispatch rules)
    from percnn_amd import _lib as _pl
    plan = _pl.rollout_plan(0 if reaction == "poly" else hc, shape, esz, ",".join(f"{k}={v}" for k, v in opts.items()) or None)
    K, Kf = plan["bwd_steps_per_launch"], plan["fwd_steps_per_launch"]
    res = {
        "value": value, "unit": "steps/s", "steps": steps, "warmup": warmup, "ms_per_step": elapsed / steps * 1e3,
        "timed_region_s": elapsed,
        "dtype": "f32" if dtype == torch.float32 else "f64",
        "config": {"workload": f"{name}: {family} {'x'.join(map(str, shape))}, 2 species, Hc={hc}, "
                               f"T={T} forward+backward rollout per step, dense dL/dtraj",
                   "reaction": reaction,
                   "parallelism": "single GPU" if world == 1 else f"{world} independent replicas (no collective)",
                   "points": npts, "T": T, "time_steps_per_launch": K, "kernel_plan": plan},
        "fwd_us_per_time_step": fwd_ms * 1e3 / T, "bwd_us_per_time_step": bwd_ms * 1e3 / T,
        "fwd_only_steps_per_sec": T / (fwd_ms * 1e-3),
    }
    # what the last timed pass handed its caller (the trajectory is filled in place), for --dump-outputs
    live = {"cell": cell, "family": family, "traj": traj, "gtraj": gtraj, "P": P, "T": T, "fwd_ms": fwd_ms, "sd": sd,
            "shape": shape, "esz": esz, "npts": npts, "g0": g0, "pg": pg}
    if not full:
        return res, live

    # ---- per-kernel roofline, measured live with HIP events on the launch stream ------------------
    # The backward is two kernels where the schedule is split: the sequential adjoint sweep and ONE time-parallel
    # gradient reduction.  The sweep is timed alone through a PER-CALL option (no process-wide state is touched).
    reps = max(1, min(steps, 20))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pa.rollout_bwd(traj, gtraj, P, options={"skip_wgrad": 1})
    e0.record()
    for _ in range(reps):
        pa.rollout_bwd(traj, gtraj, P, options={"skip_wgrad": 1})
    e1.record()
    torch.cuda.synchronize()
    sweep_ms = e0.elapsed_time(e1) / reps
    red_ms = max(bwd_ms - sweep_ms, 1e-6)
    tiled = plan["bwd"] == "tile2d"
    poly = reaction == "poly"
    # algorithmic bytes per point and time step: fwd read+write state = 2*C*s;
    # sweep read h, adj, dL/dout + write adj = 4*C*s; gradient reduction read h + adj = 2*C*s
    # (the factored Hc=8 reduction streams h once per species: 3*C*s)
    Cs = 2 * esz
    red_bytes_pt = 2 * Cs if (poly or hc <= 4) else 3 * Cs
    # `fused`: the parameter gradients are reduced inside the sweep launches (no separate time-parallel pass); the
    # sweep-only timing above then only serves as a lower bound of that kernel
    fused = plan["fused_gradients"]
    fwd_names = {"tile2d": "pi_fwd2d_tile_kernel", "stream3d": "pi_stream3d_kernel<fwd>", "brick3d": "pi_fwd3d_brick_kernel",
                 "direct": "pi_fwd_kernel", "advective": "pi_adv_fwd_kernel"}
    bwd_names = {"tile2d": "pi_adj2d_tile_kernel", "stream3d": "pi_stream3d_kernel<adj>", "brick3d": "pi_adj3d_brick_kernel",
                 "direct": "pi_bwd_kernel", "advective": "pi_adv_bwd_kernel"}
    fwd_kernel = fwd_names[plan["fwd"]]
    bwd_kernel = bwd_names[plan["bwd"]] + (("<sweep+moments>" if fused else "") if tiled else ("<sweep+moments>" if fused else "<sweep>"))
    persistent = bool(plan.get("bwd_persistent")) and tiled and fused and not opts.get("tile_persist") == "0" and T // K >= 2
    # the small-tile regime (32 x 8 tiles, split schedule): its sweep is one resident launch too (pi_adj2d_persist_small_kernel)
    persistent_small = bool(plan.get("bwd_persistent")) and tiled and not fused and not opts.get("tile_persist") == "0" and \
        str(opts.get("persist_small", "1")) != "0" and T // K >= 2
    if fused:
        sweep_ms, red_ms = bwd_ms, 1e-6
    clock = "HIP events on the launch stream, this run (fwd / bwd phases of every pass; sweep alone via options=skip_wgrad)"
    kernels = [
        {"kernel": fwd_kernel, "launches_per_pass": T // Kf,
         "algorithmic_bytes_per_launch": 2 * Cs * npts * Kf, "avg_launch_us": fwd_ms * 1e3 / (T / Kf)},
        {"kernel": bwd_kernel, "launches_per_pass": T // K,
         "algorithmic_bytes_per_launch": 4 * Cs * npts * K, "avg_launch_us": sweep_ms * 1e3 / (T / K)},
        {"kernel": ("pi_moments_kernel" if poly else "pi_wgrad_kernel"), "launches_per_pass": 1,
         "algorithmic_bytes_per_launch": red_bytes_pt * npts * T, "avg_launch_us": red_ms * 1e3},
    ]
    if fused:
        kernels.pop()                                   # no separate reduction launch
    if persistent:
        # the whole tile sweep of the rollout is ONE launch of resident workgroups (pi_adj2d_persist_kernel): T // K groups of
        # K steps inside it; the < K remaining steps (none at T = 1000) run on the direct kernels
        # (round 4: the split flavour -- halo-independent pyramid under the hand-over -- unless the option says otherwise)
        pname = "pi_adj2d_persist_kernel" if str(opts.get("persist_split", "1")) == "0" else "pi_adj2d_persist_split_kernel"
        kernels[1] = {"kernel": pname + "<sweep+moments, %d groups of %d steps per launch>" % (T // K, K),
                      "launches_per_pass": 1, "algorithmic_bytes_per_launch": 4 * Cs * npts * (T // K) * K,
                      "avg_launch_us": sweep_ms * 1e3}
    # the forward of such a grid is one resident launch as well (pi_fwd2d_persist_kernel, round 4), unless switched off
    # (rollouts of at least eight groups; round 5: the small-tile regime -- pi_fwd2d_persist_small_kernel -- and float64 too)
    fwd_persistent = bool(plan.get("fwd_persistent")) and Kf == 4 and T // Kf >= 8 and not opts.get("tile_persist") == "0" and \
        str(opts.get("fwd_persist", "1")) != "0"
    if fwd_persistent:
        small_fwd = plan.get("tile_fwd") is not None and plan["tile_fwd"][1] < 32
        kernels[0] = {"kernel": ("pi_fwd2d_persist_small_kernel" if small_fwd else "pi_fwd2d_persist_kernel") +
                                "<%d groups of %d steps per launch>" % (T // Kf, Kf),
                      "launches_per_pass": 1, "algorithmic_bytes_per_launch": 2 * Cs * npts * (T // Kf) * Kf,
                      "avg_launch_us": fwd_ms * 1e3}
    if persistent_small:
        kernels[1] = {"kernel": "pi_adj2d_persist_small_kernel<sweep, %d groups of %d steps per launch>" % (T // K, K),
                      "launches_per_pass": 1, "algorithmic_bytes_per_launch": 4 * Cs * npts * (T // K) * K,
                      "avg_launch_us": sweep_ms * 1e3}
    # 3D float32 pre-contracted blocks on whole 16 x 16 x 32 blocks (128^3): the whole sweep is ONE resident launch with the adjoint
    # state in LDS (pi_adj3d_resident_kernel, round 6) -- the plan says so unless res3d=0 / a device that aborted one
    resident3d = bool(plan.get("bwd_persistent")) and plan["bwd"] == "brick3d" and fused and 16 <= T < 4096 and \
        str(opts.get("res3d", "1")) != "0" and not opts.get("tile_persist") == "0"
    if resident3d:
        kernels[1] = {"kernel": "pi_adj3d_resident_kernel<sweep+moments, %d steps per launch>" % T,
                      "launches_per_pass": 1, "algorithmic_bytes_per_launch": 4 * Cs * npts * T, "avg_launch_us": bwd_ms * 1e3}
    # the SAME kernels under rocprofv3 --kernel-trace --stats (committed by tools/gpu_final_profiles.sh from the same command;
    # the profiler's own begin/end stamps, typically a few per cent longer than the HIP-event figure of an unprofiled run): both
    # clocks are printed so a reader can recompute either fraction
    rp = {}
    rfile = os.path.join(ROOT, "profiles", f"rocprof_kernel_avg_{name}.json")
    if os.path.exists(rfile) and reaction == "poly" and not opts:
        rp = json.load(open(rfile))
    for k in kernels:
        k["achieved"] = k["algorithmic_bytes_per_launch"] / (k["avg_launch_us"] * 1e-6) / 1e9
        k["frac"] = k["achieved"] / HBM_PEAK_GBS
        k["frac_of_copy_ceiling"] = k["achieved"] / HBM_COPY_CEILING_GBS
        k["share_of_pass"] = k["avg_launch_us"] * k["launches_per_pass"] / ((fwd_ms + bwd_ms) * 1e3)
        k["clock"] = "hip_events"
        base = k["kernel"].split("<")[0]
        r = (rp.get("kernels") or {}).get(base)
        if r and int(rp.get("T", 0)) == T:
            k["rocprofv3_avg_launch_us"] = r["avg_us"]
            k["frac_by_rocprofv3"] = k["algorithmic_bytes_per_launch"] / (r["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS
        k["limiter"] = LIMITERS.get(base)
    dom = max(kernels, key=lambda k: k["share_of_pass"])
    traffic, traffic_source = None, None
    tfile = os.path.join(ROOT, "profiles", f"traffic_{name}.json")
    if os.path.exists(tfile):
        tj = json.load(open(tfile))
        traffic = tj.get(dom["kernel"].split("<")[0])
        if dom["kernel"].startswith("pi_adj2d_persist") and tj.get("pi_adj2d_persist_kernel_per_group"):
            traffic = tj["pi_adj2d_persist_kernel_per_group"] * (T // K)        # measured at T = 100: per group of K steps
        if dom["kernel"].startswith("pi_adj3d_resident") and tj.get("pi_adj3d_resident_kernel_per_step"):
            traffic = tj["pi_adj3d_resident_kernel_per_step"] * T
        traffic_source = (f"profiles/traffic_{name}.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE of this command at T = "
                          f"{tj.get('_T', 100)}, collected {tj.get('_date', 'in round 5')} in separate passes on MI355X and committed "
                          "(not re-measured in this run; per-group / per-step figures are scaled to this run's T)")
    res["roofline"] = {"bound": "hbm", "kernel": dom["kernel"], "achieved": dom["achieved"], "peak": HBM_PEAK_GBS,
                       "unit": "GB/s", "frac": dom["frac"], "traffic": traffic, "traffic_source": traffic_source,
                       "algorithmic_bytes_per_launch": dom["algorithmic_bytes_per_launch"],
                       "avg_launch_us": dom["avg_launch_us"], "clock": clock,
                       # the roofline SURVEY 8(d) prices the path against is HBM; what the counters say actually limits the kernel:
                       "limiter": dom.get("limiter"),
                       "frac_of_copy_ceiling": dom["frac_of_copy_ceiling"], "copy_ceiling": HBM_COPY_CEILING_GBS,
                       "rocprofv3_avg_launch_us": dom.get("rocprofv3_avg_launch_us"), "frac_by_rocprofv3": dom.get("frac_by_rocprofv3"),
                       "rocprofv3_source": (rp.get("source") if dom.get("rocprofv3_avg_launch_us") else None),
                       "all_kernels": kernels}
    return res, live


def dump_outputs(path, arrays, budget_bytes=64 << 20):
    """--dump-outputs: each array as path/<name>.npy, float32 or float64 as computed, at most `budget_bytes` in all."""
    os.makedirs(path, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        host[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
    total = sum(a.nbytes for a in host.values())
    if total > budget_bytes:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes (limit {budget_bytes})")
    for name, a in host.items():
        np.save(os.path.join(path, name + ".npy"), a)


def trajectory_outputs(traj, g0, pg, sample=1 << 20):
    """What a caller of the timed path receives: the trajectory (filled in place; its final frame whole, plus a fixed, seeded
    sample of `sample` points of the whole buffer), dL/dh0 and the parameter-block gradient."""
    n = traj.numel()
    idx = np.unique(np.random.default_rng(0).integers(0, n, size=min(n, sample)))
    return {"traj_final": traj[-1], "traj_sample": traj.reshape(-1)[torch.from_numpy(idx).to(traj.device)],
            "grad_h0": g0, "grad_param_block": pg}




def module_path_extra(pa, family, sd, shape, T, dev, reaction, reps=3):
    """What a user of the reference's interface pays per training iteration (SURVEY 8b call sites train_2drd.py:393-407):
    (a) ``outputs, _ = model(); torch.cat(outputs); loss; loss.backward()`` -- the list-of-frames path, dense loss;
    (b) ``model.observe(slice(0, -1, 20), 4)`` + the reference's strided data loss + backward."""
    cell = make_cell(family, sd, dev, reaction)
    h0 = initial_state(family, shape).to(dev).requires_grad_(True)
    model = pa.RCNN(cell, step=T, effective_step=list(range(T)), init_state=h0)
    params = [p for p in cell.parameters() if p.requires_grad]

    def it_list():
        outs, _ = model()
        traj = torch.cat(tuple(outs), dim=0)
        loss = (traj ** 2).mean()
        torch.autograd.grad(loss, params + [h0])

    def it_list_copy():                                  # what that line cost before round 5: the stock, copying torch.cat
        outs, _ = model()
        traj = torch.cat(tuple(f.as_subclass(torch.Tensor) for f in outs), dim=0)
        loss = (traj ** 2).mean()
        torch.autograd.grad(loss, params + [h0])

    def it_stacked():
        outs, _ = model()
        loss = (outs.stacked ** 2).mean()                # the reference's call pattern minus its torch.cat
        torch.autograd.grad(loss, params + [h0])

    def it_traj():
        loss = (model.trajectory() ** 2).mean()
        torch.autograd.grad(loss, params + [h0])

    def it_observe():
        pred = model.observe(slice(0, -1, 20), 4)
        loss = ((pred - 0.5) ** 2).mean()
        torch.autograd.grad(loss, params + [h0])

    def it_list_strided():                               # the reference's own lines, unchanged (train_2drd.py:393-401)
        outs, _ = model()
        output = torch.cat(tuple(outs), dim=0)
        pred = output[0:-1:20, :, ::4, ::4]
        loss = ((pred - 0.5) ** 2).mean()
        torch.autograd.grad(loss, params + [h0])

    def it_loss_mse():
        loss = model.loss_mse()                          # mean(traj^2) inside the rollout's autograd node
        torch.autograd.grad(loss, params + [h0])

    out = {}
    for key, fn in (("list_cat_dense_loss_ms", it_list), ("list_copying_cat_dense_loss_ms", it_list_copy),
                    ("list_stacked_dense_loss_ms", it_stacked),
                    ("trajectory_dense_loss_ms", it_traj),
                    ("loss_mse_dense_ms", it_loss_mse), ("list_cat_strided_loss_ms", it_list_strided),
                    ("observe_strided_loss_ms", it_observe)):
        fn()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        marks[0].record()
        for i in range(reps):
            fn()
            marks[i + 1].record()
        torch.cuda.synchronize()
        per_it = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(reps))
        # median of the iterations: the boxes show an occasional one-off stall of tens of ms (seen once on either side of an
        # otherwise 6 ms iteration), which a mean over three would turn into the number
        out[key] = {"gpu_ms": per_it[reps // 2], "gpu_ms_mean": marks[0].elapsed_time(marks[reps]) / reps,
                    "wall_ms": (time.perf_counter() - t0) / reps * 1e3}
    out["what"] = (f"one training iteration through the drop-in modules at {'x'.join(map(str, shape))} x T={T}: RCNN.forward() "
                   "+ torch.cat(tuple(outputs), dim=0) (the reference's own line: since round 5 it returns the trajectory buffer, functional.Frame) + mean(traj^2) + backward; the same with the stock copying cat (frames as plain tensors); the same with outputs.stacked in place of the cat; RCNN.trajectory() (torch.ops.percnn.pi_rollout, no list / cat) + the same loss; "
                   "RCNN.loss_mse() = the same dense loss as ONE autograd node with the rollout (gradient formed inside the sweep); "
                   "the reference's unchanged strided data loss torch.cat(tuple(output))[0:-1:20, :, ::4, ::4] + MSE + backward (autograd hands the sweep a dense, mostly zero dL/dtraj); "
                   "RCNN.observe(0:-1:20, ::4) + MSE + backward (the same loss with the caller edit of INTEGRATION.md 1: masked sweep, no dL/dtraj buffer) "
                   "(forward, loss, full backward incl. parameter gradients; wall = host clock around the same loop)")
    return out


def cell_loop_extra(pa, dev, reaction):
    """The reference's OWN step loop (train_2drd.py:169-188) with `cell(h)` swapped in -- what a maintainer
    pays who keeps the loop instead of calling the fused rollout: per time step, forward loop alone (no_grad / recording)
    and the whole training iteration (torch.cat + dense loss + backward + Adam step).  VERDICT r2 #4."""
    from percnn_amd import synthetic
    sd = load_params(WORKLOADS["gs2d_512"][5])
    out = {"what": "for step in range(T): h, _ = cell(h) -- wall-clock us per time step through the operator library's eager path "
                   "(csrc/torch_ext.cpp): one call validates the cached block; a loop that feeds every output back in gets its next "
                   "4 / 8 / 16 states from ONE fused launch (bit-identical), as ONE autograd node per group whose backward is one "
                   "fused sweep; parameter-gradient sums are delivered once per backward pass"}
    for n, T in ((100, 200), (512, 100)):
        cell = make_cell("gs2d", sd, dev, reaction)
        h0 = synthetic.gs_initial_state((n, n), seed=0).to(dev)
        opt = torch.optim.Adam(cell.parameters(), lr=1e-6)

        def loop():
            h, outs = h0, [h0]
            for _ in range(T):
                h, _ = cell(h)
                outs.append(h)
            return outs

        def iteration():
            opt.zero_grad(set_to_none=True)
            ((torch.cat(loop(), 0) ** 2).mean()).backward()
            opt.step()

        def timeit(fn, k=5):
            fn(); fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            torch.cuda.synchronize()
            return 1e6 * (time.perf_counter() - t0) / k / T
        with torch.no_grad():
            t_ng = timeit(loop)
        out[f"{n}x{n}_T{T}"] = {"forward_loop_no_grad_us_per_step": t_ng, "forward_loop_recording_us_per_step": timeit(loop),
                                "training_iteration_us_per_step": timeit(iteration)}
    return out


def lo2d_physics_path_extra(pa, dev, reaction, reps=3):
    """The lambda-omega training iteration of the reference (percnn_LO_eqn.py:371-373: the loss IS the physics residual of
    the rollout, no data term) through the drop-in modules at BASELINE configs[2]: 512^2, float64, T = 400 -- RCNN.trajectory()
    -> physics_loss (one residual launch over all frames) -> backward (one residual-adjoint launch, then the sweep)."""
    from percnn_amd import physics
    family, shape, hc, dtype, T, golden = WORKLOADS["lo2d_512"]
    cell = make_cell(family, load_params(golden), dev, reaction)
    h0 = initial_state(family, shape).to(dev).requires_grad_(True)
    model = pa.RCNN(cell, step=T, effective_step=list(range(T)), init_state=h0)
    params = [p for p in cell.parameters() if p.requires_grad]
    Q = physics.lambda_omega_block(cell, 0.1)

    def it():
        loss = physics.physics_loss(model.trajectory(), Q)
        torch.autograd.grad(loss, params + [h0])
        return loss

    it()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for i in range(reps):
        loss = it()
        marks[i].record()
    e1.record()
    torch.cuda.synchronize()
    per_it = [([e0] + marks)[i].elapsed_time(marks[i]) for i in range(reps)]
    med = sorted(per_it)[reps // 2]
    return {"per_iteration_ms": per_it, "what": f"lambda-omega {shape[0]}x{shape[1]} float64, T={T}: RCNN.trajectory() + physics_loss + backward per iteration "
                    "(the loss of percnn_LO_eqn.py:371-373, in the gradient path; physics_loss = one autograd node since round 3, "
                    "the residual-tensor expression took 16.2 ms)",
            "gpu_ms": med, "gpu_ms_mean": e0.elapsed_time(e1) / reps, "wall_ms": (time.perf_counter() - t0) / reps * 1e3,
            "time_steps_per_sec": T / (med * 1e-3), "loss_value": float(loss.detach())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)       # 200 passes x ~5 ms: a timed region of >= 1 s
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="gs2d_512", choices=list(WORKLOADS) + list(STAGE1))
    ap.add_argument("--T", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--reaction", default="poly", choices=["poly", "factored"],
                    help="poly: branch product pre-contracted to a cubic (module default); factored: per-point 1x1 branches")
    ap.add_argument("--opt", action="append", default=[], help="library tuning option key=value (repeatable)")
    ap.add_argument("--slab-extra", action="store_true", help="also time the slab-sharded 3D path at N=1")
    ap.add_argument("--no-extras", action="store_true",
                    help="headline measurement only (profiling runs: keeps per-kernel averages free of the add-on passes)")
    ap.add_argument("--no-also", action="store_true", help="skip the second half of the BASELINE metric (3D-GS 128^3)")
    ap.add_argument("--slab-timeout", type=float, default=420.0)
    ap.add_argument("--slab-in-process", action="store_true",
                    help="run the slab series inside each rank instead of an isolated child process per rank (one-GPU test "
                         "runs of many ranks: half the processes holding the device)")
    ap.add_argument("--slab-child", action="store_true", help=argparse.SUPPRESS)   # see slab_extra_isolated
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: roofline (sweep timed alone), CPU baselines, add-ons, the 3D-GS "
                         "128^3 half of the metric, the slab series at N = 1 (--no-* options trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the timed path returned in its last step as DIR/<name>.npy (float32 / float64)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus > 1 and world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} needs torch.distributed.run with {a.gpus} ranks (WORLD_SIZE={world})")
    if a.dump_outputs and world > 1:
        raise SystemExit("bench.py: --dump-outputs needs a single-process run (--gpus 1)")
    # PERCNN_BENCH_ONE_GPU=1: every rank on cuda:0, gloo as the control plane (RCCL refuses two ranks on one device) -- how
    # tests/test_slab_dist_gpu.py::test_bench_two_ranks_on_one_gpu proves the N > 1 control flow of this file on a 1-GPU box
    one_gpu = bool(int(os.environ.get("PERCNN_BENCH_ONE_GPU", "0")))
    dev = torch.device("cuda", 0 if one_gpu else local_rank)
    torch.cuda.set_device(dev)
    dist = None
    if world > 1 or "MASTER_ADDR" in os.environ:          # launched by torch.distributed.run
        import torch.distributed as dist
        if one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    ensure_library(local_rank)
    import percnn_amd as pa
    if one_gpu:
        # several PROCESSES on one GPU (test mode): two persistent sweeps would each hold part of the CUs (include/percnn_pi.h,
        # option tile_persist) -- the launch-per-group sweep here
        pa.set_option("tile_persist", 0)
    if a.slab_child:
        def checkpoint(res):
            flush_c_stdio()
            print(json.dumps(res), flush=True)
        res = sharded_series(dev, dist, rank, world, one_gpu, checkpoint, steps=a.steps, warmup=a.warmup)
        try:
            pa.slab.close_exchangers()
        except Exception:
            pass
        if dist is not None:
            dist.destroy_process_group()
        checkpoint(res)
        return
    if a.workload in STAGE1:
        return stage1_main(a, pa, dev, dist, rank, world)
    for kv in a.opt:
        k, v = kv.split("=")
        pa.set_option(k, int(v))                      # the CLI's explicit process-wide defaults for this run
    opts = dict(kv.split("=") for kv in a.opt)

    res, live = measure_workload(pa, dev, dist, rank, world, a.workload, a.steps, a.warmup, a.reaction, opts, a.T, full=a.full)
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, trajectory_outputs(live["traj"], live["g0"], live["pg"]))
    out = {"metric": "pi_block_rollout_fwd_bwd_steps_per_sec", "value": res["value"], "unit": "steps/s",
           "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": res["ms_per_step"],
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": res["dtype"], "data": "synthetic",
           "config": res["config"], **({"roofline": res["roofline"]} if a.full else {}), "timed_region_s": res["timed_region_s"],
           "fwd_us_per_time_step": res["fwd_us_per_time_step"], "bwd_us_per_time_step": res["bwd_us_per_time_step"],
           "fwd_only_steps_per_sec": res["fwd_only_steps_per_sec"]}
    family, sd, shape, T = live["family"], live["sd"], live["shape"], live["T"]
    cpu_threads = None
    if rank == 0 and world == 1 and a.full and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(family, sd, shape)
        cpu_threads = out["cpu_baseline"]["cores"]
    if world == 1 and a.full and not a.no_extras:
        try:
            out["physics_residual"] = physics_extra(pa, live["cell"], family, live["traj"], live["esz"], live["npts"])
        except Exception as e:                       # an add-on measurement must never cost the headline line
            out["physics_residual"] = {"error": repr(e)[:200]}
        try:
            out["strided_data_loss"] = strided_loss_extra(pa, live["traj"], live["gtraj"], live["P"], T, live["fwd_ms"],
                                                          min(a.steps, 10))
        except Exception as e:
            out["strided_data_loss"] = {"error": repr(e)[:200]}
        try:
            out["sqerr_loss_in_sweep"] = sqerr_extra(pa, live["traj"], live["P"], T, live["fwd_ms"], min(a.steps, 10))
        except Exception as e:
            out["sqerr_loss_in_sweep"] = {"error": repr(e)[:200]}
    del live, res
    torch.cuda.empty_cache()
    if world == 1 and a.full and not a.no_extras:
        try:
            out["module_path"] = module_path_extra(pa, family, sd, shape, T, dev, a.reaction)
        except Exception as e:
            out["module_path"] = {"error": repr(e)[:200]}
        torch.cuda.empty_cache()
        if a.workload == "gs2d_512" and not a.T:
            try:
                out["module_path"]["per_step_cell_loop"] = cell_loop_extra(pa, dev, a.reaction)
            except Exception as e:
                out["module_path"]["per_step_cell_loop"] = {"error": repr(e)[:200]}
            try:
                out["module_path"]["lo2d_512_physics_loss"] = lo2d_physics_path_extra(pa, dev, a.reaction)
            except Exception as e:
                out["module_path"]["lo2d_512_physics_loss"] = {"error": repr(e)[:200]}
            torch.cuda.empty_cache()

    # ---- the other half of BASELINE.json's metric ("2D-GS 512^2 & 3D-GS 128^3") in the same line --------------------
    if a.full and a.workload == "gs2d_512" and not a.no_also and not a.T:
        try:
            n3 = max(3, a.steps // 4)
            r3, l3 = measure_workload(pa, dev, dist, rank, world, "gs3d_128", n3, max(1, a.warmup // 2), a.reaction, opts)
            also = {k: r3[k] for k in ("value", "unit", "steps", "warmup", "ms_per_step", "timed_region_s", "dtype", "config",
                                       "roofline", "fwd_us_per_time_step", "bwd_us_per_time_step")}
            if world == 1 and not a.no_extras:
                try:
                    also["sqerr_loss_in_sweep"] = sqerr_extra(pa, l3["traj"], l3["P"], l3["T"], l3["fwd_ms"], min(n3, 5))
                except Exception as e:
                    also["sqerr_loss_in_sweep"] = {"error": repr(e)[:200]}
            if rank == 0 and world == 1 and not a.no_cpu_baseline:
                also["cpu_baseline"] = cpu_baseline("gs3d", l3["sd"], l3["shape"], budget_s=8.0, threads=cpu_threads,
                                                    extra_counts=False)
            del r3, l3
            torch.cuda.empty_cache()
            out["also"] = {"gs3d_128": also}
        except Exception as e:
            out["also"] = {"gs3d_128": {"error": repr(e)[:300]}}

    # N > 1: additionally time the spatially sharded path (slab decomposition + RCCL halo exchange over
    # xGMI) on the configs[4]-shaped problem, weak-scaled: 32 planes of 256^2 per rank (256^3 at N = 8).
    # A watchdog guarantees the single JSON line is printed even if the collective path stalls.
    printed = threading.Event()

    def emit():
        if not printed.is_set():
            printed.set()
            if rank == 0:
                flush_c_stdio()                              # RCCL's version banner sits in the C stdio buffer
                print(json.dumps(out), flush=True)           # -> the JSON line is the last line on stdout

    if world > 1 or a.slab_extra or (a.full and not a.no_extras):
        def watchdog():
            if not printed.wait(a.slab_timeout + 60.0):
                out["slab_3d"] = {"error": f"timed out after {a.slab_timeout + 60.0}s"}
                emit()
                os._exit(0)
        threading.Thread(target=watchdog, daemon=True).start()
        try:
            torch.cuda.empty_cache()
            # own process per rank: a fault in there cannot cost the line above
            out["slab_3d"] = slab_extra_isolated(a, dev, dist, rank, world, local_rank)
        except Exception as e:                       # keep the headline number whatever happens here
            out["slab_3d"] = {"error": repr(e)[:300]}
    # what the schedules do against a wire: measured once with an injected link time, committed, quoted here
    wf = os.path.join(ROOT, "profiles", "slab_injected_wire.json")
    if isinstance(out.get("slab_3d"), dict) and os.path.exists(wf):
        try:
            out["slab_3d"]["injected_wire"] = json.load(open(wf))
        except Exception:
            pass
    if world > 1:
        promote_sharded_headline(out, world)
    if dist is not None:
        dist.destroy_process_group()
    emit()


def promote_sharded_headline(out, world):
    """N > 1: the line's top level carries the SHARDED path -- configs[4], the fixed 256^3 grid cut into N slabs with a halo
    exchange per step (north_star: 'the rollout shards over the spatial domain across the 8 GPUs of one node') -- not N
    independent replicas of the 2D problem, which scale trivially and show RCCL nothing.  The replica
    figure stays in the line as `replicas_2d`.  Without a valid sharded measurement the replica line is kept and says why."""
    slab3 = out.get("slab_3d") or {}
    h = slab3.get("headline")
    if not isinstance(h, dict) or "error" in h or "steps_per_sec_fwd_bwd" not in h:
        out["sharded_headline_missing"] = (h or {}).get("error") or slab3.get("error") or slab3.get("incomplete") or "no headline phase in the child's report"
        return
    replicas = {k: out.get(k) for k in ("value", "unit", "ms_per_step", "scaling", "dtype", "config", "roofline", "timed_region_s",
                                        "fwd_us_per_time_step", "bwd_us_per_time_step", "fwd_only_steps_per_sec", "also")
                if k in out}
    replicas["what"] = (f"{world} independent replicas of the 2D headline problem, one per GPU, no data-path collective (the 512^2 grid "
                        "does not shard profitably: 8 KB halos); whole-job aggregate")
    for k in ("roofline", "fwd_us_per_time_step", "bwd_us_per_time_step", "fwd_only_steps_per_sec", "also"):
        out.pop(k, None)
    anchor = slab3.get("headline_n1_anchor") or {}
    npts = h.get("global_points", 0)
    out.update({
        "value": h["steps_per_sec_fwd_bwd"], "ms_per_step": h["ms_per_step"], "steps": h["steps"], "warmup": h["warmup"],
        "scaling": "strong", "dtype": "f32", "timed_region_s": h["timed_region_s"],
        "config": {"workload": f"gs3d_{h['grid'][0]} strong scaling: gs3d {'x'.join(map(str, h['grid']))}"
                               f"{' (BASELINE configs[4])' if h['grid'][0] == 256 else ' (test-sized stand-in for configs[4])'}, "
                               f"2 species, Hc=2, cut into {world} slabs "
                               f"along axis 0, T={h['T']} forward+backward rollout per step, dense dL/dtraj, halo exchange every "
                               "2 forward steps (4 planes) / every adjoint step (2 planes), one gradient all-reduce per pass",
                   "reaction": (out.get("config") or {}).get("reaction", "poly"), "parallelism": f"spatial slabs x{world}",
                   "grid": h["grid"], "points": npts, "points_per_rank": h.get("points_per_rank"), "T": h["T"]},
        "transport": h.get("transport"), "transport_exchange": h.get("exchange"), "schedule": h.get("schedule"),
        "ranks_seen_by_transport": h.get("ranks_seen_by_transport"),
        "forward_state_equals_single_domain_rollout": h.get("forward_state_equals_single_domain_rollout"),
        "frames_compared": h.get("frames_compared"), "us_per_time_step_fwd_bwd": h.get("us_per_time_step_fwd_bwd"),
        "n1_anchor": {"what": "the same 256^3 grid as ONE periodic domain on one GPU of this box, same run, same clock",
                      "steps_per_sec": anchor.get("steps_per_sec_fwd_bwd"), "us_per_time_step_fwd_bwd": anchor.get("us_per_time_step_fwd_bwd"),
                      "T": anchor.get("T"), "error": anchor.get("error"),
                      "r04_driver_figure_steps_per_sec": 4568.7},
        "speedup_vs_n1_anchor": (h["steps_per_sec_fwd_bwd"] / anchor["steps_per_sec_fwd_bwd"]) if anchor.get("steps_per_sec_fwd_bwd") else None,
        # effective bandwidth of the whole job on algorithmic bytes (48 B per point and fwd+bwd step)
        "roofline": {"bound": "hbm", "kernel": "slab rollout: pi_fwd3d_brick_kernel + pi_adj3d_brick_kernel per rank, exchanges included",
                     "achieved": 48.0 * npts * h["steps_per_sec_fwd_bwd"] / 1e9, "peak": 8000.0 * world, "unit": "GB/s",
                     "frac": 48.0 * npts * h["steps_per_sec_fwd_bwd"] / 1e9 / (8000.0 * world), "traffic": None,
                     "clock": "wall clock of the timed region (barrier + synchronize on both sides, max over ranks)"},
        "replicas_2d": replicas,
    })


def stage1_main(a, pa, dev, dist, rank, world):
    """Stage-1 Pi-block: T-step rollout forward + backward on the matrix cores.  Same JSON contract; the roofline of the
    dominant kernel is priced against the dense f32 MFMA peak (the branch evaluation is a K = 51 contraction)."""
    family, shape, T_def, golden = STAGE1[a.workload]
    T = a.T or T_def
    sd = load_params(golden)
    cell = pa.Stage1Cell(family).to(dev)
    cell.load_state_dict(sd)
    for kv in a.opt:
        k, v = kv.split("=")
        pa.stage1.set_option(k, int(v))
    n = shape[0] * shape[1]
    ys, xs = torch.meshgrid(torch.arange(shape[0]) / shape[0], torch.arange(shape[1]) / shape[1], indexing="ij")
    h0 = torch.stack((0.6 * torch.sin(2 * np.pi * xs) * torch.cos(2 * np.pi * ys) + 0.3 * torch.cos(4 * np.pi * xs + 0.5),
                      0.6 * torch.cos(2 * np.pi * xs) * torch.sin(2 * np.pi * ys) - 0.2 * torch.sin(2 * np.pi * (xs + 2 * ys))))
    traj = torch.empty((T + 1, 2) + shape, dtype=torch.float32, device=dev)
    traj[0] = h0.to(dev)
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    gtraj = torch.randn(traj.shape, dtype=torch.float32, device=dev, generator=gen) * (2.0 / traj.numel())

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.steps)]

    def one_pass(e=None):
        if e: e[0].record()
        with torch.no_grad():
            P = cell.param_block().contiguous()       # packing is part of every pass
        pa.stage1.rollout_fwd_(traj, P)
        if e: e[1].record()
        g0, pg = pa.stage1.rollout_bwd(traj, gtraj, P)
        if e: e[2].record()
        return g0, pg, P

    for _ in range(a.warmup):
        one_pass()
    barrier()
    t0 = time.perf_counter()
    for k in range(a.steps):
        g0, pg, P = one_pass(ev[k])
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = tt.item()
    assert torch.isfinite(g0).all() and torch.isfinite(pg).all() and torch.isfinite(traj[-1]).all()
    fwd_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))
    bwd_ms = float(np.mean([e[1].elapsed_time(e[2]) for e in ev]))
    value = world * a.steps * T / elapsed
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, trajectory_outputs(traj, g0, pg))
    out = {
        "metric": "pi_block_rollout_fwd_bwd_steps_per_sec", "value": value, "unit": "steps/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": elapsed / a.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{a.workload}: Stage-1 Pi-block ({family}; three 5x5 conv branches 2->16 per species) "
                               f"{shape[0]}x{shape[1]}, T={T} forward+backward rollout per step, dense dL/dtraj",
                   "parallelism": "single GPU" if world == 1 else f"{world} independent replicas (no collective)",
                   "points": n, "T": T},
        "fwd_us_per_time_step": fwd_ms * 1e3 / T, "bwd_us_per_time_step": bwd_ms * 1e3 / T,
        "fwd_only_steps_per_sec": T / (fwd_ms * 1e-3),
    }
    if a.full:
        stage1_roofline(a, pa, out, traj, gtraj, P, n, T, fwd_ms, bwd_ms)
    if rank == 0 and world == 1 and a.full and not a.no_cpu_baseline:
        out["cpu_baseline"] = stage1_cpu_baseline(family, sd, h0, shape)
    if dist is not None:
        dist.destroy_process_group()
    if rank == 0:
        flush_c_stdio()
        print(json.dumps(out), flush=True)


def stage1_roofline(a, pa, out, traj, gtraj, P, n, T, fwd_ms, bwd_ms):
    """--full: the sweep timed alone, which launches were resident, per-kernel MFMA fractions -> out["roofline"]"""
    pa.stage1.set_option("skip_wgrad", 1)            # time the sweep kernel alone
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pa.stage1.rollout_bwd(traj, gtraj, P)
    e0.record()
    for _ in range(a.steps):
        pa.stage1.rollout_bwd(traj, gtraj, P)
    e1.record()
    torch.cuda.synchronize()
    pa.stage1.set_option("skip_wgrad", 0)
    sweep_ms = e0.elapsed_time(e1) / a.steps
    red_ms = max(bwd_ms - sweep_ms, 1e-6)

    # algorithmic flops per point and time step: one branch evaluation = 2 species x 3 branches x 16 channels x 50 taps
    # MACs = 9600 flop; the sweep adds the input-gradient contraction (same size), the gradient kernel recomputes the
    # branches and adds the weight-gradient contraction (same size)
    FB = 2 * 2 * 3 * 16 * 50
    # round 5: rollouts of whole 4x4 patches whose tasks fit on the device run as ONE resident launch each way (persist_status
    # counts them); the entries below then describe that launch (flops and duration of all its time steps)
    st0 = pa._lib.persist_status()["launches"]
    pa.stage1.rollout_fwd_(traj, P)
    fwd_res = pa._lib.persist_status()["launches"] > st0
    st0 = pa._lib.persist_status()["launches"]
    pa.stage1.set_option("skip_wgrad", 1)
    pa.stage1.rollout_bwd(traj, gtraj, P)
    pa.stage1.set_option("skip_wgrad", 0)
    adj_res = pa._lib.persist_status()["launches"] > st0
    torch.cuda.synchronize()
    kernels = [
        ({"kernel": "s1_fwd_persist_kernel", "launches_per_pass": 1, "algorithmic_flops_per_launch": FB * n * T,
          "avg_launch_us": fwd_ms * 1e3, "time_steps_per_launch": T, "us_per_time_step": fwd_ms * 1e3 / T} if fwd_res else
         {"kernel": "s1_fwd_kernel", "launches_per_pass": T, "algorithmic_flops_per_launch": FB * n,
          "avg_launch_us": fwd_ms * 1e3 / T}),
        ({"kernel": "s1_adj_persist_kernel", "launches_per_pass": 1, "algorithmic_flops_per_launch": 2 * FB * n * T,
          "avg_launch_us": sweep_ms * 1e3, "time_steps_per_launch": T + 1, "us_per_time_step": sweep_ms * 1e3 / T} if adj_res else
         {"kernel": "s1_adj_kernel", "launches_per_pass": T + 1, "algorithmic_flops_per_launch": 2 * FB * n,
          "avg_launch_us": sweep_ms * 1e3 / (T + 1)}),
        {"kernel": "s1_wgrad_kernel", "launches_per_pass": 1, "algorithmic_flops_per_launch": 2 * FB * n * T,
         "avg_launch_us": red_ms * 1e3},
    ]
    for k in kernels:
        k["achieved"] = k["algorithmic_flops_per_launch"] / (k["avg_launch_us"] * 1e-6) / 1e12
        k["frac"] = k["achieved"] / MFMA_F32_PEAK_TFS
        k["share_of_pass"] = k["avg_launch_us"] * k["launches_per_pass"] / ((fwd_ms + bwd_ms) * 1e3)
    dom = max(kernels, key=lambda k: k["share_of_pass"])
    out["config"]["time_steps_per_launch"] = T if (fwd_res and adj_res) else 1
    out["roofline"] = {"bound": "mfma", "kernel": dom["kernel"], "achieved": dom["achieved"], "peak": MFMA_F32_PEAK_TFS,
                       "unit": "TFLOP/s", "frac": dom["frac"], "traffic": None,
                       "algorithmic_flops_per_launch": dom["algorithmic_flops_per_launch"],
                       "avg_launch_us": dom["avg_launch_us"], "all_kernels": kernels}


def stage1_cpu_baseline(family, sd, h0, shape, budget_s=15.0):
    """The torch restatement of the reference's Stage-1 cell (bit-identical to the imported reference scripts, trajectory
    and gradients) on this box's host cores."""
    from oracle import restatement as R
    cell = R.OracleStage1Cell(family)
    cell.load_state_dict(sd)

    def run(nsteps):
        t0 = time.perf_counter()
        h = h0[None].clone().requires_grad_(True)
        outs, x = [h], h
        for _ in range(nsteps):
            x, _ = cell(x)
            outs.append(x)
        (torch.cat(outs) ** 2).mean().backward()
        return time.perf_counter() - t0

    ncpu = os.cpu_count() or 1
    best = None
    for th in sorted({min(ncpu, c) for c in (8, 16, 32, 64)}):
        torch.set_num_threads(th)
        run(1)
        t1 = run(4) / 4
        if best is None or t1 < best[1]:
            best = (th, t1)
    cores, t_probe = best
    torch.set_num_threads(cores)
    nsteps = int(max(4, min(400, budget_s / max(t_probe, 1e-6))))
    t = run(nsteps)
    return {"value": nsteps / t, "unit": "steps/s", "cores": cores, "kind": "port",
            "sample": f"{nsteps}-step fwd+bwd rollout of the same {shape[0]}x{shape[1]} Stage-1 problem, "
                      f"torch {torch.__version__} CPU ({cores} threads), loss=mean(traj^2)"}


def physics_extra(pa, cell, family, traj, esz, npts):
    """the physics-residual loss consumer on the trajectory just produced -- one
    frame-parallel residual launch and one adjoint launch, timed with HIP events."""
    from percnn_amd import physics
    Q = {"gs2d": lambda: physics.gray_scott_block(cell, 2e-5, 2e-5 / 4, 1 / 25, 3 / 50),
         "gs3d": lambda: physics.gray_scott_block(cell, 0.2, 0.1, 0.025, 0.055),
         "lo2d": lambda: physics.lambda_omega_block(cell, 0.1)}[family]()
    F = min(traj.shape[0] - 1, 200)                   # frames (bounded: the residual tensor is another F frames)
    sub = traj[:F + 1]
    R = physics.physics_residual(sub, Q)              # warm-up
    gR = torch.ones_like(R)
    g = torch.zeros_like(sub)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    for _ in range(3):
        physics._call("percnn_pi_residual_fwd_", sub, R, Q=Q, nframes=F)
    ev[1].record()
    for _ in range(3):
        physics._call("percnn_pi_residual_bwd_", sub, gR, g[:F], Q=Q, nframes=F)
    ev[2].record()
    torch.cuda.synchronize()
    tf, tb = ev[0].elapsed_time(ev[1]) / 3 * 1e-3, ev[1].elapsed_time(ev[2]) / 3 * 1e-3
    # algorithmic bytes per point-frame: fwd read h_f, h_{f+1}, write R = 3*C*s; adjoint read h_f, g_f, write = 3*C*s
    b = 3 * 2 * esz * npts * F
    out = {"frames": F, "fwd_us": tf * 1e6, "bwd_us": tb * 1e6, "fwd_GBps": b / tf / 1e9, "bwd_GBps": b / tb / 1e9,
           "fwd_frac_of_8TBps": b / tf / 1e9 / HBM_PEAK_GBS, "bwd_frac_of_8TBps": b / tb / 1e9 / HBM_PEAK_GBS,
           "loss_value": float(physics.physics_loss(sub, Q))}
    # the loss AS the consumer sees it (physics.physics_loss = one autograd node: a reducing pass, then two launches that write
    # dL/dtraj) next to the residual-tensor expression it replaced; algorithmic bytes: loss pass reads the trajectory once
    # (C*s per point-frame), gradient = scaled residual (read + write) + adjoint (read h, G, write) = 5*C*s
    del R, gR, g
    torch.cuda.empty_cache()
    res = {}
    for name, fused in (("one_node", True), ("residual_tensor_expression", False)):
        t = sub.detach().requires_grad_(True)
        physics.physics_loss(t, Q, fused=fused).backward()
        t.grad = None
        # several passes between two events: one pass is 0.1-0.3 ms of device work behind ~60 us of host-side launch path
        n = 5 if fused else 2
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        with torch.no_grad():
            physics.physics_loss(t, Q, fused=fused)
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(n):
                physics.physics_loss(t, Q, fused=fused)
            ev[1].record()
        for _ in range(n):
            physics.physics_loss(t, Q, fused=fused).backward()
            t.grad = None
        ev[2].record()
        torch.cuda.synchronize()
        lo = ev[0].elapsed_time(ev[1]) * 1e3 / n
        res[name] = {"loss_us": lo, "gradient_us": max(0.0, ev[1].elapsed_time(ev[2]) * 1e3 / n - lo)}
        del t
        torch.cuda.empty_cache()
    cs = 2 * esz * npts * F
    res["one_node"]["loss_frac_of_8TBps"] = cs / (res["one_node"]["loss_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS
    res["one_node"]["gradient_frac_of_8TBps"] = 5 * cs / (res["one_node"]["gradient_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS
    out["loss_and_gradient"] = res
    return out


def sqerr_extra(pa, traj, P, T, fwd_ms, reps):
    """the same fwd+bwd rollout with the loss INSIDE the backward -- L = mean(traj^2) (SURVEY 8d's dense loss) is
    reduced by one streaming pass and its gradient 2/N * h_t is formed by the sweep from the state it reads anyway: no dL/dtraj
    buffer (2 GB at 512^2 x 1000), 24 instead of 32 algorithmic bytes per point and step in the sweep."""
    from percnn_amd import functional as F_pi
    w = 1.0 / traj.numel()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    F_pi.rollout_bwd_sqerr(traj, P, None, None, 2.0 * w)
    loss = F_pi.traj_sqerr(traj, None, None, w)
    ev[0].record()
    for _ in range(reps):
        loss = F_pi.traj_sqerr(traj, None, None, w)
    ev[1].record()
    for _ in range(reps):
        g0, pg = F_pi.rollout_bwd_sqerr(traj, P, None, None, 2.0 * w)
    ev[2].record()
    torch.cuda.synchronize()
    loss_ms, bwd_ms = ev[0].elapsed_time(ev[1]) / reps, ev[1].elapsed_time(ev[2]) / reps
    assert torch.isfinite(g0).all() and torch.isfinite(pg).all() and torch.isfinite(loss)
    return {"what": "L = mean(traj^2): loss value by one streaming pass, gradient formed inside the sweep (no dL/dtraj)",
            "loss_pass_us_per_time_step": loss_ms * 1e3 / T, "bwd_us_per_time_step": bwd_ms * 1e3 / T,
            "sweep_algorithmic_bytes_per_point_step": 3 * 2 * traj.element_size(),
            "fwd_bwd_steps_per_sec": T / ((fwd_ms + loss_ms + bwd_ms) * 1e-3)}


def strided_loss_extra(pa, traj, gtraj, P, T, fwd_ms, reps):
    """SURVEY 8d config (2), second loss: the reference's data loss only looks at every 20th frame
    (output[0:-1:20, ...], train_2drd.py:397), so dL/dtraj is non-zero on those frames only; the backward is told so
    (frame mask) and never reads the other frames of dL/dtraj (24 instead of 32 B per point and step)."""
    mask = [False] * (T + 1)
    for t in list(range(T + 1))[0:-1:20]:
        mask[t] = True
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pa.rollout_bwd(traj, gtraj, P, frame_mask=mask)
    e0.record()
    for _ in range(reps):
        g0, pg = pa.rollout_bwd(traj, gtraj, P, frame_mask=mask)
    e1.record()
    torch.cuda.synchronize()
    bwd_ms = e0.elapsed_time(e1) / reps
    assert torch.isfinite(g0).all() and torch.isfinite(pg).all()
    return {"observed_frames": sum(mask), "bwd_us_per_time_step": bwd_ms * 1e3 / T,
            "fwd_bwd_steps_per_sec": T / ((fwd_ms + bwd_ms) * 1e-3)}


def slab_extra_isolated(a, dev, dist, rank, world, local_rank):
    """Run slab_extra in a child process per rank (its own process group on a fresh port): the halo ring hands RCCL
    function addresses to the native loop, and a crash or stall in there must not take the headline line with it.
    --slab-in-process: the same series inside this rank, on the rank's process group (one process per rank instead of two)."""
    import socket
    import subprocess
    if a.slab_in_process:
        import percnn_amd as pa
        os.environ.setdefault("PERCNN_PEER_TIMEOUT_S", "15")      # (the child's bound, see below)
        one_gpu = bool(int(os.environ.get("PERCNN_BENCH_ONE_GPU", "0")))
        try:
            res = sharded_series(dev, dist, rank, world, one_gpu, steps=a.steps, warmup=a.warmup)
        finally:
            pa.slab.close_exchangers()
        return json.loads(json.dumps(res))                       # what the child's line would carry
    if dist is None:                                 # plain `python bench.py`: one rank, no process group in the child either
        env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK=str(local_rank))
        for k in ("MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
    else:
        port = torch.zeros(1, dtype=torch.int64, device=dev)
        if rank == 0:
            with socket.socket() as so:
                so.bind(("127.0.0.1", 0))
                port[0] = so.getsockname()[1]
        if world > 1:
            dist.broadcast(port, 0)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(int(port.item())), RANK=str(rank),
                   WORLD_SIZE=str(world), LOCAL_RANK=str(local_rank))
    for k in ("TORCHELASTIC_RUN_ID", "TORCHELASTIC_USE_AGENT_STORE", "TORCHELASTIC_RESTART_COUNT",
              "TORCHELASTIC_MAX_RESTARTS", "GROUP_RANK", "ROLE_RANK", "ROLE_NAME"):
        env.pop(k, None)                             # plain env:// rendezvous on the new port
    # a mailbox exchange whose neighbour never delivers gives up after this many seconds (library default: 300) -- in a bench
    # the ranks are in lock step, and a stuck exchange must end as "timed_out_exchange" in the line, not as a spinning kernel
    # that the watchdog below has to kill
    env.setdefault("PERCNN_PEER_TIMEOUT_S", "15")
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--slab-child", "--gpus", str(a.gpus),
                              "--steps", str(a.steps), "--warmup", str(a.warmup)], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    timed_out = False
    try:
        so, se = child.communicate(timeout=a.slab_timeout)
    except subprocess.TimeoutExpired:
        timed_out = True
        child.kill()
        so, se = child.communicate()
    # the child prints a (growing) JSON line after every phase -- portable transport first, the experimental one last -- so
    # that a stall or crash in a later phase costs only that phase
    lines = [l for l in (so or "").splitlines() if l.startswith("{")]
    if not lines:
        return {"error": f"child timed out after {a.slab_timeout}s" if timed_out else f"child exit code {child.returncode}",
                "stderr_tail": (se or "")[-300:]}
    res = json.loads(lines[-1])
    if timed_out or child.returncode != 0:
        res["incomplete"] = (f"child timed out after {a.slab_timeout}s" if timed_out else f"child exit code {child.returncode}") + \
                            "; phases completed before that are reported"
        res["stderr_tail"] = (se or "")[-300:]
    return res


def _all_max(dist, dev, x):
    """max over ranks of a host float (gloo groups reduce on the host)"""
    if dist is None or dist.get_world_size() == 1:
        return x
    t = torch.tensor([x], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sharded_rollout(dev, dist, rank, world, full_shape, T, halo, reps, transport, force_p2p, P, blocks_seed=0,
                    breakdown=True, overlap=None, adj_put=False, contract=None, verify_T=None):
    """3D Gray-Scott, Hc=2, fp32: the global grid `full_shape` cut into `world` slabs along axis 0 (axis 0 must divide).
    Times T-step forward + backward rollouts of the slab path (barrier on both sides, max over ranks, median of `reps`),
    checks every rank's forward state bit for bit against the single-domain rollout of the whole grid, and -- breakdown --
    splits the time per step into compute (the same local arrays with a local wrap instead of a transport), communication
    (the rollout's exchanges alone) and what of it is exposed (total - compute).
    contract = (steps, warmup): the bench contract's clock instead of the median -- `warmup` untimed passes, then EXACTLY `steps`
    passes between two barrier + synchronize pairs, max over ranks (what the top-level line of an N > 1 run reports).
    verify_T: compare only the first verify_T + 1 frames with the single-domain rollout (long rollouts: the reference costs a
    whole-grid trajectory per rank)."""
    import percnn_amd as pa
    from percnn_amd import slab, synthetic
    planes = full_shape[0] // world
    assert planes * world == full_shape[0] and planes >= halo
    if adj_put:                              # mailboxes: the adjoint sweep launch puts its faces itself (default off)
        pa.set_option("slab_fused_put_adj", 1)
        try:
            return sharded_rollout(dev, dist, rank, world, full_shape, T, halo, reps, transport, force_p2p, P, blocks_seed,
                                   breakdown, overlap, False, contract, verify_T)
        finally:
            pa.set_option("slab_fused_put_adj", 0)
    ex = slab.make_exchanger(force_p2p=force_p2p, transport=transport)
    local_wrap = world == 1 and not force_p2p
    gen = torch.Generator().manual_seed(blocks_seed)
    h_full = synthetic.gs_initial_state(full_shape, seed=blocks_seed)[0]
    local = torch.zeros((2, planes + 2 * halo) + tuple(full_shape[1:]), device=dev)
    local[:, halo:halo + planes] = h_full[:, planes * rank:planes * (rank + 1)].to(dev)
    traj = torch.zeros((T + 1,) + tuple(local.shape), device=dev)
    traj[0] = local
    gtraj = torch.randn(traj.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(rank)) / traj.numel()

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if overlap is None:
        overlap = bool(int(os.environ.get("PERCNN_SLAB_OVERLAP", "0")))

    def timed(fn, n):
        fn()
        fn()                                # second warm-up: lazily created RCCL channels / allocator blocks
        ts = []
        for _ in range(n):                  # every pass timed on its own (barrier on both sides, max over ranks); the median is
            sync()                          # reported: one stray stall (first-use setup inside RCCL) used to dominate
            s0 = time.perf_counter()
            fn()
            sync()
            ts.append(_all_max(dist, dev, time.perf_counter() - s0))
        return float(np.median(ts))

    res = {}

    def run(e=ex):
        slab.slab_rollout_fwd_(traj, P, e, halo, overlap=overlap)
        res["g"] = slab.slab_rollout_bwd(traj, gtraj, P, e, halo, overlap=overlap)

    if contract is not None:
        K, W = int(contract[0]), int(contract[1])
        for _ in range(max(W, 1)):
            run()
        sync()
        s0 = time.perf_counter()
        for _ in range(K):
            run()
        sync()
        wall = _all_max(dist, dev, time.perf_counter() - s0)
        el = wall / K
    else:
        el = timed(run, reps)
    pg = res["g"][1]
    assert torch.isfinite(pg).all() and torch.isfinite(traj[-1][:, halo:-halo]).all()
    # verification: the whole grid as ONE periodic domain on this GPU, same kernels -> my planes must match exactly
    Tv = T if verify_T is None else min(T, int(verify_T))
    ref = torch.empty((Tv + 1, 2) + tuple(full_shape), device=dev)
    ref[0] = h_full.to(dev)
    pa.rollout_fwd_(ref, P)
    same = torch.equal(ref[:, :, planes * rank:planes * (rank + 1)], traj[:Tv + 1, :, halo:halo + planes])
    del ref
    ok = torch.tensor([1 if same else 0], dtype=torch.int32, device=dev if (dist is None or dist.get_backend() == "nccl") else "cpu")
    if dist is not None:
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    name = "none (one rank: periodic wrap by index inside the step launches)" if local_wrap else type(ex).__name__
    out = {"workload": f"gs3d {'x'.join(map(str, full_shape))} cut into {world} slab(s) of {planes} planes, Hc=2, "
                       f"T={T} fwd+bwd, forward halo {halo} (={halo // 2} steps per exchange), adjoint sweep "
                       f"exchanges 2 planes per step; native C loop (one call per rollout), overlap={int(overlap)}",
           "transport": name,
           "steps_per_sec_fwd_bwd": T / el, "us_per_time_step_fwd_bwd": el / T * 1e6,
           "exchange": ("periodic wrap by index inside the step launches (one rank, no transport, no face copies)" if local_wrap
                        else {"PeerHaloExchanger": "peer mailboxes: put / take kernels + epoch flags (csrc/pi_peer.h)",
                              "RcclHaloExchanger": "ncclSend / ncclRecv groups issued by the native loop",
                              "HaloExchanger": "torch.distributed point-to-point"}[type(ex).__name__]
                        + (" -- to the rank itself" if world == 1 else "")),
           "forward_state_equals_single_domain_rollout": bool(ok.item()), "frames_compared": Tv + 1,
           "ranks_seen_by_transport": int(ex.ranks_seen),
           "points_per_rank": planes * int(np.prod(full_shape[1:])), "global_points": int(np.prod(full_shape)),
           "halo_bytes_per_exchange_per_direction": 2 * halo * int(np.prod(full_shape[1:])) * 4}
    if breakdown and local_wrap:
        # the launches each rank of a multi-rank run issues, minus the transport: face copies into the halo planes, the outer
        # planes of every second forward step recomputed (until round 5 this WAS the one-rank schedule)
        lw = slab.LocalWrapExchanger(copies=True)
        comp = timed(lambda: run(lw), max(2, reps // 2))
        out["multi_rank_launches_with_face_copies_us_per_time_step"] = comp / T * 1e6
        run()                                    # the frames' interiors as the index-wrap schedule leaves them
    if breakdown and not local_wrap:
        lw = slab.LocalWrapExchanger()
        comp = timed(lambda: run(lw), max(2, reps // 2))
        k = halo // 2
        face = traj[0]

        def exchanges():                     # the exchanges one fwd+bwd rollout issues, nothing else
            for _ in range((T + k - 1) // k):
                ex.exchange(face, halo, halo)
            for _ in range(T):
                ex.exchange(face, halo, 2)
        comm = timed(exchanges, max(2, reps // 2))
        slab.slab_rollout_fwd_(traj, P, ex, halo, overlap=overlap)      # frame 0's halos were overwritten by the loop above
        out["per_time_step_us"] = {"total": el / T * 1e6, "compute_alone": comp / T * 1e6, "exchanges_alone": comm / T * 1e6,
                                   "exposed": max(0.0, (el - comp) / T * 1e6)}
    if contract is not None:
        out.update({"clock": "bench contract: warm-up passes, then exactly `steps` passes between barrier + synchronize pairs, max over ranks",
                    "steps": K, "warmup": W, "T": T, "ms_per_step": el * 1e3, "timed_region_s": wall})
    if hasattr(ex, "status"):
        out["timed_out_exchange"] = ex.status()
    del traj, gtraj
    torch.cuda.empty_cache()
    return out


def single_domain_anchor(dev, full_shape, T, reps, P, contract=None):
    """N = 1 anchor of a strong-scaling series: the whole grid as ONE periodic domain (no slab layout, no exchange).
    contract = (steps, warmup): the bench contract's clock (see sharded_rollout)."""
    import percnn_amd as pa
    from percnn_amd import synthetic
    traj = torch.empty((T + 1, 2) + tuple(full_shape), device=dev)
    traj[0] = synthetic.gs_initial_state(full_shape, seed=0)[0].to(dev)
    g = torch.randn(traj.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) / traj.numel()
    if contract is not None:
        K, W = int(contract[0]), int(contract[1])
        for _ in range(max(W, 1)):
            pa.rollout_fwd_(traj, P)
            pa.rollout_bwd(traj, g, P)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            pa.rollout_fwd_(traj, P)
            pa.rollout_bwd(traj, g, P)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        el = wall / K
        del traj, g
        torch.cuda.empty_cache()
        return {"workload": f"gs3d {'x'.join(map(str, full_shape))} single-domain rollout (no slab layout), Hc=2, T={T} fwd+bwd",
                "transport": "none (single domain)", "steps_per_sec_fwd_bwd": T / el, "us_per_time_step_fwd_bwd": el / T * 1e6,
                "global_points": int(np.prod(full_shape)), "steps": K, "warmup": W, "T": T, "ms_per_step": el * 1e3,
                "timed_region_s": wall}
    ts = []
    for i in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pa.rollout_fwd_(traj, P)
        pa.rollout_bwd(traj, g, P)
        torch.cuda.synchronize()
        if i >= 2:
            ts.append(time.perf_counter() - t0)
    el = float(np.median(ts))
    del traj, g
    torch.cuda.empty_cache()
    return {"workload": f"gs3d {'x'.join(map(str, full_shape))} single-domain rollout (no slab layout), Hc=2, T={T} fwd+bwd",
            "transport": "none (single domain)", "steps_per_sec_fwd_bwd": T / el, "us_per_time_step_fwd_bwd": el / T * 1e6,
            "global_points": int(np.prod(full_shape))}


def sharded_series(dev, dist, rank, world, one_gpu, checkpoint=lambda res: None, steps=20, warmup=3):
    """What the slab child reports:
      headline -- N > 1 only: configs[4], the FIXED 256^3 grid cut into N slabs, T = 100 forward + backward per pass, on the
                 bench contract's clock (`warmup` passes, exactly `steps` passes between barrier + synchronize pairs, max over
                 ranks), with the N = 1 anchor (the single-domain rollout of the same grid, same clock) measured by every rank
                 on its own GPU in the same run.  This is what the top-level line of an N > 1 run carries;
      weak    -- configs[4]-shaped, 32 planes of 256^2 per rank (256^3 at N = 8), every usable transport;
      strong  -- north_star's curve: FIXED global grids 256^3 (configs[4]) and 128^3 cut into N slabs; N = 1 is the
                 single-domain rollout.  The driver divides by its own N = 1 line.
    Order: everything on the library's proven transport first (RCCL send / recv; torch.distributed in one-GPU mode), a JSON
    line printed (`checkpoint`), THEN the peer mailboxes -- probed against the portable exchange bit for bit before they carry
    a rollout -- and the strong series once more on them if the probe found them faster.  A fault in the second phase cannot
    cost the first."""
    import percnn_amd as pa
    from percnn_amd import slab
    sd = load_params(WORKLOADS["gs3d_128"][5])
    cell = make_cell("gs3d", sd, dev)
    with torch.no_grad():
        P = cell.param_block().contiguous()
    force_p2p = bool(int(os.environ.get("PERCNN_FORCE_P2P", "0")))
    small = bool(int(os.environ.get("PERCNN_BENCH_SMALL", "0")))          # test mode: tiny grids, same control flow
    hw, planes, halo = (64, 8, 4) if small else (256, 32, 4)
    Tw, reps = (6, 2) if small else (100, 5)      # (T = 100: the rollout length of configs[4]; 40 until round 4)
    grids = (((32, 2), (16, 2)) if small else ((256, 20), (128, 40)))       # (256^3: T = 10 until round 4)
    head_n, head_T = (32, 6) if small else (256, int(os.environ.get("PERCNN_BENCH_HEADLINE_T", "100")))
    sharded = world > 1 or force_p2p
    base = "dist" if one_gpu else "rccl"
    out = {"transport_probe": {}, "weak_scaling": {"what": f"{planes} planes of {hw}^2 per rank", "by_transport": {}},
           "strong_scaling": {"what": "fixed global grid cut into N slabs along axis 0; N = 1 = single-domain rollout",
                              "transport": base if sharded else "none", "by_grid": {}}}
    weak, strong = out["weak_scaling"]["by_transport"], out["strong_scaling"]["by_grid"]

    def guarded(fn):
        try:
            return fn()
        except Exception as e:
            return {"error": repr(e)[:300]}

    SCHEDULES = {"plain": "exchange between two steps (mailboxes: forward faces put by the step launch itself)",
                 "overlap": "faces first, exchange on a side stream",
                 "adj_put": "exchange between two steps, forward AND adjoint faces put by the step / sweep launches themselves"}

    def strong_on(transport, dest, schedule="plain"):
        for n3, T in grids:
            full, key = (n3, n3, n3), f"{n3}^3"
            if n3 % world or n3 // world < halo:
                dest[key] = {"skipped": f"{n3} planes do not cut into {world} slabs of >= {halo}"}
            elif not sharded:
                dest[key] = guarded(lambda: single_domain_anchor(dev, full, T, 3, P))
            else:
                dest[key] = guarded(lambda: sharded_rollout(dev, dist, rank, world, full, T, halo, 3, transport, force_p2p, P,
                                                            overlap=schedule == "overlap", adj_put=schedule == "adj_put"))

    def weak_pair(transport):
        """-> the fastest schedule.  The weak-scaled slab on `transport` with the plain schedule (exchange between two steps) and with the faces-first
        schedule (faces of the frame about to be exchanged computed first, the exchange on a side stream under the interior
        planes).  On ONE GPU the second costs more than it hides (three launches per step: 104 us to self); whether a real
        xGMI wire turns that around is decided HERE, by measurement on the hardware the run is on -> the schedule the strong
        series then uses."""
        weak[transport] = guarded(lambda: sharded_rollout(dev, dist, rank, world, (planes * world, hw, hw), Tw, halo, reps,
                                                          transport, force_p2p, P))
        checkpoint(out)
        key = transport + "_faces_first_overlap"
        weak[key] = guarded(lambda: sharded_rollout(dev, dist, rank, world, (planes * world, hw, hw), Tw, halo, reps,
                                                    transport, force_p2p, P, breakdown=False, overlap=True))
        cands = {"plain": weak[transport], "overlap": weak[key]}
        if transport == "peer":              # third schedule, mailboxes only: the sweep launch puts the adjoint faces as well
            checkpoint(out)
            weak["peer_fused_adjoint_put"] = guarded(lambda: sharded_rollout(
                dev, dist, rank, world, (planes * world, hw, hw), Tw, halo, reps, "peer", force_p2p, P, breakdown=False, adj_put=True))
            cands["adj_put"] = weak["peer_fused_adjoint_put"]
        best, best_t = "plain", cands["plain"].get("us_per_time_step_fwd_bwd")
        for name, r in cands.items():        # every rank computes the same answer: the times are maxima over ranks
            t = r.get("us_per_time_step_fwd_bwd")
            if t and r.get("forward_state_equals_single_domain_rollout") is True and (not best_t or t < best_t):
                best, best_t = name, t
        return best

    def headline(transport, schedule):
        full = (head_n,) * 3
        r = sharded_rollout(dev, dist, rank, world, full, head_T, halo, 3, transport, force_p2p, P, breakdown=False,
                            overlap=schedule == "overlap", adj_put=schedule == "adj_put", contract=(steps, warmup),
                            verify_T=min(head_T, 10))
        r["schedule"] = SCHEDULES[schedule]
        r["transport_key"] = transport
        r["grid"] = list(full)
        return r

    def better(a, b):
        """b replaces a when it is a valid (bit-identical) measurement and faster"""
        if "error" in b or b.get("forward_state_equals_single_domain_rollout") is not True:
            return a
        if "error" in a or a.get("forward_state_equals_single_domain_rollout") is not True:
            return b
        return b if b["steps_per_sec_fwd_bwd"] > a["steps_per_sec_fwd_bwd"] else a

    # ---- phase 0 (N > 1): the line's top level -- configs[4] strong-scaled, plain schedule on the proven transport first
    if world > 1 and head_n % world == 0 and head_n // world >= halo:
        out["headline"] = guarded(lambda: headline(base, "plain"))
        checkpoint(out)
        # the N = 1 anchor of the same grid on this very box (every rank on its own GPU; rank 0's is reported)
        out["headline_n1_anchor"] = guarded(lambda: single_domain_anchor(dev, (head_n,) * 3, min(head_T, 20), 3, P,
                                                                         contract=(max(3, steps // 4), 1)))
        if dist is not None:
            dist.barrier()
        checkpoint(out)
    # ---- phase 1: the proven transport
    sched_base = "plain"
    if not sharded:
        weak["local_wrap"] = guarded(lambda: sharded_rollout(dev, dist, rank, world, (planes, hw, hw), Tw, halo, reps, "dist", False, P))
    else:
        sched_base = weak_pair(base)
        out["strong_scaling"]["schedule"] = SCHEDULES[sched_base]
        if "headline" in out and sched_base != "plain":      # the weak pair found a faster schedule on this hardware
            out["headline"] = better(out["headline"], guarded(lambda: headline(base, sched_base)))
            checkpoint(out)
    strong_on(base, strong, sched_base)
    checkpoint(out)
    # ---- phase 2: peer mailboxes (xGMI load / store + epoch flags)
    if int(os.environ.get("PERCNN_NO_PEER", "0")):
        return out
    if not sharded:                               # one rank: put / take through the rank's own mailbox
        weak["peer_to_self"] = guarded(lambda: sharded_rollout(dev, dist, rank, world, (planes, hw, hw), Tw, halo, reps, "peer", True, P))
        return out
    picked, probe = base, {}
    try:
        sample = torch.rand((2, planes + 2 * halo, hw, hw), device=dev)
        picked, probe = slab.probe_transport(sample, halo, candidates=(base, "peer"), force_p2p=force_p2p)
        del sample
    except Exception as e:
        probe = {"error": repr(e)[:300]}
    out["transport_probe"] = probe
    checkpoint(out)
    if probe.get("peer", {}).get("usable_on_every_rank"):
        sched_peer = weak_pair("peer")
        checkpoint(out)
        if picked == "peer" and "headline" in out:
            out["headline"] = better(out["headline"], guarded(lambda: headline("peer", sched_peer)))
            checkpoint(out)
        if picked == "peer":
            out["strong_scaling"]["by_grid_peer"] = {}
            out["strong_scaling"]["schedule_peer"] = SCHEDULES[sched_peer]
            strong_on("peer", out["strong_scaling"]["by_grid_peer"], sched_peer)
            out["strong_scaling"]["transport_picked_by_probe"] = "peer"
        checkpoint(out)
    return out


if __name__ == "__main__":
    main()
