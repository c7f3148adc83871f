#!/usr/bin/env python3
"""Generate tests/golden/stage2/stage2_burgers_32x32.npz: the REAL reference Stage-2 (library + STRidge) on a small trajectory.

    python tools/make_golden_stage2.py

The reference's ``derivatives.Loss_generator``, ``PDE_FIND_u.STRidgeTrainer`` / ``PDE_FIND_v.STRidgeTrainer`` and
``gen_library`` are imported in a subprocess with ``.cuda()`` shimmed to a no-op (as tools/make_golden.py does); the reference
files are neither modified nor copied, only data they compute is written.  Runs on the CPU.

Trajectory: periodic 2D Burgers, nu = 0.005, dx = 1/100, dt = 2.5e-4, 32 x 32, 21 stored frames, float32.  Initial state: four
random low Fourier modes of amplitude about 0.5 per component (numpy default_rng(0)).  Explicit Euler with the library's own
stencils and 4 sub-steps per stored frame, so the stored-frame difference is not an exact fit of the library.
The tool asserts that the reference alone returns exactly ones*lap_u, u*u_x, v*u_y and ones*lap_v, u*v_x, v*v_y on it.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGE2 = "DataDrivenDiscoveryOfPDEs/2D_Burgers_eqn/Stage-2"
# (its own directory: tests/util.py takes every tests/golden/*.npz for a Pi-block rollout case)
OUT = os.path.join(ROOT, "tests", "golden", "stage2", "stage2_burgers_32x32.npz")
NU, DX, DT, N, H, W, SUB = 0.005, 1.0 / 100, 2.5e-4, 21, 32, 32, 4
KEEP, TRAIN = 0.2, 0.8
SETTINGS = {"u": dict(maxit=100, STR_iters=40, lam=0.01, d_tol=20, kappa=1, must_have=5),
            "v": dict(maxit=150, STR_iters=40, lam=0.01, d_tol=20, kappa=1, must_have=6)}
EXPECT = {"u": ["ones*lap_u", "u*u_x", "v*u_y"], "v": ["ones*lap_v", "u*v_x", "v*v_y"]}


def d1(f, ax):
    return (np.roll(f, 2, ax) - 8 * np.roll(f, 1, ax) + 8 * np.roll(f, -1, ax) - np.roll(f, -2, ax)) / (12 * DX)


def lap(f):
    s = -5.0 * f
    for ax in (0, 1):
        s = s + (-1 / 12) * (np.roll(f, 2, ax) + np.roll(f, -2, ax)) + (4 / 3) * (np.roll(f, 1, ax) + np.roll(f, -1, ax))
    return s / DX ** 2


def trajectory():
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    h = np.zeros((2, H, W))
    for s in range(2):
        for _ in range(4):
            ky, kx = rng.integers(-2, 3, size=2)
            h[s] += 0.5 * rng.uniform(0.5, 1.0) * np.cos(2 * np.pi * (ky * yy + kx * xx) + rng.uniform(0, 2 * np.pi))
    frames = [h.copy()]
    for _ in range(N - 1):
        for _ in range(SUB):
            u, v = h
            h = h + (DT / SUB) * np.stack([NU * lap(u) - u * d1(u, 0) - v * d1(u, 1), NU * lap(v) - u * d1(v, 0) - v * d1(v, 1)])
        frames.append(h.copy())
    return np.stack(frames).astype(np.float32)


def child(traj_file, out_file):
    """the reference's own Stage-2 on the trajectory (PDE_FIND_u.py:224-266 without the .mat file and the plots)"""
    import torch
    from tools.make_golden import REF
    torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(REF, STAGE2))
    import derivatives
    import PDE_FIND_u
    import PDE_FIND_v
    traj = torch.from_numpy(np.load(traj_file))
    terms = derivatives.to_numpy_float64(derivatives.Loss_generator(dt=DT, dx=DX).get_phy_residual(traj))
    lib = PDE_FIND_u.gen_library()
    assert lib == PDE_FIND_v.gen_library()
    theta = np.concatenate([eval(e, {}, dict(terms)) for e in lib], axis=1)            # the reference's `lhs`, all rows
    y = np.concatenate([terms["u_t"], terms["v_t"]], axis=1)
    rec = {"names": np.array(lib), "G_ref": theta.T @ theta, "b_ref": theta.T @ y, "yy_ref": (y * y).sum(0), "rows": theta.shape[0]}
    n = theta.shape[0]
    for sp, mod in (("u", PDE_FIND_u), ("v", PDE_FIND_v)):
        np.random.seed(0)
        idx = np.random.choice(n, int(n * KEEP), replace=False)
        trainer = mod.STRidgeTrainer(R0=theta[idx], Ut=terms[sp + "_t"][idx], normalize=2, split_ratio=TRAIN)
        rec["w_best_" + sp] = trainer.train(**SETTINGS[sp])[:, 0]
    np.savez(out_file, **rec)


def main():
    traj = trajectory()
    with tempfile.TemporaryDirectory() as tmp:
        tf, of = os.path.join(tmp, "traj.npy"), os.path.join(tmp, "ref.npz")
        np.save(tf, traj)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tf, of], check=True, stdout=subprocess.DEVNULL)
        ref = dict(np.load(of))
    names = [str(s) for s in ref["names"]]
    for sp in ("u", "v"):
        w = ref["w_best_" + sp]
        got = [names[i] for i in np.flatnonzero(w)]
        assert got == EXPECT[sp], f"the reference found {got} for {sp}: this trajectory does not qualify as a fixture"
        print(sp, {names[i]: float(w[i]) for i in np.flatnonzero(w)})
    rec = dict(ref, traj=traj, dx=DX, dt=DT, nu=NU, keep_fraction=KEEP, train_fraction=TRAIN, substeps=SUB)
    for sp in ("u", "v"):
        for k, val in SETTINGS[sp].items():
            rec[f"settings_{sp}/{k}"] = val
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {os.path.relpath(OUT, ROOT)} ({os.path.getsize(OUT) / 1024:.0f} KiB)")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
