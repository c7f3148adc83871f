"""Shared by test_discovery_cpu.py / test_discovery_gpu.py: the Stage-2 library as an explicit float64 numpy matrix, with the
hash row classes, and STRidge on explicit matrices (both written from the definitions, independent of percnn_amd.discovery's
moment-based code except for ``row_class``, which test_discovery_cpu.py pins to hand-computed values)."""
import functools
import os

import numpy as np

GOLDEN_STAGE2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage2", "stage2_burgers_32x32.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN_STAGE2))


def _d1(f, ax, dx):
    return (np.roll(f, 2, ax) - 8 * np.roll(f, 1, ax) + 8 * np.roll(f, -1, ax) - np.roll(f, -2, ax)) / (12 * dx)


def _lap(f, dx):
    s = -5.0 * f
    for ax in (1, 2):
        s = s + (-1 / 12) * (np.roll(f, 2, ax) + np.roll(f, -2, ax)) + (4 / 3) * (np.roll(f, 1, ax) + np.roll(f, -1, ax))
    return s / dx ** 2


def explicit_library(traj, dx, dt, region):
    """traj [N, 2, H, W] -> Theta [rows, 70], y [rows, 2], r [rows] (full-grid row index), float64; rows in (f, y, x) order"""
    h = np.asarray(traj, dtype=np.float64)
    N, _, H, W = h.shape
    u, v = h[:N - 2, 0], h[:N - 2, 1]
    ut, vt = (h[1:N - 1, 0] - u) / dt, (h[1:N - 1, 1] - v) / dt
    B = [np.ones_like(u), _d1(u, 1, dx), _d1(u, 2, dx), _d1(v, 1, dx), _d1(v, 2, dx), _lap(u, dx), _lap(v, dx)]
    A = [np.ones_like(u), u, v, u * u, u * v, v * v, u ** 3, u * u * v, u * v * v, v ** 3]
    r = np.arange((N - 2) * H * W, dtype=np.int64).reshape(N - 2, H, W)
    sl = (slice(None), slice(2, H - 2), slice(2, W - 2)) if region == "interior" else (slice(None),) * 3
    theta = np.stack([(a * b)[sl].reshape(-1) for a in A for b in B], axis=1)
    y = np.stack([ut[sl].reshape(-1), vt[sl].reshape(-1)], axis=1)
    return theta, y, r[sl].reshape(-1)


def explicit_moments(traj, dx, dt, region, seed, t_train, t_keep):
    """G [2, 70, 70], b [2, 70, 2], yy [2, 2], n [2] from the explicit matrix"""
    from percnn_amd.discovery import row_class
    theta, y, r = explicit_library(traj, dx, dt, region)
    cls = row_class(r, seed, t_train, t_keep)
    G, b, yy, n = np.zeros((2, 70, 70)), np.zeros((2, 70, 2)), np.zeros((2, 2)), np.zeros(2)
    for c in (0, 1):
        X, Y = theta[cls == c], y[cls == c]
        G[c], b[c], yy[c], n[c] = X.T @ X, X.T @ Y, (Y * Y).sum(0), len(X)
    return G, b, yy, n


# ---- STRidge on explicit matrices (float64), from the algorithm -----------------------------------------------------------
def _lstsq(X, y):
    return np.linalg.lstsq(X, y, rcond=None)[0]


def explicit_stridge(X, y, lam, maxit, tol, must_have):
    d = X.shape[1]

    def ridge(idx):
        Xs = X[:, idx]
        return _lstsq(Xs.T @ Xs + lam * np.eye(len(idx)), Xs.T @ y) if lam != 0 else _lstsq(Xs, y)

    w = ridge(np.arange(d))
    count = d
    big = np.flatnonzero(np.abs(w) > tol)
    for _ in range(maxit):
        keep = sorted(set(np.flatnonzero(~(np.abs(w) < tol)).tolist()) | {must_have})
        if len(keep) == count:
            break
        count = len(keep)
        big = np.array(keep)
        w2 = np.zeros(d)
        w2[big] = ridge(big)
        w = w2
    if len(big):
        w[big] = _lstsq(X[:, big], y)
    return w


def explicit_train(theta, y, cls, *, maxit, str_iters, lam, d_tol, kappa, must_have):
    kept = cls < 2
    scale = 1.0 / np.linalg.norm(theta[kept], axis=0)
    R = theta * scale
    Xtr, ytr, Xte, yte = R[cls == 0], y[cls == 0], R[cls == 1], y[cls == 1]
    tol = float(d_tol)
    w_best = _lstsq(Xtr, ytr)
    err_f = np.mean((yte - Xte @ w_best) ** 2)
    l0 = kappa * err_f
    err_best = err_f + l0 * np.count_nonzero(w_best)
    for it in range(maxit):
        w = explicit_stridge(Xtr, ytr, lam, str_iters, tol, must_have)
        err = np.mean((yte - Xte @ w) ** 2) + l0 * np.count_nonzero(w)
        if err <= err_best:
            err_best, w_best = err, w
            tol = tol + d_tol
        else:
            tol = max(0.0, tol - 2 * d_tol)
            d_tol = 2 * d_tol / (maxit - it)
            tol = tol + d_tol
    return scale * w_best
