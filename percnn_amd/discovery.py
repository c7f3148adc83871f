"""Stage-2 equation discovery: the 70-term candidate library as second moments on the device, STRidge on 70 x 70 matrices.

Replaces DataDrivenDiscoveryOfPDEs/2D_Burgers_eqn/Stage-2/{derivatives.py:129-199, PDE_FIND_u.py, PDE_FIND_v.py} (and the
lambda-omega Stage-2, the same code with dx = 0.2, dt = 0.0125).  The reference copies the trajectory to the host, builds a
rows x 70 matrix and runs sequential-threshold ridge regression on it; the regression needs that matrix only through
``G = Theta^T Theta``, ``b = Theta^T y``, ``y^T y`` and the row count, which ``library_moments`` accumulates in one pass over the
device trajectory (csrc/pi_disc.h, include/percnn_pi_discovery.h).  ``stridge`` / ``train_stridge`` restate the reference's
``STRidgeTrainer`` on those moments, on the host, in float64.

The reference's random 20 % subsample and its random 80 / 20 train / test split become a hash of the row index
(``row_class``), which the kernel evaluates per point.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib

_A = ["ones", "u", "v", "u**2", "u*v", "v**2", "u**3", "u**2*v", "u*v**2", "v**3"]           # the order of physics._IDX
_B = ["ones", "u_x", "u_y", "v_x", "v_y", "lap_u", "lap_v"]
LIBRARY_TERMS = [a + "*" + b for a in _A for b in _B]                                        # gen_library(), PDE_FIND_u.py:185-193
REGIONS = {"interior": 0, "periodic": 1}
REFERENCE_SPLIT = (0, 0.2, 0.8)                        # seed, kept fraction of the rows, training fraction of the kept rows
DEFAULTS = {"u": dict(maxit=100, str_iters=40, lam=0.01, d_tol=20.0, kappa=1.0, must_have=5),      # PDE_FIND_u.py:266
            "v": dict(maxit=150, str_iters=40, lam=0.01, d_tol=20.0, kappa=1.0, must_have=6)}      # PDE_FIND_v.py


class LibraryMoments(NamedTuple):
    """float64, leading [B] only for batched input, then the class (0 = train, 1 = test)"""
    G: object       # [..., 2, 70, 70]  Theta^T Theta
    b: object       # [..., 2, 70, 2]   Theta^T (u_t, v_t)
    yy: object      # [..., 2, 2]       sum u_t^2, sum v_t^2
    n: object       # [..., 2]          rows


def mix32(x):
    x = np.asarray(x).astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def row_class(r, seed: int, t_train: int, t_keep: int):
    """Class of the rows with full-grid index ``r = (f*H + y)*W + x``: 0 = train, 1 = test, 2 = dropped (the kernel's rule)."""
    with np.errstate(over="ignore"):
        h = mix32(np.asarray(r).astype(np.uint32) + np.uint32(seed & 0xffffffff)).astype(np.uint64)
    return np.where(h < np.uint64(t_train), 0, np.where(h < np.uint64(t_keep), 1, 2)).astype(np.int8)


def split_thresholds(split):
    """None -> every row trains;  (seed, keep_fraction, train_fraction) -> (seed, t_train, t_keep) on the 2^32 scale"""
    if split is None:
        return 0, 1 << 32, 1 << 32
    seed, keep, train = split
    if not (0.0 <= keep <= 1.0 and 0.0 <= train <= 1.0):
        raise ValueError(f"split: fractions must lie in [0, 1], got keep = {keep}, train = {train}")
    t_keep = int(round(keep * 2.0 ** 32))
    return int(seed) & 0xffffffff, min(int(round(keep * train * 2.0 ** 32)), t_keep), t_keep


def library_moments(traj, dx: float, dt: float, region: str = "interior", split=None) -> LibraryMoments:
    """Second moments of the candidate library over a device trajectory ``[N, 2, H, W]`` or frame-major ``[N, B, 2, H, W]``
    (float32 or float64; the ``[2, H, W]`` block of a frame contiguous, any frame / sample stride: nothing is copied).
    Rows are the points of frames 0 .. N-3; ``split`` = None or (seed, keep_fraction, train_fraction)."""
    import torch
    if not isinstance(traj, torch.Tensor) or not traj.is_cuda:
        raise RuntimeError("library_moments: traj must be a tensor on the HIP device (there is no CPU path)")
    if traj.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"library_moments: traj must be float32 or float64, got {traj.dtype}")
    if traj.dim() not in (4, 5):
        raise ValueError(f"library_moments: traj must be [N, 2, H, W] or [N, B, 2, H, W], got {tuple(traj.shape)}")
    batched = traj.dim() == 5
    N, (C, H, W) = traj.shape[0], traj.shape[-3:]
    B = traj.shape[1] if batched else 1
    if C != 2:
        raise ValueError(f"library_moments: traj needs 2 channels (u, v), got {C}")
    if N < 3:
        raise ValueError(f"library_moments: traj needs N >= 3 frames, got N = {N}")
    if H < 5 or W < 5:
        raise ValueError(f"library_moments: traj needs H, W >= 5, got H = {H}, W = {W}")
    if not 1 <= B <= 65535:
        raise ValueError(f"library_moments: traj batch B must be 1 .. 65535, got {B}")
    if region not in REGIONS:
        raise ValueError(f"library_moments: region must be 'interior' or 'periodic', got {region!r}")
    if traj.stride()[-3:] != (H * W, W, 1):
        raise ValueError("library_moments: traj must have contiguous [2, H, W] frames (stride-1 inner dims)")
    if traj.stride(0) < 0 or (batched and traj.stride(1) < 0):
        raise ValueError("library_moments: traj must not have negative strides")
    seed, t_train, t_keep = split_thresholds(split)
    L = _lib.lib()
    dev = traj.device
    lead = (B,) if batched else ()
    G = torch.empty(lead + (2, 70, 70), dtype=torch.float64, device=dev)
    b = torch.empty(lead + (2, 70, 2), dtype=torch.float64, device=dev)
    yy = torch.empty(lead + (2, 2), dtype=torch.float64, device=dev)
    n = torch.empty(lead + (2,), dtype=torch.float64, device=dev)
    shape = _lib.shape_arg((H, W))
    ws_bytes = L.percnn_pi_library_moments_workspace_bytes(shape, int(N), int(B))
    if ws_bytes == 0:
        raise ValueError(f"library_moments: traj of {N} frames of {H} x {W} is beyond the 32-bit row index (N*H*W <= 2^32)")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    fn = L.percnn_pi_library_moments_f32 if traj.dtype == torch.float32 else L.percnn_pi_library_moments_f64
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream()
        rc = fn(traj.data_ptr(), traj.stride(0), traj.stride(1) if batched else 0, shape, int(N), int(B), float(dx), float(dt),
                REGIONS[region], seed, t_train, t_keep, G.data_ptr(), b.data_ptr(), yy.data_ptr(), n.data_ptr(), ws.data_ptr(),
                ws_bytes, ctypes.c_void_p(st.cuda_stream))
    _lib.check(rc, "library_moments")
    ws.record_stream(st)
    return LibraryMoments(G, b, yy, n)


# ---- sequential-threshold ridge regression on the normal equations (host, float64) ----------------------------------------
def _solve(G, b):
    """minimum-norm least-squares solution of G w = b: what lstsq(X, y) returns, from X^T X and X^T y"""
    if G.shape[0] == 0:
        return np.zeros(0)
    return np.linalg.lstsq(G, b, rcond=None)[0]


def stridge(G, b, lam: float, maxit: int, tol: float, must_have: int):
    """``STRidgeTrainer.STRidge`` (PDE_FIND_u.py:110-182) for already normalised columns, on ``G = X^T X`` [d, d] and
    ``b = X^T y`` [d]: ridge estimate, then repeatedly drop |w| < tol (``must_have`` always stays) and re-solve on the rest,
    then an unregularised least-squares fit on the final support.  Columns with a zero diagonal never enter."""
    G, b = np.asarray(G, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(-1)
    d = G.shape[0]
    alive = np.flatnonzero(np.diag(G) > 0)

    def ridge(idx):
        if lam != 0:
            return _solve(G[np.ix_(idx, idx)] + lam * np.eye(len(idx)), b[idx])
        return _solve(G[np.ix_(idx, idx)], b[idx])

    w = np.zeros(d)
    w[alive] = ridge(alive)
    num_relevant = len(alive)
    big = np.array([i for i in alive if abs(w[i]) > tol], dtype=int)
    for _ in range(maxit):
        keep = [i for i in alive if not abs(w[i]) < tol]
        if must_have not in keep:
            keep = sorted(keep + [must_have])
        if num_relevant == len(keep):                   # nothing changed
            break
        num_relevant = len(keep)
        big = np.array(keep, dtype=int)
        small = np.ones(d, dtype=bool)
        small[big] = False
        w[small] = 0.0
        w[big] = ridge(big)
    if len(big):
        w[big] = _solve(G[np.ix_(big, big)], b[big])
    return w


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def train_stridge(moments, species, *, maxit: int, str_iters: int, lam: float, d_tol: float, kappa: float, must_have: int,
                  normalize: int = 2):
    """``STRidgeTrainer.__init__`` + ``.train`` (PDE_FIND_u.py:9-108) on the moments of one trajectory: columns scaled to unit
    2-norm over ALL kept rows (the reference normalises before it splits), least-squares baseline on the training class, the
    tolerance search with its shrinking ``d_tol`` scored on the test class with ``l0_penalty = kappa * baseline error``, result
    un-normalised.  Returns the 70 coefficients (zeros off the support)."""
    if normalize != 2:
        raise ValueError("train_stridge: normalize must be 2 (unit 2-norm columns, the reference's setting)")
    s = {"u": 0, "v": 1}.get(species, species)
    if s not in (0, 1):
        raise ValueError(f"train_stridge: species must be 'u', 'v', 0 or 1, got {species!r}")
    G, b, yy, n = (np.asarray(_np(t), dtype=np.float64) for t in moments)
    if G.shape != (2, 70, 70):
        raise ValueError(f"train_stridge: moments of one trajectory expected (G of shape [2, 70, 70]), got {G.shape}")
    if n[0] < 1 or n[1] < 1:
        raise ValueError("train_stridge: the split left the training or the test class empty; pass split=(seed, keep, train) with "
                         "0 < train < 1 to library_moments")
    col = np.diag(G[0]) + np.diag(G[1])
    scale = np.where(col > 0, 1.0 / np.sqrt(np.where(col > 0, col, 1.0)), 0.0)        # Mreg; a zero column is excluded
    Gn = G * scale[None, :, None] * scale[None, None, :]
    bn = b[:, :, s] * scale[None, :]
    # test error (yy - 2 w^T b + w^T G w) / n as |Q (w, -1)|^2 / n with Q^T Q = [[G, b], [b^T, yy]] of the test class (y scaled
    # to unit norm like the columns): every term is a square, so an exact fit gives a small non-negative number instead of the
    # difference of large ones
    ys = 1.0 / np.sqrt(yy[1, s]) if yy[1, s] > 0 else 1.0
    M = np.empty((71, 71))
    M[:70, :70], M[:70, 70], M[70, :70], M[70, 70] = Gn[1], bn[1] * ys, bn[1] * ys, yy[1, s] * ys * ys
    lam_, V = np.linalg.eigh(M)
    Q = np.sqrt(np.maximum(lam_, 0.0))[:, None] * V.T

    def test_error(w):                                  # Theta_n w - y = [Theta_n, ys y] (w, -1/ys)
        z = Q @ np.concatenate([w, [-1.0 / ys]])
        return float(z @ z) / n[1]

    tol = float(d_tol)
    w_best = np.zeros(70)
    alive = np.flatnonzero(col > 0)
    w_best[alive] = _solve(Gn[0][np.ix_(alive, alive)], bn[0][alive])
    err_f = test_error(w_best)
    l0_penalty = kappa * err_f
    err_best = err_f + l0_penalty * np.count_nonzero(w_best)
    for it in range(maxit):
        w = stridge(Gn[0], bn[0], lam, str_iters, tol, must_have)
        err = test_error(w) + l0_penalty * np.count_nonzero(w)
        if err <= err_best:
            err_best, w_best = err, w
            tol = tol + d_tol
        else:
            tol = max(0.0, tol - 2 * d_tol)
            d_tol = 2 * d_tol / (maxit - it)
            tol = tol + d_tol
    return scale * w_best


def discover(traj, dx: float, dt: float, region: str = "interior", split=REFERENCE_SPLIT, u: dict | None = None,
             v: dict | None = None):
    """Device trajectory -> ``{"u": {term: coefficient}, "v": {...}}`` with the reference's settings (``DEFAULTS``; ``u`` /
    ``v`` override single settings).  A batched trajectory gives a list with one such dict per sample."""
    m = library_moments(traj, dx, dt, region=region, split=split)
    host = LibraryMoments(*(_np(t) for t in m))
    samples = [host] if host.G.ndim == 3 else [LibraryMoments(*(t[i] for t in host)) for i in range(host.G.shape[0])]
    out = []
    for mom in samples:
        eqs = {}
        for sp, over in (("u", u), ("v", v)):
            w = train_stridge(mom, sp, **{**DEFAULTS[sp], **(over or {})})
            eqs[sp] = {t: float(c) for t, c in zip(LIBRARY_TERMS, w) if c != 0}
        out.append(eqs)
    return out[0] if host.G.ndim == 3 else out
