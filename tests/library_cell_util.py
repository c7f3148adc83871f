"""Shared by test_library_cell_cpu.py / test_library_cell_gpu.py: the library cell's explicit Euler step restated twice from
include/percnn_pi_library_cell.h -- in numpy float64 in the pinned operation order (the forward kernels must give the same
bits) and on torch float64 CPU tensors (for autograd) -- plus the coefficient sets and states the tests use."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ["bur3_stage3_32x32.npz", "bur3_stage3_24x40.npz", "lo3_stage3_32x32.npz", "lo3_stage3_24x40.npz"]
A = ["ones", "u", "v", "u**2", "u*v", "v**2", "u**3", "u**2*v", "u*v**2", "v**3"]
B = ["ones", "u_x", "u_y", "v_x", "v_y", "lap_u", "lap_v"]
TERMS = [a + "*" + b for a in A for b in B]

# parameter name of the Stage-3 cells -> (species, library term)
BURGERS_TERMS = {"nu_u": ("u", "ones*lap_u"), "C1_u": ("u", "u*u_x"), "C2_u": ("u", "v*u_y"),
                 "nu_v": ("v", "ones*lap_v"), "C1_v": ("v", "u*v_x"), "C2_v": ("v", "v*v_y")}
LO_TERMS = {"nu_u": ("u", "ones*lap_u"), "C1_u": ("u", "u*ones"), "C2_u": ("u", "u**3*ones"), "C3_u": ("u", "u**2*v*ones"),
            "C4_u": ("u", "u*v**2*ones"), "C5_u": ("u", "v**3*ones"),
            "nu_v": ("v", "ones*lap_v"), "C1_v": ("v", "v*ones"), "C2_v": ("v", "u**3*ones"), "C3_v": ("v", "u**2*v*ones"),
            "C4_v": ("v", "u*v**2*ones"), "C5_v": ("v", "v**3*ones"), "C6_v": ("v", "u*ones")}


def position(species, term):
    """index into coef [2,10,7]"""
    i = TERMS.index(term)
    return "uv".index(species), i // 7, i % 7


def coefficients(eqs):
    C = np.zeros((2, 10, 7))
    for sp, terms in eqs.items():
        for t, c in terms.items():
            C[position(sp, t)] = c
    return C


def golden_coefficients(z):
    """[2,10,7] of a Stage-3 golden's parameters, and the name -> position table"""
    table = BURGERS_TERMS if "param/C3_u" not in z.files else LO_TERMS
    C = np.zeros((2, 10, 7))
    for name, (sp, t) in table.items():
        C[position(sp, t)] = float(z["param/" + name])
    return C, {n: position(sp, t) for n, (sp, t) in table.items()}


# ---- numpy, the pinned order ------------------------------------------------------------------------------------------------
def _np_fields(f, inv_12dx, inv_dx2):
    a2, a1, b1, b2 = np.roll(f, 2, 0), np.roll(f, 1, 0), np.roll(f, -1, 0), np.roll(f, -2, 0)
    l2, l1, r1, r2 = np.roll(f, 2, 1), np.roll(f, 1, 1), np.roll(f, -1, 1), np.roll(f, -2, 1)
    d0 = ((a2 - b2) + 8.0 * (b1 - a1)) * inv_12dx
    d1 = ((l2 - r2) + 8.0 * (r1 - l1)) * inv_12dx
    lap = ((-1.0 / 12.0) * ((a2 + b2) + (l2 + r2)) + (4.0 / 3.0) * ((a1 + b1) + (l1 + r1)) - 5.0 * f) * inv_dx2
    return d0, d1, lap


def np_library(h, dx):
    """phi [10], psi [7] of a state [2,H,W]"""
    u, v = h[0], h[1]
    inv_12dx, inv_dx2 = 1.0 / (12.0 * dx), 1.0 / (dx * dx)
    ux, uy, lu = _np_fields(u, inv_12dx, inv_dx2)
    vx, vy, lv = _np_fields(v, inv_12dx, inv_dx2)
    u2, uv, v2 = u * u, u * v, v * v
    phi = [np.ones_like(u), u, v, u2, uv, v2, u2 * u, u2 * v, u * v2, v2 * v]
    psi = [np.ones_like(u), ux, uy, vx, vy, lu, lv]
    return phi, psi


def np_step(h, C, dx, dt):
    phi, psi = np_library(h, dx)
    out = np.empty_like(h)
    for s in range(2):
        rhs = np.zeros_like(h[s])
        for k in range(7):
            if not (C[s, :, k] != 0).any():
                continue                                    # the kernels skip such a column
            q = C[s, 0, k] * phi[0]
            for m in range(1, 10):
                q = q + C[s, m, k] * phi[m]
            rhs = rhs + psi[k] * q
        inc = dt * rhs
        out[s] = h[s] + inc
    return out


def np_rollout(h0, C, dx, dt, steps):
    """h0 [2,H,W] -> [steps+1,2,H,W]"""
    traj = np.empty((steps + 1,) + h0.shape)
    traj[0] = h0
    for t in range(steps):
        traj[t + 1] = np_step(traj[t], C, dx, dt)
    return traj


# ---- torch float64 on the CPU, for autograd ------------------------------------------------------------------------------------
def torch_library(h, dx):
    u, v = h[0], h[1]

    def fields(f):
        a2, a1, b1, b2 = torch.roll(f, 2, 0), torch.roll(f, 1, 0), torch.roll(f, -1, 0), torch.roll(f, -2, 0)
        l2, l1, r1, r2 = torch.roll(f, 2, 1), torch.roll(f, 1, 1), torch.roll(f, -1, 1), torch.roll(f, -2, 1)
        d0 = ((a2 - b2) + 8.0 * (b1 - a1)) * (1.0 / (12.0 * dx))
        d1 = ((l2 - r2) + 8.0 * (r1 - l1)) * (1.0 / (12.0 * dx))
        lap = ((-1.0 / 12.0) * ((a2 + b2) + (l2 + r2)) + (4.0 / 3.0) * ((a1 + b1) + (l1 + r1)) - 5.0 * f) * (1.0 / (dx * dx))
        return d0, d1, lap

    ux, uy, lu = fields(u)
    vx, vy, lv = fields(v)
    u2, uv, v2 = u * u, u * v, v * v
    phi = torch.stack([torch.ones_like(u), u, v, u2, uv, v2, u2 * u, u2 * v, u * v2, v2 * v])
    psi = torch.stack([torch.ones_like(u), ux, uy, vx, vy, lu, lv])
    return phi, psi


def torch_step(h, C, dx, dt):
    """h [2,H,W], C [2,10,7] -> next state (differentiable in both)"""
    phi, psi = torch_library(h, dx)
    rhs = torch.einsum("smk,mhw,khw->shw", C, phi, psi)
    return h + dt * rhs


def torch_rollout_grads(h0, C, dx, dt, steps, weights):
    """Loss = sum_t sum(weights[t] * frame_t) over the frames with weights[t] is not None.  Returns dL/dh0 [2,H,W],
    dL/dC [2,10,7] and bound [2,10,7] = sum_t sum_p |dt lambda_{t+1,s} phi_m psi_k| with lambda the retained frame gradients:
    the sum of absolute terms each coefficient gradient is a sum of."""
    h = torch.tensor(h0, dtype=torch.float64, requires_grad=True)
    Ct = torch.tensor(C, dtype=torch.float64, requires_grad=True)
    frames = [h]
    for _ in range(steps):
        nxt = torch_step(frames[-1], Ct, dx, dt)
        nxt.retain_grad()
        frames.append(nxt)
    loss = sum((torch.as_tensor(w) * f).sum() for w, f in zip(weights, frames) if w is not None)
    loss.backward()
    bound = torch.zeros(2, 10, 7, dtype=torch.float64)
    with torch.no_grad():
        for t in range(steps):
            phi, psi = torch_library(frames[t], dx)
            a = dt * frames[t + 1].grad
            bound += torch.einsum("shw,mhw,khw->smk", a.abs(), phi.abs(), psi.abs())
    return h.grad.numpy(), Ct.grad.numpy(), bound.numpy()


# ---- what the tests run on --------------------------------------------------------------------------------------------------
SHAPES = [(5, 5), (5, 7), (6, 5), (13, 33), (20, 70), (24, 40), (32, 32)]
STEPS = [1, 2, 7]
DX, DT = 0.2, 1e-4                       # the dense set on white-noise states: max |h| stays below 2.4 over seven steps


@functools.lru_cache(maxsize=None)
def coefficient_set(name):
    if name == "dense":                                     # all 140, |c| ~ 0.1
        return 0.1 * np.random.default_rng(7).standard_normal((2, 10, 7))
    if name == "cross":                                     # terms neither Stage-3 cell can express; column u_y is empty
        return coefficients({"u": {"ones*lap_u": 0.05, "v*u_x": -0.7, "u*v*v_y": 0.5, "u*lap_v": 0.02},
                             "v": {"ones*lap_v": 0.04, "u**2*v*ones": -0.3, "v*ones": 0.4, "u*v_x": -0.6}})
    if name == "columns":                                   # one term per column, u on the even columns and v on the odd
        C = np.zeros((2, 10, 7))
        for k in range(7):
            C[k % 2, (3 * k + 1) % 10, k] = 0.3 - 0.1 * k
        return C
    raise KeyError(name)


SETS = ["dense", "cross", "columns"]


@functools.lru_cache(maxsize=None)
def state(shape):
    H, W = shape
    return 0.5 * np.random.default_rng(100 * H + W).standard_normal((2, H, W))


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))
