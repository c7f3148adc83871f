"""Shared by test_library_rk4_cpu.py / test_library_rk4_gpu.py: the library cell's classical Runge-Kutta step restated twice from
include/percnn_pi_library_cell.h -- in numpy float64 in the pinned operation order (the fused forward kernel must give the same
bits) and on torch float64 CPU tensors (for autograd).  The right-hand side is library_cell_util's, built as its Euler
restatements build it."""
import numpy as np
import torch

import library_cell_util as U

# The forward kernel's tile is 8 x 8 while that makes at most 256 workgroups and 16 x 16 beyond (csrc/pi_lib.h: rk4_tile): one row
# / one column more than a tile of either, and two grids of 17 x 16 eight-wide tiles, the smallest that take the 16 x 16 tile
SHAPES = U.SHAPES + [(9, 17), (17, 9), (17, 33), (33, 17), (136, 121), (121, 136)]


# ---- numpy, the pinned order ------------------------------------------------------------------------------------------------
def np_rhs(h, C, dx):
    """f(h) [2,H,W] exactly as U.np_step sums it (columns without a coefficient skipped)"""
    phi, psi = U.np_library(h, dx)
    out = np.empty_like(h)
    for s in range(2):
        rhs = np.zeros_like(h[s])
        for k in range(7):
            if not (C[s, :, k] != 0).any():
                continue
            q = C[s, 0, k] * phi[0]
            for m in range(1, 10):
                q = q + C[s, m, k] * phi[m]
            rhs = rhs + psi[k] * q
        out[s] = rhs
    return out


def np_rk4_step(h, C, dx, dt):
    k1 = np_rhs(h, C, dx)
    y2 = h + (k1 * dt) / 2.0
    k2 = np_rhs(y2, C, dx)
    y3 = h + (k2 * dt) / 2.0
    k3 = np_rhs(y3, C, dx)
    y4 = h + k3 * dt
    k4 = np_rhs(y4, C, dx)
    s = ((k1 + 2.0 * k2) + 2.0 * k3) + k4
    return h + (dt * s) / 6.0


def np_rk4_rollout(h0, C, dx, dt, steps):
    """h0 [2,H,W] -> [steps+1,2,H,W]"""
    traj = np.empty((steps + 1,) + h0.shape)
    traj[0] = h0
    for t in range(steps):
        traj[t + 1] = np_rk4_step(traj[t], C, dx, dt)
    return traj


# ---- torch float64 on the CPU, for autograd ------------------------------------------------------------------------------------
def torch_rhs(h, C, dx):
    phi, psi = U.torch_library(h, dx)
    return torch.einsum("smk,mhw,khw->shw", C, phi, psi)


def torch_rk4_step(h, C, dx, dt, stages=None):
    """h [2,H,W], C [2,10,7] -> next state (differentiable in both).  ``stages``: a list that receives (y_i, k_i), i = 1 .. 4,
    with the gradient of every k_i retained"""
    ys, ks = [h], []
    for frac in (0.5, 0.5, 1.0, None):
        k = torch_rhs(ys[-1], C, dx)
        ks.append(k)
        if frac is not None:
            ys.append(h + (k * dt) * frac)
    if stages is not None:
        for k in ks:
            k.retain_grad()
        stages.extend(zip(ys, ks))
    s = ((ks[0] + 2.0 * ks[1]) + 2.0 * ks[2]) + ks[3]
    return h + (dt * s) / 6.0


def torch_rk4_rollout_grads(h0, C, dx, dt, steps, weights):
    """Loss = sum_t sum(weights[t] * frame_t) over the frames with weights[t] is not None.  Returns dL/dh0 [2,H,W],
    dL/dC [2,10,7] and bound [2,10,7] = sum_t sum_i sum_p |kappa_{i,s} phi_m(y_i) psi_k(y_i)| with kappa_i = dL/dk_i the retained
    gradients of the stage tensors: the sum of absolute terms each coefficient gradient is a sum of."""
    h = torch.tensor(h0, dtype=torch.float64, requires_grad=True)
    Ct = torch.tensor(C, dtype=torch.float64, requires_grad=True)
    frames, stages = [h], []
    for _ in range(steps):
        frames.append(torch_rk4_step(frames[-1], Ct, dx, dt, stages))
    loss = sum((torch.as_tensor(w) * f).sum() for w, f in zip(weights, frames) if w is not None)
    loss.backward()
    bound = torch.zeros(2, 10, 7, dtype=torch.float64)
    with torch.no_grad():
        for y, k in stages:
            phi, psi = U.torch_library(y, dx)
            bound += torch.einsum("shw,mhw,khw->smk", k.grad.abs(), phi.abs(), psi.abs())
    return h.grad.numpy(), Ct.grad.numpy(), bound.numpy()


# ---- order of convergence: the equation and initial state of test_discover_hands_the_equation_back -------------------------------
LOOP = {"u": {"ones*lap_u": 0.005, "v*u_x": -0.8, "u*u_y": -0.9, "u*v*v_y": 1.5},
        "v": {"ones*lap_v": 0.004, "v*u_y": 0.6, "u*v_x": -1.0, "v*v_y": -0.7}}
LOOP_DX, LOOP_TIME, LOOP_STEPS = 0.01, 0.02, (10, 20, 40)


def loop_state():
    """[2,32,32]"""
    ys = np.arange(32, dtype=np.float64) / 32
    yy, xx = np.meshgrid(ys, ys, indexing="ij")
    tp = 2 * np.pi
    u = np.sin(tp * xx) * np.cos(tp * yy) + 0.3 * np.cos(2 * tp * xx + 0.5)
    v = np.cos(tp * xx) * np.sin(tp * yy) - 0.2 * np.sin(tp * (xx + 2 * yy))
    return np.stack((u, v))


def convergence_ratio(final_state):
    """final_state(n) -> the state at LOOP_TIME after n steps of LOOP_TIME / n;  ||y10 - y20|| / ||y20 - y40||: 2^p for a
    method of order p"""
    y = [np.asarray(final_state(n)) for n in LOOP_STEPS]
    return float(np.linalg.norm(y[0] - y[1]) / np.linalg.norm(y[1] - y[2]))
