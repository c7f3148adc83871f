"""No GPU: the Runge-Kutta restatements (library_rk4_util.py) against the reference-derived forward_rk4 vectors of the Stage-3
goldens, their order of convergence, the ``integrator=`` plumbing of ``LibraryCell``, and what the percnn_pi_lib_rk4_* entry
points of include/percnn_pi_library_cell.h refuse before anything is launched (refused calls only: made-up pointers)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import library_cell_util as U
import library_rk4_util as R


@pytest.mark.parametrize("name", U.GOLDENS)
def test_restatements_match_the_reference_rk4_vectors(name):
    """the project's Stage-3 bars: frames 1e-13, loss 1e-13, scalar gradients 1e-9 relative, dL/dh0 1e-11"""
    z = np.load(os.path.join(U.GOLDEN, name))
    C, pos = U.golden_coefficients(z)
    steps, dx, dt = int(z["rk4_steps"]), float(z["dx"]), float(z["dt"])
    h0 = z["h0"][0]
    traj = R.np_rk4_rollout(h0, C, dx, dt, steps)
    for t in (1, steps):
        err = U.rel_l2(traj[t], z[f"rk4/{t}"][0])
        print(name, "frame", t, err)
        assert err < 1e-13, t
    assert abs((traj[steps] ** 2).mean() - float(z["rk4_loss_meansq"])) < 1e-13
    # the torch restatement walks the same trajectory, and its autograd gives the reference's gradients
    h = torch.tensor(h0)
    for t in range(steps):
        h = R.torch_rk4_step(h, torch.tensor(C), dx, dt)
        assert U.rel_l2(h.numpy(), traj[t + 1]) < 1e-14, t
    assert U.rel_l2(h.numpy(), z[f"rk4/{steps}"][0]) < 1e-13
    assert abs(float((h ** 2).mean()) - float(z["rk4_loss_meansq"])) < 1e-13
    w = [None] * steps + [2 * traj[steps] / traj[steps].size]
    g_h0, gC, _ = R.torch_rk4_rollout_grads(h0, C, dx, dt, steps, w)
    for n, p in pos.items():
        ref = float(z["rk4_grad_meansq/" + n])
        print(name, n, gC[p], ref, abs(gC[p] - ref) / abs(ref))
        assert abs(gC[p] - ref) <= 1e-9 * abs(ref), (n, gC[p], ref)
    assert U.rel_l2(g_h0, z["rk4_grad_meansq_h0"][0]) < 1e-11


def test_order_of_convergence_of_the_restatement():
    """halving the step divides the error of a fourth-order method by 16 and of a first-order method by 2"""
    C, h0 = U.coefficients(R.LOOP), R.loop_state()
    rk4 = R.convergence_ratio(lambda n: R.np_rk4_rollout(h0, C, R.LOOP_DX, R.LOOP_TIME / n, n)[n])
    euler = R.convergence_ratio(lambda n: U.np_rollout(h0, C, R.LOOP_DX, R.LOOP_TIME / n, n)[n])
    print("rk4", rk4, "euler", euler)
    assert 15.0 <= rk4 <= 18.5
    assert 1.9 <= euler <= 2.2


def test_integrator_plumbing():
    import percnn_amd as pa
    eqs = {"u": {"ones*lap_u": 0.05, "v*u_x": -0.7}, "v": {"ones*lap_v": 0.04, "u**2*v*ones": -0.3}}
    keys = list(pa.LibraryCell(U.coefficients(eqs), 0.2, 1e-3).state_dict())
    assert keys == ["coef", "support"]
    assert pa.LibraryCell(U.coefficients(eqs), 0.2, 1e-3).integrator == "euler"
    assert pa.LibraryCell.from_equations(eqs, 0.2, 1e-3).integrator == "euler"
    assert pa.LibraryCell.from_cell(pa.Stage3BurgersCell()).integrator == "euler"
    for cell in (pa.LibraryCell(U.coefficients(eqs), 0.2, 1e-3, integrator="rk4"),
                 pa.LibraryCell.from_equations(eqs, 0.2, 1e-3, integrator="rk4"),
                 pa.LibraryCell.from_equations(eqs, 0.2, 1e-3, support="dense", integrator="rk4")):
        assert cell.integrator == "rk4" and list(cell.state_dict()) == keys and cell.equations() == eqs
    for stage3 in (pa.Stage3BurgersCell(), pa.Stage3LambdaOmegaCell()):
        cell = pa.LibraryCell.from_cell(stage3, integrator="rk4")
        euler = pa.LibraryCell.from_cell(stage3)
        assert cell.integrator == "rk4" and list(cell.state_dict()) == keys
        assert torch.equal(cell.coef, euler.coef) and torch.equal(cell.support, euler.support)
        assert (cell.dx, cell.dt) == (stage3.dx, stage3.dt)
    assert callable(pa.LibraryCell.forward_rk4)
    for make in (lambda bad: pa.LibraryCell(U.coefficients(eqs), 0.2, 1e-3, integrator=bad),
                 lambda bad: pa.LibraryCell.from_equations(eqs, 0.2, 1e-3, integrator=bad),
                 lambda bad: pa.LibraryCell.from_cell(pa.Stage3BurgersCell(), integrator=bad)):
        for bad in ("RK4", "heun", None):
            with pytest.raises(ValueError, match="integrator"):
                make(bad)


NAMES = ("percnn_pi_lib_rk4_step_fwd_f64", "percnn_pi_lib_rk4_rollout_fwd_f64", "percnn_pi_lib_rk4_rollout_bwd_workspace_bytes",
         "percnn_pi_lib_rk4_rollout_bwd_f64")


def test_the_rk4_entry_points_are_registered():
    from percnn_amd import _lib
    header = open(os.path.join(os.path.dirname(U.GOLDEN), os.pardir, "include", "percnn_pi_library_cell.h")).read()
    for name in NAMES:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 3 and _lib.lib().percnn_pi_abi_version() == 3
    assert "pi_lib.h" in _lib.SOURCES["pi_lib_abi.hip"]
    assert any(d.endswith("percnn_pi_library_cell.h") for d in _lib.SOURCES["pi_lib_abi.hip"])


# ---- refusals of the C ABI: the table of test_library_cell_cpu.py on the Runge-Kutta entry points -----------------------------------
EINVAL, EWORKSPACE = -1, -2
SIG = {"step_fwd": "h out coef shape dx dt stream",
       "rollout_fwd": "traj coef shape T dx dt stream",
       "rollout_bwd": "traj g_traj mask g_h0 g_coef ws ws_bytes coef shape T dx dt stream"}


def shape(h, w):
    return (ctypes.c_int64 * 2)(h, w)


# an 8 x 8 state has 1 KiB, a 6-frame trajectory 6 KiB, the backward's workspace 8 KiB: the made-up buffers lie 64 KiB apart.
# In order except for its workspace of 16 bytes, which is what an accepted rollout_bwd call answers with
BASE = dict(h=0x100000, out=0x110000, coef=0x120000, traj=0x130000, g_traj=0x140000, g_h0=0x150000, g_coef=0x160000, ws=0x170000,
            ws_bytes=16, mask=None, shape=shape(8, 8), T=5, dx=0.2, dt=1e-3, stream=None)
ROOMY = dict(ws_bytes=1 << 30)
BAD_SIZES = (0.0, -0.1, float("nan"), float("inf"))
NEED = (7 * 2 * 64 + 140) * 8                             # the header's formula at 8 x 8


def rows():
    r = []
    for entry in SIG:
        for ptr in ("h", "out", "coef", "traj", "g_traj", "g_h0", "g_coef"):
            if ptr in SIG[entry].split():
                r.append((entry, {ptr: None}, EINVAL))
                r.append((entry, {ptr: None, "ws": None}, EINVAL))       # a missing pointer comes before the workspace
        r.append((entry, dict(shape=None), EINVAL))
        for hw in ((4, 8), (8, 4), (0, 8), (-8, 8), (8, (1 << 20) + 1), (1 << 16, 1 << 16)):
            r.append((entry, dict(shape=shape(*hw)), EINVAL))
            r.append((entry, dict(shape=shape(*hw), dx=0.0, ws=None), EINVAL))
        for bad in BAD_SIZES:
            r.append((entry, dict(dx=bad), EINVAL))
            r.append((entry, dict(dt=bad, ws=None), EINVAL))
    for entry in ("rollout_fwd", "rollout_bwd"):
        r.append((entry, dict(T=-1), EINVAL))
        r.append((entry, dict(T=-1, ws=None), EINVAL))
    # outputs on inputs
    r.append(("step_fwd", dict(out=BASE["h"]), EINVAL))
    r.append(("step_fwd", dict(out=BASE["h"] + 1016), EINVAL))           # the last double of h
    r.append(("step_fwd", dict(out=BASE["coef"]), EINVAL))
    r.append(("rollout_fwd", dict(traj=BASE["coef"] - 8), EINVAL))
    for out, nbytes in (("g_h0", 1024), ("g_coef", 1120)):
        for other, last in (("traj", 6 * 1024 - 8), ("g_traj", 6 * 1024 - 8), ("coef", 1112)):
            r.append(("rollout_bwd", {out: BASE[other]}, EINVAL))
            r.append(("rollout_bwd", {out: BASE[other] + last, "ws": None}, EINVAL))      # the alias first, then the workspace
            r.append(("rollout_bwd", {out: BASE[other] - nbytes + 8}, EINVAL))
            r.append(("rollout_bwd", {out: BASE[other] - nbytes}, EWORKSPACE))            # adjacent is in order
    r.append(("rollout_bwd", dict(g_h0=BASE["g_coef"]), EINVAL))
    # the workspace: too small (BASE), missing, misaligned, one byte short, the Euler call's size; a roomy one on the trajectory
    r.append(("rollout_bwd", dict(), EWORKSPACE))
    r.append(("rollout_bwd", dict(T=0), EWORKSPACE))
    r.append(("rollout_bwd", dict(mask=b"\x01\x00\x00\x00\x00\x01"), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws=None, **ROOMY), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws=BASE["ws"] + 4, **ROOMY), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws_bytes=NEED - 1), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws_bytes=(2 * 2 * 64 + 140) * 8), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws=BASE["traj"] - 8, ws_bytes=NEED), EINVAL))
    r.append(("rollout_bwd", dict(ws=BASE["g_h0"], ws_bytes=NEED), EINVAL))
    r.append(("rollout_bwd", dict(ws=BASE["g_h0"] - NEED + 8, ws_bytes=NEED), EINVAL))     # its last double on g_h0
    return r


def test_rk4_entry_points_refuse_before_any_launch():
    import percnn_amd
    L = percnn_amd.lib()
    table = rows()
    assert len(table) > 100 and {e for e, _, _ in table} == set(SIG)
    bad = []
    for entry, over, want in table:
        args = dict(BASE, **over)
        got = getattr(L, f"percnn_pi_lib_rk4_{entry}_f64")(*[args[k] for k in SIG[entry].split()])
        if got != want:
            bad.append((entry, {k: (v if isinstance(v, (int, float, bytes, type(None))) else list(v)) for k, v in over.items()},
                        "want", want, "got", got))
    assert not bad, "\n".join(map(str, bad))


def test_rk4_workspace_bytes():
    import percnn_amd
    f = percnn_amd.lib().percnn_pi_lib_rk4_rollout_bwd_workspace_bytes
    for (h, w), tiles in (((8, 8), 1), ((5, 5), 1), ((16, 17), 2), ((33, 100), 21), ((100, 100), 49)):
        for T in (0, 1, 200):
            assert f(shape(h, w), T) == (7 * 2 * h * w + tiles * 140) * 8, (h, w, T)
    assert f(None, 3) == 0 and f(shape(4, 8), 3) == 0 and f(shape(8, 8), -1) == 0
