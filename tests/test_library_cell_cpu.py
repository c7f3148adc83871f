"""No GPU: the library cell's restatements (library_cell_util.py) against the reference-derived Stage-3 goldens, the
equation <-> coefficient plumbing of ``LibraryCell``, and what the C ABI of include/percnn_pi_library_cell.h refuses before
anything is launched (refused calls only: the pointers are made-up numbers)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import library_cell_util as U


@pytest.mark.parametrize("name", U.GOLDENS)
def test_restatements_match_the_reference_goldens(name):
    """the bars of the existing Stage-3 tests (test_hip_parity.py): frames 1e-13, loss 1e-13, scalar gradients 1e-9 relative,
    dL/dh0 1e-11"""
    z = np.load(os.path.join(U.GOLDEN, name))
    C, pos = U.golden_coefficients(z)
    steps, dx, dt = int(z["steps"]), float(z["dx"]), float(z["dt"])
    h0 = z["h0"][0]
    traj = U.np_rollout(h0, C, dx, dt, steps)
    for t in z["keep_t"]:
        assert U.rel_l2(traj[int(t)], z[f"traj/{int(t)}"]) < 1e-13, int(t)
    assert abs((traj ** 2).mean() - float(z["loss_meansq"])) < 1e-13
    # the torch restatement walks the same trajectory, and its autograd gives the reference's gradients
    h = torch.tensor(h0)
    for t in range(steps):
        h = U.torch_step(h, torch.tensor(C), dx, dt)
        assert U.rel_l2(h.numpy(), traj[t + 1]) < 1e-14, t
    g_h0, gC, _ = U.torch_rollout_grads(h0, C, dx, dt, steps, [2 * traj[t] / traj.size for t in range(steps + 1)])
    for n, p in pos.items():
        ref = float(z["grad_meansq/" + n])
        assert abs(gC[p] - ref) <= 1e-9 * max(abs(ref), 1e-6), (n, gC[p], ref)
    assert U.rel_l2(g_h0, z["grad_meansq_h0"][0]) < 1e-11


def test_equations_round_trip():
    import percnn_amd as pa
    assert U.TERMS == pa.LIBRARY_TERMS
    eqs = {"u": {"ones*lap_u": 0.05, "v*u_x": -0.7, "u*v*v_y": 0.5, "u*lap_v": 0.02},
           "v": {"ones*ones": 0.25, "ones*lap_v": 0.04, "u**2*v*ones": -0.3, "v**3*lap_v": 1e-3}}
    cell = pa.LibraryCell.from_equations(eqs, 0.2, 1e-3)
    assert isinstance(cell, torch.nn.Module) and [n for n, _ in cell.named_parameters()] == ["coef"]
    assert cell.coef.shape == (2, 10, 7) and cell.coef.dtype == torch.float64 and cell.support.shape == (2, 10, 7)
    assert np.array_equal(cell.coef.detach().numpy(), U.coefficients(eqs))
    assert torch.equal(cell.support, (cell.coef != 0).to(torch.float64)) and int(cell.support.sum()) == 8
    got = cell.equations()
    assert got == eqs and [list(got[s]) for s in "uv"] == [sorted(eqs[s], key=U.TERMS.index) for s in "uv"]
    assert float(cell.coef.detach()[U.position("u", "u*v*v_y")]) == 0.5 and U.position("u", "u*v*v_y") == (0, 4, 4)
    dense = pa.LibraryCell(U.coefficients(eqs), 0.2, 1e-3, support="dense")
    assert int(dense.support.sum()) == 140 and dense.equations() == eqs
    # an entry off the support does not reach the block, whatever the parameter holds
    with torch.no_grad():
        cell.coef[0, 9, 3] = 7.0
    assert cell.equations() == eqs and float(cell.param_block().detach()[0, 9, 3]) == 0.0
    with pytest.raises(ValueError, match=r"u\*u_z"):
        pa.LibraryCell.from_equations({"u": {"u*u_z": 1.0}, "v": {}}, 0.2, 1e-3)
    with pytest.raises(ValueError, match="eqs"):
        pa.LibraryCell.from_equations([eqs], 0.2, 1e-3)
    with pytest.raises(ValueError, match="coefficients"):
        pa.LibraryCell(np.zeros((2, 70)), 0.2, 1e-3)
    with pytest.raises(ValueError, match="support"):
        pa.LibraryCell(np.zeros((2, 10, 7)), 0.2, 1e-3, support="all")
    with pytest.raises(ValueError, match="dx"):
        pa.LibraryCell(np.zeros((2, 10, 7)), 0.0, 1e-3)


@pytest.mark.parametrize("name", ["bur3_stage3_24x40.npz", "lo3_stage3_24x40.npz"])
def test_from_cell_has_the_stage3_cells_right_hand_side(name):
    import percnn_amd as pa
    z = np.load(os.path.join(U.GOLDEN, name))
    stage3 = pa.Stage3BurgersCell() if name.startswith("bur") else pa.Stage3LambdaOmegaCell()
    stage3.load_state_dict({k[6:]: torch.tensor(z[k]) for k in z.files if k.startswith("param/")})
    cell = pa.LibraryCell.from_cell(stage3)
    C, pos = U.golden_coefficients(z)
    assert np.array_equal(cell.coef.detach().numpy(), C) and (cell.dx, cell.dt) == (stage3.dx, stage3.dt)
    assert sorted(map(tuple, np.argwhere(cell.support.numpy() != 0))) == sorted(pos.values())
    h = torch.tensor(z["h0"])
    u, v = h[:, 0:1], h[:, 1:2]
    with torch.no_grad():
        for got, ref in zip(cell.f_rhs(u, v), stage3.f_rhs(u, v)):
            assert got.shape == ref.shape and U.rel_l2(got.numpy(), ref.numpy()) <= 1e-14
    # f_rhs is the restatement's right-hand side
    nxt = U.np_step(z["h0"][0], C, cell.dx, cell.dt)
    with torch.no_grad():
        fu, fv = cell.f_rhs(h[0, 0], h[0, 1])
    assert U.rel_l2(np.stack([fu.numpy(), fv.numpy()]) * cell.dt, nxt - z["h0"][0]) < 1e-12
    with pytest.raises(TypeError, match="cell"):
        pa.LibraryCell.from_cell(pa.lo2d_cell())


def test_the_library_cell_is_registered():
    from percnn_amd import _lib
    assert "pi_lib_abi.hip" in _lib.SOURCES and "pi_lib.h" in _lib.SOURCES["pi_lib_abi.hip"]
    for name in ("percnn_pi_lib_step_fwd_f64", "percnn_pi_lib_rollout_fwd_f64", "percnn_pi_lib_rollout_bwd_workspace_bytes",
                 "percnn_pi_lib_rollout_bwd_f64"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 3


# ---- refusals of the C ABI ---------------------------------------------------------------------------------------------------
EINVAL, EWORKSPACE = -1, -2
SIG = {"step_fwd": "h out coef shape dx dt stream",
       "rollout_fwd": "traj coef shape T dx dt stream",
       "rollout_bwd": "traj g_traj mask g_h0 g_coef ws ws_bytes coef shape T dx dt stream"}


def shape(h, w):
    return (ctypes.c_int64 * 2)(h, w)


# an 8 x 8 state has 1 KiB, a 6-frame trajectory 6 KiB: the made-up buffers lie 64 KiB apart.  In order except for its
# workspace of 16 bytes, which is what an accepted rollout_bwd call answers with
BASE = dict(h=0x100000, out=0x110000, coef=0x120000, traj=0x130000, g_traj=0x140000, g_h0=0x150000, g_coef=0x160000, ws=0x170000,
            ws_bytes=16, mask=None, shape=shape(8, 8), T=5, dx=0.2, dt=1e-3, stream=None)
ROOMY = dict(ws_bytes=1 << 30)
BAD_SIZES = (0.0, -0.1, float("nan"), float("inf"))


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
    # the workspace: too small (BASE), missing, misaligned, one byte short; a roomy one that lies on the trajectory
    need = (2 * 2 * 64 + 140) * 8
    r.append(("rollout_bwd", dict(), EWORKSPACE))
    r.append(("rollout_bwd", dict(T=0), EWORKSPACE))
    r.append(("rollout_bwd", dict(mask=b"\x01\x00\x00\x00\x00\x01"), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws=None, **ROOMY), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws=BASE["ws"] + 4, **ROOMY), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws_bytes=need - 1), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws=BASE["traj"] - 8, ws_bytes=need), EINVAL))
    r.append(("rollout_bwd", dict(ws=BASE["g_h0"], ws_bytes=need), EINVAL))
    return r


def test_library_cell_entry_points_refuse_before_any_launch():
    import percnn_amd
    L = percnn_amd.lib()
    table = rows()
    assert len(table) > 100 and {e for e, _, _ in table} == set(SIG)
    bad = []
    for entry, over, want in table:
        args = dict(BASE, **over)
        got = getattr(L, f"percnn_pi_lib_{entry}_f64")(*[args[k] for k in SIG[entry].split()])
        if got != want:
            bad.append((entry, {k: (v if isinstance(v, (int, float, bytes, type(None))) else list(v)) for k, v in over.items()},
                        "want", want, "got", got))
    assert not bad, "\n".join(map(str, bad))


def test_workspace_bytes():
    import percnn_amd
    f = percnn_amd.lib().percnn_pi_lib_rollout_bwd_workspace_bytes
    for (h, w), tiles in (((8, 8), 1), ((5, 5), 1), ((16, 17), 2), ((33, 100), 21), ((100, 100), 49)):
        for T in (0, 1, 200):
            assert f(shape(h, w), T) == (2 * 2 * h * w + tiles * 140) * 8, (h, w, T)
    assert f(None, 3) == 0 and f(shape(4, 8), 3) == 0 and f(shape(8, 8), -1) == 0
