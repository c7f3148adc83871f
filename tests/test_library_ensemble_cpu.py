"""No GPU: the eight ensemble entry points of include/percnn_pi_library_cell.h -- registration, what they refuse before anything
is launched (refused calls only: the pointers are made-up numbers), their workspace sizes -- and the plumbing of
``LibraryEnsemble`` on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import library_cell_util as U

PREFIXES = ("percnn_pi_lib_", "percnn_pi_lib_rk4_")
NAMES = [pre + "ensemble_" + n for pre in PREFIXES
         for n in ("step_fwd_f64", "rollout_fwd_f64", "rollout_bwd_workspace_bytes", "rollout_bwd_f64")]


def test_the_ensemble_entry_points_are_registered():
    from percnn_amd import _lib
    assert len(NAMES) == 8
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    assert _lib.ABI_VERSION == 3 and _lib.lib().percnn_pi_abi_version() == 3


# ---- refusals of the C ABI ---------------------------------------------------------------------------------------------------
EINVAL, EWORKSPACE = -1, -2
SIG = {"step_fwd": "h out coef shape B dx dt stream",
       "rollout_fwd": "traj coef shape B T dx dt stream",
       "rollout_bwd": "traj g_traj mask g_h0 g_coef ws ws_bytes coef shape B T dx dt stream"}


def shape(h, w):
    return (ctypes.c_int64 * 2)(h, w)


# B = 3 states of 8 x 8: a state has 3 KiB, a 6-frame trajectory 18 KiB, the coefficients 3360 bytes: the made-up buffers lie
# 64 KiB apart.  In order except for its workspace of 16 bytes, which is what an accepted rollout_bwd call answers with
NB = 3
STATE, COEF = NB * 1024, NB * 1120
BASE = dict(h=0x100000, out=0x110000, coef=0x120000, traj=0x130000, g_traj=0x140000, g_h0=0x150000, g_coef=0x160000, ws=0x170000,
            ws_bytes=16, mask=None, shape=shape(8, 8), B=NB, T=5, dx=0.2, dt=1e-3, stream=None)
ROOMY = dict(ws_bytes=1 << 30)
BAD_SIZES = (0.0, -0.1, float("nan"), float("inf"))
NEED = {"percnn_pi_lib_": NB * (2 * 2 * 64 + 140) * 8, "percnn_pi_lib_rk4_": NB * (7 * 2 * 64 + 140) * 8}


def rows(pre):
    r = []
    for entry in SIG:
        for ptr in ("h", "out", "coef", "traj", "g_traj", "g_h0", "g_coef"):
            if ptr in SIG[entry].split():
                r.append((entry, {ptr: None}, EINVAL))
                r.append((entry, {ptr: None, "ws": None}, EINVAL))       # a missing pointer comes before the workspace
        r.append((entry, dict(shape=None), EINVAL))
        for hw in ((4, 8), (8, 4), (0, 8), (-8, 8), (8, (1 << 20) + 1), (1 << 16, 1 << 16)):
            r.append((entry, dict(shape=shape(*hw)), EINVAL))
        for b in (0, -1, 65536):
            r.append((entry, dict(B=b), EINVAL))
            r.append((entry, dict(B=b, ws=None), EINVAL))                # the sample count comes before the workspace
        for bad in BAD_SIZES:
            r.append((entry, dict(dx=bad), EINVAL))
            r.append((entry, dict(dt=bad, ws=None), EINVAL))
    for entry in ("rollout_fwd", "rollout_bwd"):
        r.append((entry, dict(T=-1), EINVAL))
        r.append((entry, dict(T=-1, ws=None), EINVAL))
    # outputs on inputs, at the B-fold extents: the last double of sample B-1 is still an alias, adjacent is in order
    r.append(("step_fwd", dict(out=BASE["h"]), EINVAL))
    r.append(("step_fwd", dict(out=BASE["h"] + STATE - 8), EINVAL))
    r.append(("step_fwd", dict(out=BASE["h"] - STATE + 8), EINVAL))
    r.append(("step_fwd", dict(out=BASE["coef"] + COEF - 8), EINVAL))
    r.append(("rollout_fwd", dict(traj=BASE["coef"] + COEF - 8), EINVAL))
    r.append(("rollout_fwd", dict(traj=BASE["coef"] - 6 * STATE + 8), EINVAL))
    for out, nbytes in (("g_h0", STATE), ("g_coef", COEF)):
        for other, last in (("traj", 6 * STATE - 8), ("g_traj", 6 * STATE - 8), ("coef", COEF - 8)):
            r.append(("rollout_bwd", {out: BASE[other]}, EINVAL))
            r.append(("rollout_bwd", {out: BASE[other] + last, "ws": None}, EINVAL))      # the alias first, then the workspace
            r.append(("rollout_bwd", {out: BASE[other] - nbytes + 8}, EINVAL))
            r.append(("rollout_bwd", {out: BASE[other] - nbytes}, EWORKSPACE))            # adjacent is in order
            r.append(("rollout_bwd", {out: BASE[other] + last + 8}, EWORKSPACE))
    r.append(("rollout_bwd", dict(g_h0=BASE["g_coef"] + COEF - 8), EINVAL))
    r.append(("rollout_bwd", dict(g_coef=BASE["g_h0"] + STATE - 8), EINVAL))
    # the workspace: too small (BASE), missing, misaligned, one byte short; a roomy one that lies on the trajectory
    need = NEED[pre]
    r.append(("rollout_bwd", dict(), EWORKSPACE))
    r.append(("rollout_bwd", dict(T=0), EWORKSPACE))
    r.append(("rollout_bwd", dict(mask=b"\x01\x00\x00\x00\x00\x01"), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws=None, **ROOMY), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws=BASE["ws"] + 4, **ROOMY), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws_bytes=need - 1), EWORKSPACE))
    r.append(("rollout_bwd", dict(ws_bytes=need // NB), EWORKSPACE))     # the single-trajectory workspace is short
    r.append(("rollout_bwd", dict(ws=BASE["traj"] - 8, ws_bytes=need), EINVAL))
    r.append(("rollout_bwd", dict(ws=BASE["g_h0"] + STATE - 8, ws_bytes=need), EINVAL))
    r.append(("rollout_bwd", dict(ws=BASE["g_coef"] - need + 8, ws_bytes=need), EINVAL))
    return r


@pytest.mark.parametrize("pre", PREFIXES)
def test_ensemble_entry_points_refuse_before_any_launch(pre):
    import percnn_amd
    L = percnn_amd.lib()
    table = rows(pre)
    assert len(table) > 130 and {e for e, _, _ in table} == set(SIG)
    bad = []
    for entry, over, want in table:
        args = dict(BASE, **over)
        got = getattr(L, f"{pre}ensemble_{entry}_f64")(*[args[k] for k in SIG[entry].split()])
        if got != want:
            bad.append((entry, {k: (v if isinstance(v, (int, float, bytes, type(None))) else list(v)) for k, v in over.items()},
                        "want", want, "got", got))
    assert not bad, "\n".join(map(str, bad))


@pytest.mark.parametrize("pre", PREFIXES)
def test_workspace_is_b_single_workspaces(pre):
    import percnn_amd
    L = percnn_amd.lib()
    single, ens = getattr(L, pre + "rollout_bwd_workspace_bytes"), getattr(L, pre + "ensemble_rollout_bwd_workspace_bytes")
    for hw in ((5, 5), (16, 17), (33, 100)):
        for B in (1, 3, 16):
            for T in (0, 1, 200):
                one = single(shape(*hw), T)
                assert one > 0 and ens(shape(*hw), B, T) == B * one, (hw, B, T)
    assert ens(None, 3, 3) == 0 and ens(shape(4, 8), 3, 3) == 0 and ens(shape(8, 8), 3, -1) == 0
    for B in (0, -1, 65536):
        assert ens(shape(8, 8), B, 3) == 0, B
    assert ens(shape(8, 8), 65535, 3) == 65535 * single(shape(8, 8), 3)


# ---- the module on CPU tensors ---------------------------------------------------------------------------------------------------
EQS = [{"u": {"ones*lap_u": 0.05, "v*u_x": -0.7, "u*v*v_y": 0.5, "u*lap_v": 0.02},
        "v": {"ones*ones": 0.25, "ones*lap_v": 0.04, "u**2*v*ones": -0.3, "v**3*lap_v": 1e-3}},
       {"u": {"ones*lap_u": 0.01, "u*u_x": -1.0}, "v": {"v*v_y": -1.0}},
       {"u": {}, "v": {"u*ones": 0.5}}]


def test_from_equations_round_trip_and_state_dict():
    import percnn_amd as pa
    ens = pa.LibraryEnsemble.from_equations(EQS, 0.2, 1e-3, integrator="rk4")
    assert isinstance(ens, torch.nn.Module) and len(ens) == 3 and all(isinstance(c, pa.LibraryCell) for c in ens.cells)
    assert ens.equations() == EQS
    assert (ens.dx, ens.dy, ens.dt, ens.integrator, ens.ndim) == (0.2, 0.2, 1e-3, "rk4", 2)
    assert list(ens.state_dict()) == [f"cells.{i}.{k}" for i in range(3) for k in ("coef", "support")]
    assert [n for n, _ in ens.named_parameters()] == [f"cells.{i}.coef" for i in range(3)]
    P = ens.param_block()
    assert P.shape == (3, 2, 10, 7) and P.dtype == torch.float64 and P.requires_grad
    for b, eqs in enumerate(EQS):
        assert np.array_equal(P[b].detach().numpy(), U.coefficients(eqs))
    # the block is differentiable back to each member, on its own support
    (P * torch.arange(1.0, 4.0, dtype=torch.float64)[:, None, None, None]).sum().backward()
    for b, c in enumerate(ens.cells):
        assert torch.equal(c.coef.grad, (b + 1) * c.support)
    # one cell B times: one parameter, the sum of the sample gradients
    cell = pa.LibraryCell.from_equations(EQS[0], 0.2, 1e-3)
    shared = pa.LibraryEnsemble([cell] * 3)
    assert len(shared) == 3 and [n for n, _ in shared.named_parameters()] == ["cells.0.coef"]
    assert list(shared.state_dict()) == [f"cells.{i}.{k}" for i in range(3) for k in ("coef", "support")]
    shared.param_block().sum().backward()
    assert torch.equal(cell.coef.grad, 3 * cell.support)
    # a state dict loads member by member
    other = pa.LibraryEnsemble.from_equations(EQS[::-1], 0.2, 1e-3, support="dense")
    other.load_state_dict(pa.LibraryEnsemble.from_equations(EQS, 0.2, 1e-3).state_dict())
    assert other.equations() == EQS
    with pytest.raises(ValueError, match="LibraryEnsemble.from_equations.*list"):
        pa.LibraryEnsemble.from_equations(EQS[0], 0.2, 1e-3)
    with pytest.raises(ValueError, match="LibraryEnsemble.from_equations.*list"):
        pa.LibraryEnsemble.from_equations([], 0.2, 1e-3)


def test_members_must_share_what_one_launch_shares():
    import percnn_amd as pa
    C = U.coefficient_set("cross")
    mk = lambda dx=0.2, dt=1e-3, integrator="euler": pa.LibraryCell(C, dx, dt, integrator=integrator)
    with pytest.raises(ValueError, match="LibraryEnsemble.*at least one"):
        pa.LibraryEnsemble([])
    with pytest.raises(ValueError, match="LibraryEnsemble.*share dx"):
        pa.LibraryEnsemble([mk(), mk(dx=0.1)])
    with pytest.raises(ValueError, match="LibraryEnsemble.*share dt"):
        pa.LibraryEnsemble([mk(), mk(), mk(dt=2e-3)])
    with pytest.raises(ValueError, match="LibraryEnsemble.*share integrator"):
        pa.LibraryEnsemble([mk(), mk(integrator="rk4")])
    with pytest.raises(ValueError, match="LibraryEnsemble.*Stage3BurgersCell.*not a LibraryCell"):
        pa.LibraryEnsemble([mk(), pa.Stage3BurgersCell()])
    with pytest.raises(ValueError, match="LibraryEnsemble.*not a LibraryCell"):
        pa.LibraryEnsemble([pa.LibraryEnsemble([mk()])])


def test_cpu_states_are_refused_by_name():
    import percnn_amd as pa
    from percnn_amd import library_cell as lc
    ens = pa.LibraryEnsemble.from_equations(EQS, 0.2, 1e-3)
    h = torch.zeros(3, 2, 8, 8, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="LibraryEnsemble: h0.*no CPU path"):
        ens.rollout(h, 2)
    with pytest.raises(RuntimeError, match="LibraryEnsemble: h0.*no CPU path"):
        ens.rollout_frames(h, 2, [0, 2])
    with pytest.raises(RuntimeError, match="LibraryEnsemble: h0.*no CPU path"):
        ens(h)
    with pytest.raises(RuntimeError, match="LibraryEnsemble: h0.*no CPU path"):
        pa.RCNN(ens, step=2, effective_step=[0, 1], init_state=h)()
    with pytest.raises(RuntimeError, match="LibraryEnsemble: h .*no CPU path"):
        lc.ensemble_step_fwd(h, ens.param_block().detach(), 0.2, 1e-3)
    with pytest.raises(RuntimeError, match="LibraryEnsemble: traj.*no CPU path"):
        lc.ensemble_rollout_fwd_(torch.zeros(3, 3, 2, 8, 8, dtype=torch.float64), ens.param_block().detach(), 0.2, 1e-3)
    with pytest.raises(RuntimeError, match="LibraryEnsemble: traj.*no CPU path"):
        lc.ensemble_rollout_bwd(torch.zeros(3, 3, 2, 8, 8, dtype=torch.float64), torch.zeros(3, 3, 2, 8, 8, dtype=torch.float64),
                                ens.param_block().detach(), 0.2, 1e-3)
    with pytest.raises(ValueError, match="LibraryEnsemble: integrator"):
        lc.ensemble_step_fwd(h, ens.param_block().detach(), 0.2, 1e-3, integrator="heun")
    # the RCNN's own refusals need no device either
    for B in (1, 2, 4):
        with pytest.raises(ValueError, match=r"LibraryEnsemble of 3 cells.*\[3,2,H,W\]"):
            pa.RCNN(ens, step=2, effective_step=[0, 1], init_state=torch.zeros(B, 2, 8, 8, dtype=torch.float64))()
    model = pa.RCNN(ens, step=2, effective_step=[0, 1], init_state=h)
    for call in (model.observe, model.loss_mse, model.sample_losses, lambda: model.sample_physics_losses(torch.zeros(36))):
        with pytest.raises(ValueError, match="LibraryEnsemble"):
            call()
