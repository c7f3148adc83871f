"""CPU: C-ABI surface, operator registration and CellEnsemble of the ensemble rollouts (percnn_pi_ensemble_*,
torch.ops.percnn.*_ensemble, pa.CellEnsemble): one parameter block per sample."""
import ctypes

import pytest
import torch

ENSEMBLE_SYMBOLS = ["percnn_pi_ensemble_bwd_workspace_bytes", "percnn_pi_ensemble_rollout_bwd_workspace_bytes"] + [
    f"percnn_pi_ensemble_{op}_{suf}" for op in ("step_fwd", "step_bwd", "rollout_fwd", "rollout_bwd") for suf in ("f32", "f64")]


def test_ensemble_symbols_are_exported_and_bound():
    import percnn_amd
    from percnn_amd import _lib
    L = percnn_amd.lib()
    for name in ENSEMBLE_SYMBOLS:
        assert name in _lib.EXPORTS
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is not None, name


def test_ensemble_argument_errors_do_not_need_a_gpu():
    """Validation before any launch: bad batch / advective block / options / NULL / aliasing -> -1, small workspace -> -2."""
    import percnn_amd
    L = percnn_amd.lib()
    shape = (ctypes.c_int64 * 2)(8, 8)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"percnn_pi_ensemble_rollout_fwd_{suf}")
        bwd = getattr(L, f"percnn_pi_ensemble_rollout_bwd_{suf}")
        sfwd = getattr(L, f"percnn_pi_ensemble_step_fwd_{suf}")
        sbwd = getattr(L, f"percnn_pi_ensemble_step_bwd_{suf}")
        for batch in (0, -3, 70000):
            assert fwd(1, 2, 8, 2, shape, batch, 3, None, None) == -1
            assert sfwd(1, 2, 3, 8, 2, shape, batch, None, None) == -1
            assert bwd(1, 2, None, 3, 4, 5, 1 << 30, 6, 8, 2, shape, batch, 3, None, None) == -1
            assert sbwd(1, 2, None, 3, 4, 5, 1 << 30, 6, 8, 2, shape, batch, None, None) == -1
        # the advective block (hc = -1) has no ensemble flavour, not even for one sample
        for batch in (1, 4):
            assert fwd(1, 2, -1, 2, shape, batch, 3, None, None) == -1
            assert sfwd(1, 2, 3, -1, 2, shape, batch, None, None) == -1
            assert bwd(1, 2, None, 3, 4, 5, 1 << 30, 6, -1, 2, shape, batch, 3, None, None) == -1
            assert sbwd(1, 2, None, 3, 4, 5, 1 << 30, 6, -1, 2, shape, batch, None, None) == -1
        for bad in (b"nonsense=1", b"tile_k=3", b"tile_k"):
            assert fwd(1, 2, 8, 2, shape, 4, 3, bad, None) == -1, bad
            assert sfwd(1, 2, 3, 0, 2, shape, 4, bad, None) == -1, bad
        assert fwd(1, 2, 8, 4, shape, 4, 3, None, None) == -1                      # bad ndim
        assert fwd(1, 2, 8, 2, shape, 4, -1, None, None) == -1                     # T < 0
        # NULL pointers
        assert fwd(None, 2, 8, 2, shape, 4, 3, None, None) == -1
        assert fwd(1, None, 8, 2, shape, 4, 3, None, None) == -1
        assert sfwd(None, 2, 3, 8, 2, shape, 4, None, None) == -1
        assert sfwd(1, 2, None, 8, 2, shape, 4, None, None) == -1
        assert bwd(1, 2, None, 3, None, 5, 1 << 30, 6, 8, 2, shape, 4, 3, None, None) == -1      # param_grad
        assert bwd(1, 2, None, 3, 4, 5, 1 << 30, None, 8, 2, shape, 4, 3, None, None) == -1      # params
        assert sbwd(1, None, None, 3, 4, 5, 1 << 30, 6, 8, 2, shape, 4, None, None) == -1
        # aliasing: an output on an input
        assert sfwd(1, 1, 3, 8, 2, shape, 4, None, None) == -1
        assert sfwd(1, 3, 3, 8, 2, shape, 4, None, None) == -1
        assert sbwd(1, 2, None, 2, 4, 5, 1 << 30, 6, 8, 2, shape, 4, None, None) == -1
        assert sbwd(1, 2, None, 1, 4, 5, 1 << 30, 6, 8, 2, shape, 4, None, None) == -1
        assert bwd(1, 2, None, 1, 4, 5, 1 << 30, 6, 8, 2, shape, 4, 3, None, None) == -1
        assert bwd(1, 2, None, 2, 4, 5, 1 << 30, 6, 8, 2, shape, 4, 3, None, None) == -1
        assert fwd(1, 1, 8, 2, shape, 4, 3, None, None) == -1
        # too small a workspace
        assert bwd(1, 2, None, 3, 4, 16, 16, 6, 8, 2, shape, 4, 3, None, None) == -2
        assert sbwd(1, 2, None, 3, 4, 16, 16, 6, 8, 2, shape, 4, None, None) == -2
        # T = 0: nothing to do
        assert fwd(1, 2, 8, 2, shape, 4, 0, None, None) == 0


def test_ensemble_workspace_matches_unbatched_at_one_and_grows():
    import percnn_amd
    L = percnn_amd.lib()
    shape = (ctypes.c_int64 * 2)(100, 100)
    s3 = (ctypes.c_int64 * 3)(48, 48, 48)
    for hc in (0, 8):
        for esz in (4, 8):
            assert (L.percnn_pi_ensemble_rollout_bwd_workspace_bytes(hc, 2, shape, 1, 20, esz) ==
                    L.percnn_pi_rollout_bwd_workspace_bytes(hc, 2, shape, 20, esz))
            assert (L.percnn_pi_ensemble_bwd_workspace_bytes(hc, 2, shape, 1, esz) ==
                    L.percnn_pi_bwd_workspace_bytes(hc, 2, shape, esz))
            prev_r = prev_s = 0
            for b in (2, 4, 16, 64):
                r = L.percnn_pi_ensemble_rollout_bwd_workspace_bytes(hc, 2, shape, b, 20, esz)
                s = L.percnn_pi_ensemble_bwd_workspace_bytes(hc, 3, s3, b, esz)
                assert r > prev_r and s > prev_s
                assert r >= 21 * b * 2 * 100 * 100 * esz                         # the adjoint trajectory of every sample
                prev_r, prev_s = r, s
    assert L.percnn_pi_ensemble_rollout_bwd_workspace_bytes(8, 2, shape, 0, 20, 4) == 0
    assert L.percnn_pi_ensemble_rollout_bwd_workspace_bytes(-1, 2, shape, 2, 20, 4) == 0
    assert L.percnn_pi_ensemble_rollout_bwd_workspace_bytes(-1, 2, shape, 1, 20, 4) == 0
    assert L.percnn_pi_ensemble_bwd_workspace_bytes(8, 2, shape, 2, 3) == 0


def test_ensemble_operators_are_registered_with_schemas_and_fake_impls():
    import percnn_amd
    from percnn_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    ops.load_native()
    ns = torch.ops.percnn
    assert str(ns.pi_step_ensemble.default._schema) == 'percnn::pi_step_ensemble(Tensor h, Tensor params, str options="") -> Tensor'
    assert (str(ns.pi_rollout_ensemble.default._schema) ==
            'percnn::pi_rollout_ensemble(Tensor h0, Tensor params, SymInt steps, str options="") -> Tensor')
    assert (str(ns.pi_step_ensemble_backward.default._schema) ==
            'percnn::pi_step_ensemble_backward(Tensor h, Tensor params, Tensor g_out, str options="") -> (Tensor, Tensor)')
    assert (str(ns.pi_rollout_ensemble_backward.default._schema) ==
            'percnn::pi_rollout_ensemble_backward(Tensor traj, Tensor params, Tensor g_traj, str options="") -> (Tensor, Tensor)')
    assert percnn_amd.pi_step_ensemble is percnn_amd.functional.pi_step_ensemble
    assert percnn_amd.pi_rollout_ensemble is percnn_amd.functional.pi_rollout_ensemble
    with FakeTensorMode():
        h = torch.empty(5, 2, 16, 24, device="cuda")
        P = torch.empty(5, 36, device="cuda")
        assert ns.pi_step_ensemble(h, P).shape == (5, 2, 16, 24)
        traj = ns.pi_rollout_ensemble(h, P, 7)
        assert traj.shape == (8, 5, 2, 16, 24)
        g0, gp = ns.pi_rollout_ensemble_backward(traj, P, traj)
        assert g0.shape == (5, 2, 16, 24) and gp.shape == (5, 36)
        gi, gp = ns.pi_step_ensemble_backward(h, P, h)
        assert gi.shape == h.shape and gp.shape == (5, 36)
        h3 = torch.empty(3, 2, 8, 12, 16, device="cuda")
        P3 = torch.empty(3, 16 + 2 * 21, device="cuda")
        assert ns.pi_rollout_ensemble(h3, P3, 2).shape == (3, 3, 2, 8, 12, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.pi_step_ensemble(torch.zeros(3, 2, 8, 8), torch.zeros(3, 36))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.pi_rollout_ensemble(torch.zeros(3, 2, 8, 8), torch.zeros(3, 36), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.pi_rollout_ensemble_backward(torch.zeros(4, 3, 2, 8, 8), torch.zeros(3, 36), torch.zeros(4, 3, 2, 8, 8))


def test_cell_ensemble_rejects_mismatched_or_unsupported_members():
    import percnn_amd as pa
    from percnn_amd.stage1 import Stage1Cell
    with pytest.raises(ValueError):
        pa.CellEnsemble([])
    with pytest.raises(ValueError):
        pa.CellEnsemble([pa.gs2d_cell(8), pa.gs2d_cell(4)])                   # hidden_channels
    with pytest.raises(ValueError):
        pa.CellEnsemble([pa.gs2d_cell(2), pa.gs3d_cell(2)])                   # ndim
    with pytest.raises(ValueError):
        pa.CellEnsemble([pa.gs2d_cell(4), pa.lo2d_cell(4)])                   # dtype
    with pytest.raises(ValueError):
        pa.CellEnsemble([pa.gs2d_cell(4), pa.Stage3LambdaOmegaCell()])        # cell type
    with pytest.raises(ValueError):
        pa.CellEnsemble([pa.Stage3BurgersCell(), pa.Stage3BurgersCell()])     # advective block
    with pytest.raises(ValueError):
        pa.CellEnsemble([Stage1Cell(), Stage1Cell()])                         # Stage-1 cells
    ens = pa.CellEnsemble([pa.gs2d_cell(8), pa.gs2d_cell(8, reaction="factored")])
    assert len(ens) == 2
    assert len(pa.CellEnsemble([pa.Stage3LambdaOmegaCell(), pa.Stage3LambdaOmegaCell(dt=0.01)])) == 2


def test_cell_ensemble_state_dict_keys_load_reference_checkpoints():
    import percnn_amd as pa
    from oracle import restatement as R
    torch.manual_seed(0)
    refs = [R.gs2d_cell(8) for _ in range(3)]
    ens = pa.CellEnsemble([pa.gs2d_cell(8) for _ in range(3)])
    sd = {}
    for i, r in enumerate(refs):
        for k, v in r.state_dict().items():
            sd[f"cells.{i}.{k}"] = v
    assert set(sd) == set(ens.state_dict())
    ens.load_state_dict(sd)
    for i, r in enumerate(refs):
        for k, v in r.state_dict().items():
            assert torch.equal(ens.state_dict()[f"cells.{i}.{k}"], v)
        # member i alone loads the reference checkpoint by prefix
        one = pa.gs2d_cell(8)
        one.load_state_dict({k[len(f"cells.{i}."):]: v for k, v in ens.state_dict().items() if k.startswith(f"cells.{i}.")})
        for k, v in r.state_dict().items():
            assert torch.equal(one.state_dict()[k], v)
