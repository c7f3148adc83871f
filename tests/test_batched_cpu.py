"""CPU: C-ABI surface and operator registration of the batched rollouts (percnn_pi_batch_*, torch.ops.percnn.*_batched)."""
import ctypes

import pytest
import torch

BATCH_SYMBOLS = ["percnn_pi_batch_bwd_workspace_bytes", "percnn_pi_batch_rollout_bwd_workspace_bytes"] + [
    f"percnn_pi_batch_{op}_{suf}" for op in ("step_fwd", "step_bwd", "rollout_fwd", "rollout_bwd") for suf in ("f32", "f64")]


def test_batched_symbols_are_exported_and_bound():
    import percnn_amd
    from percnn_amd import _lib
    L = percnn_amd.lib()
    for name in BATCH_SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(L, name)


def test_batched_argument_errors_do_not_need_a_gpu():
    """Validation before any launch: bad batch / advective block / options -> -1, small workspace -> -2, T = 0 -> 0."""
    import percnn_amd
    L = percnn_amd.lib()
    shape = (ctypes.c_int64 * 2)(8, 8)
    for suf in ("f32", "f64"):
        fwd = getattr(L, f"percnn_pi_batch_rollout_fwd_{suf}")
        bwd = getattr(L, f"percnn_pi_batch_rollout_bwd_{suf}")
        sfwd = getattr(L, f"percnn_pi_batch_step_fwd_{suf}")
        sbwd = getattr(L, f"percnn_pi_batch_step_bwd_{suf}")
        for batch in (0, -3, 70000):
            assert fwd(1, 2, 8, 2, shape, batch, 3, None, None) == -1
            assert sfwd(1, 2, 3, 8, 2, shape, batch, None, None) == -1
            assert bwd(1, 2, None, 3, 4, 5, 1 << 30, 6, 8, 2, shape, batch, 3, None, None) == -1
            assert sbwd(1, 2, None, 3, 4, 5, 1 << 30, 6, 8, 2, shape, batch, None, None) == -1
        # the advective block (hc = -1) has no batched flavour
        assert fwd(1, 2, -1, 2, shape, 4, 3, None, None) == -1
        assert sfwd(1, 2, 3, -1, 2, shape, 2, None, None) == -1
        # bad options, bad ndim, bad shape, NULL pointers
        for bad in (b"nonsense=1", b"tile_k=3", b"tile_k"):
            assert fwd(1, 2, 8, 2, shape, 4, 3, bad, None) == -1, bad
            assert sfwd(1, 2, 3, 0, 2, shape, 4, bad, None) == -1, bad
        assert fwd(1, 2, 8, 4, shape, 4, 3, None, None) == -1
        assert fwd(None, 2, 8, 2, shape, 4, 3, None, None) == -1
        assert sfwd(1, 1, 3, 8, 2, shape, 4, None, None) == -1                       # aliasing
        assert fwd(1, 2, 8, 2, shape, 4, -1, None, None) == -1                       # T < 0
        # too small a workspace
        assert bwd(1, 2, None, 3, 4, 16, 16, 6, 8, 2, shape, 4, 3, None, None) == -2
        assert sbwd(1, 2, None, 3, 4, 16, 16, 6, 8, 2, shape, 4, None, None) == -2
        # T = 0: nothing to do
        assert fwd(1, 2, 8, 2, shape, 4, 0, None, None) == 0
        assert fwd(1, 2, 0, 2, shape, 4, 0, b"tile_k=4", None) == 0


def test_batched_workspace_grows_with_batch():
    import percnn_amd
    L = percnn_amd.lib()
    shape = (ctypes.c_int64 * 2)(100, 100)
    s3 = (ctypes.c_int64 * 3)(48, 48, 48)
    for hc in (0, 8):
        for esz in (4, 8):
            # batch 1 is the unbatched entry point, with its workspace
            assert (L.percnn_pi_batch_rollout_bwd_workspace_bytes(hc, 2, shape, 1, 20, esz) ==
                    L.percnn_pi_rollout_bwd_workspace_bytes(hc, 2, shape, 20, esz))
            assert L.percnn_pi_batch_bwd_workspace_bytes(hc, 2, shape, 1, esz) == L.percnn_pi_bwd_workspace_bytes(hc, 2, shape, esz)
            prev_r = prev_s = 0
            for b in (2, 4, 16, 64):
                r = L.percnn_pi_batch_rollout_bwd_workspace_bytes(hc, 2, shape, b, 20, esz)
                s = L.percnn_pi_batch_bwd_workspace_bytes(hc, 3, s3, b, esz)
                assert r > prev_r and s > prev_s
                assert r >= 21 * b * 2 * 100 * 100 * esz                         # the adjoint trajectory of every sample
                prev_r, prev_s = r, s
    assert L.percnn_pi_batch_rollout_bwd_workspace_bytes(8, 2, shape, 0, 20, 4) == 0
    assert L.percnn_pi_batch_rollout_bwd_workspace_bytes(-1, 2, shape, 2, 20, 4) == 0
    assert L.percnn_pi_batch_bwd_workspace_bytes(8, 2, shape, 2, 3) == 0


def test_batched_operators_are_registered_with_schemas_and_fake_impls():
    import percnn_amd  # noqa: F401
    from percnn_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    ops.load_native()
    ns = torch.ops.percnn
    assert str(ns.pi_step_batched.default._schema) == 'percnn::pi_step_batched(Tensor h, Tensor params, str options="") -> Tensor'
    assert "SymInt steps" in str(ns.pi_rollout_batched.default._schema)
    for name in ("pi_step_batched_backward", "pi_rollout_batched_backward"):
        assert hasattr(ns, name)
    assert percnn_amd.pi_step_batched is percnn_amd.functional.pi_step_batched
    assert percnn_amd.pi_rollout_batched is percnn_amd.functional.pi_rollout_batched
    with FakeTensorMode():
        h = torch.empty(5, 2, 16, 24, device="cuda")
        P = torch.empty(36, device="cuda")
        assert ns.pi_step_batched(h, P).shape == h.shape
        traj = ns.pi_rollout_batched(h, P, 7)
        assert traj.shape == (8, 5, 2, 16, 24)
        g0, gp = ns.pi_rollout_batched_backward(traj, P, traj)
        assert g0.shape == (5, 2, 16, 24) and gp.shape == P.shape
        gi, gp = ns.pi_step_batched_backward(h, P, h)
        assert gi.shape == h.shape and gp.shape == P.shape
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.pi_step_batched(torch.zeros(3, 2, 8, 8), torch.zeros(36))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ns.pi_rollout_batched(torch.zeros(3, 2, 8, 8), torch.zeros(36), 3)
