"""CPU: the per-sample squared-error losses on sparse observations -- C-ABI surface, host arithmetic of the operators, and the
proof that the case lists of test_observed_loss_gpu.py cover the dispatch matrix and the lattice edge cases."""
import ctypes
import os
import re

import numpy as np
import pytest

OBS_SYMBOLS = [f"percnn_pi_{op}_{suf}"
               for op in ("batch_traj_obs_sqerr", "batch_rollout_bwd_obs_sqerr", "ensemble_rollout_bwd_obs_sqerr")
               for suf in ("f32", "f64")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_types_every_symbol():
    import percnn_amd
    from percnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "percnn_pi.h")).read()
    L = percnn_amd.lib()
    ip, i64p = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
    for name in OBS_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"#define PERCNN_PI_ABI_VERSION 3\b", header) and L.percnn_pi_abi_version() == 3
    for suf in ("f32", "f64"):
        for kind in ("batch", "ensemble"):
            a = getattr(L, f"percnn_pi_{kind}_rollout_bwd_obs_sqerr_{suf}").argtypes
            # traj, target_c, frame_mask, strides, scale, ... shape, batch, T, options, stream
            assert len(a) == 18 and a[2] is ctypes.c_char_p and a[3] is ip and a[4] is ctypes.c_double
            assert a[-5:] == [i64p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p]
        a = getattr(L, f"percnn_pi_batch_traj_obs_sqerr_{suf}").argtypes
        assert len(a) == 13 and a[5] is i64p and a[6] is ip and a[7] is ctypes.c_int and a[8] is ctypes.c_double
    assert percnn_amd.pi_rollout_obs_sqerr_batched is percnn_amd.functional.pi_rollout_obs_sqerr_batched
    assert percnn_amd.pi_rollout_obs_sqerr_ensemble is percnn_amd.functional.pi_rollout_obs_sqerr_ensemble
    import inspect
    assert inspect.signature(percnn_amd.RCNN.sample_losses).parameters["space_stride"].default == 1


def test_argument_errors_do_not_need_a_gpu():
    """validation before any launch: -1 for bad arguments (strides among them), -2 for a small workspace"""
    import percnn_amd
    L = percnn_amd.lib()
    shape = (ctypes.c_int64 * 2)(8, 8)
    st, zero, neg = (ctypes.c_int * 2)(2, 3), (ctypes.c_int * 2)(2, 0), (ctypes.c_int * 2)(-1, 1)
    q = L.percnn_pi_batch_traj_sqerr_workspace_bytes
    for suf in ("f32", "f64"):
        for kind in ("batch", "ensemble"):
            f = getattr(L, f"percnn_pi_{kind}_rollout_bwd_obs_sqerr_{suf}")
            for batch in (0, -3, 65536):
                assert f(16, None, None, st, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, batch, 3, None, None) == -1
            for batch in (1, 2):                                                                                        # advective block
                assert f(16, None, None, st, 1.0, None, 32, 48, 64, 1 << 30, 80, -1, 2, shape, batch, 3, None, None) == -1
            assert f(16, None, None, st, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, b"nonsense=1", None) == -1
            assert f(None, None, None, st, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1
            assert f(16, None, None, st, 1.0, None, None, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1
            assert f(16, None, None, st, 1.0, None, 32, None, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1
            assert f(16, None, None, st, 1.0, None, 32, 48, 64, 1 << 30, None, 0, 2, shape, 2, 3, None, None) == -1
            assert f(16, None, None, st, 1.0, None, 16, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1       # g_h0 aliases traj
            assert f(16, 32, None, st, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1         # ... the target
            assert f(16, None, None, st, 1.0, 32, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1         # ... the factors
            assert f(16, None, None, st, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, -1, None, None) == -1      # T < 0
            for batch in (1, 2):
                assert f(16, None, None, None, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, batch, 3, None, None) == -1
                assert f(16, None, None, zero, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, batch, 3, None, None) == -1
                assert f(16, None, None, neg, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, batch, 3, None, None) == -1
                assert f(16, None, None, st, 1.0, None, 32, 48, 64, 16, 80, 0, 2, shape, batch, 3, None, None) == -2
                assert f(16, None, None, st, 1.0, None, 32, 48, None, 1 << 30, 80, 0, 2, shape, batch, 3, None, None) == -2
        s = getattr(L, f"percnn_pi_batch_traj_obs_sqerr_{suf}")
        for batch in (0, -1, 65536):
            assert s(16, None, None, 4, 2, shape, st, batch, 1.0, 32, 64, 1 << 20, None) == -1
        assert s(None, None, None, 4, 2, shape, st, 2, 1.0, 32, 64, 1 << 20, None) == -1
        assert s(16, None, None, 4, 2, shape, st, 2, 1.0, None, 64, 1 << 20, None) == -1
        assert s(16, None, None, 4, 2, shape, st, 2, 1.0, 16, 64, 1 << 20, None) == -1                                  # out aliases traj
        assert s(16, 32, None, 4, 2, shape, st, 2, 1.0, 32, 64, 1 << 20, None) == -1                                    # ... the target
        assert s(16, None, None, -1, 2, shape, st, 2, 1.0, 32, 64, 1 << 20, None) == -1
        for batch in (1, 2):
            assert s(16, None, None, 4, 2, shape, None, batch, 1.0, 32, 64, 1 << 20, None) == -1
            assert s(16, None, None, 4, 2, shape, zero, batch, 1.0, 32, 64, 1 << 20, None) == -1
            assert s(16, None, None, 4, 2, shape, st, batch, 1.0, 32, 64, q(batch) - 8, None) == -2
            assert s(16, None, None, 4, 2, shape, st, batch, 1.0, 32, None, 1 << 20, None) == -2


def test_frame_indices_strides_and_the_mean_weight():
    """host arithmetic of the operators: t_idx normalisation, strides, compact extents, 1 / (n * 2 * prod(ceil(S / s)))"""
    from percnn_amd.functional import obs_selection
    sel, mask, st, Sc, w = obs_selection(200, range(201)[0:-1:20], 4, (100, 100))
    assert sel == list(range(0, 200, 20)) and st == (4, 4) and Sc == (25, 25) and w == 1.0 / (10 * 2 * 25 * 25)
    assert mask == [t % 20 == 0 and t < 200 for t in range(201)]
    sel, mask, st, Sc, w = obs_selection(9, [2, -3, -1], (2, 5), (64, 96), "mean")
    assert sel == [2, 7, 9] and Sc == (32, 20) and w == 1.0 / (3 * 2 * 32 * 20)           # 96 / 5 rounds up
    sel, mask, st, Sc, w = obs_selection(9, range(10), (1, 3, 2), (6, 10, 9), "sum")
    assert mask is None and Sc == (6, 4, 5) and w == 1.0
    assert obs_selection(0, [-1], 7, (2, 3))[1:] == (None, (7, 7), (1, 1), 0.5)
    for bad in ([], [3, 3], [4, 2], [0, -10], [-1, 0]):
        with pytest.raises(ValueError, match="my_op"):
            obs_selection(9, bad, 2, (8, 8), "mean", "my_op")
    with pytest.raises(ValueError, match="one stride per axis"):
        obs_selection(9, [0], (2, 2, 2), (8, 8))
    with pytest.raises(ValueError, match=">= 1"):
        obs_selection(9, [0], (2, 0), (8, 8))
    with pytest.raises(KeyError):
        obs_selection(9, [0], 2, (8, 8), "median")
    # what the operators hand the autograd node, whatever B; the shape errors
    import torch
    from percnn_amd import functional as F_pi
    seen = {}

    class Stop(Exception):
        pass

    def apply(h0, P, steps, target, mask, strides, weight, options):
        seen.update(mask=mask, strides=strides, weight=weight)
        raise Stop

    keep = F_pi.PiRolloutObsSqErrBatchedFunction.apply
    F_pi.PiRolloutObsSqErrBatchedFunction.apply = staticmethod(apply)
    try:
        for B in (1, 4):
            with pytest.raises(Stop):
                F_pi.pi_rollout_obs_sqerr_batched(torch.zeros(B, 2, 6, 8), torch.zeros(36), 5, torch.zeros(2, B, 2, 2, 3), [0, -1], 3)
            assert seen == {"mask": [True, False, False, False, False, True], "strides": (3, 3), "weight": 1.0 / (2 * 2 * 2 * 3)}
        h, Pe = torch.zeros(4, 2, 6, 8), torch.zeros(4, 36)
        for bad in ((2, 4, 2, 3, 3), (1, 4, 2, 2, 3), (2, 2, 2, 2, 3), (2, 4, 2, 6, 8)):
            with pytest.raises(ValueError, match="target must be"):
                F_pi.pi_rollout_obs_sqerr_ensemble(h, Pe, 5, torch.zeros(bad), [0, -1], 3)
        with pytest.raises(ValueError, match="per sample"):
            F_pi.pi_rollout_obs_sqerr_ensemble(h, torch.zeros(36), 5, None, [0], 3)
        with pytest.raises(ValueError, match="one parameter block"):
            F_pi.pi_rollout_obs_sqerr_batched(h, Pe, 5, None, [0], 3)
        with pytest.raises(ValueError, match="strictly increasing"):
            F_pi.pi_rollout_obs_sqerr_batched(h, torch.zeros(36), 5, None, [1, 0], 3)
        with pytest.raises(ValueError, match="one stride per axis"):
            F_pi.pi_rollout_obs_sqerr_batched(h, torch.zeros(36), 5, None, [0], (3,))
    finally:
        F_pi.PiRolloutObsSqErrBatchedFunction.apply = keep


def test_case_lists_cover_the_dispatch_matrix_and_the_lattice_edges():
    """{tile fused, tile unfused, direct 2D vector, direct 2D scalar, direct 3D} x {batched, ensemble} x {target, none}, and per
    family a stride that does not divide an extent, one that is no power of two, an anisotropic one and the reference's own --
    read from the GPU file's case lists alone: test_observed_losses_inside_the_sweep crosses every case with PATHS, TARGETS and
    obs_pairs."""
    import observed_loss_util as U
    from test_batched_loss_cpu import _family
    cases = U.sweep_cases()
    fams = {_family(c) for c in cases}
    assert fams == {"tile fused", "tile unfused", "direct 2D vector", "direct 2D scalar", "direct 3D"}, fams
    assert set(U.PATHS) == {"batch", "ensemble"} and set(U.TARGETS) == {False, True}
    assert all(c["T"] == U.T_SWEEP == 9 for c in cases) and U.SWEEP_B == (2, 3)
    assert {c["shape"] for c in cases} >= {(64, 96), (40, 100), (33, 37), (12, 16, 64), (6, 10, 9)}
    for ndim, ref in ((2, 4), (3, 2)):
        pairs = U.obs_pairs(ndim)
        assert [p[0] for p in pairs] == [list(range(10)), [0, 3, 6], [9], [0], [2, 3, 4, 7]]
        assert [p[1] for p in pairs] == [ref, 3, (2, 5) if ndim == 2 else (1, 3, 2), ref, 3]
    for fam in fams:
        members = [c for c in cases if _family(c) == fam]
        assert {c["B"] for c in members} == {2, 3}, fam
        strides = {U.strides_of(s, len(c["shape"])) for c in members for _, s in U.obs_pairs(len(c["shape"]))}
        ragged = any(n % s for c in members for _, st in U.obs_pairs(len(c["shape"]))
                     for n, s in zip(c["shape"], U.strides_of(st, len(c["shape"]))))
        assert ragged, fam
        assert any(s & (s - 1) for st in strides for s in st), fam                       # no power of two
        assert any(len(set(st)) > 1 for st in strides), fam                              # anisotropic
        assert any(set(st) == {4 if len(st) == 2 else 2} for st in strides), fam         # the reference's
    # the extents the issue names as not divided by their stride
    assert 64 % 3 and 96 % 5 and 37 % 4 and 9 % 2
    assert U.MANY_CASE["B"] == 513 and U.MANY_CASE["shape"] == (2, 3)
    assert U.compact_shape((2, 3), (4, 4)) == (1, 1) and U.compact_shape((2, 3), (2, 2)) == (1, 2)


def test_references_by_tensor_ops_agree_with_plain_loops():
    """the materialised gradient and the float64 loss of observed_loss_util.py against explicit loops over the lattice"""
    import torch
    import observed_loss_util as U
    rs = np.random.RandomState(1)
    traj = torch.from_numpy(rs.uniform(0, 1, (4, 2, 2, 5, 7)))
    t_idx, st = [1, 3], (2, 3)
    tg = torch.from_numpy(rs.uniform(0, 1, (2, 2, 2, 3, 3)))
    fac = torch.tensor([0.5, -1.25], dtype=torch.float64)
    g = U.materialised_obs_gradient(traj, tg, t_idx, st, 0.25, fac)
    want = torch.zeros_like(traj)
    loss = torch.zeros(2, dtype=torch.float64)
    for k, t in enumerate(t_idx):
        for b in range(2):
            for y in range(0, 5, 2):
                for x in range(0, 7, 3):
                    d = traj[t, b, :, y, x] - tg[k, b, :, y // 2, x // 3]
                    want[t, b, :, y, x] = (0.25 * fac[b]) * d
                    loss[b] += (d ** 2).sum() * 0.125
    assert torch.equal(g, want)
    assert torch.allclose(U.obs_losses_f64(traj, tg, t_idx, st, 0.125), loss, rtol=1e-14, atol=0)
    assert U.mean_weight(2, (5, 7), st) == 1.0 / (2 * 2 * 3 * 3)


def test_sweep_case_inputs_are_well_conditioned():
    """the oracle's trajectories of the cases stay finite and of order one (no GPU needed)"""
    import observed_loss_util as U
    from util import o_batch_reference
    for c in U.sweep_cases() + [U.MANY_CASE, U.MISALIGNED_CASE]:
        inp = U.obs_inputs(c)
        for P in (inp["P"], inp["Pe"]):
            traj = o_batch_reference(inp["h0"], P, c["T"])[0]
            assert np.isfinite(traj).all() and np.abs(traj).max() < 10, (c["id"], float(np.abs(traj).max()))
