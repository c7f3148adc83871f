"""CPU: the per-sample squared-error losses of batches and ensembles -- C-ABI surface, host arithmetic of the operators, and the
proof that the case lists of test_batched_loss_gpu.py cover the dispatch matrix."""
import ctypes
import os
import re

import numpy as np
import pytest

LOSS_SYMBOLS = ["percnn_pi_batch_traj_sqerr_workspace_bytes"] + [
    f"percnn_pi_{op}_{suf}" for op in ("batch_traj_sqerr", "batch_rollout_bwd_sqerr", "ensemble_rollout_bwd_sqerr")
    for suf in ("f32", "f64")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_types_every_symbol():
    import percnn_amd
    from percnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "percnn_pi.h")).read()
    L = percnn_amd.lib()
    for name in LOSS_SYMBOLS:
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.percnn_pi_batch_traj_sqerr_workspace_bytes.restype is ctypes.c_size_t
    for suf in ("f32", "f64"):
        # batch after shape, then T, the options string and the stream
        for kind in ("batch", "ensemble"):
            a = getattr(L, f"percnn_pi_{kind}_rollout_bwd_sqerr_{suf}").argtypes
            assert len(a) == 17 and a[3] is ctypes.c_double and a[-5:] == [ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int,
                                                                           ctypes.c_char_p, ctypes.c_void_p]
        a = getattr(L, f"percnn_pi_batch_traj_sqerr_{suf}").argtypes
        assert len(a) == 12 and a[5] is ctypes.POINTER(ctypes.c_int64) and a[6] is ctypes.c_int and a[7] is ctypes.c_double
    assert percnn_amd.pi_rollout_sqerr_batched is percnn_amd.functional.pi_rollout_sqerr_batched
    assert percnn_amd.pi_rollout_sqerr_ensemble is percnn_amd.functional.pi_rollout_sqerr_ensemble
    assert callable(percnn_amd.RCNN.sample_losses)


def test_argument_errors_do_not_need_a_gpu():
    """validation before any launch: -1 for bad arguments, -2 for a small workspace; the workspace query"""
    import percnn_amd
    L = percnn_amd.lib()
    shape = (ctypes.c_int64 * 2)(8, 8)
    q = L.percnn_pi_batch_traj_sqerr_workspace_bytes
    assert q(0) == 0 and q(-2) == 0 and q(65536) == 0
    assert q(1) == 8192                                   # batch 1 is the unbatched entry point, with its workspace
    assert all(q(b) >= 8 * b for b in (2, 3, 64, 513, 65535))
    for suf in ("f32", "f64"):
        for kind in ("batch", "ensemble"):
            f = getattr(L, f"percnn_pi_{kind}_rollout_bwd_sqerr_{suf}")
            for batch in (0, -3, 65536):
                assert f(16, None, None, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, batch, 3, None, None) == -1
            assert f(16, None, None, 1.0, None, 32, 48, 64, 1 << 30, 80, -1, 2, shape, 2, 3, None, None) == -1     # advective block
            assert f(16, None, None, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, b"nonsense=1", None) == -1
            assert f(None, None, None, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1
            assert f(16, None, None, 1.0, None, None, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1
            assert f(16, None, None, 1.0, None, 32, None, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1
            assert f(16, None, None, 1.0, None, 32, 48, 64, 1 << 30, None, 0, 2, shape, 2, 3, None, None) == -1
            assert f(16, None, None, 1.0, None, 16, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1       # g_h0 aliases traj
            assert f(16, 32, None, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1         # ... the target
            assert f(16, None, None, 1.0, 32, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -1         # ... the factors
            assert f(16, None, None, 1.0, None, 32, 48, 64, 1 << 30, 80, 0, 2, shape, 2, -1, None, None) == -1      # T < 0
            assert f(16, None, None, 1.0, None, 32, 48, 64, 16, 80, 0, 2, shape, 2, 3, None, None) == -2
            assert f(16, None, None, 1.0, None, 32, 48, None, 1 << 30, 80, 0, 2, shape, 2, 3, None, None) == -2
        s = getattr(L, f"percnn_pi_batch_traj_sqerr_{suf}")
        for batch in (0, -1, 65536):
            assert s(16, None, None, 4, 2, shape, batch, 1.0, 32, 64, 1 << 20, None) == -1
        assert s(None, None, None, 4, 2, shape, 2, 1.0, 32, 64, 1 << 20, None) == -1
        assert s(16, None, None, 4, 2, shape, 2, 1.0, None, 64, 1 << 20, None) == -1
        assert s(16, None, None, 4, 2, shape, 2, 1.0, 16, 64, 1 << 20, None) == -1                                  # out aliases traj
        assert s(16, 32, None, 4, 2, shape, 2, 1.0, 32, 64, 1 << 20, None) == -1                                    # ... the target
        assert s(16, None, None, -1, 2, shape, 2, 1.0, 32, 64, 1 << 20, None) == -1
        assert s(16, None, None, 4, 2, shape, 2, 1.0, 32, 64, q(2) - 8, None) == -2
        assert s(16, None, None, 4, 2, shape, 2, 1.0, 32, None, 1 << 20, None) == -2


def test_frame_selection_mask_and_weight():
    """host arithmetic of the operators: negative indices, duplicates, the dense selection, an empty one"""
    from percnn_amd.functional import sqerr_selection
    assert sqerr_selection(9, None, "mean", 200) == (None, 1.0 / (10 * 200))
    assert sqerr_selection(9, range(10), "sum", 200) == (None, 1.0)
    mask, w = sqerr_selection(9, [-1, 9, 2, 2, -10], "mean", 7)
    assert mask == [True, False, True, False, False, False, False, False, False, True] and w == 1.0 / (3 * 7)
    mask, w = sqerr_selection(9, list(range(0, 9, 3)), "mean", 12288)
    assert mask == [t % 3 == 0 and t < 9 for t in range(10)] and w == 1.0 / (3 * 12288)
    assert sqerr_selection(0, [0, -1], "mean", 5) == (None, 0.2)
    assert sqerr_selection(4, [3], "sum", 5) == ([False, False, False, True, False], 1.0)
    with pytest.raises(ValueError, match="my_op: no frame selected"):
        sqerr_selection(9, [], "mean", 5, "my_op")
    with pytest.raises(KeyError):
        sqerr_selection(9, None, "median", 5)
    # the weight is per SAMPLE: the operators pass the elements of one sample's frame, whatever B
    import torch
    from percnn_amd import functional as F_pi
    seen = {}

    class Stop(Exception):
        pass

    def apply(h0, P, steps, target, mask, weight, options):
        seen.update(mask=mask, weight=weight)
        raise Stop

    keep = F_pi.PiRolloutSqErrBatchedFunction.apply
    F_pi.PiRolloutSqErrBatchedFunction.apply = staticmethod(apply)
    try:
        for B in (1, 4):
            with pytest.raises(Stop):
                F_pi.pi_rollout_sqerr_batched(torch.zeros(B, 2, 6, 8), torch.zeros(36), 5, None, [-1, 0])
            assert seen == {"mask": [True, False, False, False, False, True], "weight": 1.0 / (2 * 2 * 6 * 8)}
        with pytest.raises(ValueError, match="trajectory's shape"):
            F_pi.pi_rollout_sqerr_ensemble(torch.zeros(4, 2, 6, 8), torch.zeros(4, 36), 5, torch.zeros(6, 2, 6, 8))
        with pytest.raises(ValueError, match="per sample"):
            F_pi.pi_rollout_sqerr_ensemble(torch.zeros(4, 2, 6, 8), torch.zeros(36), 5)
        with pytest.raises(ValueError, match="one parameter block"):
            F_pi.pi_rollout_sqerr_batched(torch.zeros(4, 2, 6, 8), torch.zeros(4, 36), 5)
    finally:
        F_pi.PiRolloutSqErrBatchedFunction.apply = keep


def _family(c):
    """the sweep family of a case, by the dispatch rules restated in test_batched_cpu.py"""
    from test_batched_cpu import _tile_variant, _vec
    tv = _tile_variant(c, True)
    if tv:
        return "tile fused" if tv.endswith("-fused") else "tile unfused"
    if len(c["shape"]) == 3:
        return "direct 3D"
    return "direct 2D vector" if _vec(c) > 1 else "direct 2D scalar"


def test_case_lists_cover_the_dispatch_matrix():
    """{tile fused, tile unfused, direct 2D vector, direct 2D scalar, direct 3D} x {batched, ensemble} x {mode 1, mode 2}, read
    from the GPU file's case lists alone: test_sample_losses_inside_the_sweep crosses every case of sweep_cases() with PATHS,
    MODES and the frame sets."""
    import batched_loss_util as U
    cases = U.sweep_cases()
    assert len({c["id"] for c in cases}) == len(cases)
    fams = {_family(c) for c in cases}
    assert fams == {"tile fused", "tile unfused", "direct 2D vector", "direct 2D scalar", "direct 3D"}, fams
    assert set(U.PATHS) == {"batch", "ensemble"} and set(U.MODES) == {1, 2}
    for fam in fams:
        assert {c["B"] for c in cases if _family(c) == fam} == {2, 3}, fam
    # the cases the sweep family list names: shape, type, block kind, options
    named = {(c["shape"], c["dtype"].name, c["hc"], tuple(sorted((c["options"] or {}).items()))) for c in cases}
    assert {((64, 96), "float32", 0, ()), ((64, 96), "float32", 0, (("tile_fuse", 0),)), ((40, 100), "float32", 8, ()),
            ((64, 64), "float64", 0, ()), ((48, 72), "float32", 0, (("tile", 0),)), ((33, 37), "float32", 2, ()),
            ((12, 16, 64), "float32", 0, ()), ((6, 10, 9), "float64", 3, ())} <= named
    assert all(c["T"] == 9 for c in cases)                 # two K = 4 tile launches and one direct leftover step
    assert U.frame_sets(9) == [None, [0, 3, 6], [9], [0], [2, 3, 4, 7]]
    # the gradient pass after the sweep (factored blocks) and the fused sums, either type
    assert {(c["dtype"].name, c["hc"] == 0) for c in cases} == {("float32", True), ("float32", False), ("float64", True), ("float64", False)}
    # factors: distinct, a zero among them, for B = 2 already
    assert len(set(U.FACTORS)) == 3 and 0.0 in U.FACTORS[:2] and all(f != 1.0 for f in U.FACTORS)
    assert U.MANY_CASE["B"] == 513 and U.MANY_CASE["shape"] == (2, 3) and U.MANY_CASE["T"] == 3


def test_sweep_case_inputs_are_well_conditioned():
    """the oracle's trajectories of every sweep case stay finite and of order one (no GPU needed)"""
    import batched_loss_util as U
    from util import o_batch_reference
    for c in U.sweep_cases() + [U.MANY_CASE]:
        inp = U.loss_inputs(c)
        for P in (inp["P"], inp["Pe"]):
            traj = o_batch_reference(inp["h0"], P, c["T"])[0]
            assert np.isfinite(traj).all() and np.abs(traj).max() < 10, (c["id"], float(np.abs(traj).max()))
