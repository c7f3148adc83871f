"""CPU: C-ABI surface and operator registration of the batched rollouts (percnn_pi_batch_*, torch.ops.percnn.*_batched)."""
import ctypes

import numpy as np
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


def test_batch_limit_is_the_grid_y_limit():
    """65 535 samples pass argument validation (T = 0: nothing is launched), 65 536 are PERCNN_PI_EINVAL -- batched and ensemble"""
    import percnn_amd
    L = percnn_amd.lib()
    shape = (ctypes.c_int64 * 2)(4, 4)
    for kind in ("batch", "ensemble"):
        for suf in ("f32", "f64"):
            fwd = getattr(L, f"percnn_pi_{kind}_rollout_fwd_{suf}")
            assert fwd(16, 32, 0, 2, shape, 65535, 0, None, None) == 0
            assert fwd(16, 32, 0, 2, shape, 65536, 0, None, None) == -1
            assert fwd(16, 32, 0, 2, shape, 65536, 3, None, None) == -1
        ws = getattr(L, f"percnn_pi_{kind}_rollout_bwd_workspace_bytes")
        assert ws(0, 2, shape, 65535, 3, 4) > 0 and ws(0, 2, shape, 65536, 3, 4) == 0


# ---- the case lists of test_batch_fuzz_gpu.py / test_batch_dispatch_gpu.py cover the dispatch matrix -------------------------
def _vec(c):
    V = 4 if c["dtype"].itemsize == 4 else 2
    return 1 if (c["shape"][-1] % V or (c["options"] or {}).get("vec") == 1) else V


def _hc_class(hc):
    return {0: "poly", 2: "2", 4: "4", 8: "8"}.get(hc, "generic")


def _tile_variant(c, adjoint):
    """The tile kernel a case's sample takes (None: direct kernels) -- the rules of tile_eligible, tile_by_for, tile_wide_for,
    tile_variant_for, batch_tile and PI_TILE_VARIANTS of csrc/pi_abi.hip restated, for 16-byte-aligned buffers.  The library has no
    query entry for the batched dispatch, so nothing ties this copy to it: csrc/pi_abi.hip is the source of truth, and a change
    of a rule or a threshold there must be made here too, or the coverage proof below goes stale without failing."""
    o = {"tile": 1, "tile_k": 4, "tile_nt": 512, "tile_by": 0, "vec": 0, "tile_wide": 3, "tile_fuse": 1, "skip_wgrad": 0}
    o.update(c["options"] or {})
    shape, hc, f32 = c["shape"], c["hc"], c["dtype"].itemsize == 4
    if len(shape) != 2 or hc not in (0, 2, 4, 8) or not o["tile"] or _vec(c) == 1:
        return None
    n0, W = shape
    cdiv = lambda a, b: (a + b - 1) // b

    def by_for():
        if hc != 0:
            return 32
        if o["tile_by"] in (8, 16, 32):
            return o["tile_by"]
        if o["tile_k"] != 4 or o["tile_nt"] != 512:
            return 32
        t32, t8 = cdiv(n0, 32) * cdiv(W, 32), cdiv(n0, 8) * cdiv(W, 32)
        if t8 > 256 and 112 < t32 <= 128 and n0 % 32 == 0 and W % 32 == 0:
            return 32
        return 8 if t8 <= 256 else (16 if t32 <= 128 else 32)

    def wide_for(adj):
        if not f32 or hc != 0 or o["tile_wide"] == 0 or o["tile_k"] != 4 or o["tile_nt"] != 512 or o["tile_by"] != 0:
            return 0
        if o["tile_wide"] in (1, 2):
            return o["tile_wide"]
        tiles = lambda bx, by: cdiv(n0, by) * cdiv(W, bx)
        if tiles(32, 32) <= 256:
            return 0
        if tiles(32, 40) <= 256:
            return 1
        return 2 if adj and tiles(40, 40) <= 256 else 0

    wide = wide_for(adjoint)
    bx, by = {0: (32, by_for()), 1: (32, 40), 2: (40, 40)}[wide]
    fits = lambda n, b: cdiv(n, b) * b + 16 <= 2 * n
    if not fits(n0, max(by, 32)) or not fits(W, bx):
        return None
    n = n0 * W * c["B"]
    if o["tile"] == 1 and n >= ((5 << 18) if adjoint else (3 << 20)):
        return None
    fuse_ok = (adjoint and o["tile_fuse"] and not o["skip_wgrad"] and hc == 0 and o["tile_k"] == 4 and o["tile_nt"] == 512 and
               (by_for() == 32 or wide_for(True) != 0))
    if wide:
        return f"wide{wide}" + ("-fused" if fuse_ok else "")
    if fuse_ok:                                            # (either type: TileVariant::mom does not look at it)
        return "k4-512-fused"
    if o["tile_k"] == 2:
        return "k2"
    if hc == 0:
        if o["tile_k"] == 8:
            return "k8"
        if o["tile_nt"] == 1024:
            return "k4-1024"
        if by_for() in (8, 16):
            return f"k4-by{by_for()}"
    return "k4-256" if o["tile_nt"] == 256 else "k4-512"


def _pass_vec(c):
    """lane width of the time-parallel gradient pass: vec_ok of batch / ens_rollout_bwd_impl looks at n, not at the row length"""
    V = 4 if c["dtype"].itemsize == 4 else 2
    return 1 if (int(np.prod(c["shape"])) % V or (c["options"] or {}).get("vec") == 1) else V


def _pass_runs(c):
    """the sweep leaves the branch gradients to the time-parallel pass; only masks that leave t_top > 0 whatever the draw:
    dense, t % 3 == 0 with T >= 3, and util.make_mask's "top" with T >= 2 (it sets a frame in [T - (T + 1) // 2, T - 1])"""
    o = c["options"] or {}
    live = c["mask"] == "none" or (c["mask"] == "mod3" and c["T"] >= 3) or (c["mask"] == "top" and c["T"] >= 2)
    if not live or c["T"] < 1 or o.get("skip_wgrad"):
        return False
    tv = _tile_variant(c, True)
    if tv:
        return not tv.endswith("-fused")
    fw = o.get("fuse_wgrad", 2)
    return not (fw == 1 or (fw == 2 and c["hc"] == 0))


def test_batched_case_lists_cover_the_dispatch_matrix():
    """Every case of the two files runs the batched AND the ensemble path (util.check_case), so one list serves both.  A later
    edit of a seed or a list that drops a branch fails here, without a GPU."""
    import test_batch_dispatch_gpu as D
    import test_batch_fuzz_gpu as F
    from util import MASK_KINDS
    cases = F.all_cases() + D.all_cases()
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids)
    assert 140 <= len(F._cases()) <= 160 and len(F._large2d_cases()) >= 12
    # (ndim) x (block kind) x (lane width) x (type)
    seen = {(len(c["shape"]), _hc_class(c["hc"]), "V" if _vec(c) > 1 else "1", c["dtype"].name) for c in cases}
    want = {(nd, h, v, d) for nd in (2, 3) for h in ("poly", "2", "4", "8", "generic") for v in ("1", "V") for d in ("float32", "float64")}
    assert not want - seen, sorted(want - seen)
    # the same by the fuzz sweep alone, up to the rarest corners
    seen_f = {(len(c["shape"]), "V" if _vec(c) > 1 else "1", c["dtype"].name) for c in F.all_cases()}
    assert len(seen_f) == 8
    assert {_hc_class(c["hc"]) for c in F.all_cases()} == {"poly", "2", "4", "8", "generic"}
    # the hidden-channel chunks of the gradient pass with j0 > 0: jc = 1 (hc 3), 2 (6), 4 (12: the only chunked width of four), 8 (16),
    # each in a call where the pass runs, at either lane width and type
    for hc in (3, 6, 12, 16):
        got = {(c["dtype"].name, "V" if _pass_vec(c) > 1 else "1") for c in cases if c["hc"] == hc and _pass_runs(c)}
        assert len(got) == 4, (hc, sorted(got))
        assert {len(c["shape"]) for c in cases if c["hc"] == hc and _pass_runs(c)} == {2, 3}, hc
    assert {c["hc"] for c in F.all_cases()} >= {3, 6, 16}
    # the batched pass over the flattened frame index where its lane width (n % V) and the step kernels' (W % V) disagree
    assert any(_pass_runs(c) and _pass_vec(c) > 1 and _vec(c) == 1 and (c["options"] or {}).get("vec") != 1 for c in cases)
    # tile variants, per block kind and direction
    tv = {(adj, _hc_class(c["hc"]), c["dtype"].name, _tile_variant(c, adj)) for c in cases for adj in (False, True)}
    for adj in (False, True):
        for h in ("poly", "2", "4", "8"):
            for d in ("float32", "float64"):
                need = {"k2", "k4-256", "k4-512"}
                if h == "poly":
                    need |= {"k8", "k4-1024", "k4-by8", "k4-by16"}
                got = {v for a, hh, dd, v in tv if a == adj and hh == h and dd == d}
                if (h, d) in D_KINDS_TILE:                  # the block kinds of test_tile_variants_bitwise
                    assert not need - got, (adj, h, d, sorted(need - got))
    assert {(False, "poly", "float32", "wide1"), (True, "poly", "float32", "wide1-fused"), (True, "poly", "float32", "wide2-fused"),
            (True, "poly", "float32", "k4-512-fused"), (True, "poly", "float64", "k4-512-fused"),
            (True, "poly", "float32", "wide1"), (True, "poly", "float32", "wide2"), (False, "poly", "float32", "wide2")} <= tv
    # ... the wide tiles and the fused 32 x 32 sweep also by default dispatch (no options), on ragged grids
    dflt = {(adj, _tile_variant(c, adj)) for c in F._large2d_cases() for adj in (False, True)}
    assert {(False, "wide1"), (True, "wide1-fused"), (True, "wide2-fused"), (True, "k4-512-fused"), (True, "k4-512")} <= dflt
    # the XCD tile map: tile counts that split into 8 rectangles, with and without the map
    xcd = [c for c in cases if _tile_variant(c, True) == "k4-512" and c["shape"] == (128, 256)]
    assert any((c["options"] or {}).get("tile_xcd") == 0 for c in xcd) and any(not (c["options"] or {}).get("tile_xcd", 1) == 0 for c in xcd)
    # forward on tiles and the sweep on the direct kernels within one call
    assert any(_tile_variant(c, False) and not _tile_variant(c, True) and not c["options"] for c in D._switch_cases())
    # rollout lengths around K among tile-eligible cases, every kind of mask
    tile_T = {c["T"] for c in cases if _tile_variant(c, True)}
    assert {t % 4 for t in tile_T} == {0, 1, 2, 3} and min(tile_T) < 4
    assert {c["mask"] for c in F.all_cases()} == set(MASK_KINDS)
    assert {c["B"] for c in F._cases()} == {2, 3, 5, 8} and {c["T"] for c in F._cases()} == {1, 2, 3, 4, 5, 7, 8, 9, 13}
    # extents below the stencil width along every axis
    assert {a for c in cases for a, e in enumerate(c["shape"]) if len(c["shape"]) == 2 and e < 5} == {0, 1}
    assert {a for c in cases for a, e in enumerate(c["shape"]) if len(c["shape"]) == 3 and e < 5} == {0, 1, 2}


D_KINDS_TILE = {("8", "float32"), ("2", "float32"), ("4", "float64"), ("poly", "float32"), ("poly", "float64")}
