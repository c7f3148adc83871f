"""Every dispatch branch of the batched (percnn_pi_batch_*) and ensemble (percnn_pi_ensemble_*) rollouts on purpose, against the
plain-C oracle looped over the samples: the tile variants of PI_TILE_VARIANTS and both wide tiles, the direct kernels' options,
the B-dependent tile / direct switch, the step adjoint with an injected gradient, base pointers off 16 bytes, the ensemble's
partial-row bounds, many samples on a tiny grid, and the degenerate calls.

Options travel per call (the `options` argument of the operators and of the C-ABI wrappers of util.py), never through
pa.set_option: a failing case cannot leak process defaults."""
import functools

import numpy as np
import pytest
import torch

from util import (batch_rollout_bwd, batch_rollout_fwd_, batch_step_bwd, batch_case_id, check_case, ensemble_blocks, ensemble_rollout_bwd,
                  ensemble_rollout_fwd_, ensemble_step_bwd, grad_err, make_case, make_inputs, o_batch_reference, o_step_bwd,
                  oracle, random_block, rel_l2, single_rollout_bwd, GRAD_TOL)

pytestmark = pytest.mark.gpu


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- (a) tile variants: the option sets, block kinds and shapes of test_tile_variants_bitwise -------------------------------
TILE_OPTS = [{"tile": 0}, {"tile_xcd": 0}, {"tile_k": 2}, {"tile_k": 4, "tile_nt": 256}, {"tile_k": 4, "tile_nt": 512},
             {"tile_k": 4, "tile_nt": 1024}, {"tile_k": 8}, {"tile_by": 8}, {"tile_by": 16}, {"tile_by": 32}, {"vec": 1},
             {"tile_wide": 1}, {"tile_wide": 2}, {"tile_persist": 0}]
TILE_KINDS = [(np.float32, 8), (np.float32, 2), (np.float64, 4), (np.float32, 0), (np.float64, 0)]
TILE_SHAPES = [(64, 96), (40, 100), (128, 256)]


def _tile_cases():
    """(64, 96): whole tiles; (40, 100): partial edge tiles; (128, 256): 4 x 8 tiles, the XCD tile map is active.  One seed per
    (shape, block kind): the oracle's answer is shared by the option sets, which vary fastest."""
    out = []
    k = 0
    for shape in TILE_SHAPES:
        for dtype, hc in TILE_KINDS:
            seed = 420 if k == 8 else 400 + k     # (seed 408's shared block drives (40, 100) poly to |h| ~ 3e3 by T = 19)
            k += 1
            # beyond that list: the float64 fused-moments sweep, and the split 32 x 32 sweep of float32 polynomial blocks
            # ... and the split sweeps on the wide tiles (float32 polynomial blocks)
            extra = ([{"tile_fuse": 2}] if dtype == np.float64 else []) + ([{"tile_fuse": 0, "tile_by": 32}] if hc == 0 else [])
            if hc == 0 and dtype == np.float32:
                extra += [{"tile_wide": 1, "tile_fuse": 0}, {"tile_wide": 2, "tile_fuse": 0}]
            for opts in TILE_OPTS + extra:
                for mask in ("none", "mod3"):
                    out.append(make_case(len(out) + 1000, shape, hc, dtype, 3, 19, mask, opts, seed=seed))
    return out


@functools.lru_cache(maxsize=2)
def _tile_refs(shape, hc, dtype, seed, mask):
    c = make_case(0, shape, hc, dtype, 3, 19, mask, None, seed=seed)
    inp = make_inputs(c)
    return inp, {path: oracle(c, inp, path) for path in ("batch", "ensemble")}


@pytest.mark.parametrize("case", [c for c in _tile_cases() if c["mask"] == "none"], ids=batch_case_id)
def test_tile_variants_batched_and_ensemble(case, hip_device):
    """dense dL/dtraj, then the t % 3 == 0 mask, T = 19 (not a multiple of any K)"""
    for mask in ("none", "mod3"):
        c = dict(case, mask=mask)
        inp, refs = _tile_refs(c["shape"], c["hc"], c["dtype"], c["seed"], mask)
        check_case(c, hip_device, refs=refs, inp=inp, tag=mask + ": ")


# ---- (b) direct kernels -----------------------------------------------------------------------------------------------------
DIRECT_OPTS = ([{"tile": 0, "vec": 0}, {"tile": 0, "vec": 1}] +
               [{"tile": 0, "fuse_wgrad": f} for f in (0, 1, 2)] +
               [{"tile": 0, "fuse_wgrad": 0, "vec": 1}, {"tile": 0, "fuse_wgrad": 1, "vec": 1}] +
               [{"tile": 0, "lane_x": x} for x in (-1, 2, 3, 5, 6, 7)] +                 # test_direct_2d_lane_modes_bitwise
               [{"tile": 0, "lane_x": 6, "block": 64}, {"tile": 0, "block": 64}, {"tile": 0, "block": 128},
                {"tile": 0, "block": 256, "block_small": 0}] +                            # test_direct_kernel_variants_bitwise
               [{"tile": 0, "bwd_cpl": c} for c in (1, 3)])
#                 shape        dtype       hc
DIRECT_KINDS = [((40, 100), np.float32, 0), ((33, 72), np.float32, 2), ((9, 12), np.float64, 4), ((50, 36), np.float32, 8),
                ((50, 37), np.float32, 0), ((31, 45), np.float64, 3), ((3, 5), np.float32, 16),        # odd widths, extents < 5
                ((9, 12, 64), np.float32, 0), ((6, 33, 40), np.float32, 4), ((3, 8, 16), np.float32, 8),
                ((10, 24, 48), np.float64, 2), ((2, 6, 8), np.float64, 6), ((5, 6, 33), np.float32, 0),
                ((4, 5, 7), np.float64, 5), ((3, 2, 9), np.float32, 8), ((7, 3, 5), np.float32, 4), ((4, 3, 3), np.float64, 2),
                ((3, 4, 5), np.float64, 0),
                # hc = 12: the gradient pass in chunks of four hidden channels with j0 = 4, 8 (the only chunked jc = 4 width)
                ((24, 36), np.float32, 12), ((17, 21), np.float64, 12), ((4, 6, 16), np.float64, 12), ((3, 5, 9), np.float32, 12)]


def _direct_cases():
    out = []
    for k, (shape, dtype, hc) in enumerate(DIRECT_KINDS):
        for opts in DIRECT_OPTS:
            out.append(make_case(len(out) + 3000, shape, hc, dtype, 3, 5, ("none", "random", "top")[k % 3], opts, seed=600 + k))
    # chunks per lane of the direct adjoint kernel (test_direct_adjoint_kernel_chunks_per_lane): live from 512 workgroups per
    # chunk on -- a grid of that test, fused and sweep-only
    for fuse in (2, 0):
        for cpl in (1, 2, 3):
            out.append(make_case(len(out) + 3000, (65, 125, 132), 0, np.float32, 2, 2, "none", {"fuse_wgrad": fuse, "bwd_cpl": cpl},
                                 seed=640))
    return out


@functools.lru_cache(maxsize=2)
def _case_refs(shape, hc, dtype, B, T, mask, seed):
    c = make_case(0, shape, hc, dtype, B, T, mask, None, seed=seed)
    inp = make_inputs(c)
    return inp, {path: oracle(c, inp, path) for path in ("batch", "ensemble")}


@pytest.mark.parametrize("case", _direct_cases(), ids=batch_case_id)
def test_direct_variants_batched_and_ensemble(case, hip_device):
    c = case
    inp, refs = _case_refs(c["shape"], c["hc"], c["dtype"], c["B"], c["T"], c["mask"], c["seed"])
    check_case(c, hip_device, refs=refs, inp=inp)


def _skip_wgrad_cases():
    return [make_case(3900 + k, shape, hc, dtype, 3, 9, "random" if k % 2 else "none", opts, seed=660 + k)
            for k, (shape, dtype, hc, opts) in enumerate([
                ((40, 100), np.float32, 0, {"skip_wgrad": 1}), ((40, 100), np.float32, 8, {"skip_wgrad": 1, "tile": 0}),
                ((64, 96), np.float64, 0, {"skip_wgrad": 1}), ((50, 37), np.float32, 3, {"skip_wgrad": 1}),
                ((6, 33, 40), np.float32, 0, {"skip_wgrad": 1}), ((4, 5, 7), np.float64, 4, {"skip_wgrad": 1})])]


@pytest.mark.parametrize("case", _skip_wgrad_cases(), ids=batch_case_id)
def test_skip_wgrad_batched_and_ensemble(case, hip_device):
    """state and adjoint against the oracle; param_grad comes back as from the unbatched call with the same option: the
    two diffusion coefficients' gradients (the sweep itself reduces them), to reduction round-off of the oracle's, and exact
    zeros wherever the unbatched call leaves zeros"""
    import percnn_amd as pa
    c = case
    inp = make_inputs(c)
    check_case(c, hip_device, inp=inp)
    h0, g = dev_t(inp["h0"], hip_device), dev_t(inp["g"], hip_device)
    if inp["mask"] is not None:
        g[[not m for m in inp["mask"]]] = 0
    for path, P in (("batch", inp["P"]), ("ensemble", inp["Pe"])):
        rows_o = oracle(c, inp, path)[2]
        Pd = dev_t(P, hip_device)
        fwd, bwd = ((pa.pi_rollout_batched, batch_rollout_bwd) if path == "batch" else (pa.pi_rollout_ensemble, ensemble_rollout_bwd))
        traj = fwd(h0, Pd, c["T"], c["options"]).contiguous()
        _, pg = bwd(traj, g, Pd, c["hc"], c["shape"], c["B"], c["T"], inp["mask"], c["options"])
        singles = []
        for b in range(c["B"]):
            Pb = Pd if path == "batch" else Pd[b].contiguous()
            singles.append(single_rollout_bwd(traj[:, b].contiguous(), g[:, b].contiguous(), Pb, c["hc"], c["shape"], c["T"],
                                              inp["mask"], c["options"])[1])
        singles = torch.stack(singles)
        assert not singles[:, 0].any() and not singles[:, 3:].any() and singles[:, 1:3].all()   # what the unbatched call returns
        got = pg.cpu().numpy().reshape(-1, pg.shape[-1])
        want = rows_o.sum(0, keepdims=True) if path == "batch" else rows_o
        assert not got[:, 0].any() and not got[:, 3:].any(), path
        for b in range(got.shape[0]):
            assert grad_err(got[b, 1:3], want[b, 1:3]) < GRAD_TOL[c["dtype"]], (path, b)
            assert grad_err(singles[b].cpu().numpy()[1:3] if path == "ensemble" else singles.sum(0).cpu().numpy()[1:3],
                            want[b, 1:3]) < GRAD_TOL[c["dtype"]], (path, b, "unbatched")


# ---- (c) the B-dependent tile / direct switch ---------------------------------------------------------------------------------
SWITCH_SHAPE, SWITCH_T, SWITCH_BMAX = (256, 256), 5, 48
# B * n against 5 << 18 (sweep) and 3 << 20 (forward): 19 -> both on tiles; 20, 47 -> forward on tiles, sweep on the direct
# kernels; 48 -> both direct
SWITCH_B = [19, 20, 47, 48]


def _switch_cases():
    return [make_case(4000 + i, SWITCH_SHAPE, 0, np.float32, B, SWITCH_T, "random" if B == 20 and opts is None else "none", opts, seed=700)
            for i, (B, opts) in enumerate((B, o) for B in SWITCH_B for o in (None, {"tile": 0}, {"tile": 2}))]


@functools.lru_cache(maxsize=2)
def _switch_refs(mask_kind):
    """the oracle once per sample, for the largest B: the first B samples are the inputs of a smaller batch"""
    c = make_case(0, SWITCH_SHAPE, 0, np.float32, SWITCH_BMAX, SWITCH_T, mask_kind, None, seed=700)
    inp = make_inputs(c)
    return inp, {path: oracle(c, inp, path) for path in ("batch", "ensemble")}


def test_switch_thresholds_are_where_the_cases_assume():
    """restates the limits of batch_tile (csrc/pi_abi.hip, the source of truth: edit the two together)"""
    n = SWITCH_SHAPE[0] * SWITCH_SHAPE[1]
    assert 19 * n < (5 << 18) <= 20 * n and 47 * n < (3 << 20) <= 48 * n


@pytest.mark.parametrize("case", _switch_cases(), ids=batch_case_id)
def test_batch_size_switches_tiles_to_direct(case, hip_device):
    c, B = case, case["B"]
    inp, refs = _switch_refs(c["mask"])
    sub = {"h0": inp["h0"][:B], "P": inp["P"], "Pe": inp["Pe"][:B], "g": np.ascontiguousarray(inp["g"][:, :B]), "mask": inp["mask"]}
    check_case(c, hip_device, refs={p: (r[0][:, :B], r[1][:B], r[2][:B]) for p, r in refs.items()}, inp=sub)


# ---- (d) step adjoint with an injected gradient ---------------------------------------------------------------------------------
STEP_SHAPES = [(5, 7), (2, 2), (16, 32), (64, 6), (6, 10, 9), (2, 3, 4), (8, 8, 16)]       # test_step_backward_vs_c_oracle


def _step_cases():
    return [make_case(5000 + i, shape, hc, dtype, 3, 1, "none", None)
            for i, (shape, dtype, hc) in enumerate((s, d, h) for s in STEP_SHAPES for d in (np.float32, np.float64)
                                                   for h in (0, 2, 3, 8, 16))]


@pytest.mark.parametrize("case", _step_cases(), ids=batch_case_id)
def test_step_backward_with_inject_vs_c_oracle(case, hip_device):
    """inputs and bounds of test_step_backward_vs_c_oracle (adjoint state bit-identical, reductions 2e-5 / 1e-12), three samples"""
    shape, hc, dtype, B = case["shape"], case["hc"], case["dtype"].type, case["B"]
    rs = np.random.RandomState(7)
    P = random_block(hc, len(shape), dtype, seed=hc)
    Pe = ensemble_blocks(hc, len(shape), dtype, B, hc, scale=0.5)
    h, G, inj = (rs.uniform(-1, 1, (B, 2) + shape).astype(dtype) for _ in range(3))
    tol = 2e-5 if dtype == np.float32 else 1e-12
    hd, Gd, injd = (dev_t(a, hip_device) for a in (h, G, inj))
    for use_inj in (False, True):
        for path, blocks, f in (("batch", P, batch_step_bwd), ("ensemble", Pe, ensemble_step_bwd)):
            gi, pg = f(hd, Gd, dev_t(blocks, hip_device), hc, shape, B, g_inject=injd if use_inj else None)
            gi, pg = gi.cpu().numpy(), pg.cpu().numpy()
            rows = []
            for b in range(B):
                gi_o, pg_o = o_step_bwd(h[b], G[b], inj[b] if use_inj else None, blocks if path == "batch" else blocks[b])
                assert np.array_equal(gi[b], gi_o), (path, use_inj, b)
                rows.append(np.asarray(pg_o, dtype=np.float64))
                if path == "ensemble":
                    assert rel_l2(pg[b], pg_o) < tol, (path, use_inj, b)
            if path == "batch":
                assert rel_l2(pg, np.sum(rows, axis=0)) < tol, (path, use_inj)


# ---- (e) base pointers off 16 bytes -----------------------------------------------------------------------------------------------
def _misaligned_cases():
    kinds = [((64, 96), np.float32, 0), ((40, 100), np.float32, 8), ((64, 96), np.float64, 0), ((9, 12, 64), np.float32, 0),
             ((3, 8, 16), np.float64, 4), ((128, 256), np.float32, 2)]
    return [make_case(6000 + 4 * k + j, shape, hc, dtype, 3, 9, "random" if k % 2 else "none", {"which": which}, seed=800 + k)
            for k, (shape, dtype, hc) in enumerate(kinds) for j, which in enumerate(("all", "traj", "g_traj", "g_h0"))]


def _carve(t, off):
    """a copy of t that starts `off` elements into a larger buffer"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


@pytest.mark.parametrize("case", _misaligned_cases(), ids=lambda c: batch_case_id(dict(c, options=None)) + "-" + c["options"]["which"])
def test_misaligned_bases_fall_back_to_scalar_kernels(case, hip_device):
    """traj, dL/dtraj and dL/dh0 one element off a 16-byte boundary (all three, or one at a time): the library declines the tile
    kernels and the 16-byte lanes for the launches that touch such a pointer, and the results stay the oracle's.
    (include/percnn_pi.h asks 16 bytes of the workspace alone, which stays aligned here.)"""
    c, which = dict(case, options=None), case["options"]["which"]
    inp = make_inputs(c)
    shape, hc, B, T, mask = c["shape"], c["hc"], c["B"], c["T"], inp["mask"]
    off = {n: 1 if which in ("all", n) else 0 for n in ("traj", "g_traj", "g_h0")}
    g = inp["g"].copy()
    if mask is not None:
        g[[not m for m in mask]] = np.nan
    for path in ("batch", "ensemble"):
        traj_o, g0_o, rows_o = oracle(c, inp, path)
        assert np.isfinite(traj_o).all() and np.isfinite(g0_o).all() and np.isfinite(rows_o).all()
        Pd = dev_t(inp["P"] if path == "batch" else inp["Pe"], hip_device)
        fwd, bwd = (batch_rollout_fwd_, batch_rollout_bwd) if path == "batch" else (ensemble_rollout_fwd_, ensemble_rollout_bwd)
        start = np.zeros_like(traj_o)
        start[0] = inp["h0"]
        traj = _carve(dev_t(start, hip_device), off["traj"])
        fwd(traj, Pd, hc, shape, B, T)
        assert np.array_equal(traj.cpu().numpy(), traj_o), path
        gd = _carve(dev_t(g, hip_device), off["g_traj"])
        g_h0 = _carve(torch.zeros((B, 2) + shape, dtype=traj.dtype, device=hip_device), off["g_h0"])
        _, pg = bwd(traj, gd, Pd, hc, shape, B, T, mask, None, g_h0=g_h0)
        assert np.array_equal(g_h0.cpu().numpy(), g0_o), path
        want = rows_o.sum(0) if path == "batch" else rows_o
        for got_r, want_r in zip(np.atleast_2d(pg.cpu().numpy()), np.atleast_2d(want)):
            assert grad_err(got_r, want_r) < GRAD_TOL[c["dtype"]], path


# ---- (f) partial-row bounds of the ensemble ---------------------------------------------------------------------------------------
ROWS_CASE = make_case(7000, (128, 128), 8, np.float32, 8, 260, "none", None)


def test_rows_case_makes_the_wgrad_blocks_cap_bind():
    """ens_wgrad_blocks: ceil(t_top * B * (n / vec) / 4096) workgroups before the cap -- above 2048, the largest `wgrad_blocks`
    (restates csrc/pi_abi.hip, the source of truth: edit the two together)"""
    c = ROWS_CASE
    total = c["T"] * c["B"] * (c["shape"][0] * c["shape"][1] // 4)
    assert (total + 4095) // 4096 > 2048


def test_ensemble_partial_rows_do_not_mix(hip_device):
    """the gradient pass of the ensemble with `wgrad_blocks` at its largest value (2048: 256 workgroups, 512 partial rows per
    sample), at 1 (one workgroup per sample walks everything) and at the default: every row within the bound of the oracle's;
    with one sample's dL/dtraj zeroed every other row is bit-identical and that sample's row exactly zero"""
    import percnn_amd as pa
    c = ROWS_CASE
    inp = make_inputs(c)
    shape, hc, B, T = c["shape"], c["hc"], c["B"], c["T"]
    traj_o, g0_o, rows_o = oracle(c, inp, "ensemble")
    assert np.isfinite(traj_o).all() and np.isfinite(rows_o).all()
    Pd, h0, g = dev_t(inp["Pe"], hip_device), dev_t(inp["h0"], hip_device), dev_t(inp["g"], hip_device)
    traj = pa.pi_rollout_ensemble(h0, Pd, T).contiguous()
    assert np.array_equal(traj.cpu().numpy(), traj_o)
    gz = g.clone()
    gz[:, 5] = 0
    for opts in ({"wgrad_blocks": 2048}, {"wgrad_blocks": 1}, None):
        g0, pg = ensemble_rollout_bwd(traj, g, Pd, hc, shape, B, T, None, opts)
        assert np.array_equal(g0.cpu().numpy(), g0_o), opts
        for b in range(B):
            err = grad_err(pg[b].cpu().numpy(), rows_o[b])
            print(f"{opts}: row {b} rel-L2 {err:.3g}")
            assert err < GRAD_TOL[c["dtype"]], (opts, b)
        g0z, pgz = ensemble_rollout_bwd(traj, gz, Pd, hc, shape, B, T, None, opts)
        for b in range(B):
            if b == 5:
                assert not pgz[b].any() and not g0z[b].any(), opts
            else:
                assert torch.equal(pgz[b], pg[b]) and torch.equal(g0z[b], g0[b]), (opts, b)


# ---- (g) many samples, tiny grid --------------------------------------------------------------------------------------------------
def _many_cases():
    return [make_case(8000 + i, shape, hc, dtype, 513, 3, ("none", "random")[i % 2], None)
            for i, (shape, hc, dtype) in enumerate((s, h, d) for s in ((4, 4), (5, 7), (2, 3, 4)) for h in (0, 3)
                                                   for d in (np.float32, np.float64))]


@pytest.mark.parametrize("case", _many_cases(), ids=batch_case_id)
def test_many_samples_on_a_tiny_grid(case, hip_device):
    """B = 513 samples in grid y, one workgroup each (the gradient workspace is B * 4096 * np doubles: 0.6 GB for the polynomial
    block, 1.3 GB for hc = 3)"""
    check_case(case, hip_device)


# ---- (h) degenerate calls -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype,hc", [((40, 100), np.float32, 0), ((33, 37), np.float32, 8), ((6, 10, 9), np.float64, 3)])
def test_degenerate_calls(shape, dtype, hc, hip_device):
    """B = 1 through the ensemble and batched entry points (P [1,np] / [np]) is the unbatched call; T = 0 returns the initial
    states, and its backward dL/dtraj[0]"""
    import percnn_amd as pa
    T = 6
    c = make_case(9000 + hc, shape, hc, dtype, 1, T, "none", None)
    inp = make_inputs(c)
    h0, g = dev_t(inp["h0"], hip_device), dev_t(inp["g"], hip_device)
    for path, P in (("batch", inp["P"]), ("ensemble", inp["Pe"])):
        traj_o, g0_o, rows_o = oracle(c, inp, path)
        Pd = dev_t(P, hip_device)
        P1 = Pd.reshape(-1)
        fwd, bwd = ((pa.pi_rollout_batched, batch_rollout_bwd) if path == "batch" else (pa.pi_rollout_ensemble, ensemble_rollout_bwd))
        traj = fwd(h0, Pd, T).contiguous()
        assert traj.shape == (T + 1, 1, 2) + shape
        assert np.array_equal(traj.cpu().numpy(), traj_o), path
        assert torch.equal(traj[:, 0], pa.pi_rollout(h0, P1, T)), path
        g0, pg = bwd(traj, g, Pd, hc, shape, 1, T)
        s0, sp = single_rollout_bwd(traj[:, 0].contiguous(), g[:, 0].contiguous(), P1, hc, shape, T)
        assert np.array_equal(g0.cpu().numpy(), g0_o) and torch.equal(g0[0], s0), path
        assert torch.equal(pg.reshape(-1), sp), path
        assert grad_err(pg.cpu().numpy().reshape(-1), rows_o[0]) < GRAD_TOL[c["dtype"]], path
    # T = 0, three samples
    c0 = make_case(9100 + hc, shape, hc, dtype, 3, 0, "none", None)
    inp = make_inputs(c0)
    h0, g = dev_t(inp["h0"], hip_device), dev_t(inp["g"], hip_device)
    for path, P in (("batch", inp["P"]), ("ensemble", inp["Pe"])):
        Pd = dev_t(P, hip_device)
        fwd, bwd = ((pa.pi_rollout_batched, batch_rollout_bwd) if path == "batch" else (pa.pi_rollout_ensemble, ensemble_rollout_bwd))
        traj = fwd(h0, Pd, 0).contiguous()
        assert traj.shape == (1, 3, 2) + shape and torch.equal(traj[0], h0), path
        assert np.array_equal(traj.cpu().numpy(), o_batch_reference(inp["h0"], P, 0)[0]), path
        g0, pg = bwd(traj, g, Pd, hc, shape, 3, 0)
        assert torch.equal(g0, g[0]) and not pg.any(), path


def all_cases():
    """every case whose inputs come from util.make_inputs (the coverage test and the oracle's finiteness pass read this)"""
    return (_tile_cases() + _direct_cases() + _skip_wgrad_cases() + _switch_cases() + [dict(c, options=None) for c in _misaligned_cases()] +
            [ROWS_CASE] + _many_cases())
