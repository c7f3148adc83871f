"""Batched and ensemble 3D calls on the sample flavours of the brick kernels (csrc/pi_brick3d.h; dispatch: csrc/pi_abi.hip "batch on
bricks"), against the plain-C oracle looped over the samples.  Every case first asks percnn_pi_debug_batch_plan -- the launchers'
own rule -- that its options put the launches on bricks: the bit-identity below is then a statement about those kernels.

Options travel per call, never through pa.set_option."""
import functools

import numpy as np
import pytest
import torch

from percnn_amd import _lib
from util import (GRAD_TOL, batch_case_id, batch_rollout_bwd, batch_rollout_fwd_, batch_step_bwd, check_case, ensemble_blocks,
                  ensemble_rollout_bwd, ensemble_rollout_fwd_, ensemble_step_bwd, grad_err, make_case, make_inputs, o_step_bwd, o_step_fwd,
                  oracle, random_block, rel_l2)

pytestmark = pytest.mark.gpu


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def assert_on_bricks(c, options=None, adjoint=True):
    """forward on bricks; the adjoint too, except for factored blocks whose gradients are all reduced inside the sweep launches
    (fuse_wgrad = 1: the direct kernel's job, as unbatched)"""
    options = c["options"] if options is None else options
    plan = _lib.batch_plan(c["hc"], c["shape"], c["dtype"].itemsize, c["B"], options)
    assert plan["fwd"] == "brick3d", plan
    if adjoint:
        direct_adj = c["hc"] != 0 and options.get("fuse_wgrad") == 1
        assert plan["bwd"] == ("direct" if direct_adj else "brick3d"), plan
    want_rz = options.get("brick_rz", 1) if c["hc"] == 0 else 1
    assert plan["fwd_planes_per_pass"] == want_rz, plan
    return plan


# ---- (a) oracle parity: the smallest shapes that exercise each brick hazard (test_brick3d_bitwise) ----------------------------------
POLY_KINDS = [
    ((9, 12, 64), np.float32),      # baseline: one brick of 192 chunks per plane
    ((6, 33, 40), np.float32),      # ragged plane of 330 chunks: a partial second brick, rows straddling bricks
    ((3, 8, 16), np.float32),       # plane smaller than a brick; odd n0: partial last plane group with two planes per brick
    ((5, 2, 256), np.float32),      # 64-chunk rows, two rows
    ((8, 32, 64), np.float32),      # nblk % 8 == 0: XCD regions split in z and y
    ((16, 64, 32), np.float32),
    ((10, 24, 48), np.float64),
    ((2, 6, 8), np.float64),
    ((7, 5, 128), np.float64),
]
FACTORED_KINDS = [((9, 12, 64), np.float32, 2), ((6, 33, 40), np.float32, 8), ((5, 9, 24), np.float64, 4), ((4, 7, 20), np.float32, 3)]
POLY_OPTS = [{"brick3d": 2, "brick_rz": 1}, {"brick3d": 2, "brick_rz": 2}, {"brick3d": 2, "brick_rz": 1, "brick_xcd": 0, "brick_wgs": 1},
             {"brick3d": 2, "fuse_wgrad": 0}, {"brick3d": 2, "fuse_wgrad": 1}, {"brick3d": 2, "fuse_wgrad": 2}]
FACTORED_OPTS = [o for o in POLY_OPTS if o.get("brick_rz") != 2]
MASKS = ("none", "random", "top")


def _parity_cases():
    out = []
    for k, (shape, dtype) in enumerate(POLY_KINDS):
        out += [make_case(13000 + len(out) + i, shape, 0, dtype, 3, 5, MASKS[k % 3], o, seed=1300 + k) for i, o in enumerate(POLY_OPTS)]
    for k, (shape, dtype, hc) in enumerate(FACTORED_KINDS):
        out += [make_case(13000 + len(out) + i, shape, hc, dtype, 3, 5, MASKS[k % 3], o, seed=1320 + k)
                for i, o in enumerate(FACTORED_OPTS)]
    return out


@functools.lru_cache(maxsize=2)
def _case_refs(shape, hc, dtype, B, T, mask, seed):
    c = make_case(0, shape, hc, dtype, B, T, mask, None, seed=seed)
    inp = make_inputs(c)
    return inp, {path: oracle(c, inp, path) for path in ("batch", "ensemble")}


@pytest.mark.parametrize("case", _parity_cases(), ids=batch_case_id)
def test_brick_batches_match_the_oracle(case, hip_device):
    c = case
    assert_on_bricks(c)
    inp, refs = _case_refs(c["shape"], c["hc"], c["dtype"], c["B"], c["T"], c["mask"], c["seed"])
    check_case(c, hip_device, refs=refs, inp=inp)


# ---- (b) many samples: the adjoint grid of a sample is the resident workgroups spread over the batch --------------------------------
# (3,8,16): three one-brick workgroups per sample.  (9,12,64) with one workgroup per CU: nine bricks per sample and room for
# CUs / 65 workgroups each, so every workgroup walks several bricks and owns one partial row per (sample, workgroup)
MANY_CASES = [make_case(13500, (3, 8, 16), 0, np.float32, 65, 3, "none", {"brick3d": 2}),
              make_case(13501, (9, 12, 64), 0, np.float32, 65, 3, "none", {"brick3d": 2, "brick_wgs": 1})]


@pytest.mark.parametrize("case", MANY_CASES, ids=batch_case_id)
def test_many_samples_on_bricks(case, hip_device):
    assert_on_bricks(case)
    check_case(case, hip_device)


# ---- (c) one-step entry points ------------------------------------------------------------------------------------------------------
STEP_KINDS = [((6, 33, 40), np.float32), ((10, 24, 48), np.float64)]
STEP_OPTS = {"brick3d": 2}


@pytest.mark.parametrize("shape,dtype", STEP_KINDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name)
@pytest.mark.parametrize("hc", [0, 8])
def test_step_forward_on_bricks(shape, dtype, hc, hip_device):
    import percnn_amd as pa
    B = 3
    assert_on_bricks(make_case(0, shape, hc, dtype, B, 1), STEP_OPTS, adjoint=False)
    rs = np.random.RandomState(11)
    P = random_block(hc, 3, dtype, seed=hc)
    Pe = ensemble_blocks(hc, 3, dtype, B, hc, scale=0.5)
    h = rs.uniform(-1, 1, (B, 2) + shape).astype(dtype)
    hd = dev_t(h, hip_device)
    for path, blocks, f in (("batch", P, pa.pi_step_batched), ("ensemble", Pe, pa.pi_step_ensemble)):
        got = f(hd, dev_t(blocks, hip_device), STEP_OPTS).cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[b], o_step_fwd(h[b], blocks if path == "batch" else blocks[b])), (path, b)


@pytest.mark.parametrize("shape,dtype", STEP_KINDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name)
def test_step_backward_on_bricks(shape, dtype, hip_device):
    """inputs and bounds of test_step_backward_with_inject_vs_c_oracle (adjoint state bit-identical, reductions 2e-5 / 1e-12).  The
    step adjoint reduces every gradient in its launch, which bricks do for pre-contracted blocks: hc = 0."""
    hc, B = 0, 3
    assert_on_bricks(make_case(0, shape, hc, dtype, B, 1), dict(STEP_OPTS, fuse_wgrad=1))
    rs = np.random.RandomState(7)
    P = random_block(hc, 3, dtype, seed=hc)
    Pe = ensemble_blocks(hc, 3, dtype, B, hc, scale=0.5)
    h, G, inj = (rs.uniform(-1, 1, (B, 2) + shape).astype(dtype) for _ in range(3))
    tol = 2e-5 if dtype == np.float32 else 1e-12
    hd, Gd, injd = (dev_t(a, hip_device) for a in (h, G, inj))
    for use_inj in (False, True):
        for path, blocks, f in (("batch", P, batch_step_bwd), ("ensemble", Pe, ensemble_step_bwd)):
            gi, pg = f(hd, Gd, dev_t(blocks, hip_device), hc, shape, B, g_inject=injd if use_inj else None, options=STEP_OPTS)
            gi, pg = gi.cpu().numpy(), pg.cpu().numpy()
            rows = []
            for b in range(B):
                gi_o, pg_o = o_step_bwd(h[b], G[b], inj[b] if use_inj else None, blocks if path == "batch" else blocks[b])
                assert np.array_equal(gi[b], gi_o), (path, use_inj, b)
                rows.append(np.asarray(pg_o, dtype=np.float64))
                if path == "ensemble":
                    err = rel_l2(pg[b], pg_o)
                    print(f"{path} inject={use_inj} row {b}: rel-L2 {err:.3g}")
                    assert err < tol, (path, use_inj, b)
            if path == "batch":
                err = rel_l2(pg, np.sum(rows, axis=0))
                print(f"{path} inject={use_inj}: rel-L2 {err:.3g}")
                assert err < tol, (path, use_inj)


# ---- (d) loss forms inside the sweep: bricks against the direct kernels -------------------------------------------------------------
@pytest.mark.parametrize("path", ["batch", "ensemble"])
@pytest.mark.parametrize("with_target", [False, True], ids=["no_target", "target"])
@pytest.mark.parametrize("shape,dtype", [((9, 12, 64), np.float32), ((10, 24, 48), np.float64)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name)
def test_loss_forms_on_bricks_equal_the_direct_kernels(shape, dtype, with_target, path, hip_device):
    import percnn_amd as pa
    B, T, frames = 3, 5, [0, 2, 5]
    c = make_case(13700, shape, 0, dtype, B, T, "none", {"brick3d": 2})
    assert_on_bricks(c)
    assert _lib.batch_plan(0, shape, c["dtype"].itemsize, B, {"brick3d": 0})["bwd"] == "direct"
    inp = make_inputs(c)
    rs = np.random.RandomState(77)
    target = dev_t(rs.uniform(0, 1, (T + 1, B, 2) + shape).astype(dtype), hip_device) if with_target else None
    op = pa.pi_rollout_sqerr_batched if path == "batch" else pa.pi_rollout_sqerr_ensemble
    blocks = inp["P"] if path == "batch" else inp["Pe"]

    def run(brick3d, upstream):
        h0 = dev_t(inp["h0"], hip_device).requires_grad_(True)
        P = dev_t(blocks, hip_device).requires_grad_(True)
        loss, _ = op(h0, P, T, target, frames, "mean", {"brick3d": brick3d})
        loss.backward(torch.tensor(upstream, dtype=loss.dtype, device=hip_device))
        return loss.detach(), h0.grad, P.grad

    for upstream in ([1.0, 1.0, 1.0], [1.0, 0.0, 2.0]):
        lb, hb, pb = run(2, upstream)
        ld, hd, pd = run(0, upstream)
        assert torch.equal(lb, ld) and bool(torch.isfinite(lb).all())
        assert torch.equal(hb, hd), "dL/dh0: bricks against the direct kernels"
        assert float(hb.abs().max()) > 0
        pbn, pdn = np.atleast_2d(pb.cpu().numpy()), np.atleast_2d(pd.cpu().numpy())
        for b, (r_b, r_d) in enumerate(zip(pbn, pdn)):
            if upstream[1] == 0.0 and path == "ensemble" and b == 1:
                continue
            err = grad_err(r_b, r_d)
            print(f"{path} upstream {upstream} row {b}: rel-L2 {err:.3g}")
            assert err < GRAD_TOL[c["dtype"]], (upstream, b, err)
        if upstream[1] == 0.0:
            assert not hb[1].any(), "sample 1 has a zero upstream gradient"
            if path == "ensemble":
                assert not pb[1].any(), "gradient row of sample 1"


# ---- (e) base pointer off 16 bytes: the plan for aligned buffers says bricks, the call must decline them ----------------------------
def _carve(t, off):
    """a copy of t that starts `off` elements into a larger buffer"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


def test_misaligned_trajectory_falls_back_from_bricks(hip_device):
    opts = {"brick3d": 2}
    c = make_case(13800, (9, 12, 64), 0, np.float32, 3, 5, "none", opts)
    assert_on_bricks(c)
    inp = make_inputs(c)
    shape, hc, B, T = c["shape"], c["hc"], c["B"], c["T"]
    for path in ("batch", "ensemble"):
        traj_o, g0_o, rows_o = oracle(c, inp, path)
        assert np.isfinite(traj_o).all() and np.isfinite(g0_o).all() and np.isfinite(rows_o).all()
        Pd = dev_t(inp["P"] if path == "batch" else inp["Pe"], hip_device)
        fwd, bwd = (batch_rollout_fwd_, batch_rollout_bwd) if path == "batch" else (ensemble_rollout_fwd_, ensemble_rollout_bwd)
        start = np.zeros_like(traj_o)
        start[0] = inp["h0"]
        traj = _carve(dev_t(start, hip_device), 1)
        fwd(traj, Pd, hc, shape, B, T, opts)
        assert np.array_equal(traj.cpu().numpy(), traj_o), path
        g_h0, pg = bwd(traj, dev_t(inp["g"], hip_device), Pd, hc, shape, B, T, None, opts)
        assert np.array_equal(g_h0.cpu().numpy(), g0_o), path
        want = rows_o.sum(0) if path == "batch" else rows_o
        for got_r, want_r in zip(np.atleast_2d(pg.cpu().numpy()), np.atleast_2d(want)):
            assert grad_err(got_r, want_r) < GRAD_TOL[c["dtype"]], path
