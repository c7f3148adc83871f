"""GPU: the per-sample squared-error loss on sparse observations, differentiated inside the batched / ensemble sweep
(percnn_pi_{batch,ensemble}_rollout_bwd_obs_sqerr_*, percnn_pi_batch_traj_obs_sqerr_*, pa.pi_rollout_obs_sqerr_{batched,ensemble},
RCNN.sample_losses(space_stride > 1)).  The loss lives on the lattice x_d % s_d == 0 of the selected frames; the target is compact
in time and space.  References of every sweep family: the batched / ensemble sweep on the gradient materialised by tensor ops
(dL/dh0 equal, gradients MAT_TOL = 2e-5 / 1e-11 rel-L2: the same kernels, the injected values formed elsewhere), the plain-C
oracle looped over the samples (trajectory and dL/dh0 equal, gradient rows util.GRAD_TOL), float64 tensor operations for the
loss value (1e-6 relative), and the one-sample call for sample independence."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from observed_loss_util import (MANY_CASE, MISALIGNED_CASE, PATHS, TARGETS, compact_shape, compact_target, factors, lattice,
                                materialised_obs_gradient, mean_weight, obs_inputs, obs_losses_f64, obs_pairs, strides_of,
                                sweep_cases)
from util import (GRAD_TOL, batch_case_id, batch_rollout_bwd, block_of, ensemble_rollout_bwd, grad_err, make_case,
                  o_batch_reference, rel_l2)

pytestmark = pytest.mark.gpu

MAT_TOL = {np.dtype("float32"): 2e-5, np.dtype("float64"): 1e-11}


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _mask(T, t_idx):
    return None if len(t_idx) == T + 1 else [t in t_idx for t in range(T + 1)]


def _fwd(path):
    import percnn_amd as pa
    return pa.pi_rollout_batched if path == "batch" else pa.pi_rollout_ensemble


def _mat_bwd(path):
    return batch_rollout_bwd if path == "batch" else ensemble_rollout_bwd


def _rows_close(tag, what, got, want, tol, err=rel_l2):
    for b, (got_r, want_r) in enumerate(zip(np.atleast_2d(got), np.atleast_2d(want))):
        e = err(got_r, want_r) if np.any(want_r) else float(np.abs(got_r).max())
        print(f"{tag}: gradient row {b} vs {what} rel-L2 {e:.3g}")
        assert e < tol, (tag, what, b, e)


def _check_config(c, inp, path, with_target, t_idx, strides, dev, traj, oracle=True, singles=True):
    """one (path, target, frames, strides) of a case against the references; -> nothing, asserts"""
    from percnn_amd import functional as F_pi
    shape, hc, B, T, opts = c["shape"], c["hc"], c["B"], c["T"], c["options"]
    strides = strides_of(strides, len(shape))
    tag = (batch_case_id(c), path, with_target, tuple(t_idx), strides)
    Pn = block_of(inp, path)
    Pd = dev_t(Pn, dev)
    target = dev_t(compact_target(c, len(t_idx), strides), dev) if with_target else None
    mask = _mask(T, t_idx)
    w = mean_weight(len(t_idx), shape, strides)
    fac = factors(B, traj.dtype, dev)
    # 1. loss value, per sample
    want = obs_losses_f64(traj, target, t_idx, strides, w)
    got = F_pi.traj_obs_sqerr_batched(traj, target, mask, strides, w)
    assert got.shape == (B,) and got.dtype == traj.dtype
    for b in range(B):
        print(f"{tag}: loss[{b}] {float(got[b]):.9g} want {float(want[b]):.9g}")
        assert abs(float(got[b]) - float(want[b])) <= 1e-6 * abs(float(want[b])) + 1e-30, (tag, b)
    assert torch.equal(F_pi.traj_obs_sqerr_batched(traj, target, mask, strides, w), got), (tag, "loss run to run")
    # the sweep
    g0, pg = F_pi.rollout_bwd_obs_sqerr_batched(traj, Pd, target, mask, strides, 2.0 * w, fac, options=opts)
    g0b, pgb = F_pi.rollout_bwd_obs_sqerr_batched(traj, Pd, target, mask, strides, 2.0 * w, fac, options=opts)
    assert torch.equal(g0, g0b) and torch.equal(pg, pgb), (tag, "sweep run to run")
    assert torch.isfinite(g0).all() and torch.isfinite(pg).all(), tag
    # 2. the batched / ensemble sweep on the materialised gradient (torch.equal: a zero may differ in sign)
    g = materialised_obs_gradient(traj, target, t_idx, strides, 2.0 * w, fac).contiguous()
    m0, mpg = _mat_bwd(path)(traj, g, Pd, hc, shape, B, T, mask, opts)
    assert torch.equal(g0, m0), (tag, "materialised dL/dh0", float((g0 - m0).abs().max()))
    _rows_close(tag, "materialised", pg.cpu().numpy(), mpg.cpu().numpy(), MAT_TOL[c["dtype"]])
    # 3. the plain-C oracle looped over the samples, same materialised gradient
    if oracle:
        traj_o, g0_o, rows_o = o_batch_reference(inp["h0"], Pn, T, g.cpu().numpy(), mask)
        assert np.array_equal(traj_o, traj.cpu().numpy()), (tag, "oracle trajectory")
        assert np.isfinite(g0_o).all() and np.isfinite(rows_o).all(), "ill-conditioned input"
        assert np.array_equal(g0.cpu().numpy(), g0_o), (tag, "oracle dL/dh0")
        want_rows = rows_o.sum(0, keepdims=True) if path == "batch" else rows_o
        _rows_close(tag, "oracle", pg.cpu().numpy(), want_rows, GRAD_TOL[c["dtype"]], grad_err)
    # 4. sample b alone through the same entry point with batch = 1
    if singles:
        for b in range(B):
            s0, _ = F_pi.rollout_bwd_obs_sqerr_batched(traj[:, b:b + 1].contiguous(), Pd if path == "batch" else Pd[b:b + 1].contiguous(),
                                                       None if target is None else target[:, b:b + 1].contiguous(), mask, strides,
                                                       2.0 * w, fac[b:b + 1], options=opts, ensemble=path == "ensemble")
            assert torch.equal(g0[b], s0[0]), (tag, "one-sample call", b)


@functools.lru_cache(maxsize=2)
def _inputs(cid):
    c = next(c for c in sweep_cases() if c["id"] == cid)
    return obs_inputs(c)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", sweep_cases(), ids=batch_case_id)
def test_observed_losses_inside_the_sweep(case, path, hip_device):
    """every sweep family x B in {2, 3} x {batched, ensemble} x {target, none} x the five (frames, strides) pairs"""
    c = case
    inp = _inputs(c["id"])
    traj = _fwd(path)(dev_t(inp["h0"], hip_device), dev_t(block_of(inp, path), hip_device), c["T"], c["options"]).contiguous()
    assert torch.isfinite(traj).all()
    for with_target in TARGETS:
        for t_idx, strides in obs_pairs(len(c["shape"])):
            _check_config(c, inp, path, with_target, t_idx, strides, hip_device, traj)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", [0, 8, 12, 14, 16, 18])
def test_unit_strides_are_the_dense_loss_bit_for_bit(k, path, hip_device):
    """all strides 1, every frame: rollout_bwd_sqerr_batched / traj_sqerr_batched bit for bit (tile, direct 2D vector and
    scalar, 3D)"""
    from percnn_amd import functional as F_pi
    c = sweep_cases()[k]
    inp = _inputs(c["id"])
    shape, B, T, opts = c["shape"], c["B"], c["T"], c["options"]
    Pd = dev_t(block_of(inp, path), hip_device)
    traj = _fwd(path)(dev_t(inp["h0"], hip_device), Pd, T, opts).contiguous()
    ones = (1,) * len(shape)
    fac = factors(B, traj.dtype, hip_device)
    w = mean_weight(T + 1, shape, ones)
    for tg in (None, dev_t(compact_target(c, T + 1, ones), hip_device)):
        d0, dpg = F_pi.rollout_bwd_sqerr_batched(traj, Pd, tg, None, 2.0 * w, fac, options=opts)
        g0, pg = F_pi.rollout_bwd_obs_sqerr_batched(traj, Pd, tg, None, ones, 2.0 * w, fac, options=opts)
        assert torch.equal(g0, d0) and torch.equal(pg, dpg), (batch_case_id(c), path)
        assert torch.equal(F_pi.traj_obs_sqerr_batched(traj, tg, None, ones, w), F_pi.traj_sqerr_batched(traj, tg, None, w))


def test_strides_beyond_the_extent_and_many_samples(hip_device):
    """B = 513 samples in grid y on a (2, 3) grid, T = 3: stride 4 leaves a compact frame (1, 1), stride 2 one of (1, 2)"""
    c = MANY_CASE
    inp = obs_inputs(c)
    assert compact_shape(c["shape"], (4, 4)) == (1, 1) and compact_shape(c["shape"], (2, 2)) == (1, 2)
    for path in PATHS:
        traj = _fwd(path)(dev_t(inp["h0"], hip_device), dev_t(block_of(inp, path), hip_device), c["T"]).contiguous()
        _check_config(c, inp, path, True, [0, 1, 2, 3], 4, hip_device, traj, singles=False)
        _check_config(c, inp, path, False, [1, 3], 2, hip_device, traj, oracle=False, singles=False)
        _check_config(c, inp, path, True, [1, 3], 2, hip_device, traj, oracle=False, singles=False)


@pytest.mark.parametrize("shape,dtype,hc,strides", [((40, 100), np.float32, 0, (4, 4)), ((33, 37), np.float32, 8, (3, 3)),
                                                     ((6, 10, 9), np.float64, 3, (1, 3, 2))])
def test_no_steps(shape, dtype, hc, strides, hip_device):
    """T = 0 writes dL/dh0 = a_b * (h0 - target_0) on the lattice and zero off it, and no parameter gradient"""
    from percnn_amd import functional as F_pi
    c0 = make_case(12850 + hc, shape, hc, dtype, 3, 0, "none", None)
    inp = obs_inputs(c0)
    for path in PATHS:
        Pd = dev_t(block_of(inp, path), hip_device)
        traj = _fwd(path)(dev_t(inp["h0"], hip_device), Pd, 0).contiguous()
        fac = factors(3, traj.dtype, hip_device)
        w = mean_weight(1, shape, strides)
        for tg in (None, dev_t(compact_target(c0, 1, strides), hip_device)):
            g0, pg = F_pi.rollout_bwd_obs_sqerr_batched(traj, Pd, tg, None, strides, 2.0 * w, fac)
            want = materialised_obs_gradient(traj, tg, [0], strides, 2.0 * w, fac)[0]
            assert torch.equal(g0, want) and not pg.any(), path
            off = torch.ones_like(g0, dtype=torch.bool)
            off[lattice(strides)] = False
            assert not g0[off].any() and g0[~off].any()
            got = F_pi.traj_obs_sqerr_batched(traj, tg, None, strides, w)
            assert torch.allclose(got.double(), obs_losses_f64(traj, tg, [0], strides, w), rtol=1e-6, atol=0), path


def _carve(t, off):
    """a copy of t that starts `off` elements into a larger buffer"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


def test_target_base_four_bytes_off_sixteen(hip_device):
    """the compact target carved one float off a 16-byte boundary: it is read element-wise, the numbers are the same bits"""
    from percnn_amd import functional as F_pi
    c = MISALIGNED_CASE
    shape, B, T = c["shape"], c["B"], c["T"]
    inp = obs_inputs(c)
    for path in PATHS:
        Pd = dev_t(block_of(inp, path), hip_device)
        traj = _fwd(path)(dev_t(inp["h0"], hip_device), Pd, T).contiguous()
        fac = factors(B, traj.dtype, hip_device)
        for t_idx, strides in (([2, 3, 4, 7], (3, 3)), (list(range(T + 1)), (4, 4)), (list(range(T + 1)), (1, 1))):
            aligned = dev_t(compact_target(c, len(t_idx), strides), hip_device)
            target = _carve(aligned, 1)
            assert aligned.data_ptr() % 16 == 0 and target.data_ptr() % 16 == 4
            mask, w = _mask(T, t_idx), mean_weight(len(t_idx), shape, strides)
            a0, apg = F_pi.rollout_bwd_obs_sqerr_batched(traj, Pd, aligned, mask, strides, 2.0 * w, fac)
            g0, pg = F_pi.rollout_bwd_obs_sqerr_batched(traj, Pd, target, mask, strides, 2.0 * w, fac)
            assert torch.equal(g0, a0) and torch.equal(pg, apg), (path, strides)
            got = F_pi.traj_obs_sqerr_batched(traj, target, mask, strides, w)
            want = obs_losses_f64(traj, aligned, t_idx, strides, w)
            assert torch.allclose(got.double(), want, rtol=1e-6, atol=0), (path, strides)


def test_per_sample_factor_is_not_element_zero(hip_device):
    """the factors of two calls differ in every element but the first: every sample but the first must change"""
    from percnn_amd import functional as F_pi
    for k in (1, 13, 17):                                   # (64, 96) tiles, (48, 72) direct, (12, 16, 64) 3D; B = 3
        c = sweep_cases()[k]
        assert c["B"] == 3
        inp = _inputs(c["id"])
        s = strides_of(2, len(c["shape"]))
        for path in PATHS:
            Pd = dev_t(block_of(inp, path), hip_device)
            traj = _fwd(path)(dev_t(inp["h0"], hip_device), Pd, c["T"], c["options"]).contiguous()
            f1 = torch.tensor([0.5, -1.25, 0.0], dtype=traj.dtype, device=hip_device)
            f2 = torch.tensor([0.5, 2.0, 3.0], dtype=traj.dtype, device=hip_device)
            a0, _ = F_pi.rollout_bwd_obs_sqerr_batched(traj, Pd, None, None, s, 1e-3, f1, options=c["options"])
            b0, _ = F_pi.rollout_bwd_obs_sqerr_batched(traj, Pd, None, None, s, 1e-3, f2, options=c["options"])
            assert torch.equal(a0[0], b0[0]) and not a0[2].any() and b0[2].any() and not torch.equal(a0[1], b0[1]), (k, path)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape,dtype,hc,T,strides", [((40, 100), np.float32, 0, 9, 4), ((6, 10, 9), np.float64, 3, 5, (1, 3, 2))])
def test_operator_equals_the_materialised_autograd_route(shape, dtype, hc, T, strides, path, hip_device):
    """pa.pi_rollout_obs_sqerr_{batched,ensemble}(...)[0] weighted by a random [B] vector and summed, against pi_rollout_* +
    strided slice + tensor-op MSE + backward().  ATen forms dL/dtraj in another order of multiplications than the kernels
    (w_b * 2/N * d against (2/N * w_b) * d), so dL/dh0 is held to the rel-L2 bound of the gradients (MAT_TOL), not to bits."""
    import percnn_amd as pa
    B = 3
    c = make_case(12700 + hc, shape, hc, dtype, B, T, "none", None)
    inp = obs_inputs(c)
    st = strides_of(strides, len(shape))
    wts = dev_t(np.random.RandomState(5).uniform(-1, 1, B).astype(c["dtype"].type), hip_device)
    op = pa.pi_rollout_obs_sqerr_batched if path == "batch" else pa.pi_rollout_obs_sqerr_ensemble
    tol = MAT_TOL[c["dtype"]]
    for t_idx in (list(range(T + 1)), [0, 2, -1], list(range(T + 1))[0:-1:3]):
        sel = [t % (T + 1) for t in t_idx]
        for tg in (None, dev_t(compact_target(c, len(sel), st), hip_device)):
            h0 = dev_t(inp["h0"], hip_device).requires_grad_(True)
            P = dev_t(block_of(inp, path), hip_device).requires_grad_(True)
            traj = _fwd(path)(h0, P, T)
            pred = traj[sel][lattice(st)]
            d = pred if tg is None else pred - tg
            ref = (d ** 2).mean(dim=tuple(i for i in range(d.dim()) if i != 1))
            (ref * wts).sum().backward()
            want_h0, want_P = h0.grad.clone(), P.grad.clone()
            h0.grad = P.grad = None
            loss, tr = op(h0, P, T, tg, t_idx, strides)
            assert loss.shape == (B,) and not tr.requires_grad and torch.equal(tr, traj.detach())
            ref64 = (d.detach().double() ** 2).mean(dim=tuple(i for i in range(d.dim()) if i != 1))
            assert torch.allclose(loss.double(), ref64, rtol=1e-6, atol=0)
            (loss * wts).sum().backward()
            assert h0.grad.shape == h0.shape and P.grad.shape == P.shape
            e = rel_l2(h0.grad.cpu().numpy(), want_h0.cpu().numpy())
            print(f"{(path, shape, t_idx)}: dL/dh0 rel-L2 {e:.3g}")
            assert e < tol, (path, t_idx)
            _rows_close((path, shape, tuple(t_idx)), "autograd", P.grad.cpu().numpy(), want_P.cpu().numpy(), tol)
    tgr = dev_t(compact_target(c, T + 1, st), hip_device).requires_grad_(True)
    loss, _ = op(dev_t(inp["h0"], hip_device).requires_grad_(True), dev_t(block_of(inp, path), hip_device), T, tgr,
                 list(range(T + 1)), strides)
    loss.sum().backward()
    assert tgr.grad is None                                  # the target gets no gradient


def _cells(hip_device, n):
    import percnn_amd as pa
    torch.manual_seed(3)
    cells = []
    for _ in range(n):
        cell = pa.gs2d_cell(8, reaction="factored").to(hip_device)   # (one block kind whatever the poly guard would decide)
        for p in cell.filter_list:
            p.weight.data.mul_(20.0)
        cells.append(cell)
    return cells


def test_sample_losses_of_a_cell_ensemble_are_the_members_observed_loss(hip_device):
    """RCNN.sample_losses(target, slice(0, -1, 3), space_stride=4) on a CellEnsemble of three cells: loss b and every parameter
    gradient of member b equal the member's own RCNN.loss_mse(target[:, b], slice(0, -1, 3), space_stride=4) (1e-6; 2e-5)"""
    import copy
    import percnn_amd as pa
    from percnn_amd import synthetic
    T, shape, tsl, s = 10, (48, 64), slice(0, -1, 3), 4
    cells = _cells(hip_device, 3)
    refs = copy.deepcopy(cells)
    h0 = torch.cat([synthetic.gs_initial_state(shape, seed=k) for k in range(3)]).to(hip_device)
    n = len(list(range(T + 1))[tsl])
    target = torch.rand((n, 3, 2) + compact_shape(shape, (s, s)), device=hip_device)
    wts = torch.tensor([0.5, -1.25, 2.0], device=hip_device)
    ens = pa.CellEnsemble(cells)
    ens.zero_grad()
    hb = h0.clone().requires_grad_(True)
    model = pa.RCNN(ens, step=T, effective_step=list(range(T)), init_state=hb)
    losses = model.sample_losses(target, tsl, space_stride=s)
    assert losses.shape == (3,)
    assert model.last_trajectory.shape == (T + 1, 3, 2) + shape and not model.last_trajectory.requires_grad
    (losses * wts).sum().backward()
    for b in range(3):
        refs[b].zero_grad()
        h1 = h0[b:b + 1].clone().requires_grad_(True)
        m1 = pa.RCNN(refs[b], step=T, effective_step=list(range(T)), init_state=h1)
        one = m1.loss_mse(target[:, b].contiguous(), tsl, space_stride=s)
        assert abs(float(losses[b]) - float(one)) <= 1e-6 * abs(float(one)), b
        (one * wts[b]).backward()
        assert rel_l2(hb.grad[b].cpu().numpy(), h1.grad[0].cpu().numpy()) < 2e-5, b
        got = dict(cells[b].named_parameters())
        seen = 0
        for name, p in refs[b].named_parameters():
            if p.grad is None:
                assert got[name].grad is None or not got[name].grad.any(), name
                continue
            seen += 1
            assert rel_l2(got[name].grad.cpu().numpy(), p.grad.cpu().numpy()) < 2e-5, (b, name)
        assert seen > 0


def test_sample_losses_batched_and_single(hip_device):
    """a batched initial state with one cell, and B = 1 -> [1], against loss_mse(space_stride=4) per sample"""
    import percnn_amd as pa
    from percnn_amd import synthetic
    T, shape, tsl, s = 6, (32, 48), slice(0, -1, 3), 4
    cell = _cells(hip_device, 1)[0]
    h0 = torch.cat([synthetic.gs_initial_state(shape, seed=k) for k in range(2)]).to(hip_device)
    n = len(list(range(T + 1))[tsl])
    target = torch.rand((n, 2, 2) + compact_shape(shape, (s, s)), device=hip_device)
    model = pa.RCNN(cell, step=T, effective_step=list(range(T)), init_state=h0)
    losses = model.sample_losses(target, tsl, space_stride=s)
    assert losses.shape == (2,) and model.last_trajectory.shape == (T + 1, 2, 2) + shape
    cell.zero_grad()
    losses.mean().backward()
    got = {k: p.grad.clone() for k, p in cell.named_parameters() if p.grad is not None}
    cell.zero_grad()
    total = 0
    for b in range(2):
        m1 = pa.RCNN(cell, step=T, effective_step=list(range(T)), init_state=h0[b:b + 1])
        one = m1.loss_mse(target[:, b].contiguous(), tsl, space_stride=s)
        assert abs(float(losses[b]) - float(one)) <= 1e-6 * abs(float(one))
        total = total + one / 2
        l1 = m1.sample_losses(target[:, b:b + 1].contiguous(), tsl, space_stride=s)
        assert l1.shape == (1,) and abs(float(l1[0]) - float(one)) <= 1e-6 * abs(float(one))
    total.backward()
    assert got
    for k, g in got.items():
        assert rel_l2(g.cpu().numpy(), dict(cell.named_parameters())[k].grad.cpu().numpy()) < 2e-5, k


def test_error_paths(hip_device):
    import percnn_amd as pa
    from percnn_amd import _lib
    L = _lib.lib()
    shape = (ctypes.c_int64 * 2)(8, 8)
    B, T, n = 3, 2, 2 * 8 * 8
    buf = torch.zeros((T + 1) * B * n + 64, device=hip_device)
    tr, g0, P = buf.data_ptr(), torch.zeros(B * n, device=hip_device), torch.zeros(B * 36, device=hip_device)
    pg = torch.zeros(B * 36, dtype=torch.float64, device=hip_device)
    nbytes = L.percnn_pi_batch_rollout_bwd_workspace_bytes(0, 2, shape, B, T, 4)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=hip_device)
    out = torch.zeros(B, device=hip_device)
    sws = torch.zeros(L.percnn_pi_batch_traj_sqerr_workspace_bytes(B), dtype=torch.uint8, device=hip_device)
    good, bad = (ctypes.c_int * 2)(3, 2), (ctypes.c_int * 2)(2, 0)
    for kind in ("batch", "ensemble"):
        f = getattr(L, f"percnn_pi_{kind}_rollout_bwd_obs_sqerr_f32")
        ok = lambda **k: f(k.get("traj", tr), None, None, k.get("strides", good), 1.0, None, k.get("g_h0", g0.data_ptr()),
                           k.get("pg", pg.data_ptr()), ws.data_ptr(), k.get("ws_bytes", ws.numel()), k.get("P", P.data_ptr()),
                           k.get("hc", 0), 2, shape, k.get("batch", B), T, k.get("options"), None)
        assert ok(traj=None) == -1 and ok(g_h0=None) == -1 and ok(pg=None) == -1 and ok(P=None) == -1, kind
        assert ok(g_h0=tr) == -1, kind                                   # dL/dh0 would overwrite the trajectory
        assert ok(batch=0) == -1 and ok(batch=65536) == -1 and ok(options=b"tile_k=3") == -1, kind
        assert ok(hc=-1) == -1 and ok(hc=-1, batch=1) == -1, kind
        assert ok(strides=None) == -1 and ok(strides=bad) == -1, kind
        assert ok(ws_bytes=16) == -2, kind
        assert ok() == 0 and ok(batch=1) == 0, kind
    s = L.percnn_pi_batch_traj_obs_sqerr_f32
    args = lambda **k: s(k.get("traj", tr), None, None, T + 1, 2, shape, k.get("strides", good), k.get("batch", B), 1.0,
                         k.get("out", out.data_ptr()), sws.data_ptr(), k.get("ws_bytes", sws.numel()), None)
    assert args(traj=None) == -1 and args(out=None) == -1 and args(out=tr) == -1 and args(batch=0) == -1 and args(batch=65536) == -1
    assert args(strides=None) == -1 and args(strides=bad) == -1
    assert args(ws_bytes=8) == -2 and args() == 0
    torch.cuda.synchronize()
    # the operators
    h = torch.rand(2, 2, 16, 16, device=hip_device)
    blk = torch.zeros(36, device=hip_device)
    with pytest.raises(ValueError, match="no frame selected"):
        pa.pi_rollout_obs_sqerr_batched(h, blk, 3, None, [], 2)
    with pytest.raises(ValueError, match="strictly increasing"):
        pa.pi_rollout_obs_sqerr_batched(h, blk, 3, None, [1, 1], 2)
    with pytest.raises(ValueError, match="target must be"):
        pa.pi_rollout_obs_sqerr_batched(h, blk, 3, torch.zeros(2, 2, 2, 16, 16, device=hip_device), [0, 1], 2)
    with pytest.raises(ValueError, match="one stride per axis"):
        pa.pi_rollout_obs_sqerr_batched(h, blk, 3, None, [0], (2, 2, 2))
    with pytest.raises(ValueError, match=">= 1"):
        pa.pi_rollout_obs_sqerr_batched(h, blk, 3, None, [0], (2, 0))
    with pytest.raises(ValueError, match="one parameter block"):
        pa.pi_rollout_obs_sqerr_batched(h, blk.repeat(2, 1), 3, None, [0], 2)
    with pytest.raises(ValueError, match="per sample"):
        pa.pi_rollout_obs_sqerr_ensemble(h, blk, 3, None, [0], 2)
    # cells without a Pi-block kernel path
    for cell in (pa.Stage3BurgersCell().to(hip_device), pa.Stage1Cell("burgers").to(hip_device)):
        with pytest.raises(ValueError):
            pa.RCNN(cell, step=3, effective_step=[0, 1, 2], init_state=h).sample_losses(space_stride=2)
    # the single-trajectory losses still refuse a batch
    cell = pa.gs2d_cell(8).to(hip_device)
    m = pa.RCNN(cell, step=3, effective_step=[0, 1, 2], init_state=h)
    with pytest.raises(ValueError):
        m.loss_mse(space_stride=2)
    with pytest.raises(ValueError):
        m.observe(slice(None), 2)
    assert m.sample_losses(space_stride=2).shape == (2,)
