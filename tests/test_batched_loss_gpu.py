"""GPU: the squared-error loss per sample of a batch / an ensemble, differentiated inside the sweep
(percnn_pi_{batch,ensemble}_rollout_bwd_sqerr_*, percnn_pi_batch_traj_sqerr_*, pa.pi_rollout_sqerr_{batched,ensemble},
RCNN.sample_losses).  Three references hold every sweep family: the unbatched in-kernel form on each sample alone, the batched /
ensemble sweep on the gradient materialised by tensor ops, and the plain-C oracle looped over the samples.  Tolerances: those of
test_hip_parity.py::test_squared_error_loss_inside_the_sweep (adjoint bit for bit, gradients 2e-5 / 1e-11 rel-L2 against the same
kernels on a materialised gradient, loss value 1e-6) and util.GRAD_TOL against the oracle's reductions (1e-4 / 1e-10)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from batched_loss_util import (MANY_CASE, MISALIGNED_CASE, MODES, PATHS, factors, frame_sets, loss_inputs, materialised_gradient,
                               sample_losses_f64, sweep_cases)
from util import (GRAD_TOL, batch_case_id, batch_rollout_bwd, batch_rollout_fwd_, block_of, ensemble_rollout_bwd,
                  ensemble_rollout_fwd_, grad_err, o_batch_reference, rel_l2)

pytestmark = pytest.mark.gpu

MAT_TOL = {np.dtype("float32"): 2e-5, np.dtype("float64"): 1e-11}


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _weight(T, frames, sample_numel):
    return 1.0 / (((T + 1) if frames is None else len(frames)) * sample_numel)


def _mask(T, frames):
    return None if frames is None else [t in frames for t in range(T + 1)]


def _fwd(path):
    import percnn_amd as pa
    return pa.pi_rollout_batched if path == "batch" else pa.pi_rollout_ensemble


def _mat_bwd(path):
    return batch_rollout_bwd if path == "batch" else ensemble_rollout_bwd


def _check_config(c, inp, path, with_target, frames, dev, traj, oracle=True, singles=True):
    """one (path, mode, frame set) of a case against the three references; -> nothing, asserts"""
    from percnn_amd import functional as F_pi
    shape, hc, B, T, opts = c["shape"], c["hc"], c["B"], c["T"], c["options"]
    tag = (batch_case_id(c), path, with_target, frames)
    Pn = block_of(inp, path)
    Pd = dev_t(Pn, dev)
    target = dev_t(inp["target"], dev) if with_target else None
    mask = _mask(T, frames)
    w = _weight(T, frames, traj[0, 0].numel())
    fac = factors(B, traj.dtype, dev)
    # loss value, per sample
    want = sample_losses_f64(traj, target, frames, w)
    got = F_pi.traj_sqerr_batched(traj, target, mask, w)
    assert got.shape == (B,) and got.dtype == traj.dtype
    for b in range(B):
        print(f"{tag}: loss[{b}] {float(got[b]):.9g} want {float(want[b]):.9g}")
        assert abs(float(got[b]) - float(want[b])) <= 1e-6 * abs(float(want[b])) + 1e-30, (tag, b)
    assert torch.equal(F_pi.traj_sqerr_batched(traj, target, mask, w), got), (tag, "loss run to run")
    # the sweep
    g0, pg = F_pi.rollout_bwd_sqerr_batched(traj, Pd, target, mask, 2.0 * w, fac, options=opts)
    g0b, pgb = F_pi.rollout_bwd_sqerr_batched(traj, Pd, target, mask, 2.0 * w, fac, options=opts)
    assert torch.equal(g0, g0b) and torch.equal(pg, pgb), (tag, "sweep run to run")
    assert torch.isfinite(g0).all() and torch.isfinite(pg).all(), tag
    # (1) the unbatched in-kernel form on each sample alone, with its factor
    if singles:
        for b in range(B):
            s0, _ = F_pi.rollout_bwd_sqerr(traj[:, b].contiguous(), Pd if path == "batch" else Pd[b].contiguous(),
                                           None if target is None else target[:, b].contiguous(), mask, 2.0 * w,
                                           dev_scale=fac[b:b + 1], options=opts)
            assert torch.equal(g0[b], s0), (tag, "unbatched sample", b)
    # (2) the batched / ensemble sweep on the materialised gradient
    g = materialised_gradient(traj, target, 2.0 * w, fac).contiguous()
    m0, mpg = _mat_bwd(path)(traj, g, Pd, hc, shape, B, T, mask, opts)
    assert torch.equal(g0, m0), (tag, "materialised dL/dh0")
    tol = MAT_TOL[c["dtype"]]
    for got_r, want_r in zip(np.atleast_2d(pg.cpu().numpy()), np.atleast_2d(mpg.cpu().numpy())):
        err = rel_l2(got_r, want_r) if np.any(want_r) else float(np.abs(got_r).max())
        print(f"{tag}: gradient vs materialised rel-L2 {err:.3g}")
        assert err < tol, (tag, "materialised gradient", err)
    # (3) the plain-C oracle looped over the samples, same materialised gradient
    if oracle:
        traj_o, g0_o, rows_o = o_batch_reference(inp["h0"], Pn, T, g.cpu().numpy(), mask)
        assert np.array_equal(traj_o, traj.cpu().numpy()), (tag, "oracle trajectory")
        assert np.isfinite(g0_o).all() and np.isfinite(rows_o).all(), "ill-conditioned input"
        assert np.array_equal(g0.cpu().numpy(), g0_o), (tag, "oracle dL/dh0")
        want_rows = rows_o.sum(0, keepdims=True) if path == "batch" else rows_o
        for b, (got_r, want_r) in enumerate(zip(np.atleast_2d(pg.cpu().numpy()), want_rows)):
            err = grad_err(got_r, want_r) if np.any(want_r) else float(np.abs(got_r).max())
            print(f"{tag}: gradient row {b} vs oracle rel-L2 {err:.3g}")
            assert err < GRAD_TOL[c["dtype"]], (tag, "oracle gradient", b, err)


@functools.lru_cache(maxsize=2)
def _inputs(cid):
    c = next(c for c in sweep_cases() if c["id"] == cid)
    return loss_inputs(c)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", sweep_cases(), ids=batch_case_id)
def test_sample_losses_inside_the_sweep(case, path, hip_device):
    """every sweep family x B in {2, 3} x {batched, ensemble} x {mode 1, mode 2} x the five frame sets"""
    c = case
    inp = _inputs(c["id"])
    traj = _fwd(path)(dev_t(inp["h0"], hip_device), dev_t(block_of(inp, path), hip_device), c["T"], c["options"]).contiguous()
    assert torch.isfinite(traj).all()
    for mode in MODES:
        for frames in frame_sets(c["T"]):
            _check_config(c, inp, path, mode == 2, frames, hip_device, traj)


def test_per_sample_factor_is_not_element_zero(hip_device):
    """the factors of two calls differ in every element but the first: every sample but the first must change"""
    from percnn_amd import functional as F_pi
    c = sweep_cases()[1]                                   # (64, 96), B = 3
    assert c["B"] == 3
    inp = _inputs(c["id"])
    for path in PATHS:
        Pd = dev_t(block_of(inp, path), hip_device)
        traj = _fwd(path)(dev_t(inp["h0"], hip_device), Pd, c["T"], c["options"]).contiguous()
        f1 = torch.tensor([0.5, -1.25, 0.0], device=hip_device)
        f2 = torch.tensor([0.5, 2.0, 3.0], device=hip_device)
        a0, _ = F_pi.rollout_bwd_sqerr_batched(traj, Pd, None, None, 1e-3, f1, options=c["options"])
        b0, _ = F_pi.rollout_bwd_sqerr_batched(traj, Pd, None, None, 1e-3, f2, options=c["options"])
        assert torch.equal(a0[0], b0[0]) and not a0[2].any() and b0[2].any() and not torch.equal(a0[1], b0[1]), path


@pytest.mark.parametrize("shape,dtype,hc", [((40, 100), np.float32, 0), ((33, 37), np.float32, 8), ((6, 10, 9), np.float64, 3)])
def test_degenerate_batch_of_one_and_no_steps(shape, dtype, hc, hip_device):
    """B = 1 is the unbatched entry point (the ensemble's on P[0]); T = 0 writes dL/dh0 = a_b * (h0 - target_0)"""
    from percnn_amd import functional as F_pi
    from util import make_case
    T = 6
    c = make_case(11800 + hc, shape, hc, dtype, 1, T, "none", None)
    inp = loss_inputs(c)
    for path in PATHS:
        Pd = dev_t(block_of(inp, path), hip_device)
        traj = _fwd(path)(dev_t(inp["h0"], hip_device), Pd, T).contiguous()
        target = dev_t(inp["target"], hip_device)
        fac = torch.tensor([-1.25], dtype=traj.dtype, device=hip_device)
        for tg in (None, target):
            for frames in (None, [2, 3]):
                mask, w = _mask(T, frames), _weight(T, frames, traj[0, 0].numel())
                g0, pg = F_pi.rollout_bwd_sqerr_batched(traj, Pd, tg, mask, 2.0 * w, fac)
                s0, sp = F_pi.rollout_bwd_sqerr(traj[:, 0].contiguous(), Pd.reshape(-1), None if tg is None else tg[:, 0].contiguous(),
                                                mask, 2.0 * w, dev_scale=fac)
                assert torch.equal(g0[0], s0) and torch.equal(pg.reshape(-1), sp), (path, frames)
                loss = F_pi.traj_sqerr_batched(traj, tg, mask, w)
                one = F_pi.traj_sqerr(traj[:, 0].contiguous(), None if tg is None else tg[:, 0].contiguous(), mask, w)
                assert loss.shape == (1,) and torch.equal(loss[0], one), (path, frames)
        _check_config(c, inp, path, True, None, hip_device, traj)
    # T = 0, three samples
    c0 = make_case(11850 + hc, shape, hc, dtype, 3, 0, "none", None)
    inp = loss_inputs(c0)
    for path in PATHS:
        Pd = dev_t(block_of(inp, path), hip_device)
        h0, target = dev_t(inp["h0"], hip_device), dev_t(inp["target"], hip_device)
        traj = _fwd(path)(h0, Pd, 0).contiguous()
        fac = factors(3, traj.dtype, hip_device)
        w = _weight(0, None, traj[0, 0].numel())
        for tg in (None, target):
            g0, pg = F_pi.rollout_bwd_sqerr_batched(traj, Pd, tg, None, 2.0 * w, fac)
            assert torch.equal(g0, materialised_gradient(traj, tg, 2.0 * w, fac)[0]) and not pg.any(), path
            want = sample_losses_f64(traj, tg, None, w)
            got = F_pi.traj_sqerr_batched(traj, tg, None, w)
            assert torch.allclose(got.double(), want, rtol=1e-6, atol=0), path


def test_many_samples_on_a_tiny_grid(hip_device):
    """B = 513 samples in grid y on a (2, 3) grid, T = 3"""
    c = MANY_CASE
    inp = loss_inputs(c)
    for path in PATHS:
        traj = _fwd(path)(dev_t(inp["h0"], hip_device), dev_t(block_of(inp, path), hip_device), c["T"]).contiguous()
        _check_config(c, inp, path, True, None, hip_device, traj, singles=False)
        _check_config(c, inp, path, False, [1, 3], hip_device, traj, oracle=False, singles=False)


def _carve(t, off):
    """a copy of t that starts `off` elements into a larger buffer"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


def test_bases_four_bytes_off_sixteen(hip_device):
    """trajectory, target and dL/dh0 carved one float off a 16-byte boundary: scalar lanes, no tiles, the same numbers"""
    from percnn_amd import functional as F_pi
    c = MISALIGNED_CASE
    shape, hc, B, T = c["shape"], c["hc"], c["B"], c["T"]
    inp = loss_inputs(c)
    for path in PATHS:
        Pd = dev_t(block_of(inp, path), hip_device)
        start = np.zeros((T + 1, B, 2) + shape, dtype=c["dtype"].type)
        start[0] = inp["h0"]
        traj = _carve(dev_t(start, hip_device), 1)
        (batch_rollout_fwd_ if path == "batch" else ensemble_rollout_fwd_)(traj, Pd, hc, shape, B, T)
        target = _carve(dev_t(inp["target"], hip_device), 1)
        fac = factors(B, traj.dtype, hip_device)
        aligned, aligned_target = traj.clone(), target.clone()
        assert aligned.data_ptr() % 16 == 0 and aligned_target.data_ptr() % 16 == 0
        for tg, atg in ((None, None), (target, aligned_target)):
            for frames in (None, [2, 3, 4, 7]):
                mask, w = _mask(T, frames), _weight(T, frames, traj[0, 0].numel())
                g_h0 = _carve(torch.zeros((B, 2) + shape, dtype=traj.dtype, device=hip_device), 1)
                _, pg = F_pi.rollout_bwd_sqerr_batched(traj, Pd, tg, mask, 2.0 * w, fac, g_h0=g_h0)
                a0, apg = F_pi.rollout_bwd_sqerr_batched(aligned, Pd, atg, mask, 2.0 * w, fac)
                assert torch.equal(g_h0, a0), (path, frames)
                for got_r, want_r in zip(np.atleast_2d(pg.cpu().numpy()), np.atleast_2d(apg.cpu().numpy())):
                    assert rel_l2(got_r, want_r) < MAT_TOL[c["dtype"]] or not np.any(want_r), (path, frames)
                want = sample_losses_f64(aligned, atg, frames, w)
                got = F_pi.traj_sqerr_batched(traj, tg, mask, w)
                assert torch.allclose(got.double(), want, rtol=1e-6, atol=0), (path, frames)
        _check_config(c, inp, path, True, None, hip_device, aligned)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape,dtype,hc,T", [((40, 100), np.float32, 0, 9), ((6, 10, 9), np.float64, 3, 5)])
def test_operator_equals_the_materialised_autograd_route(shape, dtype, hc, T, path, hip_device):
    """pa.pi_rollout_sqerr_{batched,ensemble}(...)[0] weighted by a random [B] vector and summed, against pi_rollout_* + tensor-op
    MSE + backward().  ATen forms dL/dtraj in another order of multiplications than the kernels (w_b * 2/N * d against
    (2/N * w_b) * d), so dL/dh0 is held to the rel-L2 bound of the gradients (2e-5 / 1e-11), not to bit equality."""
    import percnn_amd as pa
    from util import make_case
    B = 3
    c = make_case(11700 + hc, shape, hc, dtype, B, T, "none", None)
    inp = loss_inputs(c)
    target = dev_t(inp["target"], hip_device)
    wts = dev_t(np.random.RandomState(5).uniform(-1, 1, B).astype(c["dtype"].type), hip_device)
    op = pa.pi_rollout_sqerr_batched if path == "batch" else pa.pi_rollout_sqerr_ensemble
    tol = MAT_TOL[c["dtype"]]
    for tg in (None, target):
        for frames in (None, [-1, 2, 2, 0]):
            sel = slice(None) if frames is None else sorted({f % (T + 1) for f in frames})
            h0 = dev_t(inp["h0"], hip_device).requires_grad_(True)
            P = dev_t(block_of(inp, path), hip_device).requires_grad_(True)
            traj = _fwd(path)(h0, P, T)
            d = traj[sel] if tg is None else traj[sel] - tg[sel]
            ref = (d ** 2).mean(dim=tuple(i for i in range(d.dim()) if i != 1))
            (ref * wts).sum().backward()
            want_h0, want_P = h0.grad.clone(), P.grad.clone()
            h0.grad = P.grad = None
            loss, tr = op(h0, P, T, tg, frames)
            assert loss.shape == (B,) and not tr.requires_grad and torch.equal(tr, traj.detach())
            ref64 = (d.detach().double() ** 2).mean(dim=tuple(i for i in range(d.dim()) if i != 1))
            assert torch.allclose(loss.double(), ref64, rtol=1e-6, atol=0)
            (loss * wts).sum().backward()
            assert h0.grad.shape == h0.shape and P.grad.shape == P.shape
            assert rel_l2(h0.grad.cpu().numpy(), want_h0.cpu().numpy()) < tol, (path, frames)
            for got_r, want_r in zip(np.atleast_2d(P.grad.cpu().numpy()), np.atleast_2d(want_P.cpu().numpy())):
                assert rel_l2(got_r, want_r) < tol, (path, frames)
    tgr = target.clone().requires_grad_(True)
    loss, _ = op(dev_t(inp["h0"], hip_device).requires_grad_(True), dev_t(block_of(inp, path), hip_device), T, tgr)
    loss.sum().backward()
    assert tgr.grad is None                                  # the target gets no gradient
    with pytest.raises(ValueError, match="no frame selected"):
        op(dev_t(inp["h0"], hip_device), dev_t(block_of(inp, path), hip_device), T, None, [])


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


def test_sample_losses_of_a_cell_ensemble_are_the_members_loss_mse(hip_device):
    """RCNN.sample_losses on a CellEnsemble of three cells: loss b and every parameter gradient of member b equal the member's
    own RCNN.loss_mse on its sample (loss 1e-6; gradients 2e-5 rel-L2, the bound of the gradient comparisons above)"""
    import copy
    import percnn_amd as pa
    from percnn_amd import synthetic
    T, shape = 10, (48, 64)
    cells = _cells(hip_device, 3)
    refs = copy.deepcopy(cells)
    h0 = torch.cat([synthetic.gs_initial_state(shape, seed=s) for s in range(3)]).to(hip_device)
    target = torch.rand((T + 1, 3, 2) + shape, device=hip_device)
    wts = torch.tensor([0.5, -1.25, 2.0], device=hip_device)
    for tg, tsl in ((None, slice(None)), (target, slice(None)), (target, slice(1, -1, 3))):
        ens = pa.CellEnsemble(cells)
        ens.zero_grad()
        hb = h0.clone().requires_grad_(True)
        model = pa.RCNN(ens, step=T, effective_step=list(range(T)), init_state=hb)
        losses = model.sample_losses(tg, tsl)
        assert losses.shape == (3,)
        assert model.last_trajectory.shape == (T + 1, 3, 2) + shape and not model.last_trajectory.requires_grad
        (losses * wts).sum().backward()
        for b in range(3):
            refs[b].zero_grad()
            h1 = h0[b:b + 1].clone().requires_grad_(True)
            m1 = pa.RCNN(refs[b], step=T, effective_step=list(range(T)), init_state=h1)
            one = m1.loss_mse(None if tg is None else tg[:, b].contiguous(), tsl)
            assert abs(float(losses[b]) - float(one)) <= 1e-6 * abs(float(one)), (b, tsl)
            (one * wts[b]).backward()
            assert rel_l2(hb.grad[b].cpu().numpy(), h1.grad[0].cpu().numpy()) < 2e-5, (b, tsl)
            got = dict(cells[b].named_parameters())
            n = 0
            for name, p in refs[b].named_parameters():
                if p.grad is None:
                    assert got[name].grad is None or not got[name].grad.any(), name
                    continue
                n += 1
                assert rel_l2(got[name].grad.cpu().numpy(), p.grad.cpu().numpy()) < 2e-5, (b, name, tsl)
            assert n > 0


def test_sample_losses_batched_and_single(hip_device):
    """a batched initial state with one cell, and B = 1 -> [1], against loss_mse per sample"""
    import percnn_amd as pa
    from percnn_amd import synthetic
    T, shape = 6, (32, 48)
    cell = _cells(hip_device, 1)[0]
    h0 = torch.cat([synthetic.gs_initial_state(shape, seed=s) for s in range(2)]).to(hip_device)
    target = torch.rand((T + 1, 2, 2) + shape, device=hip_device)
    model = pa.RCNN(cell, step=T, effective_step=list(range(T)), init_state=h0)
    losses = model.sample_losses(target, slice(0, -1, 2))
    cell.zero_grad()
    losses.mean().backward()
    got = {n: p.grad.clone() for n, p in cell.named_parameters() if p.grad is not None}
    cell.zero_grad()
    total = 0
    for b in range(2):
        m1 = pa.RCNN(cell, step=T, effective_step=list(range(T)), init_state=h0[b:b + 1])
        one = m1.loss_mse(target[:, b].contiguous(), slice(0, -1, 2))
        assert abs(float(losses[b]) - float(one)) <= 1e-6 * abs(float(one))
        total = total + one / 2
        l1 = m1.sample_losses(target[:, b:b + 1].contiguous(), slice(0, -1, 2))
        assert l1.shape == (1,) and abs(float(l1[0]) - float(one)) <= 1e-6 * abs(float(one))
    total.backward()
    assert got
    for n, g in got.items():
        assert rel_l2(g.cpu().numpy(), dict(cell.named_parameters())[n].grad.cpu().numpy()) < 2e-5, n


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
    for kind in ("batch", "ensemble"):
        f = getattr(L, f"percnn_pi_{kind}_rollout_bwd_sqerr_f32")
        ok = lambda **k: f(k.get("traj", tr), None, None, 1.0, None, k.get("g_h0", g0.data_ptr()), k.get("pg", pg.data_ptr()),
                           ws.data_ptr(), k.get("ws_bytes", ws.numel()), k.get("P", P.data_ptr()), k.get("hc", 0), 2, shape,
                           k.get("batch", B), T, k.get("options"), None)
        assert ok(traj=None) == -1 and ok(g_h0=None) == -1 and ok(pg=None) == -1 and ok(P=None) == -1, kind
        assert ok(g_h0=tr) == -1, kind                                   # dL/dh0 would overwrite the trajectory
        assert ok(batch=0) == -1 and ok(batch=65536) == -1 and ok(hc=-1) == -1 and ok(options=b"tile_k=3") == -1, kind
        assert ok(ws_bytes=16) == -2, kind
        assert ok() == 0, kind
    s = L.percnn_pi_batch_traj_sqerr_f32
    args = lambda **k: s(k.get("traj", tr), None, None, T + 1, 2, shape, k.get("batch", B), 1.0, k.get("out", out.data_ptr()),
                         sws.data_ptr(), k.get("ws_bytes", sws.numel()), None)
    assert args(traj=None) == -1 and args(out=None) == -1 and args(out=tr) == -1 and args(batch=0) == -1 and args(batch=65536) == -1
    assert args(ws_bytes=8) == -2 and args() == 0
    torch.cuda.synchronize()
    # cells without a Pi-block kernel path
    h = torch.rand(2, 2, 16, 16, device=hip_device)
    for cell in (pa.Stage3BurgersCell().to(hip_device), pa.Stage1Cell("burgers").to(hip_device)):
        with pytest.raises(ValueError):
            pa.RCNN(cell, step=3, effective_step=[0, 1, 2], init_state=h).sample_losses()
    # the single-trajectory losses still refuse a batch
    cell = pa.gs2d_cell(8).to(hip_device)
    m = pa.RCNN(cell, step=3, effective_step=[0, 1, 2], init_state=h)
    with pytest.raises(ValueError):
        m.loss_mse()
    with pytest.raises(ValueError):
        m.observe()
    with pytest.raises(ValueError):
        pa.RCNN(cell, step=3, effective_step=[0, 2], init_state=h).sample_losses()
    assert m.sample_losses().shape == (2,)
