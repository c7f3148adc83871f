"""GPU: the physics-residual loss per sample of a batch / an ensemble (percnn_pi_{batch,ensemble}_residual_sqloss_*,
physics.physics_loss_batched, RCNN.sample_physics_losses).  The yardstick is the unbatched ``physics.physics_loss`` of each sample
on its own (pinned to oracle/restatement.py::physics_loss_reference by test_hip_parity.py::test_physics_loss_vs_reference): loss
values at the bounds of two passes that differ only in the order of their float64 sums (1e-6 / 1e-13), gradients bit for bit --
the arithmetic per point is the unbatched kernels'."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from batched_physics_util import LOSS_TOL, block, blocks, case_id, cases, family, make_cell, trajectory
from util import rel_l2

pytestmark = pytest.mark.gpu


def _q_of(Q, b):
    return Q if Q.dim() == 1 else Q[b].contiguous()


def _unbatched(out, Q, weighted, w):
    """loss [B] and dL/d output of sum_b w[b] * physics_loss(sample b), sample by sample"""
    from percnn_amd import physics
    losses, grads = [], []
    for b in range(out.shape[1]):
        o = out[:, b].contiguous().requires_grad_(True)
        l = physics.physics_loss(o, _q_of(Q, b), weighted)
        (w[b] * l).backward()
        losses.append(l.detach())
        grads.append(o.grad)
    return torch.stack(losses), torch.stack(grads, 1)


def _close(got, want, tol, tag):
    assert got.shape == want.shape, tag
    for b in range(want.shape[0]):
        print(tag, b, float(got[b]), float(want[b]))
        assert abs(float(got[b]) - float(want[b])) <= tol * abs(float(want[b])), (tag, b, float(got[b]), float(want[b]))


def _weights(B, dtype, dev):
    return torch.tensor([(0.5, -1.25, 2.0, 0.75, -3.0)[b % 5] * (1 + b // 5) for b in range(B)], dtype=dtype, device=dev)


@pytest.mark.parametrize("c", cases(), ids=case_id)
def test_loss_and_gradient_equal_the_unbatched_pass(c, hip_device):
    import percnn_amd as pa
    from percnn_amd import physics
    cell = make_cell(c).to(hip_device)
    Q = blocks(c, cell)
    out = trajectory(c).to(hip_device).requires_grad_(True)
    B, tol = c["B"], LOSS_TOL[c["dtype"]]
    w = _weights(B, c["dtype"], hip_device)
    want, want_g = _unbatched(out.detach(), Q, c["weighted"], w)
    assert (want > 0).all()
    loss = physics.physics_loss_batched(out, Q, c["weighted"])
    assert type(loss.grad_fn).__name__ == "BatchedPhysicsLossFunctionBackward" and loss.shape == (B,) and loss.dtype == c["dtype"]
    _close(loss.detach(), want, tol, "fused")
    (w * loss).sum().backward()
    assert out.grad.shape == out.shape and not out.grad[-1].any()              # loss_gen drops the last frame
    for b in range(B):
        assert np.array_equal(out.grad[:, b].cpu().numpy(), want_g[:, b].cpu().numpy()), ("gradient of sample", b)
    # the stacking route (what a grid the fused pass turns down takes) is the yardstick itself
    _close(physics.physics_loss_batched(out.detach(), Q, c["weighted"], fused=False), want, tol, "stacked")
    assert torch.equal(physics.physics_loss_batched(out.detach(), Q, c["weighted"]), loss.detach())     # run to run
    if c["path"] == "tile":
        try:
            pa.set_option("tile", 0)
            _close(physics.physics_loss_batched(out.detach(), Q, c["weighted"]), want, tol, "tile = 0")
        finally:
            pa.set_option("tile", 1)


# one grid per loss pass, three samples
ADDRESSING = [dict(path=path, shape=shape, dtype=dtype, form="per_sample", weighted=True, B=3, F=3, seed=60 + i)
              for i, (path, shape, dtype) in enumerate([("generic", (33, 64), torch.float32), ("tile", (40, 100), torch.float32),
                                                        ("3d", (7, 6, 8), torch.float64)])]


@pytest.mark.parametrize("c", ADDRESSING, ids=case_id)
def test_upstream_factor_is_read_per_sample(c, hip_device):
    """an upstream gradient that is zero except at one sample reaches that sample's slice of dL/d output alone"""
    from percnn_amd import physics
    cell = make_cell(c).to(hip_device)
    for Q in (blocks(c, cell), block(cell, family(c))):
        for j in range(c["B"]):
            out = trajectory(c).to(hip_device).requires_grad_(True)
            up = torch.zeros(c["B"], dtype=c["dtype"], device=hip_device)
            up[j] = 1.5
            physics.physics_loss_batched(out, Q, True).backward(up)
            for b in range(c["B"]):
                assert bool(out.grad[:-1, b].any()) == (b == j), (j, b)


@pytest.mark.parametrize("c", ADDRESSING, ids=case_id)
def test_equation_block_is_read_per_sample(c, hip_device):
    """per-sample blocks that differ from the shared one in row j alone change loss j alone"""
    from percnn_amd import physics
    cell = make_cell(c).to(hip_device)
    fam = family(c)
    Q0 = block(cell, fam)
    out = trajectory(c).to(hip_device)
    base = physics.physics_loss_batched(out, Q0, True)
    for j in range(c["B"]):
        Q = torch.stack([block(cell, fam, 2) if b == j else Q0 for b in range(c["B"])])
        got = physics.physics_loss_batched(out, Q, True)
        for b in range(c["B"]):
            assert torch.equal(got[b], base[b]) == (b != j), (j, b)


def test_many_samples_on_a_tiny_grid(hip_device):
    """B = 513 on (4, 6), F = 2: more samples than any per-sample bound of the partial rows; both block forms"""
    from percnn_amd import physics
    c = dict(shape=(4, 6), dtype=torch.float64, B=513, F=2, seed=77)
    cell = make_cell(c).to(hip_device)
    fam = family(c)
    kinds = [block(cell, fam, b) for b in range(4)]
    out = trajectory(c).to(hip_device)
    w = _weights(513, torch.float64, hip_device)
    for Q in (kinds[0], torch.stack([kinds[b % 4] for b in range(513)])):
        o = out.clone().requires_grad_(True)
        loss = physics.physics_loss_batched(o, Q, True)
        (w * loss).sum().backward()
        want, want_g = _unbatched(out, Q, True, w)
        assert torch.allclose(loss.detach(), want, rtol=LOSS_TOL[torch.float64], atol=0)
        assert torch.equal(o.grad, want_g)


@pytest.mark.parametrize("fam,shape,dtype,B", [("gs2d", (40, 100), torch.float32, 3), ("gs2d", (33, 64), torch.float32, 2),
                                               ("lo2d", (34, 36), torch.float64, 2), ("lo2d", (7, 6), torch.float64, 5)])
def test_loss_vs_reference_restatement(fam, shape, dtype, B, hip_device):
    """the reference's coefficient sets: loss[b] against oracle/restatement.py::physics_loss_reference on the CPU, in float64
    on the same trajectory (the yardstick of test_physics_loss_vs_reference), at its bounds: 5e-6 (float32), 1e-7 (float64)"""
    from percnn_amd import physics
    from oracle import restatement as R
    c = dict(shape=shape, dtype=dtype, B=B, F=3, seed=41)
    cell = make_cell(c).to(hip_device)
    assert family(c) == fam
    traj = trajectory(c)
    loss = physics.physics_loss_batched(traj.to(hip_device), block(cell, fam), True)
    tol = 5e-6 if dtype == torch.float32 else 1e-7
    for b in range(B):
        ref = float(R.physics_loss_reference(traj[:, b].double(), fam, cell.dx, cell.dt))
        print(fam, shape, b, float(loss[b]), ref)
        assert abs(float(loss[b]) - ref) <= tol * abs(ref), (b, float(loss[b]), ref)


@pytest.mark.parametrize("form", ["shared", "per_sample"])
@pytest.mark.parametrize("weighted", [True, False])
def test_gradcheck_fp64(weighted, form, hip_device):
    """the tolerances of test_physics_residual_gradcheck_fp64's fused loss node"""
    from percnn_amd import physics
    for shape in ((4, 2, 2, 6, 8), (3, 2, 2, 4, 6, 4)):
        c = dict(shape=shape[3:], dtype=torch.float64, B=2, form=form)
        Q = blocks(c, make_cell(c).to(hip_device))
        traj = torch.rand(shape, dtype=torch.float64, device=hip_device, generator=torch.Generator(device=hip_device).manual_seed(11),
                          requires_grad=True)
        assert torch.autograd.gradcheck(lambda t: physics.physics_loss_batched(t, Q, weighted), (traj,), eps=1e-6, atol=1e-7, rtol=1e-5)


def _gs_cells(dev, n):
    import percnn_amd as pa
    torch.manual_seed(7)
    cells = []
    for _ in range(n):
        cell = pa.gs2d_cell(8, reaction="factored").to(dev)
        for p in cell.filter_list:
            p.weight.data.mul_(20.0)                       # make the reaction term visible at init scale
        cells.append(cell)
    return cells


def _check_param_grads(got_cell, ref_cell, tag):
    got = dict(got_cell.named_parameters())
    n = 0
    for name, p in ref_cell.named_parameters():
        if p.grad is None:
            assert got[name].grad is None or not got[name].grad.any(), (tag, name)
            continue
        n += 1
        assert rel_l2(got[name].grad.cpu().numpy(), p.grad.cpu().numpy()) < 2e-5, (tag, name)
    assert n > 0


def test_sample_physics_losses_of_a_cell_ensemble(hip_device):
    """RCNN.sample_physics_losses on a CellEnsemble, each member against its own equation: loss b and every parameter gradient
    of member b equal the member's own physics_loss(trajectory) (1e-6; 2e-5 rel-L2, the bounds of test_batched_loss_gpu.py)"""
    import percnn_amd as pa
    from percnn_amd import physics, synthetic
    T, shape, B = 6, (34, 36), 3
    cells = _gs_cells(hip_device, B)
    refs = copy.deepcopy(cells)
    h0 = torch.cat([synthetic.gs_initial_state(shape, seed=s) for s in range(B)]).to(hip_device)
    Q = torch.stack([block(cells[b], "gs2d", b) for b in range(B)])
    for weighted in (True, False):
        ens = pa.CellEnsemble(cells)
        ens.zero_grad()
        model = pa.RCNN(ens, step=T, effective_step=list(range(T)), init_state=h0)
        losses = model.sample_physics_losses(Q, weighted)
        assert losses.shape == (B,)
        assert model.last_trajectory.shape == (T + 1, B, 2) + shape and not model.last_trajectory.requires_grad
        losses.sum().backward()
        for b in range(B):
            refs[b].zero_grad()
            m1 = pa.RCNN(refs[b], step=T, effective_step=list(range(T)), init_state=h0[b:b + 1])
            one = physics.physics_loss(m1.trajectory(), Q[b].contiguous(), weighted)
            assert abs(float(losses[b]) - float(one)) <= 1e-6 * abs(float(one)), (b, weighted)
            one.backward()
            _check_param_grads(cells[b], refs[b], (b, weighted))


def test_sample_physics_losses_batched_and_single(hip_device):
    """a batched initial state with one cell and one equation, and B = 1 -> [1]"""
    import percnn_amd as pa
    from percnn_amd import physics, synthetic
    T, shape, B = 6, (34, 36), 2
    cell = _gs_cells(hip_device, 1)[0]
    ref = copy.deepcopy(cell)
    h0 = torch.cat([synthetic.gs_initial_state(shape, seed=s) for s in range(B)]).to(hip_device)
    Q = block(cell, "gs2d")
    model = pa.RCNN(cell, step=T, effective_step=list(range(T)), init_state=h0)
    losses = model.sample_physics_losses(Q)
    assert losses.shape == (B,) and model.last_trajectory.shape == (T + 1, B, 2) + shape
    cell.zero_grad()
    losses.sum().backward()
    ref.zero_grad()
    for b in range(B):
        m1 = pa.RCNN(ref, step=T, effective_step=list(range(T)), init_state=h0[b:b + 1])
        one = physics.physics_loss(m1.trajectory(), Q)
        assert abs(float(losses[b]) - float(one)) <= 1e-6 * abs(float(one)), b
        one.backward()
        l1 = m1.sample_physics_losses(Q)
        assert l1.shape == (1,) and abs(float(l1[0]) - float(one)) <= 1e-6 * abs(float(one))
        assert m1.last_trajectory.shape == (T + 1, 1, 2) + shape
    _check_param_grads(cell, ref, "batched")


def test_error_paths(hip_device):
    import percnn_amd as pa
    from percnn_amd import physics
    cell = pa.gs2d_cell().to(hip_device)
    Q = block(cell, "gs2d")
    out = torch.rand((4, 3, 2, 8, 8), device=hip_device)
    for bad in (Q[:35], torch.stack([Q, Q]), torch.stack([Q] * 3).reshape(-1), torch.stack([Q] * 3)[None]):
        with pytest.raises(ValueError):
            physics.physics_loss_batched(out, bad)
    with pytest.raises(ValueError):
        physics.physics_loss_batched(out[:2], Q)                              # fewer than 3 frames
    with pytest.raises(ValueError):
        physics.physics_loss_batched(out[:, 0], Q)                            # not frame-major [F+2, B, 2, *S]
    with pytest.raises(RuntimeError, match="no CPU path"):
        physics.physics_loss_batched(out.cpu(), Q.cpu())
    with pytest.raises(RuntimeError):
        physics.physics_loss_batched(out, Q.double())                         # block of another dtype
    # the C-ABI on device buffers: validation before any launch
    L = pa.lib()
    shape = (ctypes.c_int64 * 2)(8, 8)
    ws = torch.empty(L.percnn_pi_batch_residual_sqloss_workspace_bytes(3) // 8, dtype=torch.float64, device=hip_device)
    loss = torch.empty(3, device=hip_device)
    g, scratch = torch.empty_like(out), torch.empty_like(out[:2])
    Q3 = torch.stack([Q] * 3)
    for kind, q in (("batch", Q), ("ensemble", Q3)):
        fwd = getattr(L, f"percnn_pi_{kind}_residual_sqloss_f32")
        bwd = getattr(L, f"percnn_pi_{kind}_residual_sqloss_bwd_f32")

        def f(traj=out.data_ptr(), q=q.data_ptr(), batch=3, nframes=2, lo=loss.data_ptr(), w=ws.data_ptr(), wb=ws.numel() * 8):
            return fwd(traj, q, 2, shape, batch, nframes, 1, lo, w, wb, None)

        def b(traj=out.data_ptr(), q=q.data_ptr(), batch=3, nframes=2, nout=4, s=scratch.data_ptr(), gt=g.data_ptr()):
            return bwd(traj, None, q, 2, shape, batch, nframes, nout, 1, s, gt, None)
        assert f(traj=None) == -1 and f(q=None) == -1 and f(lo=None) == -1 and f(batch=0) == -1 and f(batch=65536) == -1, kind
        assert f(nframes=0) == -1 and f(w=None) == -2 and f(wb=8) == -2 and f(w=ws.data_ptr() + 4) == -2, kind
        assert b(traj=None) == -1 and b(q=None) == -1 and b(s=None) == -1 and b(gt=None) == -1 and b(batch=0) == -1, kind
        assert b(nframes=0) == -1 and b(nout=2) == -1 and b(batch=65536) == -1, kind
        assert f() == 0 and b() == 0, kind                                   # g_loss NULL = ones
        torch.cuda.synchronize()
        want = physics.physics_loss_batched(out, q)
        assert torch.equal(loss, want), kind
        o = out.clone().requires_grad_(True)
        physics.physics_loss_batched(o, q).sum().backward()
        assert torch.equal(g, o.grad), kind
