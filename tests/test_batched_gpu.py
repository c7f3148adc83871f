"""GPU: batched rollouts (percnn_pi_batch_*, torch.ops.percnn.*_batched, RCNNCell / RCNN on [B,2,*S]).

Every state field of sample b must be bit-identical to the unbatched entry point on that sample alone; the parameter
gradient is the sum of the per-sample gradients to reduction round-off."""
import numpy as np
import pytest
import torch

from util import TOL_GRAD, TOL_TRAJ, bits_equal, random_block, rel_l2
from util import batch_rollout_bwd as _bwd_batched, single_rollout_bwd as _bwd_single

pytestmark = pytest.mark.gpu

#        name          hc  dtype       shape          B  T
FWD_CASES = [
    ("gs2d_poly", 0, np.float32, (100, 100), 3, 37),
    ("gs2d_fact", 8, np.float32, (100, 100), 7, 5),
    ("gs2d_fact", 8, np.float32, (128, 128), 2, 37),
    ("gs2d_poly", 0, np.float32, (96, 160), 7, 1),
    ("gs3d_fact", 2, np.float32, (48, 48, 48), 2, 5),
    ("gs3d_poly", 0, np.float32, (16, 24, 32), 3, 37),
    ("lo_f64", 0, np.float64, (100, 100), 2, 37),
    ("lo_f64", 4, np.float64, (128, 128), 3, 0),
]


def _case_id(c):
    return f"{c[0]}-hc{c[1]}-{'x'.join(map(str, c[3]))}-B{c[4]}-T{c[5]}"


def _setup(hc, dtype, shape, B, dev, seed=0):
    P = torch.from_numpy(random_block(hc, len(shape), dtype, seed + 1, scale=0.1)).to(dev)
    rs = np.random.RandomState(seed)
    h0 = torch.from_numpy((0.2 + 0.3 * rs.rand(B, 2, *shape)).astype(dtype)).to(dev)     # a distinct IC per sample
    return h0, P


@pytest.mark.parametrize("case", FWD_CASES, ids=_case_id)
def test_batched_forward_is_bitwise_per_sample(case, hip_device):
    import percnn_amd as pa
    _, hc, dtype, shape, B, T = case
    h0, P = _setup(hc, dtype, shape, B, hip_device)
    traj = pa.pi_rollout_batched(h0, P, T)
    assert traj.shape == (T + 1, B, 2) + shape
    for b in range(B):
        ref = pa.pi_rollout(h0[b:b + 1], P, T)
        assert bits_equal(traj[:, b], ref), f"sample {b}"
        assert torch.isfinite(ref).all()
    # changing one sample's IC leaves the others bit-identical
    h1 = h0.clone()
    h1[B // 2] *= 0.9
    traj1 = pa.pi_rollout_batched(h1, P, T)
    for b in range(B):
        if b != B // 2:
            assert bits_equal(traj1[:, b], traj[:, b])
    # one batched step == one step per sample
    s = pa.pi_step_batched(h0, P)
    for b in range(B):
        assert bits_equal(s[b:b + 1], pa.pi_step(h0[b:b + 1], P))


def test_batched_forward_matches_oracle(hip_device):
    import percnn_amd as pa
    from oracle import pi_oracle as O
    h0, P = _setup(8, np.float32, (32, 40), 3, hip_device, seed=4)
    traj = pa.pi_rollout_batched(h0, P, 6).cpu().numpy()
    for b in range(3):
        ref = O.rollout_fwd(h0[b].cpu().numpy(), P.cpu().numpy(), 8, 6)
        assert rel_l2(traj[:, b], ref) < TOL_TRAJ[np.dtype(np.float32)]


BWD_CASES = [c for c in FWD_CASES if c[5] > 0] + [("gs2d_poly", 0, np.float32, (128, 128), 3, 24)]


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "stride20"])
@pytest.mark.parametrize("case", BWD_CASES, ids=_case_id)
def test_batched_backward_per_sample(case, masked, hip_device):
    import percnn_amd as pa
    _, hc, dtype, shape, B, T = case
    h0, P = _setup(hc, dtype, shape, B, hip_device, seed=2)
    traj = pa.pi_rollout_batched(h0, P, T).contiguous()
    g = torch.from_numpy(np.random.RandomState(3).standard_normal(tuple(traj.shape)).astype(dtype)).to(hip_device)
    mask = bytes(1 if (t % 20 == 0 or t == T) else 0 for t in range(T + 1)) if masked else None
    g_h0, pg = _bwd_batched(traj, g, P, hc, shape, B, T, mask)
    g_h0b, pgb = _bwd_batched(traj, g, P, hc, shape, B, T, mask)
    assert torch.equal(g_h0, g_h0b) and torch.equal(pg, pgb), "run to run"
    total = torch.zeros_like(pg)
    for b in range(B):
        tb, gb = traj[:, b].contiguous(), g[:, b].contiguous()
        g0, p1 = _bwd_single(tb, gb, P, hc, shape, T, mask)
        assert bits_equal(g_h0[b], g0), f"dL/dh0 of sample {b}"
        total += p1
    tol = 1e-6 if dtype == np.float32 else 1e-10
    assert rel_l2(pg.cpu().numpy(), total.cpu().numpy()) < tol


def test_batched_gradcheck_fp64(hip_device):
    """dL/dh0 and dL/d(trainable block entries): dt (slot 0) and the frozen stencil (3..15) carry no gradient by design"""
    import percnn_amd as pa
    h0, P = _setup(2, np.float64, (8, 8), 2, hip_device, seed=5)
    P0 = P.detach()
    q = torch.cat([P0[1:3], P0[16:]]).requires_grad_(True)
    h0.requires_grad_(True)

    def block(q):
        return torch.cat([P0[:1], q[:2], P0[3:16], q[2:]])

    assert torch.autograd.gradcheck(lambda h, q: pa.pi_rollout_batched(h, block(q), 3), (h0, q), eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda h, q: pa.pi_step_batched(h, block(q)), (h0, q), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_rcnncell_batch_is_bitwise_per_sample(hip_device):
    import percnn_amd as pa
    torch.manual_seed(0)
    cell = pa.gs2d_cell(8).to(hip_device)
    h = torch.rand(4, 2, 100, 100, device=hip_device)
    out, out2 = cell(h)
    assert out is out2 and out.shape == h.shape
    for b in range(4):
        assert torch.equal(out[b:b + 1], cell(h[b:b + 1])[0])


def test_rcnn_batched_init_state_vs_restatement(hip_device):
    import percnn_amd as pa
    from oracle import restatement as R
    torch.manual_seed(0)
    cell = pa.gs2d_cell(8, reaction="factored").to(hip_device)
    for p in cell.filter_list:
        p.weight.data.mul_(20.0)
    ocell = R.gs2d_cell(8).to(hip_device)
    ocell.load_state_dict(cell.state_dict())
    B, T = 3, 12
    h0 = torch.cat([R.gs_initial_state((48, 48), seed=s) for s in range(B)]).to(hip_device)
    model = pa.RCNN(cell, step=T, effective_step=list(range(T)), init_state=h0)
    outs, second = model()
    assert len(outs) == T + 1 and all(o.shape == (B, 2, 48, 48) for o in outs)
    out = torch.cat(tuple(outs), dim=0)
    assert out.shape == ((T + 1) * B, 2, 48, 48)
    assert out.data_ptr() == outs.stacked.data_ptr()                  # the cat is the trajectory buffer itself
    loss = torch.nn.functional.mse_loss(out, torch.zeros_like(out))
    loss.backward()
    oref = R.OracleRCNN(ocell, step=T, effective_step=list(range(T)), init_state=h0)
    routs, rsecond = oref()
    rout = torch.cat(tuple(routs), dim=0)
    torch.nn.functional.mse_loss(rout, torch.zeros_like(rout)).backward()
    dt = np.dtype(np.float32)
    assert rel_l2(out.detach().cpu().numpy(), rout.detach().cpu().numpy()) < TOL_TRAJ[dt]
    assert rel_l2(second.detach().cpu().numpy(), rsecond.detach().cpu().numpy()) < TOL_TRAJ[dt]
    for (n, p), (_, q) in zip(cell.named_parameters(), ocell.named_parameters()):
        if q.grad is not None and p.grad is not None and float(q.grad.abs().max()) > 0:
            assert rel_l2(p.grad.cpu().numpy(), q.grad.cpu().numpy()) < 10 * TOL_GRAD[dt], n
    # trajectory(): [T+1,B,2,*S], the same states
    assert torch.equal(model.trajectory().detach().flatten(0, 1), out.detach())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batched_ops_opcheck(dtype, hip_device):
    import percnn_amd as pa
    from percnn_amd import ops
    ops.load_native()
    h0, P = _setup(0, np.float32 if dtype == torch.float32 else np.float64, (16, 16), 3, hip_device, seed=7)
    h0.requires_grad_(True)
    P.requires_grad_(True)
    torch.library.opcheck(torch.ops.percnn.pi_step_batched.default, (h0, P, ""))
    torch.library.opcheck(torch.ops.percnn.pi_rollout_batched.default, (h0, P, 4, ""))
    assert pa.pi_rollout_batched(h0, P, 2).shape == (3, 3, 2, 16, 16)


def test_batched_torch_compile_fullgraph(hip_device):
    import percnn_amd as pa
    torch.manual_seed(0)
    cell = pa.gs2d_cell(8).to(hip_device)
    h = torch.rand(3, 2, 32, 32, device=hip_device)
    P = cell.param_block().detach()

    def f(x):
        y = cell(x)[0]
        return pa.pi_rollout_batched(y, P, 3)

    got = torch.compile(f, fullgraph=True)(h)
    assert torch.equal(got, f(h))


def test_batched_errors(hip_device):
    import percnn_amd as pa
    torch.manual_seed(0)
    h = torch.rand(2, 2, 16, 16, device=hip_device)
    burgers = pa.Stage3BurgersCell().to(hip_device)
    with pytest.raises(RuntimeError):
        pa.pi_rollout_batched(h, burgers.param_block().detach(), 3)
    with pytest.raises(ValueError):
        pa.RCNN(burgers, step=3, effective_step=[0, 1, 2], init_state=h)()
    cell = pa.gs2d_cell(8).to(hip_device)
    model = pa.RCNN(cell, step=4, effective_step=list(range(4)), init_state=h)
    with pytest.raises(ValueError):
        model.observe(slice(None), 2)
    with pytest.raises(ValueError):
        model.loss_mse()
    # the unbatched operators keep rejecting B != 1
    with pytest.raises(RuntimeError):
        pa.pi_rollout(h, cell.param_block(), 2)
