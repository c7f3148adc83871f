"""GPU: ensemble rollouts (percnn_pi_ensemble_*, torch.ops.percnn.*_ensemble, pa.CellEnsemble): B samples [B,2,*S], one
parameter block per sample [B,np].

Every state and adjoint field of sample b must be bit-identical to the unbatched entry point on (h0[b], P[b]); gradient row
b equals that call's parameter gradient to reduction round-off (rel-L2 1e-6 float32 / 1e-10 float64, the bounds of the
batched tests for the same kind of comparison).  Every block below differs per sample: its own seed and its own dt."""
import numpy as np
import pytest
import torch

from util import TOL_GRAD, TOL_TRAJ, bits_equal, rel_l2
from util import ensemble_blocks as _blocks, ensemble_rollout_bwd as _bwd_ensemble, ensemble_step_bwd, single_rollout_bwd as _bwd_single

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
    ("gs2d_poly", 0, np.float32, (100, 100), 4, 0),
    ("gs2d_fact", 8, np.float32, (100, 100), 3, 1),
]


def _case_id(c):
    return f"{c[0]}-hc{c[1]}-{'x'.join(map(str, c[3]))}-B{c[4]}-T{c[5]}"


def _setup(hc, dtype, shape, B, dev, seed=0):
    P = torch.from_numpy(_blocks(hc, len(shape), dtype, B, seed)).to(dev)
    rs = np.random.RandomState(seed)
    h0 = torch.from_numpy((0.2 + 0.3 * rs.rand(B, 2, *shape)).astype(dtype)).to(dev)
    return h0, P


@pytest.mark.parametrize("case", FWD_CASES, ids=_case_id)
def test_ensemble_forward_is_bitwise_per_sample(case, hip_device):
    import percnn_amd as pa
    _, hc, dtype, shape, B, T = case
    h0, P = _setup(hc, dtype, shape, B, hip_device)
    traj = pa.pi_rollout_ensemble(h0, P, T)
    assert traj.shape == (T + 1, B, 2) + shape
    for b in range(B):
        ref = pa.pi_rollout(h0[b:b + 1], P[b], T)
        assert bits_equal(traj[:, b], ref), f"sample {b}"
        assert torch.isfinite(ref).all()
    assert bits_equal(pa.pi_rollout_ensemble(h0, P, T), traj), "run to run"
    s = pa.pi_step_ensemble(h0, P)
    for b in range(B):
        assert bits_equal(s[b:b + 1], pa.pi_step(h0[b:b + 1], P[b]))


BWD_CASES = [c for c in FWD_CASES if c[5] > 0] + [("gs2d_poly", 0, np.float32, (128, 128), 3, 24)]


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "stride20"])
@pytest.mark.parametrize("case", BWD_CASES, ids=_case_id)
def test_ensemble_backward_per_sample(case, masked, hip_device):
    _, hc, dtype, shape, B, T = case
    import percnn_amd as pa
    h0, P = _setup(hc, dtype, shape, B, hip_device, seed=2)
    traj = pa.pi_rollout_ensemble(h0, P, T).contiguous()
    g = torch.from_numpy(np.random.RandomState(3).standard_normal(tuple(traj.shape)).astype(dtype)).to(hip_device)
    mask = bytes(1 if (t % 20 == 0 or t == T) else 0 for t in range(T + 1)) if masked else None
    g_h0, pg = _bwd_ensemble(traj, g, P, hc, shape, B, T, mask)
    g_h0b, pgb = _bwd_ensemble(traj, g, P, hc, shape, B, T, mask)
    assert torch.equal(g_h0, g_h0b) and torch.equal(pg, pgb), "run to run"
    tol = 1e-6 if dtype == np.float32 else 1e-10
    for b in range(B):
        g0, p1 = _bwd_single(traj[:, b].contiguous(), g[:, b].contiguous(), P[b].contiguous(), hc, shape, T, mask)
        assert bits_equal(g_h0[b], g0), f"dL/dh0 of sample {b}"
        err = rel_l2(pg[b].cpu().numpy(), p1.cpu().numpy())
        print(f"sample {b}: gradient row rel-L2 {err:.3g}")
        assert err < tol, f"gradient row {b}"
    # the step entry point: per-sample adjoint and gradient row
    x, gs = h0.contiguous(), g[1].contiguous()
    gi, ps = ensemble_step_bwd(x, gs, P, hc, shape, B)
    for b in range(B):
        g1, p1 = pa.step_bwd(x[b], gs[b], P[b].contiguous())
        assert bits_equal(gi[b], g1), f"step dL/dh of sample {b}"
        assert rel_l2(ps[b].cpu().numpy(), p1.double().cpu().numpy()) < tol


@pytest.mark.parametrize("hc", [0, 8])
def test_ensemble_matches_oracle(hc, hip_device):
    """each sample against the plain-C oracle with its own block: states and dL/dh0 bit-identical, gradient rows within 5e-5"""
    import percnn_amd as pa
    from oracle import pi_oracle as O
    B, T, shape = 3, 9, (32, 40)
    h0, P = _setup(hc, np.float32, shape, B, hip_device, seed=4)
    traj = pa.pi_rollout_ensemble(h0, P, T).contiguous()
    g = torch.from_numpy(np.random.RandomState(5).standard_normal(tuple(traj.shape)).astype(np.float32)).to(hip_device)
    g_h0, pg = _bwd_ensemble(traj, g, P, hc, shape, B, T, None)
    for b in range(B):
        hb, Pb, gb = h0[b].cpu().numpy(), P[b].cpu().numpy(), g[:, b].cpu().numpy()
        if hc == 0:
            ref = O.poly_rollout_fwd(hb, Pb, T)
            g0_o, pg_o = O.poly_rollout_bwd(ref, gb, Pb)
        else:
            ref = O.rollout_fwd(hb, Pb, hc, T)
            g0_o, pg_o = O.rollout_bwd(ref, gb, Pb, hc)
        assert np.array_equal(traj[:, b].cpu().numpy(), ref), f"states of sample {b}"
        assert np.array_equal(g_h0[b].cpu().numpy(), g0_o), f"dL/dh0 of sample {b}"
        err = rel_l2(pg[b].cpu().numpy(), pg_o)
        print(f"sample {b}: gradient row vs oracle rel-L2 {err:.3g}")
        assert err < 5e-5


def test_cell_ensemble_rcnn_vs_restatement(hip_device):
    import percnn_amd as pa
    from oracle import restatement as R
    B, T = 3, 12
    cells, ocells = [], []
    for b in range(B):
        torch.manual_seed(10 + b)
        c = pa.gs2d_cell(8, reaction="factored").to(hip_device)
        for p in c.filter_list:
            p.weight.data.mul_(20.0)
        c.dt = 0.5 * (1.0 - 0.1 * b)
        oc = R.gs2d_cell(8).to(hip_device)
        oc.load_state_dict(c.state_dict())
        oc.dt = c.dt
        cells.append(c)
        ocells.append(oc)
    ens = pa.CellEnsemble(cells)
    h0 = torch.cat([R.gs_initial_state((48, 48), seed=s) for s in range(B)]).to(hip_device)
    model = pa.RCNN(ens, step=T, effective_step=list(range(T)), init_state=h0)
    outs, second = model()
    assert len(outs) == T + 1 and all(o.shape == (B, 2, 48, 48) for o in outs)
    out = torch.cat(tuple(outs), dim=0)
    assert out.shape == ((T + 1) * B, 2, 48, 48)
    assert out.data_ptr() == outs.stacked.data_ptr()
    torch.nn.functional.mse_loss(out, torch.zeros_like(out)).backward()
    dt = np.dtype(np.float32)
    got = out.detach().view(T + 1, B, 2, 48, 48)
    for b in range(B):
        oref = R.OracleRCNN(ocells[b], step=T, effective_step=list(range(T)), init_state=h0[b:b + 1])
        routs, rsecond = oref()
        rout = torch.cat(tuple(routs), dim=0)
        # the ensemble's loss averages over B samples: sample b's share is 1/B of its own mean
        (torch.nn.functional.mse_loss(rout, torch.zeros_like(rout)) / B).backward()
        assert rel_l2(got[:, b].cpu().numpy(), rout.detach().cpu().numpy()) < TOL_TRAJ[dt]
        assert rel_l2(second[b:b + 1].detach().cpu().numpy(), rsecond.detach().cpu().numpy()) < TOL_TRAJ[dt]
        nq = 0
        for (n, p), (_, q) in zip(cells[b].named_parameters(), ocells[b].named_parameters()):
            if q.grad is not None and p.grad is not None and float(q.grad.abs().max()) > 0:
                assert rel_l2(p.grad.cpu().numpy(), q.grad.cpu().numpy()) < 10 * TOL_GRAD[dt], (b, n)
                nq += 1
        assert nq > 0
    assert torch.equal(model.trajectory().detach().flatten(0, 1), out.detach())
    # one step of the ensemble module
    s, s2 = ens(h0)
    assert s is s2
    for b in range(B):
        assert torch.equal(s[b:b + 1], cells[b](h0[b:b + 1])[0])
    with pytest.raises(ValueError):
        pa.RCNN(ens, step=T, effective_step=list(range(T)), init_state=h0[:2])()
    with pytest.raises(ValueError):
        model.observe(slice(None), 2)
    with pytest.raises(ValueError):
        model.loss_mse()


@pytest.mark.parametrize("hc", [0, 8])
def test_ensemble_with_identical_blocks_is_the_batched_path(hc, hip_device):
    import percnn_amd as pa
    B, T, shape = 4, 13, (100, 100)
    h0, P = _setup(hc, np.float32, shape, 1, hip_device, seed=6)
    h0 = torch.from_numpy((0.2 + 0.3 * np.random.RandomState(7).rand(B, 2, *shape)).astype(np.float32)).to(hip_device)
    Pe = P.expand(B, -1).contiguous()
    traj = pa.pi_rollout_ensemble(h0, Pe, T)
    ref = pa.pi_rollout_batched(h0, P[0], T)
    assert bits_equal(traj, ref)
    g = torch.from_numpy(np.random.RandomState(8).standard_normal(tuple(traj.shape)).astype(np.float32)).to(hip_device)
    g0e, pge = torch.ops.percnn.pi_rollout_ensemble_backward(traj.contiguous(), Pe, g, "")
    g0b, pgb = torch.ops.percnn.pi_rollout_batched_backward(ref.contiguous(), P[0], g, "")
    assert bits_equal(g0e, g0b)
    assert rel_l2(pge.double().sum(0).cpu().numpy(), pgb.double().cpu().numpy()) < 1e-6


def test_ensemble_guard_packs_every_member_factored(hip_device):
    """one member past the poly guard's bound (A > 10, test_safety_gpu.py): the whole ensemble runs factored, each sample bit
    for bit its own cell's factored rollout"""
    import percnn_amd as pa
    from test_host_logic import _cubic_well_block
    from test_safety_gpu import _cell_from_block
    T, a = 30, 50.0
    blocks = [_cubic_well_block(0.0, 1.0, 0.1), _cubic_well_block(a, 1.0, 0.1), _cubic_well_block(0.0, 1.0, 0.08)]
    cells = [_cell_from_block(P.astype(np.float32), hip_device) for P in blocks]
    refs = [_cell_from_block(P.astype(np.float32), hip_device, reaction="factored") for P in blocks]
    for c in cells:
        c.state_bound = (a + 1.0, a + 1.0) if c is cells[1] else (1.0, 1.0)
    rs = np.random.RandomState(0)
    h0 = torch.from_numpy(np.concatenate([(a if b == 1 else 0.0) + rs.uniform(-1, 1, (1, 2, 48, 48))
                                          for b in range(3)]).astype(np.float32)).to(hip_device)
    ens = pa.CellEnsemble(cells)
    with torch.no_grad(), pytest.warns(RuntimeWarning, match="ill-conditioned"):
        Pe = ens.param_block()
        got = pa.RCNN(ens, step=T, effective_step=list(range(T)), init_state=h0).trajectory()
    assert Pe.shape == (3, 16 + 2 * 81)
    assert cells[1].effective_reaction == "factored" and cells[0].effective_reaction == "poly"
    with torch.no_grad():
        for b in range(3):
            want = pa.RCNN(refs[b], step=T, effective_step=list(range(T)), init_state=h0[b:b + 1]).trajectory()
            assert bits_equal(got[:, b], want), f"sample {b}"


def test_gray_scott_fk_map(hip_device):
    import percnn_amd as pa
    from percnn_amd import physics
    from oracle import restatement as R
    cell = pa.gs2d_cell(8).to(hip_device)
    fk = [(0.025, 0.055), (0.04, 0.06), (0.03, 0.062), (0.022, 0.051)]
    P = torch.stack([physics.gray_scott_block(cell, 2e-5, 5e-6, f, k) for f, k in fk]).detach()
    assert P.shape == (4, 36)
    h0 = torch.cat([R.gs_initial_state((100, 100), seed=s) for s in range(4)]).to(hip_device)
    T = 40
    traj = pa.pi_rollout_ensemble(h0, P, T)
    for b in range(4):
        assert bits_equal(traj[:, b], pa.pi_rollout(h0[b:b + 1], P[b], T)), f"(f, k) = {fk[b]}"
    assert not torch.equal(traj[-1, 0], traj[-1, 1])


def test_ensemble_gradcheck_fp64(hip_device):
    """dL/dh0 and dL/d(trainable block entries) of every sample: dt (slot 0) and the frozen stencil (3..15) carry no gradient"""
    import percnn_amd as pa
    h0, P = _setup(2, np.float64, (8, 8), 2, hip_device, seed=5)
    P0 = P.detach()
    q = torch.cat([P0[:, 1:3], P0[:, 16:]], 1).requires_grad_(True)
    h0.requires_grad_(True)

    def block(q):
        return torch.cat([P0[:, :1], q[:, :2], P0[:, 3:16], q[:, 2:]], 1)

    assert torch.autograd.gradcheck(lambda h, q: pa.pi_rollout_ensemble(h, block(q), 3), (h0, q), eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda h, q: pa.pi_step_ensemble(h, block(q)), (h0, q), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_ensemble_ops_opcheck(dtype, hip_device):
    import percnn_amd as pa
    from percnn_amd import ops
    ops.load_native()
    h0, P = _setup(0, np.float32 if dtype == torch.float32 else np.float64, (16, 16), 3, hip_device, seed=7)
    h0.requires_grad_(True)
    P.requires_grad_(True)
    torch.library.opcheck(torch.ops.percnn.pi_step_ensemble.default, (h0, P, ""))
    torch.library.opcheck(torch.ops.percnn.pi_rollout_ensemble.default, (h0, P, 4, ""))
    assert pa.pi_rollout_ensemble(h0, P, 2).shape == (3, 3, 2, 16, 16)


def test_ensemble_torch_compile_fullgraph(hip_device):
    import percnn_amd as pa
    h, P = _setup(0, np.float32, (32, 32), 3, hip_device, seed=9)

    def f(x):
        y = pa.pi_step_ensemble(x, P)
        return pa.pi_rollout_ensemble(y, P, 3)

    got = torch.compile(f, fullgraph=True)(h)
    assert torch.equal(got, f(h))


def test_ensemble_errors(hip_device):
    import percnn_amd as pa
    h, P = _setup(0, np.float32, (16, 16), 3, hip_device, seed=11)
    with pytest.raises(RuntimeError):
        pa.pi_rollout_ensemble(h, P[:2], 3)                              # B mismatch
    with pytest.raises(RuntimeError):
        pa.pi_rollout_ensemble(h, P[0], 3)                               # a 1-D block
    with pytest.raises(RuntimeError):
        pa.pi_step_ensemble(h, P[:, :30].contiguous())                    # not a block length
    burgers = pa.Stage3BurgersCell().to(hip_device)
    Pa = burgers.param_block().detach()
    hb = torch.rand(2, 2, 16, 16, device=hip_device, dtype=Pa.dtype)
    with pytest.raises(RuntimeError):
        pa.pi_rollout_ensemble(hb, torch.stack([Pa, Pa]), 3)              # advective blocks
    with pytest.raises(RuntimeError):
        pa.pi_step_ensemble(hb[:1], Pa[None])
    # the batched operators keep rejecting 2-D blocks
    with pytest.raises(RuntimeError):
        pa.pi_rollout_batched(h, P, 2)
    with pytest.raises(RuntimeError):
        pa.pi_step_batched(h, P)
