"""GPU: the library cell's Runge-Kutta kernels (csrc/pi_lib.h: rk4_kernel, rk4_stage_kernel) -- the fused forward step bit for bit
against the numpy restatement, the rollout through ``pa.RCNN`` against the reference's forward_rk4 vectors in the Stage-3
goldens, the stage-by-stage adjoint and the dense coefficient gradient against autograd of the torch restatement, determinism,
order of convergence, refusals."""
import functools
import os

import numpy as np
import pytest
import torch

import library_cell_util as U
import library_rk4_util as R

pytestmark = pytest.mark.gpu


def _cell(name, support="dense", integrator="rk4"):
    import percnn_amd as pa
    return pa.LibraryCell(U.coefficient_set(name), U.DX, U.DT, support=support, integrator=integrator).cuda()


def _h0(shape, requires_grad=False):
    return torch.from_numpy(U.state(shape))[None].cuda().requires_grad_(requires_grad)


@functools.lru_cache(maxsize=None)
def _reference_rollout(shape, name):
    """max(STEPS) steps of the numpy restatement, computed once; shorter rollouts are its leading frames"""
    return R.np_rk4_rollout(U.state(shape), U.coefficient_set(name), U.DX, U.DT, max(U.STEPS))


@pytest.mark.parametrize("name", U.SETS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_is_the_restatement_bit_for_bit(shape, name):
    """(5, 5): the 8-wide halo wraps the grid more than once; (9, 17) .. (33, 17): one row / column beyond a tile; (136, 121),
    (121, 136): the 16 x 16 tile, with partial tiles on both axes"""
    from percnn_amd import library_cell as lc
    cell = _cell(name, support=None if name == "cross" else "dense")
    ref = _reference_rollout(shape, name)
    h0 = _h0(shape)
    # a fall-through to the Euler step would not pass: the two steps differ far beyond rounding
    assert U.rel_l2(U.np_step(ref[0], U.coefficient_set(name), U.DX, U.DT), ref[1]) > 1e-9
    with torch.no_grad():
        for T in U.STEPS:
            traj = cell.rollout(h0, T)
            assert traj.shape == (T + 1, 2) + shape and traj.dtype == torch.float64
            assert np.array_equal(traj.cpu().numpy(), ref[:T + 1]), (shape, name, T)
        a, b = cell(h0)
        assert a is b and a.shape == h0.shape and np.array_equal(a.cpu().numpy()[0], ref[1])
        C = cell.param_block().detach()
        one = lc.step_fwd(h0, C, U.DX, U.DT, integrator="rk4")
        assert one.shape == h0.shape and np.array_equal(one.cpu().numpy()[0], ref[1])
        out = torch.full_like(h0, float("nan"))
        assert lc.step_fwd(h0, C, U.DX, U.DT, out=out, integrator="rk4") is out and torch.equal(out, one)
        # forward_rk4 of an Euler cell is the same step; the Euler cell's own step stays Euler
        euler = _cell(name, support=None if name == "cross" else "dense", integrator="euler")
        a, b = euler.forward_rk4(h0)
        assert a is b and a.shape == h0.shape and np.array_equal(a.cpu().numpy()[0], ref[1])
        assert np.array_equal(euler(h0)[0].cpu().numpy()[0], U.np_step(ref[0], U.coefficient_set(name), U.DX, U.DT))


def _golden_bars(z, pos, traj, loss, g, g_h0):
    """frames 1e-13, loss 1e-13, scalar gradients 1e-9 relative, dL/dh0 1e-11"""
    steps = int(z["rk4_steps"])
    for t in (1, steps):
        err = U.rel_l2(traj[t].detach().cpu().numpy(), z[f"rk4/{t}"][0])
        print("frame", t, err)
        assert err < 1e-13, t
    assert abs(loss - float(z["rk4_loss_meansq"])) < 1e-13
    for n, p in pos.items():
        ref = float(z["rk4_grad_meansq/" + n])
        print(n, g[p], ref, abs(g[p] - ref) / abs(ref))
        assert abs(g[p] - ref) <= 1e-9 * abs(ref), (n, g[p], ref)
    assert U.rel_l2(g_h0, z["rk4_grad_meansq_h0"]) < 1e-11


@pytest.mark.parametrize("name", U.GOLDENS)
def test_rcnn_rk4_rollout_vs_reference_goldens(name, hip_device):
    import percnn_amd as pa
    z = np.load(os.path.join(U.GOLDEN, name))
    stage3 = pa.Stage3BurgersCell() if name.startswith("bur") else pa.Stage3LambdaOmegaCell()
    stage3.load_state_dict({k[6:]: torch.tensor(z[k]) for k in z.files if k.startswith("param/")})
    cell = pa.LibraryCell.from_cell(stage3.to(hip_device), integrator="rk4")
    assert cell.coef.is_cuda and cell.integrator == "rk4"
    _, pos = U.golden_coefficients(z)
    steps = int(z["rk4_steps"])
    h0 = torch.from_numpy(z["h0"]).to(hip_device).requires_grad_(True)
    outs, second_last = pa.RCNN(cell, step=steps, effective_step=list(range(steps)), init_state=h0)()
    traj = torch.cat(tuple(outs), 0)
    assert traj.shape == (steps + 1,) + tuple(h0.shape[1:]) and traj.data_ptr() == outs[0].data_ptr()      # a view, no copy
    assert traj.data_ptr() == outs.stacked.data_ptr() and outs[3].data_ptr() == traj[3].data_ptr()
    assert torch.equal(second_last, traj[steps - 1:steps])
    loss = (traj[steps] ** 2).mean()
    loss.backward()
    g = cell.coef.grad.cpu().numpy()
    _golden_bars(z, pos, traj, loss.item(), g, h0.grad.cpu().numpy())
    off = np.ones((2, 10, 7), dtype=bool)
    for p in pos.values():
        off[p] = False
    assert (g[off] == 0).all()                                      # default support: nothing off the equation's form
    # the reference method's name on an Euler cell of the same equation: five forward_rk4 calls, stock autograd between them
    euler = pa.LibraryCell.from_cell(stage3)
    h0b = torch.from_numpy(z["h0"]).to(hip_device).requires_grad_(True)
    frames = [h0b]
    for _ in range(steps):
        frames.append(euler.forward_rk4(frames[-1])[0])
    assert torch.equal(torch.cat(frames, 0).detach(), traj.detach())
    loss = (frames[-1] ** 2).mean()
    loss.backward()
    _golden_bars(z, pos, torch.cat(frames, 0), loss.item(), euler.coef.grad.cpu().numpy(), h0b.grad.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _reference_grads(shape, name, T, selected):
    rng = np.random.default_rng(10000 * shape[0] + 100 * shape[1] + 10 * T + U.SETS.index(name))
    w = list(rng.standard_normal((T + 1, 2) + shape))
    if selected:                                                    # a loss on some frames only: first and last, or the last
        keep = {0, T} if T >= 2 else {T}
        w = [x if t in keep else None for t, x in enumerate(w)]
    return (w,) + R.torch_rk4_rollout_grads(U.state(shape), U.coefficient_set(name), U.DX, U.DT, T, w)


@pytest.mark.parametrize("name", U.SETS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_adjoint_and_dense_gradient_vs_autograd(shape, name):
    """loss = sum_t <w_t, frame_t> with random weights, on all frames and on a selection (the frame mask).  dL/dh0: rel-L2
    1e-11.  Each of the 140 coefficient gradients: |g - ref| <= 1e-10 sum_t sum_i sum_p |kappa_{i,s} phi_m(y_i) psi_k(y_i)|, the
    bars of the Euler test on the sum of absolute terms of the four stages."""
    cell = _cell(name)
    for T in U.STEPS:
        for selected in (False, True):
            w, g_h0, g_C, bound = _reference_grads(shape, name, T, selected)
            frames = [t for t in range(T + 1) if w[t] is not None]
            h0 = _h0(shape, requires_grad=True)
            cell.coef.grad = None
            outs = cell.rollout_frames(h0, T, frames)
            assert len(outs) == len(frames)
            sum((torch.from_numpy(w[t]).cuda() * f[0]).sum() for t, f in zip(frames, outs)).backward()
            what = (shape, name, T, selected)
            err_h = U.rel_l2(h0.grad.cpu().numpy()[0], g_h0)
            excess = np.abs(cell.coef.grad.cpu().numpy() - g_C) / bound
            print(what, "dL/dh0", err_h, "dL/dC / bound", float(excess.max()))
            assert err_h <= 1e-11, what
            assert (excess <= 1e-10).all(), (what, float(excess.max()), np.argwhere(excess > 1e-10)[:5])
    # the trajectory output carries the same gradient as its frames
    T = max(U.STEPS)
    w, g_h0, g_C, bound = _reference_grads(shape, name, T, False)
    h0 = _h0(shape, requires_grad=True)
    cell.coef.grad = None
    (torch.from_numpy(np.stack(w)).cuda() * cell.rollout(h0, T)).sum().backward()
    assert U.rel_l2(h0.grad.cpu().numpy()[0], g_h0) <= 1e-11
    assert (np.abs(cell.coef.grad.cpu().numpy() - g_C) <= 1e-10 * bound).all()


@pytest.mark.parametrize("shape", [(5, 5), (20, 70), (32, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_backward_twice_gives_the_same_bits(shape):
    from percnn_amd import library_cell as lc
    C = torch.from_numpy(U.coefficient_set("dense")).cuda()
    traj = torch.empty((8, 2) + shape, dtype=torch.float64, device="cuda")
    traj[0] = torch.from_numpy(U.state(shape))
    lc.rollout_fwd_(traj, C, U.DX, U.DT, integrator="rk4")
    assert np.array_equal(traj.cpu().numpy(), _reference_rollout(shape, "dense"))
    g_traj = torch.from_numpy(np.random.default_rng(3).standard_normal(traj.shape)).cuda()
    for mask in (None, [1, 0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0, 1, 0]):
        a = lc.rollout_bwd(traj, g_traj, C, U.DX, U.DT, frame_mask=mask, integrator="rk4")
        b = lc.rollout_bwd(traj, g_traj, C, U.DX, U.DT, frame_mask=mask, integrator="rk4")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (shape, mask)
        assert a[1].shape == (2, 10, 7) and bool(torch.isfinite(a[1]).all()) and bool(torch.isfinite(a[0]).all())


def test_order_of_convergence_on_the_kernels():
    """the setup of test_library_rk4_cpu.py::test_order_of_convergence_of_the_restatement through ``cell.rollout``"""
    import percnn_amd as pa
    h0 = torch.from_numpy(R.loop_state())[None].cuda()

    def final(integrator):
        def run(n):
            cell = pa.LibraryCell.from_equations(R.LOOP, R.LOOP_DX, R.LOOP_TIME / n, integrator=integrator).cuda()
            with torch.no_grad():
                return cell.rollout(h0, n)[n].cpu().numpy()
        return run

    rk4, euler = R.convergence_ratio(final("rk4")), R.convergence_ratio(final("euler"))
    print("rk4", rk4, "euler", euler)
    assert 15.0 <= rk4 <= 18.5
    assert 1.9 <= euler <= 2.2


def test_refused_inputs_name_the_argument():
    import percnn_amd as pa
    from percnn_amd import library_cell as lc
    cell = _cell("cross")
    ok = torch.zeros(1, 2, 8, 8, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="h0.*device"):
        cell.rollout(ok.cpu(), 2)
    with pytest.raises(RuntimeError, match="h0.*device"):
        cell(ok.cpu())
    with pytest.raises(RuntimeError, match="h0.*device"):
        _cell("cross", integrator="euler").forward_rk4(ok.cpu())
    with pytest.raises(TypeError, match="h0.*float64"):
        cell.rollout(ok.float(), 2)
    with pytest.raises(TypeError, match="h0.*float64"):
        cell.forward_rk4(ok.float())
    for bad in (ok[0], torch.zeros(3, 2, 8, 8, dtype=torch.float64, device="cuda"),
                torch.zeros(1, 3, 8, 8, dtype=torch.float64, device="cuda"),
                torch.zeros(1, 2, 8, 8, 8, dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError, match=r"h0.*\[1,2,H,W\]"):
            cell.rollout_frames(bad, 2, [0, 2])
        with pytest.raises(ValueError, match=r"h0.*\[1,2,H,W\]"):
            cell.forward_rk4(bad)
    for bad in ((4, 8), (8, 4)):
        with pytest.raises(ValueError, match="h0.*H, W >= 5"):
            cell.rollout(torch.zeros((1, 2) + bad, dtype=torch.float64, device="cuda"), 2)
        with pytest.raises(ValueError, match="h.*H, W >= 5"):
            lc.step_fwd(torch.zeros((1, 2) + bad, dtype=torch.float64, device="cuda"), cell.coef.detach(), 0.2, 1e-3,
                        integrator="rk4")
    with pytest.raises(RuntimeError, match="coef.*device"):
        lc.step_fwd(ok, cell.coef.detach().cpu(), 0.2, 1e-3, integrator="rk4")
    with pytest.raises(ValueError, match="coef"):
        lc.step_fwd(ok, cell.coef.detach().float(), 0.2, 1e-3, integrator="rk4")
    with pytest.raises(ValueError, match="g_traj"):
        lc.rollout_bwd(torch.zeros(3, 2, 8, 8, dtype=torch.float64, device="cuda"),
                       torch.zeros(2, 2, 8, 8, dtype=torch.float64, device="cuda"), cell.coef.detach(), 0.2, 1e-3,
                       integrator="rk4")
    with pytest.raises(RuntimeError, match="invalid argument"):
        lc.step_fwd(ok, cell.coef.detach(), 0.0, 1e-3, integrator="rk4")
    with pytest.raises(ValueError, match="integrator"):
        lc.step_fwd(ok, cell.coef.detach(), 0.2, 1e-3, integrator="rk2")
    with pytest.raises(ValueError, match="integrator"):
        lc.rollout_bwd(torch.zeros(3, 2, 8, 8, dtype=torch.float64, device="cuda"),
                       torch.zeros(3, 2, 8, 8, dtype=torch.float64, device="cuda"), cell.coef.detach(), 0.2, 1e-3,
                       integrator="rk2")
    # batched initial states have no path on this cell
    with pytest.raises(ValueError, match="batched"):
        pa.RCNN(cell, step=2, effective_step=[0, 1], init_state=torch.zeros(2, 2, 8, 8, dtype=torch.float64, device="cuda"))()
