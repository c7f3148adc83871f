"""GPU: the library cell's kernels (csrc/pi_lib.h) -- the forward step bit for bit against the numpy restatement, the rollout
through ``pa.RCNN`` against the reference-derived Stage-3 goldens, the adjoint and the dense coefficient gradient against
autograd of the torch restatement, determinism, discover -> from_equations -> the same trajectory, refusals."""
import functools
import os

import numpy as np
import pytest
import torch

import library_cell_util as U

pytestmark = pytest.mark.gpu


def _cell(name, support="dense"):
    import percnn_amd as pa
    return pa.LibraryCell(U.coefficient_set(name), U.DX, U.DT, support=support).cuda()


def _h0(shape, requires_grad=False):
    return torch.from_numpy(U.state(shape))[None].cuda().requires_grad_(requires_grad)


@functools.lru_cache(maxsize=None)
def _reference_rollout(shape, name):
    """max(STEPS) steps of the numpy restatement, computed once; shorter rollouts are its leading frames"""
    return U.np_rollout(U.state(shape), U.coefficient_set(name), U.DX, U.DT, max(U.STEPS))


@pytest.mark.parametrize("name", U.SETS)
@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_is_the_restatement_bit_for_bit(shape, name):
    cell = _cell(name, support=None if name == "cross" else "dense")
    ref = _reference_rollout(shape, name)
    h0 = _h0(shape)
    with torch.no_grad():
        for T in U.STEPS:
            traj = cell.rollout(h0, T)
            assert traj.shape == (T + 1, 2) + shape and traj.dtype == torch.float64
            assert np.array_equal(traj.cpu().numpy(), ref[:T + 1]), (shape, name, T)
        a, b = cell(h0)
        assert a is b and a.shape == h0.shape and np.array_equal(a.cpu().numpy()[0], ref[1])
        # the single-step entry point: the same bits as the rollout's first frame
        from percnn_amd import library_cell as lc
        one = lc.step_fwd(h0, cell.param_block().detach(), U.DX, U.DT)
        assert one.shape == h0.shape and np.array_equal(one.cpu().numpy()[0], ref[1])
        out = torch.full_like(h0, float("nan"))
        assert lc.step_fwd(h0, cell.param_block().detach(), U.DX, U.DT, out=out) is out and torch.equal(out, one)


@pytest.mark.parametrize("name", U.GOLDENS)
def test_rcnn_rollout_vs_reference_goldens(name, hip_device):
    """the bars of test_stage3_{burgers,lambda_omega}_cell_vs_reference: frames 1e-13, loss 1e-13, scalar gradients 1e-9
    relative (read from coef.grad at their positions), dL/dh0 1e-11"""
    import percnn_amd as pa
    z = np.load(os.path.join(U.GOLDEN, name))
    stage3 = pa.Stage3BurgersCell() if name.startswith("bur") else pa.Stage3LambdaOmegaCell()
    stage3.load_state_dict({k[6:]: torch.tensor(z[k]) for k in z.files if k.startswith("param/")})
    cell = pa.LibraryCell.from_cell(stage3.to(hip_device))
    assert cell.coef.is_cuda
    _, pos = U.golden_coefficients(z)
    steps = int(z["steps"])
    h0 = torch.from_numpy(z["h0"]).to(hip_device).requires_grad_(True)
    outs, second_last = pa.RCNN(cell, step=steps, effective_step=list(range(steps)), init_state=h0)()
    traj = torch.cat(tuple(outs), 0)
    assert traj.shape == (steps + 1,) + tuple(h0.shape[1:]) and traj.data_ptr() == outs[0].data_ptr()      # a view, no copy
    assert traj.data_ptr() == outs.stacked.data_ptr() and outs[3].data_ptr() == traj[3].data_ptr()
    assert torch.equal(second_last, traj[steps - 1:steps])
    for t in z["keep_t"]:
        assert U.rel_l2(traj[int(t)].detach().cpu().numpy(), z[f"traj/{int(t)}"]) < 1e-13, int(t)
    loss = (traj ** 2).mean()
    assert abs(loss.item() - float(z["loss_meansq"])) < 1e-13
    loss.backward()
    g = cell.coef.grad.cpu().numpy()
    for n, p in pos.items():
        ref = float(z["grad_meansq/" + n])
        print(name, n, g[p], ref, abs(g[p] - ref) / abs(ref))
        assert abs(g[p] - ref) <= 1e-9 * abs(ref), (n, g[p], ref)
    off = np.ones((2, 10, 7), dtype=bool)
    for p in pos.values():
        off[p] = False
    assert (g[off] == 0).all()                                      # default support: nothing off the equation's form
    assert U.rel_l2(h0.grad.cpu().numpy(), z["grad_meansq_h0"]) < 1e-11


@functools.lru_cache(maxsize=None)
def _reference_grads(shape, name, T, selected):
    rng = np.random.default_rng(10000 * shape[0] + 100 * shape[1] + 10 * T + U.SETS.index(name))
    w = list(rng.standard_normal((T + 1, 2) + shape))
    if selected:                                                    # a loss on some frames only: first and last, or the last
        keep = {0, T} if T >= 2 else {T}
        w = [x if t in keep else None for t, x in enumerate(w)]
    return (w,) + U.torch_rollout_grads(U.state(shape), U.coefficient_set(name), U.DX, U.DT, T, w)


@pytest.mark.parametrize("name", U.SETS)
@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_adjoint_and_dense_gradient_vs_autograd(shape, name):
    """loss = sum_t <w_t, frame_t> with random weights, on all frames and on a selection (the frame mask).  dL/dh0: rel-L2
    1e-11.  Each of the 140 coefficient gradients: |g - ref| <= 1e-10 sum_t sum_p |a_s phi_m psi_k|, the float64 reduction bar
    of DESIGN section 3 on the sum of absolute terms (many entries cancel heavily: no bar relative to the entry itself)."""
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


def test_default_support_leaves_the_other_entries_at_zero_gradient():
    cell = _cell("cross", support=None)
    C = U.coefficient_set("cross")
    h0 = _h0((13, 33), requires_grad=True)
    (cell.rollout(h0, 3) ** 2).sum().backward()
    g = cell.coef.grad.cpu().numpy()
    assert (g[C == 0] == 0).all() and (g[C != 0] != 0).all()
    dense = _cell("cross")                                          # the same equation, every entry trainable
    (dense.rollout(_h0((13, 33)), 3) ** 2).sum().backward()
    gd = dense.coef.grad.cpu().numpy()
    assert np.array_equal(gd[C != 0], g[C != 0]) and np.count_nonzero(gd[C == 0]) > 100


@pytest.mark.parametrize("shape", [(5, 5), (20, 70), (32, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_backward_twice_gives_the_same_bits(shape):
    from percnn_amd import library_cell as lc
    C = torch.from_numpy(U.coefficient_set("dense")).cuda()
    traj = torch.empty((8, 2) + shape, dtype=torch.float64, device="cuda")
    traj[0] = torch.from_numpy(U.state(shape))
    lc.rollout_fwd_(traj, C, U.DX, U.DT)
    g_traj = torch.from_numpy(np.random.default_rng(3).standard_normal(traj.shape)).cuda()
    for mask in (None, [1, 0, 0, 1, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0, 1, 0]):
        a = lc.rollout_bwd(traj, g_traj, C, U.DX, U.DT, frame_mask=mask)
        b = lc.rollout_bwd(traj, g_traj, C, U.DX, U.DT, frame_mask=mask)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (shape, mask)
        assert a[1].shape == (2, 10, 7) and bool(torch.isfinite(a[1]).all())


LOOP = {"u": {"ones*lap_u": 0.005, "v*u_x": -0.8, "u*u_y": -0.9, "u*v*v_y": 1.5},
        "v": {"ones*lap_v": 0.004, "v*u_y": 0.6, "u*v_x": -1.0, "v*v_y": -0.7}}


def test_discover_hands_the_equation_back():
    """An equation neither Stage-3 cell can express (transposed advection, a quadratic prefactor, the other species'
    derivative) on 32 x 32 periodic, 40 steps: ``discover`` returns exactly its eight terms, and the cell made from that result
    walks the same trajectory.

    Coefficient bar: the same equation and initial state on the CPU (numpy restatement -> stage2_util.explicit_moments ->
    train_stridge) recover the support with a worst relative coefficient error of 7.4e-15 (u; v: 4.7e-15); times four: 3e-14.
    Trajectory bar: a relative coefficient error d scales every increment by at most d, the 40 Euler steps add 40 roundings of
    2^-52, and a deviation grows by at most 1 + dt * 150 * 1.3 (the first-derivative stencil's norm 18 / (12 dx) times
    max |u|) < 1.05 per step, 1.05^40 < 7.1:  7.1 * (3e-14 + 40 * 2.2e-16) < 3e-13 rel-L2."""
    import percnn_amd as pa
    dx, dt, steps = 1.0 / 100, 2.5e-4, 40
    ys = torch.arange(32, dtype=torch.float64) / 32
    yy, xx = torch.meshgrid(ys, ys, indexing="ij")
    tp = 2 * np.pi
    u = torch.sin(tp * xx) * torch.cos(tp * yy) + 0.3 * torch.cos(2 * tp * xx + 0.5)
    v = torch.cos(tp * xx) * torch.sin(tp * yy) - 0.2 * torch.sin(tp * (xx + 2 * yy))
    h0 = torch.stack((u, v))[None].cuda()
    cell = pa.LibraryCell.from_equations(LOOP, dx, dt).cuda()
    with torch.no_grad():
        traj = cell.rollout(h0, steps)
    eqs = pa.discover(traj, dx, dt, region="periodic")
    for sp in "uv":
        assert list(eqs[sp]) == sorted(LOOP[sp], key=U.TERMS.index), eqs[sp]
    for sp in "uv":
        for t, c in eqs[sp].items():
            print(sp, t, c, LOOP[sp][t], abs(c - LOOP[sp][t]) / abs(LOOP[sp][t]))
    again = pa.LibraryCell.from_equations(eqs, dx, dt).cuda()
    assert torch.equal(again.support, cell.support)
    with torch.no_grad():
        err = U.rel_l2(again.rollout(h0, steps).cpu().numpy(), traj.cpu().numpy())
    print("trajectory", err)
    for sp in "uv":
        for t, c in eqs[sp].items():
            assert abs(c - LOOP[sp][t]) <= 3e-14 * abs(LOOP[sp][t]), (sp, t, c, LOOP[sp][t])
    assert err <= 3e-13


def test_refused_inputs_name_the_argument():
    import percnn_amd as pa
    from percnn_amd import library_cell as lc
    cell = _cell("cross")
    ok = torch.zeros(1, 2, 8, 8, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="h0.*device"):
        cell.rollout(ok.cpu(), 2)
    with pytest.raises(RuntimeError, match="h0.*device"):
        cell(ok.cpu())
    with pytest.raises(TypeError, match="h0.*float64"):
        cell.rollout(ok.float(), 2)
    for bad in (ok[0], torch.zeros(3, 2, 8, 8, dtype=torch.float64, device="cuda"),
                torch.zeros(1, 3, 8, 8, dtype=torch.float64, device="cuda"),
                torch.zeros(1, 2, 8, 8, 8, dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError, match=r"h0.*\[1,2,H,W\]"):
            cell.rollout_frames(bad, 2, [0, 2])
    for bad in ((4, 8), (8, 4)):
        with pytest.raises(ValueError, match="h0.*H, W >= 5"):
            cell.rollout(torch.zeros((1, 2) + bad, dtype=torch.float64, device="cuda"), 2)
    with pytest.raises(RuntimeError, match="coef.*device"):
        lc.step_fwd(ok, cell.coef.detach().cpu(), 0.2, 1e-3)
    with pytest.raises(ValueError, match="coef"):
        lc.step_fwd(ok, cell.coef.detach().float(), 0.2, 1e-3)
    with pytest.raises(ValueError, match="g_traj"):
        lc.rollout_bwd(torch.zeros(3, 2, 8, 8, dtype=torch.float64, device="cuda"),
                       torch.zeros(2, 2, 8, 8, dtype=torch.float64, device="cuda"), cell.coef.detach(), 0.2, 1e-3)
    with pytest.raises(RuntimeError, match="invalid argument"):
        lc.step_fwd(ok, cell.coef.detach(), 0.0, 1e-3)
    # batched initial states have no path on this cell
    with pytest.raises(ValueError, match="batched"):
        pa.RCNN(cell, step=2, effective_step=[0, 1], init_state=torch.zeros(2, 2, 8, 8, dtype=torch.float64, device="cuda"))()
