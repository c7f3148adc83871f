"""GPU: the frame-list protocol of ``functional.frame_outputs`` / ``frame_grads`` on every fused rollout node that hands its
trajectory back as frames -- Pi single, batched and ensemble, Stage-1, LibraryCell and LibraryEnsemble (both integrators).
However the loss reaches the node -- on the frames, on the stacked output, on both, or on a few frames only -- dL/dh0 and the
parameter gradient are the same bits.  8x8 grid (one 8-wide Runge-Kutta tile; the library kernels need H, W >= 5), T = 3, B = 3."""
import numpy as np
import pytest
import torch

import library_cell_util as LU
import util as U

pytestmark = pytest.mark.gpu

T, B, S = 3, 3, (8, 8)


def _pi(rows, ensemble=False):
    from percnn_amd import functional as F
    P = U.ensemble_blocks(2, 2, np.float64, B, 11) if ensemble else U.random_block(2, 2, np.float64, 11)
    fn = F.pi_rollout_frames if rows == 1 else F.pi_rollout_ensemble_frames if ensemble else F.pi_rollout_batched_frames
    return torch.float64, rows, torch.as_tensor(P), lambda h0, P, frames: fn(h0, P, T, frames, with_stacked=True)


def _stage1():
    import percnn_amd as pa
    torch.manual_seed(5)
    P = pa.Stage1Cell("lo").param_block().detach()
    return torch.float32, 1, P, lambda h0, P, frames: pa.stage1.Stage1RolloutFramesFunction.apply(h0, P, T, tuple(frames))


def _library(rows, integrator):
    from percnn_amd import library_cell as lc
    C = np.stack([LU.coefficient_set(LU.SETS[b % 3]) for b in range(rows)])
    node = lc.LibraryRolloutFramesFunction if rows == 1 else lc.LibraryEnsembleRolloutFramesFunction
    return (torch.float64, rows, torch.as_tensor(C[0] if rows == 1 else C),
            lambda h0, C, frames: node.apply(h0, C, LU.DX, LU.DT, T, tuple(frames), integrator))


NODES = {"pi": lambda: _pi(1), "pi_batched": lambda: _pi(B), "pi_ensemble": lambda: _pi(B, ensemble=True), "stage1": _stage1,
         "library_euler": lambda: _library(1, "euler"), "library_rk4": lambda: _library(1, "rk4"),
         "library_ensemble_euler": lambda: _library(B, "euler"), "library_ensemble_rk4": lambda: _library(B, "rk4")}


@pytest.mark.parametrize("name", list(NODES))
def test_every_gradient_routing_gives_the_same_bits(name, hip_device):
    dtype, R, param, rollout = NODES[name]()
    gen = torch.Generator().manual_seed(7)
    state = (0.5 * torch.randn((R, 2) + S, generator=gen, dtype=torch.float64)).to(dtype).to(hip_device)
    w = torch.randn(((T + 1) * R, 2) + S, generator=gen, dtype=torch.float64).to(dtype).to(hip_device)     # the upstream gradient
    param = param.to(hip_device)

    def grads(frames, loss):
        h0, p = state.clone().requires_grad_(True), param.clone().requires_grad_(True)
        outs = rollout(h0, p, frames)
        assert len(outs) == len(frames) + 1 and outs[-1].shape == w.shape and all(f.shape == state.shape for f in outs[:-1])
        loss(outs[:-1], outs[-1]).backward()
        assert h0.grad.shape == h0.shape and p.grad.shape == p.shape and p.grad.dtype == p.dtype
        return h0.grad, p.grad

    every = tuple(range(T + 1))
    on_frames = grads(every, lambda fr, st: (torch.cat(tuple(fr)) * w).sum())
    on_stacked = grads(every, lambda fr, st: (st * w).sum())
    on_both = grads(every, lambda fr, st: 0.5 * (torch.cat(tuple(fr)) * w).sum() + 0.5 * (st * w).sum())      # 0.5 w + 0.5 w == w
    assert bool(on_frames[0].abs().sum() > 0) and bool(on_frames[1].abs().sum() > 0)
    for other in (on_stacked, on_both):
        assert torch.equal(on_frames[0], other[0]) and torch.equal(on_frames[1], other[1]), name

    # frames 0 and 2 only, frame 2 handed out twice: the dense route fed the same gradient scattered into zeros
    wf = w.view((T + 1, R, 2) + S)
    sparse = grads((0, 2, 2), lambda fr, st: (fr[0] * wf[0]).sum() + (fr[1] * wf[2]).sum() + (fr[2] * wf[1]).sum())
    scattered = torch.zeros_like(wf)
    scattered[0], scattered[2] = wf[0], wf[2] + wf[1]
    dense = grads((), lambda fr, st: (st * scattered.view(w.shape)).sum())
    assert torch.equal(sparse[0], dense[0]) and torch.equal(sparse[1], dense[1]), name
