"""Case lists and references of test_observed_loss_gpu.py, read without a GPU by test_observed_loss_cpu.py.  The grids, batch
sizes and T are those of batched_loss_util.py; every case is crossed with the (frames, strides) pairs below."""
import numpy as np
import torch

from batched_loss_util import FACTORS, MANY_CASE, MISALIGNED_CASE, PATHS, SWEEP_B, SWEEP_KINDS, T_SWEEP, factors, sweep_cases  # noqa: F401
from util import make_inputs

TARGETS = (False, True)         # without / with a compact target


def obs_pairs(ndim):
    """(t_idx, strides): every frame with the reference's own stride; a progression inside the K-groups with a stride that is
    no power of two and divides none of 64, 100, 37, 16; the top frame alone with an anisotropic stride; frame 0 alone; a run
    inside one K-group"""
    ref = 4 if ndim == 2 else 2
    return [(list(range(T_SWEEP + 1)), ref), ([0, 3, 6], 3), ([T_SWEEP], (2, 5) if ndim == 2 else (1, 3, 2)), ([0], ref),
            ([2, 3, 4, 7], 3)]


def strides_of(s, ndim):
    return (int(s),) * ndim if isinstance(s, int) else tuple(int(x) for x in s)


def compact_shape(shape, strides):
    return tuple(-(-n // s) for n, s in zip(shape, strides))


def lattice(strides):
    """index of the lattice points of a [..., *S] tensor"""
    return (Ellipsis,) + tuple(slice(None, None, s) for s in strides)


def obs_inputs(c):
    return make_inputs(c)


def compact_target(c, n, strides, seed=0):
    """[n,B,2,*Sc], uniform in [0, 1) as the dense tests' target"""
    rs = np.random.RandomState(3000 + c["seed"] + seed)
    return rs.uniform(0, 1, (n, c["B"], 2) + compact_shape(c["shape"], strides)).astype(c["dtype"].type)


def materialised_obs_gradient(traj, target_c, t_idx, strides, scale, dev_scale):
    """dense g [T+1,B,2,*S]: a_b * (traj - target_c) on the lattice of the frames t_idx, rounded as the kernels round (a_b =
    (T)scale * dev_scale[b], one subtraction, one multiplication), zero everywhere else"""
    a = (torch.tensor(scale, dtype=traj.dtype, device=traj.device) * dev_scale).view((-1,) + (1,) * (traj.dim() - 2))
    g = torch.zeros_like(traj)
    sub = lattice(strides)
    for k, t in enumerate(t_idx):
        d = traj[t][sub] if target_c is None else traj[t][sub] - target_c[k]
        g[t][sub] = a * d
    return g


def obs_losses_f64(traj, target_c, t_idx, strides, weight):
    """[B] float64: weight * sum over the frames t_idx and the lattice of (traj - target_c)^2, per sample, by tensor ops"""
    pred = traj[list(t_idx)][lattice(strides)].double()
    d = pred if target_c is None else pred - target_c.double()
    return (d ** 2).sum(dim=tuple(i for i in range(d.dim()) if i != 1)) * weight


def mean_weight(n, shape, strides):
    return 1.0 / (n * 2 * int(np.prod(compact_shape(shape, strides))))
