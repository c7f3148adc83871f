"""Case lists and references of test_batched_loss_gpu.py, read without a GPU by test_batched_loss_cpu.py."""
import numpy as np
import torch

from util import make_case, make_inputs

T_SWEEP = 9                     # two K = 4 tile launches plus one direct leftover step
FACTORS = [0.5, 0.0, -1.25]     # per-sample factors handed to the sweep: distinct, a zero among them, also for B = 2

# (shape, dtype, hc, options): the sweep families.  (64, 96) float32 poly by default dispatch runs 8-row tiles, whose sweep has
# no fused-moments flavour (TileVariant::mom, tile_variant_for of csrc/pi_abi.hip); "tile_by": 32 is the same grid on the 32 x 32 tiles that do fuse.
SWEEP_KINDS = [
    ((64, 96), np.float32, 0, None),
    ((64, 96), np.float32, 0, {"tile_fuse": 0}),
    ((64, 96), np.float32, 0, {"tile_by": 32}),                 # tile sweep, fused moments
    ((64, 96), np.float32, 0, {"tile_by": 32, "tile_fuse": 0}),  # the same tiles, split schedule
    ((40, 100), np.float32, 8, None),                           # ragged tiles, gradient pass
    ((64, 64), np.float64, 0, None),
    ((48, 72), np.float32, 0, {"tile": 0}),                     # direct 2D, vector lanes
    ((33, 37), np.float32, 2, None),                            # odd rows, VEC = 1
    ((12, 16, 64), np.float32, 0, None),                        # 3D, direct kernels
    ((6, 10, 9), np.float64, 3, None),
]
SWEEP_B = (2, 3)
PATHS = ("batch", "ensemble")
MODES = (1, 2)                  # without / with a target


def frame_sets(T):
    """the frame sets of test_squared_error_loss_inside_the_sweep"""
    return [None, list(range(0, T, 3)), [T], [0], [2, 3, 4, 7]]


def sweep_cases():
    return [make_case(11000 + 10 * k + B, shape, hc, dtype, B, T_SWEEP, "none", opts, seed=900 + k)
            for k, (shape, dtype, hc, opts) in enumerate(SWEEP_KINDS) for B in SWEEP_B]


MANY_CASE = make_case(11900, (2, 3), 0, np.float32, 513, 3, "none", None)
MISALIGNED_CASE = make_case(11910, (64, 96), 0, np.float32, 3, T_SWEEP, "none", None, seed=900)


def loss_inputs(c):
    """make_inputs of the case plus a target trajectory [T+1,B,2,*S] (uniform in [0, 1), as the unbatched test's)"""
    inp = make_inputs(c)
    rs = np.random.RandomState(2000 + c["seed"])
    inp["target"] = rs.uniform(0, 1, (c["T"] + 1, c["B"], 2) + c["shape"]).astype(c["dtype"].type)
    return inp


def factors(B, dtype, device):
    return torch.tensor([FACTORS[b % 3] * (1 + b // 3) for b in range(B)], dtype=dtype, device=device)


def materialised_gradient(traj, target, scale, dev_scale):
    """g[t, b] = a_b * (traj[t, b] - target[t, b]) by tensor ops, rounded as the kernels round: a_b = (T)scale * dev_scale[b],
    one subtraction, one multiplication"""
    a = torch.tensor(scale, dtype=traj.dtype, device=traj.device) * dev_scale
    d = traj if target is None else traj - target
    return a.view((1, -1) + (1,) * (traj.dim() - 2)) * d


def sample_losses_f64(traj, target, frames, weight):
    """[B] float64: weight * sum over the selected frames of sum_x (traj - target)^2, per sample, by tensor ops"""
    sel = slice(None) if frames is None else frames
    d = traj[sel].double() if target is None else traj[sel].double() - target[sel].double()
    return (d ** 2).sum(dim=tuple(i for i in range(d.dim()) if i != 1)) * weight
