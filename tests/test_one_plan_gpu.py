"""The plan queries and the rollout entry points follow one plan (csrc/pi_abi.hip "the rollout plan").  On the device: the two option
combinations where percnn_pi_debug_plan once differed from what was launched, and -- where the process can see which path a call
took, through the launch counter of the residency guard -- that plan and launch agree.

Options travel per call, never through pa.set_option."""
import numpy as np
import pytest
import torch

from percnn_amd import _lib
from util import random_block, rel_l2

pytestmark = pytest.mark.gpu


def dev_t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def rollout(shape, dtype, T, device, seed, options=None):
    import percnn_amd as pa
    rs = np.random.RandomState(seed)
    P = dev_t(random_block(0, len(shape), dtype, seed + 12, scale=0.1), device)
    traj = torch.empty((T + 1, 2) + shape, dtype=torch.float32 if dtype == np.float32 else torch.float64, device=device)
    traj[0] = dev_t(rs.uniform(0, 1, (2,) + shape).astype(dtype), device)
    pa.rollout_fwd_(traj, P, options=options)
    g = torch.randn(traj.shape, dtype=traj.dtype, device=device, generator=torch.Generator(device=device).manual_seed(seed)) / traj[0].numel()
    return P, traj, g


def test_resident_3d_sweep_does_not_ask_for_the_brick_kernels(hip_device):
    """(32, 32, 64), T = 17: the smallest grid the resident 3D sweep admits (2 x 2 x 2 blocks, 16 steps at least).  The sweep takes it
    for every 3D problem whose steps are launches of their own and carry the gradient sums; brick3d = 0 only moves the
    launch-per-step fall-back to the direct kernels.  The query used to demand the adjoint family "bricks" on top and said
    `bwd_persistent: False` for a call that ran the resident kernel."""
    import percnn_amd as pa
    shape, T = (32, 32, 64), 17
    P, traj, g = rollout(shape, np.float32, T, hip_device, 17)
    plan = _lib.rollout_plan(0, shape, 4, {"res3d": 2, "brick3d": 0})
    assert plan["bwd_persistent"] and plan["bwd"] == "direct" and plan["fused_gradients"]
    n0 = _lib.persist_status()["launches"]
    a0, ag = pa.rollout_bwd(traj, g, P, options={"res3d": 2, "brick3d": 0})
    assert _lib.persist_status()["launches"] == n0 + 1
    b0, bg = pa.rollout_bwd(traj, g, P, options={"res3d": 2})       # the same resident kernel
    assert _lib.persist_status()["launches"] == n0 + 2 and _lib.persist_status()["aborts"] == 0
    assert torch.equal(a0, b0)
    assert rel_l2(ag.cpu().numpy(), bg.cpu().numpy()) < 2e-6
    assert not _lib.rollout_plan(0, shape, 4, {"res3d": 0, "brick3d": 0})["bwd_persistent"]
    pa.rollout_bwd(traj, g, P, options={"res3d": 0, "brick3d": 0})
    assert _lib.persist_status()["launches"] == n0 + 2


def test_tile_height_next_to_two_steps_per_launch_is_ignored(hip_device):
    """(64, 64), T = 6, one frame mask: tile_k = 2 selects the kernel of 32 x 32 tiles on 256 lanes whatever tile_by says, so
    trajectory, dL/dh0 and the parameter gradient are the bits of tile_k = 2 alone -- and so is the plan, which used to report
    (and count partial rows for) 8-row tiles."""
    import percnn_amd as pa
    shape, T = (64, 64), 6
    mask = [t != 3 for t in range(T + 1)]
    both, alone = "tile_k=2,tile_by=8", "tile_k=2"
    assert _lib.rollout_plan(0, shape, 4, both) == _lib.rollout_plan(0, shape, 4, alone)
    assert _lib.rollout_plan(0, shape, 4, both)["tile"] == (32, 32, 256)
    P, traj_a, g = rollout(shape, np.float32, T, hip_device, 23, options=both)
    _, traj_b, _ = rollout(shape, np.float32, T, hip_device, 23, options=alone)
    assert torch.equal(traj_a, traj_b)
    a0, ag = pa.rollout_bwd(traj_a, g, P, frame_mask=mask, options=both)
    b0, bg = pa.rollout_bwd(traj_b, g, P, frame_mask=mask, options=alone)
    assert torch.equal(a0, b0) and torch.equal(ag, bg)


@pytest.mark.parametrize("options", [None, {"tile_persist": 0}], ids=["default", "tile_persist=0"])
@pytest.mark.parametrize("shape,dtype", [((128, 128), np.float32), ((128, 128), np.float64), ((100, 100), np.float32)])
def test_resident_launches_are_the_ones_the_plan_names(shape, dtype, options, hip_device):
    """T = 32 (eight groups, the shortest rollout the resident forward takes): the guard counts one launch for a forward and one
    for a backward exactly when fwd_persistent / bwd_persistent say so."""
    import percnn_amd as pa
    plan = _lib.rollout_plan(0, shape, np.dtype(dtype).itemsize, options)
    if options is not None:
        assert not plan["fwd_persistent"] and not plan["bwd_persistent"]
    n0 = _lib.persist_status()["launches"]
    P, traj, g = rollout(shape, dtype, 32, hip_device, 31, options=options)
    n1 = _lib.persist_status()["launches"]
    assert n1 - n0 == int(plan["fwd_persistent"]), plan
    pa.rollout_bwd(traj, g, P, options=options)
    assert _lib.persist_status()["launches"] - n1 == int(plan["bwd_persistent"]), plan
    assert _lib.persist_status()["aborts"] == 0
