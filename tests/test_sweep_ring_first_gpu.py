"""GPU: the resident split sweep (pi_adj2d_persist_split_kernel) on its smallest grids, over the first hand-overs.

Pass P1 of a group asks for pass P2's pointwise operands after its own arithmetic instead of before it, and the wait for the
halo ring looks at the ring's granules only (docs/NOTEBOOK.md section 24).  Only the moment at which loads are issued and waited
for moved: no value and no order of a sum did.  So dL/dh0 is the launch-per-group sweep's bit for bit and the parameter-block
gradient agrees with it within the bounds test_hip_parity.py holds the same comparison to (float32: 2e-6,
test_persistent_sweep_equals_launch_per_group; float64: 1e-12, test_persistent_sweep_float64_equals_launch_per_group).

Grids: 128 x 128 is the smallest the dispatch runs resident (16 tiles of 32 x 32; asserted from the plan), 128 x 256 tells rows
from columns.  Horizons: T = 8 is two groups -- one hand-over, the first --, T = 11 leaves three steps to the direct kernels,
T = 20 is five groups.  dL/dtraj dense, and under frame masks that skip frames: a skipped frame reaches the moved request as a
null injection frame (its lanes then read the state frame, as everywhere)."""
import numpy as np
import pytest
import torch

from util import random_block, rel_l2

pytestmark = pytest.mark.gpu

# grids this small take 8-row tiles by default; with the small-tile resident sweep off, "bwd_persistent" means the 32 x 32 one
BASE = {"tile_by": 32, "persist_small": 0}
TOL = {4: 2e-6, 8: 1e-12}


def test_smallest_resident_grid_is_128_by_128(hip_device):
    from percnn_amd import _lib
    for esz in (4, 8):
        for shape in ((128, 128), (128, 256)):
            plan = _lib.rollout_plan(0, shape, esz, BASE)
            assert plan["bwd_persistent"] and plan["bwd"] == "tile2d" and plan["tile"][:2] == (32, 32), plan
            assert not _lib.rollout_plan(0, shape, esz, dict(BASE, tile_persist=0))["bwd_persistent"]
        # fewer than 16 tiles, in either direction: launch per group
        assert not _lib.rollout_plan(0, (96, 128), esz, BASE)["bwd_persistent"]
        assert not _lib.rollout_plan(0, (128, 96), esz, BASE)["bwd_persistent"]
    # the split flavour is what runs (the unsplit one is an option, float32 only)
    assert _lib.rollout_plan(0, (128, 128), 4, dict(BASE, persist_split=0))["bwd_persistent"]
    assert not _lib.rollout_plan(0, (128, 128), 8, dict(BASE, persist_split=0))["bwd_persistent"]


@pytest.mark.parametrize("T", [8, 11, 20])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(128, 128), (128, 256)], ids=lambda s: "x".join(map(str, s)))
def test_resident_split_sweep_equals_launch_per_group(shape, dtype, T, hip_device):
    import percnn_amd as pa
    from percnn_amd import _lib
    esz = np.dtype(dtype).itemsize
    tdt = torch.float32 if esz == 4 else torch.float64
    assert _lib.rollout_plan(0, shape, esz, BASE)["bwd_persistent"]
    P = torch.tensor(random_block(0, 2, dtype, 21, scale=0.1), device=hip_device)
    traj = torch.empty((T + 1, 2) + shape, dtype=tdt, device=hip_device)
    traj[0] = torch.tensor(np.random.RandomState(4).uniform(0, 1, (2,) + shape).astype(dtype), device=hip_device)
    pa.rollout_fwd_(traj, P, options=dict(BASE, tile_persist=0))
    assert torch.isfinite(traj[-1]).all()
    g = (torch.randn(traj.shape, dtype=tdt, device=hip_device, generator=torch.Generator(device=hip_device).manual_seed(1))
         / traj[0].numel())
    masks = (None, [t % 3 != 1 for t in range(T + 1)], [t == T or t % 5 == 0 for t in range(T + 1)])
    n0 = _lib.persist_status()
    for i, mask in enumerate(masks):
        a0, ag = pa.rollout_bwd(traj, g, P, frame_mask=mask, options=BASE)
        torch.cuda.synchronize()
        n1 = _lib.persist_status()
        b0, bg = pa.rollout_bwd(traj, g, P, frame_mask=mask, options=dict(BASE, tile_persist=0))
        torch.cuda.synchronize()
        n2 = _lib.persist_status()
        # one resident launch for the first sweep, none for the second, nothing aborted
        assert n1["launches"] == n0["launches"] + i + 1 and n2["launches"] == n1["launches"], (n0, n1, n2)
        assert n2["aborts"] == n0["aborts"] and not n2["disabled_on_current_device"]
        assert float(a0.abs().max()) > 0
        it = torch.int32 if esz == 4 else torch.int64
        assert torch.equal(a0.view(it), b0.view(it)), f"dL/dh0, mask {i}"
        err = rel_l2(ag.cpu().numpy(), bg.cpu().numpy())
        print(f"mask {i}: parameter-block gradient against the launch-per-group sweep, rel-L2 {err:.3e} (bound {TOL[esz]:.0e})")
        assert err < TOL[esz], f"parameter gradient, mask {i}: {err:.3e}"
