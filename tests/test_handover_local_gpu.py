"""GPU: option handover_local of the 32 x 32 resident forward (pi_fwd2d_persist_kernel; the resident sweep,
pi_adj2d_persist_split_kernel, runs in every case below and is always written through).  Band granules whose readers all run on
the publisher's XCD are published with plain stores and stay in that XCD's L2, the others are written through.  The policy
decides how a granule travels, never what it holds or in which order anything is summed: the trajectory, dL/dh0 AND the parameter-block gradient are the same bits with the option on and off, and trajectory and dL/dh0
are the launch-per-group path's bits.  percnn_pi_persist_status proves that the resident launches ran and none aborted.

The float64 parameter-block gradient is taken from a sweep that is deterministic by construction.  The resident float64 sweep
(pi_adj2d_persist_split_kernel<double>, which this option never reaches) lets lanes tid and tid + 256 add their moments to ONE
LDS slot with ds_add_f64 atomics, so two runs of the SAME call may differ in the last bit of a component
(test_persistent_sweep_float64_equals_launch_per_group holds it to 1e-12 for that reason): compared between two settings it
would measure that kernel's reproducibility, not the hand-over.  So the float64 cases sweep each setting's own trajectory once
more with adj_persist_f64 = 0 -- per-lane moment rows, fixed order -- and compare THOSE gradients bitwise; the resident sweep
still runs for dL/dh0 and the launch count.  The float32 sweep keeps per-lane sums: its gradient is compared as it comes."""
import numpy as np
import pytest
import torch

from util import random_block

pytestmark = pytest.mark.gpu

# 128 x 128: 16 tiles in rectangles of 2 x 1 tiles -- every tile has local and remote readers across the periodic wrap;
# 256 x 128: rectangles of 2 x 2 tiles, the first shape with a local diagonal reader; 160 x 160: 25 tiles, identity map,
# nothing local; float64: the 16-byte granules of one value (lambda-omega's kernels).  T = 38 leaves two steps to the direct kernels.
CASES = [((128, 128), np.float32), ((256, 128), np.float32), ((160, 160), np.float32), ((128, 128), np.float64)]


@pytest.mark.parametrize("T", [40, 38])
@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name)
def test_local_handover_is_bit_identical(shape, dtype, T, hip_device):
    import percnn_amd as pa
    from percnn_amd import _lib
    esz = np.dtype(dtype).itemsize
    base = {"tile_by": 32}                                 # (grids this small take 8-row tiles by default)
    for hl in (0, 1):
        plan = _lib.rollout_plan(0, shape, esz, dict(base, handover_local=hl))
        assert plan["fwd_persistent"] and plan["bwd_persistent"], plan
    off = _lib.rollout_plan(0, shape, esz, dict(base, tile_persist=0))
    assert not off["fwd_persistent"] and not off["bwd_persistent"]

    tdt = torch.float32 if esz == 4 else torch.float64
    P = torch.tensor(random_block(0, 2, dtype, 21, scale=0.1), device=hip_device)
    h0 = torch.tensor(np.random.RandomState(4).uniform(0, 1, (2,) + shape).astype(dtype), device=hip_device)
    g = (torch.randn((T + 1, 2) + shape, dtype=tdt, device=hip_device,
                     generator=torch.Generator(device=hip_device).manual_seed(1)) / h0.numel())

    def run(options):
        traj = torch.empty((T + 1, 2) + shape, dtype=tdt, device=hip_device)
        traj[0] = h0
        pa.rollout_fwd_(traj, P, options=options)
        g0, pg = pa.rollout_bwd(traj, g, P, options=options)
        torch.cuda.synchronize()
        return traj, g0, pg

    n0 = _lib.persist_status()
    t1, a1, p1 = run(dict(base, handover_local=1))
    n1 = _lib.persist_status()
    t0, a0, p0 = run(dict(base, handover_local=0))
    n2 = _lib.persist_status()
    tr, ar, _ = run(dict(base, tile_persist=0))
    n3 = _lib.persist_status()
    # one resident forward and one resident sweep per run, none aborted: nothing below passed on the fallback path
    assert n1["launches"] == n0["launches"] + 2 and n2["launches"] == n1["launches"] + 2 and n3["launches"] == n2["launches"]
    assert n3["aborts"] == n0["aborts"] and not n3["disabled_on_current_device"]
    assert torch.isfinite(t1[-1]).all() and float(a1.abs().max()) > 0
    assert torch.equal(t1, t0) and torch.equal(a1, a0)
    assert torch.equal(t1, tr) and torch.equal(a1, ar)
    if esz == 8:                                           # (see the docstring: the sweep whose sums have a fixed order)
        d1, p1 = pa.rollout_bwd(t1, g, P, options=dict(base, handover_local=1, adj_persist_f64=0))
        d0, p0 = pa.rollout_bwd(t0, g, P, options=dict(base, handover_local=0, adj_persist_f64=0))
        torch.cuda.synchronize()
        assert torch.equal(d1, a1) and torch.equal(d0, a0)
        assert _lib.persist_status()["launches"] == n3["launches"]
    dp = float((p1 - p0).abs().max() / p0.abs().max())
    print(f"parameter-block gradient, handover_local 1 vs 0: {int((p1 != p0).sum())} of {p1.numel()} components differ, "
          f"max |difference| / max |gradient| = {dp:.3e}")
    assert torch.equal(p1, p0)
