"""GPU: the kernels against the plain-C oracle past 2^31 elements and 2^32 bytes, and at the documented length limits.

Every other test hands a kernel buffers inside the range where 32-bit index arithmetic is trivially right.  Here trajectories,
frames and chunk counts cross 2^31 / 2^32, on periodically tiled data (tiled_oracle.py): the oracle runs on a 40 x 48 tile in
milliseconds, the device result must be the tiling of it bit for bit, the parameter gradient (number of tiles) x the tile's
float64 row within util.GRAD_TOL.  `wraps_are_visible` is evaluated on the reference, on the CPU, before anything is launched:
a shift by 2^29 .. 2^32 elements must change at least 99 % of the values, so no power-of-two extents and no steady states.

Each test names the kernel family that ran (the plan, or the launch counter of the residency guard), holds at most 40 GiB of
device memory (asserted), and fails -- never skips -- where that memory is not available.

Not here: hash splits of the discovery rows (they hash the global row index and are not periodic), the zero-padded 3D IC
generator, multi-GPU slabs."""
import functools
import gc
import time

import numpy as np
import pytest
import torch

import tiled_oracle as TO
import util
from percnn_amd import _lib
from util import GRAD_TOL, grad_err, random_block

pytestmark = pytest.mark.gpu

GIB = 1 << 30
MEM_LIMIT = 40 * GIB
P2D, S2D = (40, 48), (480, 480)              # 480 = 32 * 15: 225 tiles of 32 x 32 (one resident workgroup each), 12 x 10 periods
P3D, S3D = (28, 16, 24), (112, 128, 96)      # 7 x 8 x 3 blocks of 16 x 16 x 32 for the resident 3D sweep, 4 x 8 x 4 periods


def frames_beyond(T, elems_per_frame, threshold):
    """whole frames of a [T + 1] trajectory that start at or beyond `threshold` elements"""
    return T + 1 - -(-threshold // elems_per_frame)


# horizons: multiples of four (whole tile groups) that put a few WHOLE frames beyond the threshold, so both species of a frame,
# and a whole group of four, are addressed past it -- not just the tail of the last frame
T_2D, T_2D_F64, T_3D = 4672, 1168, 784                     # 2.15e9 elements (8.6 GB); 4.3 GB of float64; 2.16e9 elements
T_BATCH = {2: 1556, 3: 264}                                # B = 3
assert 4 <= frames_beyond(T_2D, 2 * 480 * 480, 1 << 31) < 16 and 1 <= frames_beyond(T_2D_F64, 2 * 480 * 480 * 8, 1 << 32) < 8
assert 4 <= frames_beyond(T_3D, 2 * 112 * 128 * 96, 1 << 31) < 8
assert 1 <= frames_beyond(T_BATCH[2], 3 * 2 * 480 * 480, 1 << 31) < 8 and 4 <= frames_beyond(T_BATCH[3], 3 * 2 * 112 * 128 * 96, 1 << 31) < 8


# ---- bookkeeping every test shares ----
def begin(dev, need_gib):
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info(dev)
    if free < need_gib * GIB:
        pytest.fail(f"this test needs {need_gib} GiB of device memory, {free / GIB:.1f} GiB are free (it does not skip: "
                    f"a skip would hide what this file exists for)")
    torch.cuda.reset_peak_memory_stats(dev)
    return time.perf_counter()


def finish(dev, t0, what, family):
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    print(f"[large-extent] {what}: {time.perf_counter() - t0:.1f} s, peak {peak / GIB:.1f} GiB, ran on {family}")
    assert peak <= MEM_LIMIT, f"{what}: {peak / GIB:.1f} GiB of device memory at the peak"
    assert _lib.persist_status()["aborts"] == 0


def launches():
    return _lib.persist_status()["launches"]


def check_grad(got, tile_row, tiles, dtype, what):
    err = grad_err(got.cpu().numpy(), tiles * np.asarray(tile_row, dtype=np.float64))
    print(f"[large-extent] {what}: parameter gradient rel-L2 {err:.3g} against tiles x the tile's float64 row")
    assert err < GRAD_TOL[np.dtype(dtype)], f"{what}: parameter gradient {err:.3g}"


def visible(tile_buf, layout, elem_size, must_cross):
    """the precondition, on the CPU; must_cross: distances (elements) this buffer exists to cross"""
    seen = TO.wraps_are_visible(tile_buf, layout, elem_size)
    for D in must_cross:
        assert D in seen, f"the buffer {layout} does not reach {D} elements"
    return seen


def comparison_sees(dev_t, tile, ndim, index, beyond=1 << 31):
    """the comparison itself reaches past 2^31 elements: one unit in the last place at `index`, put there on purpose, is found and
    reported at that index; the value is restored"""
    flat = int(np.ravel_multi_index(index, tuple(dev_t.shape)))
    assert flat >= beyond, (index, flat)
    iv = dev_t.view(torch.int32 if dev_t.element_size() == 4 else torch.int64)
    iv[index] += 1
    k = dev_t.dim() - ndim
    where = f"{tuple(index[:k])} + {tuple(index[k:])}".replace("(", r"\(").replace(")", r"\)").replace("+", r"\+")
    with pytest.raises(AssertionError, match="first difference from the tiled oracle at " + where):
        TO.assert_is_tiling(dev_t, tile, ndim)
    iv[index] -= 1


# ---- the references: the oracle on the tile, computed once per session and never written to ----
def gs_block(ndim, hc, dtype):
    """the Gray-Scott checkpoint blocks of tests/golden: patterns that neither blow up nor settle over thousands of steps.
    2D hc = 2: the header (dt, coefficients, stencil) of the 2D checkpoint with the reaction branches of the 3D one (hc = 2)"""
    g2 = util.Golden(util.GOLDEN + "/gs2d_ckpt_64x64.npz")
    g3 = util.Golden(util.GOLDEN + "/gs3d_ckpt_16x16x16.npz")
    if hc == 0:
        P = (g2 if ndim == 2 else g3).packed("poly")
    elif ndim == 2:
        assert hc == 2 and g3.hc == 2
        P = np.concatenate([g2.packed("factored")[:16], g3.packed("factored")[16:]])
    else:
        assert hc == g3.hc
        P = g3.packed("factored")
    return np.ascontiguousarray(P.astype(dtype))


def sparse_mask(T, top):
    """every 7th frame below `top`, frame `top`, nothing above"""
    return [(t % 7 == 3 and t < top) or t == top for t in range(T + 1)]


@functools.lru_cache(maxsize=None)
def reference(ndim, hc, dtype, T, seed=3):
    """{P, h0, traj, g, cases: {name: (mask, dL/dh0, float64 row)}} on the tile; dL/dtraj is scaled as a mean over the GRID"""
    from percnn_amd import synthetic
    dtype = np.dtype(dtype)
    p, S = (P2D, S2D) if ndim == 2 else (P3D, S3D)
    P = gs_block(ndim, hc, dtype.type)
    h0 = synthetic.gs_initial_state(p, seed=seed)[0].numpy().astype(dtype)
    traj = TO.rollout_fwd(h0, P, T)
    assert np.isfinite(traj).all()
    g = (np.random.RandomState(7 + seed).standard_normal(traj.shape) / (2 * np.prod(S))).astype(dtype)
    ref = {"P": P, "h0": h0, "traj": traj, "g": g, "cases": {}}
    for a in (traj, g):
        a.setflags(write=False)
    return ref


def sweep_reference(ref, name, mask):
    if name not in ref["cases"]:
        g0, row = TO.rollout_bwd(ref["traj"], ref["g"], ref["P"], mask)
        assert np.isfinite(g0).all() and np.isfinite(row).all() and np.abs(g0).max() > 0 and np.abs(row).max() > 0
        ref["cases"][name] = (mask, g0, row)
    return ref["cases"][name]


def poisoned(g, mask):
    """frames a mask switches off must never be read"""
    off = torch.tensor([not m for m in mask], device=g.device)
    g[off] = float("nan")
    return g


def run_sweeps(dev, ref, shape, traj, cases, resident_opts, fallback_opts, what, tiles):
    """cases: [(name, mask, resident expected)] on one device trajectory; dL/dtraj is the tiling of the reference's, masked-out
    frames NaN.  Resident and launch-per-group / per-step results: dL/dh0 the tiling of the oracle's, both; gradients within
    GRAD_TOL, both."""
    import percnn_amd as pa
    nd = len(shape)
    P = torch.from_numpy(ref["P"]).to(dev)
    g = TO.tile_up(ref["g"], shape, dev)
    dirty = False
    for name, mask, resident in cases:
        _, g0_t, row_t = sweep_reference(ref, name, mask)
        if dirty:
            TO.tile_up(ref["g"], shape, dev, out=g)
        if mask is not None:
            poisoned(g, mask)
            dirty = True
        n0 = launches()
        a0, ag = pa.rollout_bwd(traj, g, P, frame_mask=mask, options=resident_opts)
        torch.cuda.synchronize()
        assert launches() - n0 == int(resident), f"{what} {name}: resident launches {launches() - n0}, expected {int(resident)}"
        TO.assert_is_tiling(a0, g0_t, nd, f"{what} {name}: dL/dh0")
        check_grad(ag, row_t, tiles, np.float32 if traj.element_size() == 4 else np.float64, f"{what} {name}")
        n1 = launches()
        b0, bg = pa.rollout_bwd(traj, g, P, frame_mask=mask, options=fallback_opts)
        torch.cuda.synchronize()
        assert launches() == n1, f"{what} {name}: {fallback_opts} ran a resident kernel"
        assert util.bits_equal(a0, b0), f"{what} {name}: resident dL/dh0 differs from {fallback_opts}"
        check_grad(bg, row_t, tiles, np.float32 if traj.element_size() == 4 else np.float64, f"{what} {name} {fallback_opts}")
        del a0, b0
    del g


# ---- 1. trajectory offsets, 2D float32 poly: resident forward + fused resident sweep ----
def test_trajectory_past_2_31_elements_2d_resident(hip_device):
    """(480, 480), T = 4672: 2.15e9 elements.  One resident forward launch, one resident sweep launch for dense dL/dtraj: these
    address past 2^31 elements.  A masked resident sweep cannot at this grid: its top frame stays below 4096, so the case
    "sparse, top 4092" (frames above it NaN) starts at 1.89e9 elements -- past 2^32 bytes (7.5 GB), not past 2^31 elements.  The
    sparse mask with top frame T falls back to one launch per group of four (t_top >= 4096), whose kernels index frames
    relative to the top frame themselves, past 2^31 elements."""
    import percnn_amd as pa
    dev, shape, T = hip_device, S2D, T_2D
    ref = reference(2, 0, "float32", T)
    visible(ref["traj"], (T + 1, 2) + shape, 4, [1 << 29, 1 << 30, 1 << 31])
    t0 = begin(dev, 30)
    plan = _lib.rollout_plan(0, shape, 4)
    assert plan["fwd_persistent"] and plan["bwd_persistent"] and plan["tile"] == (32, 32, 512), plan
    off = _lib.rollout_plan(0, shape, 4, {"tile_persist": 0})
    assert not off["fwd_persistent"] and not off["bwd_persistent"] and off["fwd"] == off["bwd"] == "tile2d", off
    P = torch.from_numpy(ref["P"]).to(dev)
    traj = torch.empty((T + 1, 2) + shape, dtype=torch.float32, device=dev)
    other = torch.full_like(traj, float("nan"))
    traj[0] = TO.tile_up(ref["h0"], shape, dev)
    other[0] = traj[0]
    n0 = launches()
    pa.rollout_fwd_(traj, P)
    torch.cuda.synchronize()
    assert launches() == n0 + 1
    TO.assert_is_tiling(traj, ref["traj"], 2, "resident forward")
    comparison_sees(traj, ref["traj"], 2, (T, 1, 479, 477))
    pa.rollout_fwd_(other, P, options={"tile_persist": 0})       # frame pointers formed on the host in size_t
    torch.cuda.synchronize()
    assert launches() == n0 + 1
    TO.assert_is_tiling(other, ref["traj"], 2, "forward, one launch per group")
    del other
    cases = [("dense", None, True), ("sparse, top 4092", tuple(sparse_mask(T, 4092)), True),
             ("sparse, top T", tuple(sparse_mask(T, T)), False)]
    run_sweeps(dev, ref, shape, traj, cases, None, {"tile_persist": 0}, "2D poly float32", TO.tiles_of(shape, P2D))
    finish(dev, t0, "1. 2D float32 poly, T = 4672", "pi_fwd2d_persist_kernel + pi_adj2d_persist_kernel (resident), tile2d groups")


# ---- 2. the same horizon on the factored blocks: tile kernels per group + pi_moments_kernel; float64 past 2^32 bytes ----
def test_trajectory_past_2_31_elements_2d_factored(hip_device):
    """hc = 2 float32, T = 4672: the adjoint tile kernels launched per group and the gradient pass (pi_moments_kernel indexes the
    frames itself), dense and masked."""
    import percnn_amd as pa
    dev, shape, T = hip_device, S2D, T_2D
    ref = reference(2, 2, "float32", T)
    visible(ref["traj"], (T + 1, 2) + shape, 4, [1 << 29, 1 << 30, 1 << 31])
    t0 = begin(dev, 30)
    plan = _lib.rollout_plan(2, shape, 4)
    assert plan["fwd"] == "tile2d" and plan["bwd"] == "tile2d" and not plan["fused_gradients"], plan
    P = torch.from_numpy(ref["P"]).to(dev)
    traj = torch.empty((T + 1, 2) + shape, dtype=torch.float32, device=dev)
    traj[0] = TO.tile_up(ref["h0"], shape, dev)
    n0 = launches()
    pa.rollout_fwd_(traj, P)
    torch.cuda.synchronize()
    TO.assert_is_tiling(traj, ref["traj"], 2, "forward hc = 2")
    fwd_resident = launches() - n0
    assert fwd_resident == int(plan["fwd_persistent"]), plan
    cases = [("dense", None, plan["bwd_persistent"]), ("sparse, top T", tuple(sparse_mask(T, T)), False)]
    run_sweeps(dev, ref, shape, traj, cases, None, {"tile_persist": 0}, "2D hc = 2 float32", TO.tiles_of(shape, P2D))
    finish(dev, t0, "2a. 2D float32 hc = 2, T = 4672",
           f"tile2d groups + pi_moments_kernel (resident fwd {bool(fwd_resident)}, bwd {plan['bwd_persistent']})")


def test_trajectory_past_2_32_bytes_2d_float64(hip_device):
    """float64 pre-contracted, T = 1168: a trajectory just over 4 GiB (5.4e8 elements), resident forward and sweep"""
    import percnn_amd as pa
    dev, shape, T = hip_device, S2D, T_2D_F64
    ref = reference(2, 0, "float64", T)
    visible(ref["traj"], (T + 1, 2) + shape, 8, [1 << 28, 1 << 29])
    t0 = begin(dev, 20)
    plan = _lib.rollout_plan(0, shape, 8)
    assert plan["fwd_persistent"] and plan["bwd_persistent"], plan
    P = torch.from_numpy(ref["P"]).to(dev)
    traj = torch.empty((T + 1, 2) + shape, dtype=torch.float64, device=dev)
    traj[0] = TO.tile_up(ref["h0"], shape, dev)
    n0 = launches()
    pa.rollout_fwd_(traj, P)
    torch.cuda.synchronize()
    assert launches() == n0 + 1
    TO.assert_is_tiling(traj, ref["traj"], 2, "resident forward float64")
    cases = [("dense", None, True), ("sparse, top T", tuple(sparse_mask(T, T)), True)]
    run_sweeps(dev, ref, shape, traj, cases, None, {"tile_persist": 0}, "2D poly float64", TO.tiles_of(shape, P2D))
    finish(dev, t0, "2b. 2D float64 poly, T = 1168", "pi_fwd2d_persist_kernel<double> + pi_adj2d_persist_split_kernel<double>")


# ---- 3. 3D float32 poly past 2^31 elements: brick forward, resident sweep against the brick sweep ----
def test_trajectory_past_2_31_elements_3d(hip_device):
    """(112, 128, 96), T = 784: brick forward; the resident 3D sweep (res3d = 2; 168 blocks) against res3d = 0 and the oracle"""
    import percnn_amd as pa
    dev, shape, T = hip_device, S3D, T_3D
    ref = reference(3, 0, "float32", T, seed=4)
    visible(ref["traj"], (T + 1, 2) + shape, 4, [1 << 29, 1 << 30, 1 << 31])
    t0 = begin(dev, 30)
    plan = _lib.rollout_plan(0, shape, 4, {"res3d": 2})
    assert plan["fwd"] == "brick3d" and plan["bwd_persistent"], plan
    off = _lib.rollout_plan(0, shape, 4, {"res3d": 0})
    assert off["bwd"] == "brick3d" and not off["bwd_persistent"], off
    P = torch.from_numpy(ref["P"]).to(dev)
    traj = torch.empty((T + 1, 2) + shape, dtype=torch.float32, device=dev)
    traj[0] = TO.tile_up(ref["h0"], shape, dev)
    pa.rollout_fwd_(traj, P)
    torch.cuda.synchronize()
    TO.assert_is_tiling(traj, ref["traj"], 3, "brick forward")
    cases = [("dense", None, True), ("sparse, top T", tuple(sparse_mask(T, T)), True)]
    run_sweeps(dev, ref, shape, traj, cases, {"res3d": 2}, {"res3d": 0}, "3D poly float32", TO.tiles_of(shape, P3D))
    finish(dev, t0, "3. 3D float32 poly, T = 784", "brick3d forward, pi_res3d resident sweep, brick3d sweep")


# ---- 4. batch and ensemble strides ----
@functools.lru_cache(maxsize=None)
def sample_reference(ndim, T, B=3):
    """per-sample tiles that differ (initial states of their own), one shared block and one block per sample (a dt of its own)"""
    from percnn_amd import synthetic
    p, S = (P2D, S2D) if ndim == 2 else (P3D, S3D)
    P = gs_block(ndim, 0, np.float32)
    Pe = np.stack([P.copy() for _ in range(B)])
    Pe[:, 0] *= np.array([1.0, 0.9375, 0.875], dtype=np.float32)[:B]
    h0 = np.stack([synthetic.gs_initial_state(p, seed=11 + b)[0].numpy() for b in range(B)])
    g = (np.random.RandomState(23).standard_normal((T + 1, B, 2) + p) / (2 * np.prod(S))).astype(np.float32)
    out = {"h0": h0, "g": g, "T": T}
    for kind, blk in (("batch", P), ("ensemble", Pe)):
        traj, g0, rows = util.o_batch_reference(h0, blk, T, g)
        assert np.isfinite(traj).all() and np.isfinite(g0).all() and np.isfinite(rows).all() and np.abs(rows).max() > 0
        out[kind] = (blk, traj, g0, rows)
    return out


@pytest.mark.parametrize("ndim", [2, 3], ids=["2D", "3D"])
def test_batch_and_ensemble_strides(ndim, hip_device):
    """B = 3, (T + 1) * B * 2 * n > 2^31: 2D on tile groups (T = 1556), 3D on the sample flavours of the brick kernels (T = 264);
    sample b of the result is the tiling of sample b's own tile"""
    import percnn_amd as pa
    dev, B = hip_device, 3
    p, shape = (P2D, S2D) if ndim == 2 else (P3D, S3D)
    n = int(np.prod(shape))
    T = T_BATCH[ndim]
    assert (T + 1) * B * 2 * n > (1 << 31)
    ref = sample_reference(ndim, T)
    for kind in ("batch", "ensemble"):
        visible(ref[kind][1], (T + 1, B, 2) + shape, 4, [1 << 29, 1 << 30, 1 << 31])
    t0 = begin(dev, 38)
    if ndim == 3:
        from test_batch_brick_gpu import assert_on_bricks
        assert_on_bricks(util.make_case(4, shape, 0, np.float32, B, T), options={})
    else:
        # percnn_pi_debug_batch_plan answers for the launch-per-step part of a sample call alone (it says "direct" here); T is
        # a multiple of four, so every step runs in a tile group, and whether tiles apply is the unbatched plan's `tile`
        assert T % 4 == 0 and _lib.rollout_plan(0, shape, 4)["tile"] == (32, 32, 512)
    tiles = TO.tiles_of(shape, p)
    h0 = TO.tile_up(ref["h0"], shape, dev)
    g = TO.tile_up(ref["g"], shape, dev)
    n0 = launches()
    for kind in ("batch", "ensemble"):
        blk, traj_t, g0_t, rows = ref[kind]
        Pd = torch.from_numpy(blk).to(dev)
        fwd = pa.pi_rollout_batched if kind == "batch" else pa.pi_rollout_ensemble
        bwd = util.batch_rollout_bwd if kind == "batch" else util.ensemble_rollout_bwd
        traj = fwd(h0, Pd, T).contiguous()
        torch.cuda.synchronize()
        TO.assert_is_tiling(traj, traj_t, ndim, f"{kind} forward")
        g0, pg = bwd(traj, g, Pd, 0, shape, B, T)
        TO.assert_is_tiling(g0, g0_t, ndim, f"{kind} dL/dh0")
        if kind == "batch":
            check_grad(pg, rows.sum(0), tiles, np.float32, f"{ndim}D batch")
        else:
            for b in range(B):
                check_grad(pg[b], rows[b], tiles, np.float32, f"{ndim}D ensemble row {b}")
        del traj, g0, pg
    assert launches() == n0                                 # the resident kernels have no sample flavour
    finish(dev, t0, f"4. {ndim}D batch + ensemble, B = 3, T = {T}",
           "tile2d groups, sample flavour" if ndim == 2 else "brick3d, sample flavour")


# ---- 5. losses that index frames in-kernel ----
def residual_sums(traj, Q):
    """float64: sum over frames 0 .. F-3 and the tile of R_s^2, R_s = D_s Lap(h_f)_s + r_s(h_f) - (h_{f+1} - h_f) / dt, per species"""
    h = np.asarray(traj, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    cur, nxt = h[:-2], h[1:-1]
    u, v = cur[:, 0], cur[:, 1]
    mono = [np.ones_like(u), u, v, u * u, u * v, v * v, u ** 3, u * u * v, u * v * v, v ** 3]
    out = []
    for s in (0, 1):
        f = cur[:, s]
        lap = Q[3] * f
        for a in range(f.ndim - 1):
            for i, o in enumerate((-2, -1, 1, 2)):
                lap = lap + Q[4 + 4 * a + i] * np.roll(f, -o, axis=1 + a)
        r = sum(Q[16 + 10 * s + m] * mono[m] for m in range(10))
        R = Q[1 + s] * lap + r - (nxt[:, s] - f) / Q[0]
        out.append(float((R * R).sum()))
    return out


def test_losses_over_a_trajectory_past_2_31_elements(hip_device, monkeypatch):
    """physics.physics_loss (fused: one reducing pass that walks the frames itself) over the whole T = 4672 trajectory against
    tiles x the tile's float64 residual sums, and the squared-error-in-sweep flavour (rollout_bwd_sqerr: the loss gradient formed
    from the state the sweep reads) against the oracle with the materialised gradient.
    Bar of the loss value: float32 data, partial sums in float64 -- 1e-5 relative (util.TOL_TRAJ)."""
    from percnn_amd import functional as F_pi, physics
    dev, shape, T = hip_device, S2D, T_2D
    ref = reference(2, 0, "float32", T)
    visible(ref["traj"], (T + 1, 2) + shape, 4, [1 << 29, 1 << 30, 1 << 31])
    # the "true equation" of the residual: the block itself with other reaction coefficients, so the residual is not round-off
    Q = ref["P"].copy()
    Q[16:] *= np.float32(0.75)
    su, sv = residual_sums(ref["traj"], Q)
    want = (su + sv) / ((T - 1) * float(np.prod(P2D)))      # plain mean over the periodic grid: tiles cancel
    t0 = begin(dev, 30)
    tiles = TO.tiles_of(shape, P2D)
    traj = TO.tile_up(ref["traj"], shape, dev)

    def declined(*a, **k):
        raise AssertionError("the fused residual pass declined the trajectory: the residual-tensor expression would have run")

    monkeypatch.setattr(physics, "physics_residual", declined)
    got = float(physics.physics_loss(traj, torch.from_numpy(Q).to(dev), reference_weighting=False, fused=True))
    monkeypatch.undo()
    slow = float(physics.physics_loss(traj[:42], torch.from_numpy(Q).to(dev), reference_weighting=False, fused=False))
    fast = float(physics.physics_loss(traj[:42], torch.from_numpy(Q).to(dev), reference_weighting=False, fused=True))
    print(f"[large-extent] physics loss {got!r} against {want!r}: rel {abs(got - want) / want:.3g}")
    assert abs(got - want) <= 1e-5 * want, (got, want)
    assert abs(fast - slow) <= 1e-5 * slow, (fast, slow)
    # squared error inside the sweep, resident (dense) and one launch per group
    P = torch.from_numpy(ref["P"]).to(dev)
    scale = 2.0 / ((T + 1) * 2 * float(np.prod(shape)))
    g_t = (np.float32(scale) * ref["traj"]).astype(np.float32)
    g0_t, row_t = TO.rollout_bwd(ref["traj"], g_t, ref["P"])
    assert np.abs(g0_t).max() > 0 and np.isfinite(row_t).all()
    n0 = launches()
    for opts, resident in ((None, True), ({"tile_persist": 0}, False)):
        n1 = launches()
        g0, pg = F_pi.rollout_bwd_sqerr(traj, P, None, None, scale, options=opts)
        torch.cuda.synchronize()
        assert launches() - n1 == int(resident), (opts, launches() - n1)
        TO.assert_is_tiling(g0, g0_t, 2, f"sqerr sweep {opts}: dL/dh0")
        check_grad(pg, row_t, tiles, np.float32, f"sqerr sweep {opts}")
    assert launches() == n0 + 1
    finish(dev, t0, "5. losses over T = 4672", "residual_sqloss (fused), pi_adj2d_persist_kernel with the in-kernel loss gradient")


# ---- 6. in-frame offsets: one step forward + backward with the second species past 2^31 / 2^32 bytes ----
@pytest.mark.parametrize("shape,period,dtype,hc", [((24576, 24624), (48, 48), np.float32, 0), ((16384, 16416), (32, 48), np.float64, 4)],
                         ids=["float32-hc0-24576x24624", "float64-hc4-16384x16416"])
def test_one_step_with_a_plane_between_2_and_4_gib(shape, period, dtype, hc, hip_device):
    """the step kernels address a frame with 32-bit offsets and take a 2D field below 4 GiB per species: here the plane has 2.25
    (2.0) GiB, so species 1 lies at byte offsets in [2^31, 2^33); and the refusal one step beyond the limit still holds"""
    from percnn_amd import functional as F_pi
    dev = hip_device
    es = np.dtype(dtype).itemsize
    assert (1 << 31) < shape[0] * shape[1] * es < (1 << 32)
    rs = np.random.RandomState(61)
    P = random_block(hc, 2, dtype, 62, scale=0.3)
    h_t = rs.uniform(0.1, 0.9, (2,) + period).astype(dtype)
    G_t = rs.standard_normal((2,) + period).astype(dtype)
    inj_t = rs.standard_normal((2,) + period).astype(dtype)
    for buf in (h_t, G_t, inj_t):
        visible(buf, (2,) + shape, es, [(1 << 31) // es, (1 << 32) // es])
    out_t = TO.step_fwd(h_t, P)
    gin_t, row_t = TO.step_bwd(h_t, G_t, inj_t, P)
    t0 = begin(dev, 32)
    plan = _lib.rollout_plan(hc, shape, es)
    assert plan["fwd"] == "direct" and plan["bwd"] == "direct", plan
    Pd = torch.from_numpy(P).to(dev)
    h = TO.tile_up(h_t, shape, dev)
    out = F_pi.step_fwd(h, Pd)
    torch.cuda.synchronize()
    TO.assert_is_tiling(out, out_t, 2, "step forward")
    del out
    G = TO.tile_up(G_t, shape, dev)
    inj = TO.tile_up(inj_t, shape, dev)
    gin, pg = F_pi.step_bwd(h, G, Pd, g_inject=inj)
    torch.cuda.synchronize()
    TO.assert_is_tiling(gin, gin_t, 2, "step backward")
    check_grad(pg, row_t, TO.tiles_of(shape, period), dtype, f"one step {shape}")
    # one step beyond: a plane of exactly 4 GiB is refused before any launch (the pointers are never dereferenced)
    import ctypes
    side = 32768 if es == 4 else 16384
    beyond = (ctypes.c_int64 * 2)(side, (1 << 32) // es // side)
    f = getattr(_lib.lib(), "percnn_pi_step_fwd_f32" if es == 4 else "percnn_pi_step_fwd_f64")
    assert f(h.data_ptr(), G.data_ptr(), Pd.data_ptr(), hc, 2, beyond, None) == -3
    finish(dev, t0, f"6. one step {shape} {np.dtype(dtype).name} hc = {hc}", "direct step kernels")


# ---- 7. the 64-bit chunk path ----
def test_one_forward_step_with_2_31_chunks(hip_device):
    """(2048, 1026, 1023) float32: odd W, so a chunk is one point and the grid has 2.15e9 of them -- the geometry's division by the
    chunks per plane takes its 64-bit path -- while a plane (4 MiB) stays small.  Forward only: state and result take 34.4 GB."""
    from percnn_amd import functional as F_pi
    dev, shape, period = hip_device, (2048, 1026, 1023), (16, 18, 33)
    assert int(np.prod(shape)) >= (1 << 31)
    rs = np.random.RandomState(71)
    P = random_block(0, 3, np.float32, 72, scale=0.3)
    h_t = rs.uniform(0.1, 0.9, (2,) + period).astype(np.float32)
    visible(h_t, (2,) + shape, 4, [1 << 29, 1 << 30, 1 << 31, 1 << 32])
    out_t = TO.step_fwd(h_t, P)
    t0 = begin(dev, 36)
    plan = _lib.rollout_plan(0, shape, 4)
    assert plan["fwd"] == "direct", plan
    h = TO.tile_up(h_t, shape, dev)
    out = F_pi.step_fwd(h, torch.from_numpy(P).to(dev))
    torch.cuda.synchronize()
    TO.assert_is_tiling(out, out_t, 3, "step forward, 2^31 chunks")
    comparison_sees(out, out_t, 3, (1, 2047, 1025, 1022))       # (here one species is compared in slabs of periods)
    del h, out
    finish(dev, t0, "7. one forward step (2048, 1026, 1023)", "direct 3D step kernel, one point per chunk")


# ---- 8. length limits on small grids (the plain oracle, no tiling) ----
@functools.lru_cache(maxsize=None)
def limit_reference(shape):
    from percnn_amd import synthetic
    rs = np.random.RandomState(81)
    P = gs_block(2, 0, np.float32)
    h0 = synthetic.gs_initial_state(shape, seed=8)[0].numpy()
    traj = util.o_rollout_fwd(h0, P, 4096)
    assert np.isfinite(traj).all()
    g = (rs.standard_normal(traj.shape) / traj[0].size).astype(np.float32)
    out = {"P": P, "traj": traj, "g": g}
    for T in (4095, 4096):
        mask = sparse_mask(T, T)
        gm = g[:T + 1].copy()
        gm[[not m for m in mask]] = 0
        out[T] = (mask,) + tuple(util.o_rollout_bwd(np.ascontiguousarray(traj[:T + 1]), gm, P))
        assert np.isfinite(out[T][1]).all() and np.isfinite(out[T][2]).all() and np.abs(out[T][1]).max() > 0
    return out


@pytest.mark.parametrize("shape", [(64, 64), (100, 100)], ids=["64x64", "100x100"])
def test_masked_sweep_at_the_4096_frame_limit(shape, hip_device):
    """a frame mask travels to the resident sweeps as 4096 bits of kernel argument: top frame 4095 runs resident (counter + 1),
    4096 falls back to one launch per group (+ 0); each is the oracle's dL/dh0 bit for bit, the two trajectories agree on the
    frames they share"""
    import percnn_amd as pa
    dev = hip_device
    ref = limit_reference(shape)
    t0 = begin(dev, 4)
    assert _lib.rollout_plan(0, shape, 4)["bwd_persistent"]
    P = torch.from_numpy(ref["P"]).to(dev)
    trajs = {}
    for T, resident in ((4095, True), (4096, False)):
        mask, g0_o, row_o = ref[T]
        traj = torch.empty((T + 1, 2) + shape, dtype=torch.float32, device=dev)
        traj[0] = torch.from_numpy(ref["traj"][0]).to(dev)
        pa.rollout_fwd_(traj, P)
        assert np.array_equal(traj.cpu().numpy(), ref["traj"][:T + 1]), f"forward T = {T}"
        trajs[T] = traj
        g = poisoned(torch.from_numpy(ref["g"][:T + 1]).to(dev), mask)
        n0 = launches()
        g0, pg = pa.rollout_bwd(traj, g, P, frame_mask=mask)
        torch.cuda.synchronize()
        assert launches() - n0 == int(resident), f"T = {T}: {launches() - n0} resident launches"
        assert np.array_equal(g0.cpu().numpy(), g0_o), f"dL/dh0, T = {T}"
        check_grad(pg, row_o, 1, np.float32, f"{shape} masked, T = {T}")
    assert util.bits_equal(trajs[4095], trajs[4096][:4096])
    finish(dev, t0, f"8a. masked sweeps at t_top = 4095 / 4096, {shape}", "resident small-tile sweep / tile2d groups")


def test_resident_3d_sweep_at_the_4096_step_limit(hip_device):
    """(32, 32, 64): the resident 3D sweep takes nsteps < 4096 -- T = 4095 resident (+ 1), T = 4096 on the bricks (+ 0); both bit
    for bit the res3d = 0 sweep"""
    import percnn_amd as pa
    dev, shape = hip_device, (32, 32, 64)
    t0 = begin(dev, 12)
    from percnn_amd import synthetic
    P = torch.from_numpy(gs_block(3, 0, np.float32)).to(dev)
    traj = torch.empty((4096 + 1, 2) + shape, dtype=torch.float32, device=dev)
    traj[0] = synthetic.gs_initial_state(shape, seed=9)[0].to(dev)
    pa.rollout_fwd_(traj, P)
    assert torch.isfinite(traj[-1]).all()
    g = torch.randn(traj.shape, dtype=traj.dtype, device=dev, generator=torch.Generator(device=dev).manual_seed(93)) / traj[0].numel()
    assert _lib.rollout_plan(0, shape, 4, {"res3d": 2})["bwd_persistent"]
    for T, resident in ((4095, True), (4096, False)):
        n0 = launches()
        a0, ag = pa.rollout_bwd(traj[:T + 1], g[:T + 1], P, options={"res3d": 2})
        torch.cuda.synchronize()
        assert launches() - n0 == int(resident), f"T = {T}: {launches() - n0} resident launches"
        n1 = launches()
        b0, bg = pa.rollout_bwd(traj[:T + 1], g[:T + 1], P, options={"res3d": 0})
        torch.cuda.synchronize()
        assert launches() == n1
        assert util.bits_equal(a0, b0) and torch.isfinite(a0).all() and float(a0.abs().max()) > 0, f"T = {T}"
        err = grad_err(ag.cpu().numpy(), bg.cpu().numpy())
        print(f"[large-extent] (32, 32, 64) T = {T}: gradient res3d = 2 against res3d = 0 rel-L2 {err:.3g}")
        assert err < GRAD_TOL[np.dtype(np.float32)]
    finish(dev, t0, "8b. resident 3D sweep at nsteps = 4095 / 4096", "pi_res3d resident sweep / brick3d sweep")


# ---- 10. discovery: the Stage-2 library over more than 2^31 rows ----
def test_library_moments_past_2_31_rows(hip_device):
    """pa.library_moments, float32, region "periodic", every row trains: (2400, 2400) x 375 frames = 2.148e9 rows on a 32-bit row
    index, 17.3 GB.  Against tiles x stage2_util.explicit_moments on the 20 x 24 tile (float64), the bar of test_discovery_gpu.
    The hash splits are left out: they hash the global row index, which is not periodic."""
    import percnn_amd as pa
    from stage2_util import explicit_moments
    from test_discovery_gpu import DT, DX, _check
    dev, shape, period, N = hip_device, (2400, 2400), (20, 24), 375
    assert (1 << 31) < (N - 2) * shape[0] * shape[1] <= (1 << 32)
    tile = (0.5 * np.random.default_rng(101).standard_normal((N, 2) + period)).astype(np.float32)
    visible(tile, (N, 2) + shape, 4, [1 << 29, 1 << 30, 1 << 31, 1 << 32])
    tiles = TO.tiles_of(shape, period)
    G, b, yy, n = explicit_moments(tile, DX, DT, "periodic", 0, 1 << 32, 1 << 32)
    assert n[0] == (N - 2) * period[0] * period[1] and n[1] == 0
    t0 = begin(dev, 20)
    traj = TO.tile_up(tile, shape, dev)
    got = pa.library_moments(traj, DX, DT, region="periodic", split=None)
    torch.cuda.synchronize()
    assert float(got.n[0]) == float(tiles) * n[0] > (1 << 31)
    _check(list(got), (tiles * G, tiles * b, tiles * yy, tiles * n), "2.148e9 rows")
    finish(dev, t0, "10. library moments, 2.148e9 rows", "pi_disc moments kernel")


# ---- 9. Stage-1 Pi-block rollouts ----
# The resident Stage-1 kernels take T < 4096 and at most 2048 patches of 4 x 4 points (four workgroups per CU): 4096 frames of
# 2 x 32768 floats are 2^30 bytes, so no call can send them past 2^31 bytes, let alone 2^32 -- a rollout of (100, 100) past
# 2^32 bytes (T = 53 700) runs one launch per step, with frame pointers formed on the host, and the gradient kernel
# (s1_wgrad_kernel), which walks the frames itself.  9a holds the resident kernels to launch-per-step at their own limit, 9b the
# long rollout to the oracle and to the tile.  2^31 ELEMENTS (T = 107 400) is left out: it would double a test that is already
# this file's slowest, and crosses no other threshold of this path (offsets are in elements, 64-bit on the host).
S1_SHAPE, S1_PERIOD, S1_PREFIX = (100, 100), (20, 25), 300


@functools.lru_cache(maxsize=None)
def stage1_reference():
    """the lambda-omega Stage-1 checkpoint of tests/golden: over the long horizon it neither blows up (the Burgers one does) nor
    comes to rest (it ends in an oscillation, so frames a wrap apart differ); the oracle on the tile for the first 300 steps only
    -- it needs 300 s for 53 700"""
    from oracle import pi_oracle as O
    z = np.load(util.GOLDEN + "/lo1_stage1_24x40.npz")
    sd = {k[6:]: z[k] for k in z.files if k.startswith("param/")}
    nu = float(z["nu_up"])
    cu, cv = (nu / (1.0 + np.exp(-float(sd[k]))) for k in ("CA", "CB"))
    P = O.s1_pack(sd, float(z["dt"]), cu, cv)
    h0 = np.ascontiguousarray(z["h0"][0][:, :S1_PERIOD[0], :S1_PERIOD[1]])
    return {"P": P, "h0": h0, "prefix": O.s1_rollout_fwd(h0, P, S1_PREFIX)}


def s1_forward(dev, P, h0, T, persist):
    import percnn_amd as pa
    traj = torch.full((T + 1,) + tuple(h0.shape), float("nan"), dtype=torch.float32, device=dev)
    traj[0] = h0
    pa.stage1.set_option("persist", persist)
    try:
        pa.stage1.rollout_fwd_(traj, P)
        torch.cuda.synchronize()
    finally:
        pa.stage1.set_option("persist", 1)
    return traj


def s1_backward(traj, g, P, mask, persist, etile=1):
    import percnn_amd as pa
    pa.stage1.set_option("persist", persist)
    pa.stage1.set_option("etile", etile)
    try:
        out = pa.stage1.rollout_bwd(traj, g, P, frame_mask=mask)
        torch.cuda.synchronize()
    finally:
        pa.stage1.set_option("persist", 1)
        pa.stage1.set_option("etile", 1)
    return out


def test_stage1_resident_rollouts_at_the_4096_step_limit(hip_device):
    """(100, 100): T = 4095 runs resident (forward + 1, sweep + 1), T = 4096 one launch per step (+ 0); trajectory, dL/dh0 and the
    parameter gradient bit for bit those of persist = 0, dense and masked; the first 300 frames the tiling of the oracle's"""
    dev, shape = hip_device, S1_SHAPE
    ref = stage1_reference()
    t0 = begin(dev, 4)
    P = torch.from_numpy(ref["P"]).to(dev)
    h0 = TO.tile_up(ref["h0"], shape, dev)
    for T, resident in ((4095, True), (4096, False)):
        n0 = launches()
        a = s1_forward(dev, P, h0, T, 1)
        assert launches() - n0 == int(resident), f"forward T = {T}: {launches() - n0} resident launches"
        n1 = launches()
        b = s1_forward(dev, P, h0, T, 0)
        assert launches() == n1 and torch.isfinite(b).all() and util.bits_equal(a, b), f"forward T = {T}"
        TO.assert_is_tiling(a[:S1_PREFIX + 1].contiguous(), ref["prefix"], 2, f"Stage-1 forward T = {T}")
        del b
        g = torch.randn(a.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(95)) / a[0].numel()
        for mask in (None, sparse_mask(T, T)):
            r0, rg = s1_backward(a, poisoned(g.clone(), mask) if mask else g, P, mask, 0)
            n2 = launches()
            a0, ag = s1_backward(a, poisoned(g.clone(), mask) if mask else g, P, mask, 1)
            assert launches() - n2 == int(resident), f"sweep T = {T}: {launches() - n2} resident launches"
            assert torch.isfinite(a0).all() and float(a0.abs().max()) > 0 and torch.isfinite(ag).all()
            assert util.bits_equal(a0, r0) and torch.equal(ag, rg), f"sweep T = {T}, mask {mask is not None}"
        del a, g
    finish(dev, t0, "9a. Stage-1 rollouts at T = 4095 / 4096, (100, 100)", "s1_fwd_persist_kernel + s1_adj_persist_kernel / one launch per step")


def test_stage1_rollout_past_2_32_bytes(hip_device):
    """(100, 100) over periods (20, 25), T = 53 700: 4.3 GB.  One launch per step (the resident kernels stop at 4096 steps:
    counter + 0), and s1_wgrad_kernel walking the frames of the trajectory and of the adjoint itself.  Forward: the tiling of the
    same rollout of the (20, 25) grid bit for bit, whose first 300 frames are the oracle's.  Backward (the oracle has none; both
    runs on the per-tap hand-over, which takes any shape): dL/dh0 within 1e-5 relative L2 of the tiling of the tile grid's --
    the bar test_stage1.py holds dL/dh0 to -- and the gradient within util.GRAD_TOL of 20 x the tile grid's."""
    dev, shape, p, T = hip_device, S1_SHAPE, S1_PERIOD, 53700
    assert (T + 1) * 2 * shape[0] * shape[1] * 4 > (1 << 32)
    ref = stage1_reference()
    t0 = begin(dev, 20)
    P = torch.from_numpy(ref["P"]).to(dev)
    small = s1_forward(dev, P, torch.from_numpy(ref["h0"]).to(dev), T, 0)        # the reference of this test: the tile grid
    assert torch.isfinite(small).all()
    TO.assert_is_tiling(small[:S1_PREFIX + 1].contiguous(), ref["prefix"], 2, "Stage-1 forward on the tile grid")
    small_host = small.cpu().numpy()
    visible(small_host, (T + 1, 2) + shape, 4, [1 << 29, 1 << 30])               # on the CPU, before the grid's launches
    n0 = launches()
    traj = s1_forward(dev, P, TO.tile_up(ref["h0"], shape, dev), T, 1)
    assert launches() == n0, "a resident Stage-1 launch at T >= 4096"
    TO.assert_is_tiling(traj, small, 2, "Stage-1 forward, T = 53 700")
    g_t = torch.randn(small.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(96)) / (2 * shape[0] * shape[1])
    g0_t, pg_t = s1_backward(small, g_t, P, None, 0, etile=0)
    g = TO.tile_up(g_t, shape)
    del g_t, small
    g0, pg = s1_backward(traj, g, P, None, 1, etile=0)
    assert launches() == n0
    assert torch.isfinite(g0).all() and float(g0.abs().max()) > 0 and torch.isfinite(pg).all() and float(pg.abs().max()) > 0
    want = TO.tile_up(g0_t, shape)
    e0 = util.rel_l2(g0.cpu().numpy(), want.cpu().numpy())
    print(f"[large-extent] Stage-1 dL/dh0 against the tiling of the tile grid's: rel-L2 {e0:.3g}, bit-identical {util.bits_equal(g0, want)}")
    assert e0 < 1e-5
    check_grad(pg, pg_t.cpu().numpy(), TO.tiles_of(shape, p), np.float32, "Stage-1 T = 53 700")
    finish(dev, t0, "9b. Stage-1 rollout (100, 100), T = 53 700", "s1_fwd_kernel / s1_adj_kernel per step, s1_wgrad_kernel")
