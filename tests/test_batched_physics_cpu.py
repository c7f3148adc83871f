"""CPU: C-ABI surface and case list of the physics-residual loss per sample (percnn_pi_{batch,ensemble}_residual_sqloss_*,
physics.physics_loss_batched, RCNN.sample_physics_losses)."""
import ctypes
import os
import re

import torch

from batched_physics_util import BATCHES, FORMS, FRAMES, GRIDS, case_id, cases, family, make_cell, trajectory

SYMBOLS = ["percnn_pi_batch_residual_sqloss_workspace_bytes", "percnn_pi_debug_residual_sqloss_accepts"] + [
    f"percnn_pi_{kind}_residual_sqloss{bwd}_{suf}" for kind in ("batch", "ensemble") for bwd in ("", "_bwd") for suf in ("f32", "f64")]


def test_header_declares_and_lib_binds_every_symbol():
    import percnn_amd
    from percnn_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "percnn_pi.h")).read()
    L = percnn_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b(int|size_t) " + name + r"\(", header), name
        assert name in _lib.EXPORTS, name
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is not None, name
    for kind in ("batch", "ensemble"):
        for suf in ("f32", "f64"):
            # the unbatched signatures with `batch` after `shape`
            for bwd in ("", "_bwd"):
                one = list(getattr(L, f"percnn_pi_residual_sqloss{bwd}_{suf}").argtypes)
                many = list(getattr(L, f"percnn_pi_{kind}_residual_sqloss{bwd}_{suf}").argtypes)
                at = one.index(ctypes.POINTER(ctypes.c_int64)) + 1
                assert many[:at] == one[:at] and many[at] is ctypes.c_int and many[at + 1:] == one[at:], (kind, suf, bwd)
    assert percnn_amd.physics_loss_batched is percnn_amd.physics.physics_loss_batched
    assert callable(percnn_amd.RCNN.sample_physics_losses)


def test_argument_errors_do_not_need_a_gpu():
    """validation before any launch: bad batch / NULL / frame counts / ndim -> -1; workspace NULL, small or misaligned -> -2"""
    import percnn_amd
    L = percnn_amd.lib()
    shape = (ctypes.c_int64 * 2)(8, 8)
    big = 1 << 30
    for kind in ("batch", "ensemble"):
        for suf in ("f32", "f64"):
            fwd = getattr(L, f"percnn_pi_{kind}_residual_sqloss_{suf}")
            bwd = getattr(L, f"percnn_pi_{kind}_residual_sqloss_bwd_{suf}")
            for batch in (0, -3, 65536, 70000):
                assert fwd(16, 32, 2, shape, batch, 3, 1, 48, 64, big, None) == -1
                assert bwd(16, None, 32, 2, shape, batch, 3, 5, 1, 48, 64, None) == -1
            assert fwd(None, 32, 2, shape, 4, 3, 1, 48, 64, big, None) == -1          # traj
            assert fwd(16, None, 2, shape, 4, 3, 1, 48, 64, big, None) == -1          # params
            assert fwd(16, 32, 2, shape, 4, 3, 1, None, 64, big, None) == -1          # loss_out
            assert fwd(16, 32, 2, shape, 4, 0, 1, 48, 64, big, None) == -1            # nframes < 1
            assert fwd(16, 32, 4, shape, 4, 3, 1, 48, 64, big, None) == -1            # ndim
            assert fwd(16, 32, 2, None, 4, 3, 1, 48, 64, big, None) == -1             # shape
            rows = ctypes.c_int(0)
            assert L.percnn_pi_debug_residual_sqloss_accepts(2, shape, 4 if suf == "f32" else 8, 4, 3, 1, ctypes.byref(rows)) == 3
            assert 1 <= rows.value <= 16384 // 4
            assert fwd(16, 32, 2, shape, 4, 3, 1, 48, None, big, None) == -2          # no workspace
            assert fwd(16, 32, 2, shape, 4, 3, 1, 48, 64, 4 * rows.value * 8 - 8, None) == -2   # one row short
            assert fwd(16, 32, 2, shape, 4, 3, 1, 48, 64, 16, None) == -2
            assert fwd(16, 32, 2, shape, 4, 3, 1, 48, 68, big, None) == -2            # not 8-byte aligned
            assert bwd(None, None, 32, 2, shape, 4, 3, 5, 1, 48, 64, None) == -1      # traj
            assert bwd(16, None, None, 2, shape, 4, 3, 5, 1, 48, 64, None) == -1      # params
            assert bwd(16, None, 32, 2, shape, 4, 3, 5, 1, None, 64, None) == -1      # scratch
            assert bwd(16, None, 32, 2, shape, 4, 3, 5, 1, 48, None, None) == -1      # g_traj
            assert bwd(16, None, 32, 2, shape, 4, 0, 5, 1, 48, 64, None) == -1        # nframes < 1
            assert bwd(16, None, 32, 2, shape, 4, 3, 3, 1, 48, 64, None) == -1        # nout_frames < nframes + 1
            assert bwd(16, None, 32, 5, shape, 4, 3, 5, 1, 48, 64, None) == -1        # ndim


def test_workspace_query_suffices_for_every_grid_and_grows_with_the_batch():
    """the query is batch * 32768 rows, the most workgroups per frame and sample the entries take; a call needs only the rows it
    writes, max(workgroups per frame, 16384 / batch) at the most"""
    import percnn_amd
    L = percnn_amd.lib()
    prev = 0
    for b in (1, 2, 3, 64, 513, 65535):
        w = L.percnn_pi_batch_residual_sqloss_workspace_bytes(b)
        assert w > prev and w == b * 32768 * 8
        prev = w
    assert L.percnn_pi_batch_residual_sqloss_workspace_bytes(0) == 0 and L.percnn_pi_batch_residual_sqloss_workspace_bytes(-2) == 0
    rows = ctypes.c_int(0)
    for shape, esz, batch, frames in (((4, 6), 8, 513, 2), ((100, 100), 4, 64, 200), ((100, 100), 4, 1, 200), ((48, 48, 48), 4, 8, 300),
                                      ((300, 300, 128), 8, 2, 5), ((33, 37), 4, 3, 1)):
        for aligned in (1, 0):
            arr = (ctypes.c_int64 * len(shape))(*shape)
            got = L.percnn_pi_debug_residual_sqloss_accepts(len(shape), arr, esz, batch, frames, aligned, ctypes.byref(rows))
            if not got & 2:                                  # (300, 300, 128) without 16-byte lanes: declined for one sample too
                assert not aligned and got == 0 and rows.value == 0, (shape, got)
                continue
            points = 1
            for n in shape:
                points *= n
            assert 1 <= rows.value <= max((points + 255) // 256, 16384 // batch), (shape, batch, rows.value)
            assert rows.value * batch * 8 <= L.percnn_pi_batch_residual_sqloss_workspace_bytes(batch)


# grids on both sides of each bound: 16384 generic workgroups per frame (unbatched, 2D and 3D off the bricks), 16384 bricks of
# one or two planes (unbatched 3D), 32768 generic workgroups (batched); float32 chunks are 4 points, float64 chunks 2
BOUNDARY = [((300, 300, 128), 8), ((320, 320, 256), 4), ((256, 256, 256), 4), ((256, 256, 128), 8), ((512, 512, 64), 4),
            ((512, 512, 128), 4), ((384, 384, 128), 8), ((512, 512, 128), 8), ((400, 400, 256), 4), ((2048, 2048), 4),
            ((4096, 4096), 4), ((4100, 4100), 4), ((2048, 2048), 8), ((4097, 4097), 4), ((2049, 2049), 8), ((4096, 8192), 4),
            ((1023, 4099), 4), ((2047, 4099), 4), ((4099, 4099), 4), ((161, 161, 161), 4), ((203, 203, 203), 4),
            ((129, 129, 257), 8), ((255, 255, 130), 4), ((48, 48, 48), 4), ((100, 100), 4), ((3, 5), 8)]


def test_no_grid_the_unbatched_call_takes_is_declined_for_a_batch():
    """the issue's condition, from the library's own dispatch rules (host only, nothing is launched) and at the entry points: with
    a workspace of 8 bytes a grid that is taken answers -2, a grid that is declined -3 -- the decline comes first"""
    import percnn_amd
    L = percnn_amd.lib()
    seen = set()
    for shape, esz in BOUNDARY:
        arr = (ctypes.c_int64 * len(shape))(*shape)
        suf = "f32" if esz == 4 else "f64"
        for batch in (1, 3, 64):
            for aligned in (1, 0):
                got = L.percnn_pi_debug_residual_sqloss_accepts(len(shape), arr, esz, batch, 3, aligned, None)
                assert got >= 0, (shape, esz)
                assert not (got & 1) or (got & 2), ("declined for a batch, taken for one sample", shape, esz, batch, aligned)
                seen.add(got)
                for kind in ("batch", "ensemble"):
                    fwd = getattr(L, f"percnn_pi_{kind}_residual_sqloss_{suf}")
                    rc = fwd(16 if aligned else 16 + esz, 32, len(shape), arr, batch, 3, 1, 48, 64, 8, None)
                    assert rc == (-2 if got & 2 else -3), (shape, esz, batch, aligned, kind, rc)
    # the list has grids only the batched entries take, grids both take and grids both decline
    assert seen == {0, 2, 3}
    # the two grids of the bricks' band: 16384 < generic workgroups <= 32768, taken on bricks for one sample
    for shape, esz in (((300, 300, 128), 8), ((320, 320, 256), 4)):
        arr = (ctypes.c_int64 * 3)(*shape)
        rows = ctypes.c_int(0)
        assert L.percnn_pi_debug_residual_sqloss_accepts(3, arr, esz, 2, 3, 1, ctypes.byref(rows)) == 3
        assert 16384 < rows.value <= 32768


def test_case_list_covers_every_combination():
    """{generic 2D, tile, 3D} x {shared, per-sample} x {weighted, plain} x {float32, float64}, every B and F, every grid -- from
    the list alone"""
    cs = cases()
    assert len({case_id(c) for c in cs}) == len(cs)
    combos = {(c["path"], c["form"], c["weighted"], c["dtype"]) for c in cs}
    assert combos == {(p, f, w, d) for p in ("generic", "tile", "3d") for f in FORMS for w in (True, False)
                      for d in (torch.float32, torch.float64)}
    assert {(c["path"], c["shape"], c["dtype"]) for c in cs} == set(GRIDS)
    for path in ("generic", "tile", "3d"):
        mine = [c for c in cs if c["path"] == path]
        assert {c["B"] for c in mine} == set(BATCHES) and {c["F"] for c in mine} == set(FRAMES), path
    for form in FORMS:
        assert {c["B"] for c in cs if c["form"] == form} == set(BATCHES) and {c["F"] for c in cs if c["form"] == form} == set(FRAMES)
    for c in cs:
        # the path named is the path taken: the unbatched rule (both extents >= 34, 16-byte lanes) decides tile / generic
        lanes = 16 // (4 if c["dtype"] == torch.float32 else 8)
        if len(c["shape"]) == 2:
            tile = min(c["shape"]) >= 34 and c["shape"][1] % lanes == 0
            assert c["path"] == ("tile" if tile else "generic"), case_id(c)
        else:
            assert c["path"] == "3d"


def test_reference_loss_of_every_case_is_finite_and_positive():
    """the inputs are far from a solution: relative bounds on the loss mean something"""
    from oracle import restatement as R
    for c in cases():
        cell = make_cell(c)
        traj = trajectory(c).double()
        assert traj.shape == (c["F"] + 2, c["B"], 2) + c["shape"]
        for b in range(c["B"]):
            ref = R.physics_loss_reference(traj[:, b], family(c), cell.dx, cell.dt)
            assert torch.isfinite(ref) and float(ref) > 1e-6, (case_id(c), b, float(ref))
