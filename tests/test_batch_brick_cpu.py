"""Host side of the batched / ensemble brick launches (csrc/pi_abi.hip "batch on bricks"), no device involved: which kernel family
the launch-per-step part of a batched call takes (percnn_pi_debug_batch_plan evaluates the launchers' own rule, batch_brick_rz),
and the workspace sizes, which the brick launches must not change."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT, BRICK = 0, 3


def plan(hc, shape, esz, batch, options=None):
    import percnn_amd
    from percnn_amd import _lib
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    rc = percnn_amd.lib().percnn_pi_debug_batch_plan(hc, len(shape), _lib.shape_arg(tuple(shape)), esz, batch, _lib.options_arg(options),
                                                     out)
    return rc, list(out)


def test_symbol_is_declared_bound_and_wrapped():
    import percnn_amd
    from percnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "percnn_pi.h")).read()
    assert re.search(r"\bint percnn_pi_debug_batch_plan\(int hc, int ndim, const int64_t\* shape, int elem_size, int batch, "
                     r"const char\* options, int\* out\);", header)
    assert "percnn_pi_debug_batch_plan" in _lib.EXPORTS
    assert percnn_amd.lib().percnn_pi_debug_batch_plan.argtypes is not None
    assert _lib.batch_plan(0, (9, 12, 64), 4, 3, {"brick3d": 2}) == {"fwd": "brick3d", "bwd": "brick3d", "fwd_planes_per_pass": 1,
                                                                       "bwd_planes_per_pass": 1}


@pytest.mark.parametrize("rz", [1, 2])
def test_eligible_batch_takes_the_bricks_with_the_planes_asked_for(rz):
    assert plan(0, (9, 12, 64), 4, 3, {"brick3d": 2, "brick_rz": rz}) == (0, [BRICK, BRICK, rz, rz])


def test_planes_per_brick_by_size_are_the_unbatched_rule():
    # brick_rz_for: one plane below 2 M points (forward) / 12 M (adjoint); factored blocks always one
    assert plan(0, (9, 12, 64), 4, 3, {"brick3d": 2}) == (0, [BRICK, BRICK, 1, 1])
    assert plan(0, (128, 128, 128), 4, 2, {"brick3d": 2}) == (0, [BRICK, BRICK, 2, 1])
    assert plan(8, (9, 12, 64), 4, 3, {"brick3d": 2, "brick_rz": 2}) == (0, [BRICK, BRICK, 1, 1])


def test_declined_batches_stay_on_the_direct_kernels():
    for esz in (4, 8):
        assert plan(0, (9, 12, 64), esz, 3, {"brick3d": 0}) == (0, [DIRECT, DIRECT, 1, 1])
    assert plan(0, (5, 6, 384), 4, 3, {"brick3d": 2}) == (0, [DIRECT, DIRECT, 1, 1])           # rows of 96 chunks: no 512-lane flavour
    assert plan(0, (5, 6, 260), 4, 3, {"brick3d": 2, "brick_wide": 1, "brick_nt": 512})[1][:2] == [DIRECT, DIRECT]
    assert plan(0, (5, 2, 256), 4, 3, {"brick3d": 2})[1][:2] == [BRICK, BRICK]                 # 64 chunks: the widest that fits
    assert plan(0, (5, 2, 128), 8, 3, {"brick3d": 2})[1][:2] == [BRICK, BRICK]
    assert plan(0, (64, 96), 4, 3, {"brick3d": 2}) == (0, [DIRECT, DIRECT, 1, 1])              # 2D
    assert plan(0, (9, 12, 64), 4, 3, {"brick3d": 2, "brick_rz": 4})[1][:2] == [DIRECT, DIRECT]   # no four-plane sample flavour
    assert plan(0, (9, 12, 64), 4, 3, {"brick3d": 2, "vec": 1})[1][:2] == [DIRECT, DIRECT]      # scalar lanes
    assert plan(0, (9, 12, 66), 4, 3, {"brick3d": 2})[1][:2] == [DIRECT, DIRECT]                # rows that are no whole chunks
    rc, out = plan(-1, (9, 12, 64), 4, 3, {"brick3d": 2})                                        # no batched advective block
    assert rc == -1 and out == [-7] * 4
    assert plan(0, (9, 12, 64), 2, 3, None)[0] == -1 and plan(0, (9, 12, 64), 4, 0, None)[0] == -1


def test_factored_blocks_with_all_gradients_in_the_launch_keep_the_direct_adjoint():
    # the WGRAD rule of step_bwd: fuse_wgrad = 1 reduces every gradient inside the sweep launches, which the brick kernel does for
    # pre-contracted blocks only
    assert plan(8, (9, 12, 64), 4, 3, {"brick3d": 2, "fuse_wgrad": 1}) == (0, [BRICK, DIRECT, 1, 1])
    assert plan(0, (9, 12, 64), 4, 3, {"brick3d": 2, "fuse_wgrad": 1}) == (0, [BRICK, BRICK, 1, 1])
    for fw in (0, 2):
        assert plan(8, (9, 12, 64), 4, 3, {"brick3d": 2, "fuse_wgrad": fw}) == (0, [BRICK, BRICK, 1, 1])


@pytest.mark.parametrize("hc,shape,esz,options", [(0, (9, 12, 64), 4, {"brick3d": 2}), (0, (9, 12, 64), 4, {"brick3d": 0}),
                                                  (0, (128, 128, 128), 4, None), (8, (48, 48, 48), 8, None), (0, (64, 96), 4, None),
                                                  (-1, (33, 37), 4, None), (0, (5, 6, 384), 4, None)])
def test_batch_of_one_is_the_unbatched_plan(hc, shape, esz, options):
    import percnn_amd
    from percnn_amd import _lib
    ref = (ctypes.c_int * 15)()
    assert percnn_amd.lib().percnn_pi_debug_plan(hc, len(shape), _lib.shape_arg(tuple(shape)), esz, _lib.options_arg(options), ref) == 0
    assert plan(hc, shape, esz, 1, options) == (0, [ref[0], ref[1], ref[5], ref[6]])


def test_workspace_sizes_are_the_documented_ones():
    """(16,16,16), B = 3, T = 4: adjoint trajectory [T+1][B][2][*S] (step: two frames) + B x MAX_BWD_BLOCKS partial rows of np
    doubles, each part rounded up to 256 bytes -- the brick launches fit their rows into the same B x 4096"""
    import percnn_amd
    from percnn_amd import _lib
    L = percnn_amd.lib()
    shape, n, B, T = _lib.shape_arg((16, 16, 16)), 16 ** 3, 3, 4
    up = lambda x: (x + 255) // 256 * 256
    for hc, npar in ((0, 36), (8, 16 + 2 * 81)):
        partials = B * up(4096 * npar * 8)
        for esz in (4, 8):
            for kind in ("batch", "ensemble"):
                assert getattr(L, f"percnn_pi_{kind}_rollout_bwd_workspace_bytes")(hc, 3, shape, B, T, esz) == \
                    up((T + 1) * B * 2 * n * esz) + partials, (kind, hc, esz)
                assert getattr(L, f"percnn_pi_{kind}_bwd_workspace_bytes")(hc, 3, shape, B, esz) == \
                    2 * up(B * 2 * n * esz) + partials, (kind, hc, esz)


def test_default_sends_only_the_measured_winners_to_the_bricks():
    """brick3d = 1 (batch_brick_default; profiles/batch_brick_throughput.json): pre-contracted blocks of 48^3 .. 128^3 points
    per sample in launches of at least 8 x 48^3 points; factored blocks lost on every row and everything unmeasured stays direct"""
    assert plan(0, (48, 48, 48), 4, 8) == (0, [BRICK, BRICK, 1, 1])
    assert plan(0, (48, 48, 48), 4, 64) == (0, [BRICK, BRICK, 1, 1])
    assert plan(0, (128, 128, 128), 4, 4) == (0, [BRICK, BRICK, 2, 1])
    assert plan(0, (48, 48, 48), 4, 7)[1][:2] == [DIRECT, DIRECT]            # a smaller launch than any measured
    assert plan(0, (48, 48, 47), 4, 64)[1][:2] == [DIRECT, DIRECT]           # smaller samples
    assert plan(0, (128, 128, 132), 4, 4)[1][:2] == [DIRECT, DIRECT]         # larger samples
    assert plan(0, (48, 48, 48), 8, 8)[1][:2] == [BRICK, BRICK]              # float64 follows the float32 figures
    for hc in (2, 8):
        assert plan(hc, (48, 48, 48), 4, 8)[1][:2] == [DIRECT, DIRECT]
        assert plan(hc, (48, 48, 48), 4, 8, {"brick3d": 2})[1][:2] == [BRICK, BRICK]
    assert plan(0, (48, 48, 48), 4, 8, {"brick3d": 0})[1][:2] == [DIRECT, DIRECT]
    assert plan(0, (9, 12, 64), 4, 3)[1][:2] == [DIRECT, DIRECT]
