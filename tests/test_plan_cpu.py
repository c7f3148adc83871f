"""percnn_pi_debug_plan / percnn_pi_debug_batch_plan print the plan the rollout entry points follow (csrc/pi_abi.hip "the rollout
plan": tile_variant_for, step_route, plan_fwd / plan_sweep).  Host side only, no device involved: the answers from before the
two shared one plan, held unchanged; the option combinations where the query used to differ from the launch; and that a tile
the query names is a tile kernel the library has."""
import ctypes
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "one_plan_parent_answers.json")))

# The tile kernels fwd_tile / adj_tile can launch (PI_TILE_VARIANTS and the wide shapes in csrc/pi_abi.hip), as
# (steps per launch, tile width, tile height, lanes); `poly`: instantiated for pre-contracted blocks (hc = 0) only
TILE_KERNELS = {
    (2, 32, 32, 256): "any", (8, 32, 32, 1024): "poly", (4, 32, 32, 1024): "poly", (4, 32, 16, 320): "poly", (4, 32, 8, 256): "poly",
    (4, 32, 32, 256): "any", (4, 32, 32, 512): "any",
    (4, 32, 40, 640): "poly", (4, 40, 40, 768): "poly",             # wide shapes: float32 only
}
# an explicit tile height next to an option that selects a 32-row kernel: (option string, lanes, steps per launch)
HEIGHT_IGNORED = [("tile_k=2,tile_by=8", 256, 2), ("tile_k=8,tile_by=16", 1024, 8), ("tile_nt=1024,tile_by=8", 1024, 4)]
OPTION_STRINGS = sorted({o for row in GOLDEN["plan"] for o in [row[3]]} | {o for o, _, _ in HEIGHT_IGNORED} | {
    "tile_k=2", "tile_k=8", "tile_nt=256", "tile_nt=1024", "tile_by=8", "tile_by=16", "tile_by=32", "tile_k=2,tile_by=16",
    "tile_k=8,tile_by=8", "tile_nt=1024,tile_by=16", "tile_nt=256,tile_by=16", "tile_nt=256,tile_by=8", "tile_wide=1", "tile_wide=2",
    "tile_fuse=0", "tile=2", "tile=2,tile_k=2,tile_by=8", "skip_wgrad=1", "res3d=2,brick3d=0", "res3d=0,brick3d=0"})


def raw_plan(hc, shape, esz, options):
    import percnn_amd
    from percnn_amd import _lib
    out = (ctypes.c_int * 15)(*([-7] * 15))
    rc = percnn_amd.lib().percnn_pi_debug_plan(hc, len(shape), _lib.shape_arg(tuple(shape)), esz, _lib.options_arg(options), out)
    return rc, list(out)


def raw_batch_plan(hc, shape, esz, batch, options):
    import percnn_amd
    from percnn_amd import _lib
    out = (ctypes.c_int * 4)(*([-7] * 4))
    rc = percnn_amd.lib().percnn_pi_debug_batch_plan(hc, len(shape), _lib.shape_arg(tuple(shape)), esz, batch,
                                                     _lib.options_arg(options), out)
    return rc, list(out)


def test_plans_pinned_before_are_unchanged():
    """every row test_host_logic.py::test_rollout_plan_follows_the_dispatch_rules and test_batch_brick_cpu.py pin, all fields.
    The fixture was taken without a device, where nothing can be resident; with one, the resident bits are not compared."""
    for hc, shape, esz, options, rc, ints in GOLDEN["plan"]:
        got_rc, got = raw_plan(hc, shape, esz, options)
        if torch.cuda.is_available():
            got[14] = ints[14]
        assert (got_rc, got) == (rc, ints), (hc, shape, esz, options)
    for hc, shape, esz, batch, options, rc, ints in GOLDEN["batch_plan"]:
        assert raw_batch_plan(hc, shape, esz, batch, options) == (rc, ints), (hc, shape, esz, batch, options)


@pytest.mark.parametrize("shape", [(64, 64), (100, 100)])
@pytest.mark.parametrize("options,lanes,steps", HEIGHT_IGNORED)
def test_a_tile_height_no_kernel_has_is_not_reported(shape, options, lanes, steps):
    """tile_k = 2, tile_k = 8 and tile_nt = 1024 each select one kernel, on 32 x 32 tiles; an explicit tile_by next to them is
    ignored by the launch, and the plan (tile geometry, partial rows) says so.  (Before: the query and the partial-row count
    took the explicit height while the launch ran 32 rows.)"""
    from percnn_amd import _lib
    p = _lib.rollout_plan(0, shape, 4, options)
    assert p["fwd"] == "tile2d" and p["bwd"] == "tile2d"
    assert p["tile"] == (32, 32, lanes) and p["tile_fwd"] == (32, 32, lanes)
    assert p["fwd_steps_per_launch"] == steps and p["bwd_steps_per_launch"] == steps
    assert p == _lib.rollout_plan(0, shape, 4, options.split(",")[0])


@pytest.mark.parametrize("esz", [4, 8])
@pytest.mark.parametrize("hc", [0, 2, 8])
def test_every_reported_tile_is_a_tile_kernel(hc, esz):
    from percnn_amd import _lib
    seen = set()
    for options in OPTION_STRINGS:
        for shape in [(64, 64), (100, 100), (128, 128), (320, 320), (352, 352), (512, 512), (544, 544), (640, 640), (1000, 1000)]:
            p = _lib.rollout_plan(hc, shape, esz, options)
            for tile, steps in ((p["tile"], p["bwd_steps_per_launch"]), (p["tile_fwd"], p["fwd_steps_per_launch"])):
                if tile is None:
                    assert steps == 1
                    continue
                kind = TILE_KERNELS.get((steps,) + tuple(tile))
                assert kind is not None, (hc, esz, shape, options, steps, tile)
                assert kind == "any" or hc == 0, (hc, esz, shape, options, steps, tile)
                assert tile[1] <= 32 or esz == 4, (hc, esz, shape, options, tile)
                seen.add((steps,) + tuple(tile))
    if hc == 0 and esz == 4:
        assert seen == set(TILE_KERNELS)                        # the option strings reach every kernel of the table
