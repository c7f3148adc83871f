"""No GPU: the tiling trick of tiled_oracle.py held to the plain-C oracle itself on grids the oracle can still afford, and its
helpers (which take CPU tensors as well) on the cases where they could lie."""
import numpy as np
import pytest
import torch

import tiled_oracle as TO
import util
from util import random_block


@pytest.mark.parametrize("shape,period,hc,dtype", [((16, 36), (8, 12), 0, np.float32), ((24, 20), (8, 10), 2, np.float32),
                                                   ((16, 24), (8, 12), 0, np.float64), ((12, 8, 20), (6, 8, 10), 0, np.float32)])
def test_the_oracle_of_a_tiled_field_is_the_tiling_of_the_oracle(shape, period, hc, dtype):
    """forward, dL/dh0 (dense and masked) bit for bit; the gradient row is tiles x the tile's up to the order of float64 sums"""
    rs = np.random.RandomState(3)
    T, nd = 9, len(shape)
    reps = TO.reps_of(shape, period)
    P = random_block(hc, nd, dtype, 5, scale=0.3)
    h0_t = rs.uniform(0.1, 0.9, (2,) + period).astype(dtype)
    g_t = rs.standard_normal((T + 1, 2) + period).astype(dtype)
    traj_t = TO.rollout_fwd(h0_t, P, T)
    traj = util.o_rollout_fwd(np.tile(h0_t, (1,) + reps), P, T)
    TO.assert_is_tiling(torch.from_numpy(traj), traj_t, nd, "oracle forward")
    for mask in (None, [t % 3 != 1 for t in range(T + 1)]):
        g0_t, row_t = TO.rollout_bwd(traj_t, g_t, P, mask)
        g = np.tile(g_t, (1, 1) + reps)
        if mask is not None:
            g[[not m for m in mask]] = 0
        g0, row = util.o_rollout_bwd(traj, g, P)
        TO.assert_is_tiling(torch.from_numpy(g0), g0_t, nd, "oracle dL/dh0")
        assert util.grad_err(row, TO.tiles_of(shape, period) * row_t) < 1e-12
    TO.assert_is_tiling(torch.from_numpy(util.o_step_fwd(traj[3], P)), TO.step_fwd(traj_t[3], P), nd, "oracle step")


def test_tile_up_and_the_comparison_find_one_wrong_bit(monkeypatch):
    rs = np.random.RandomState(0)
    tile = rs.standard_normal((3, 2, 4, 6)).astype(np.float32)
    full = TO.tile_up(tile, (12, 18))
    assert full.shape == (3, 2, 12, 18) and np.array_equal(full.numpy(), np.tile(tile, (1, 1, 3, 3)))
    out = torch.full((3, 2, 12, 18), float("nan"))
    assert TO.tile_up(tile, (12, 18), out=out) is out and torch.equal(out, full)
    for chunk in (1 << 30, 2 * 12 * 18, 100, 1):           # rows per chunk: all, two, (one row split in periods), one period
        monkeypatch.setattr(TO, "CHUNK_ELEMS", chunk)
        TO.assert_is_tiling(full, tile, 2)
        bad = full.clone()
        bad.view(torch.int32)[2, 1, 9, 4] += 1            # one unit in the last place
        bad[2, 1, 11, 17] = 0
        with pytest.raises(AssertionError, match=r"first difference .* at \(2, 1\) \+ \(9, 4\)"):
            TO.assert_is_tiling(bad, tile, 2, "x")
    nan = full.clone()
    nan[0, 0, 0, 0] = float("nan")
    tile_nan = tile.copy()
    tile_nan[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        TO.assert_is_tiling(nan, tile, 2)
    with pytest.raises(AssertionError):                    # the tiling of a NaN is a NaN at every repeat
        TO.assert_is_tiling(nan, tile_nan, 2)
    TO.assert_is_tiling(TO.tile_up(tile_nan, (12, 18)), tile_nan, 2)
    t3 = rs.standard_normal((2, 2, 3, 5)).astype(np.float64)
    TO.assert_is_tiling(TO.tile_up(t3, (4, 9, 5)), t3, 3)


def test_wraps_are_visible_refuses_what_would_hide_a_wrap():
    rs = np.random.RandomState(1)
    T = 4672
    moving = rs.standard_normal((T + 1, 2, 40, 48)).astype(np.float32)
    seen = TO.wraps_are_visible(moving, (T + 1, 2, 480, 480), 4)
    assert sorted(seen) == [1 << 29, 1 << 30, 1 << 31] and min(seen.values()) >= 0.99
    # a buffer that crosses nothing: nothing to check (the caller insists on the distances it means to cross)
    assert TO.wraps_are_visible(moving[:10], (10, 2, 480, 480), 4) == {}
    # a trajectory that has settled to a uniform steady state: one value per species, at every time
    steady = np.broadcast_to(np.array([0.4, 0.2], dtype=np.float32)[None, :, None, None], moving.shape)
    with pytest.raises(AssertionError, match="would not see a 32-bit wrap"):
        TO.wraps_are_visible(steady, (T + 1, 2, 480, 480), 4)
    # powers of two all the way: a shift by 2^29 elements is a whole number of frames of a [*, 2, 512, 512] trajectory, and
    # with a period in time (here: two alternating frames) it lands on an equal value
    two = np.broadcast_to(rs.standard_normal((2, 2, 32, 32)).astype(np.float32)[None], (2049, 2, 2, 32, 32)).reshape(4098, 2, 32, 32)
    with pytest.raises(AssertionError, match="would not see a 32-bit wrap"):
        TO.wraps_are_visible(two, (4098, 2, 512, 512), 4)
    # in-frame: a plane of 2^31 bytes in a power-of-two grid puts species 1 exactly one wrap away from species 0
    same = np.broadcast_to(rs.standard_normal((1, 32, 32)).astype(np.float32), (2, 32, 32))
    with pytest.raises(AssertionError, match="would not see a 32-bit wrap"):
        TO.wraps_are_visible(same, (2, 16384, 32768), 4)
    TO.wraps_are_visible(rs.standard_normal((2, 48, 48)).astype(np.float32), (2, 24576, 24624), 4)
    # float64: the byte distances are 2^28 and 2^29 elements
    assert (1 << 28) in TO.wraps_are_visible(rs.standard_normal((1169, 2, 40, 48)), (1169, 2, 480, 480), 8)
