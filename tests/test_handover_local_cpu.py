"""No GPU: which band granules option handover_local publishes with plain stores.  percnn_pi_debug_plan with the per-call key
debug_handover_local=N evaluates the kernels' own rule (HandOver<>::pub_local, pi_tile2d.h) on the host and returns one bit per
band granule; here every band value's readers are enumerated by brute force -- every neighbour tile whose 48 x 48 window holds
the value, periodic wrap applied -- with their XCDs taken from the rectangle map and the granule numbering of the outbox both
stated independently, and the two are compared granule by granule."""
import ctypes

import numpy as np
import pytest

from percnn_amd import _lib

B, HW, NXCD = 32, 8, 8                                     # tile edge, halo width (2 K, K = 4), XCDs


def rectangles(tiles_y, tiles_x):
    """the tile_xcd map: 8 equal rectangles, smallest perimeter, first of equals in the order 1, 2, 4, 8 per row; None: identity"""
    best = None
    for rx in (1, 2, 4, 8):
        ry = NXCD // rx
        if tiles_x % rx or tiles_y % ry:
            continue
        rw, rh = tiles_x // rx, tiles_y // ry
        if best is None or rw + rh < best[0]:
            best = (rw + rh, rx, rw, rh)
    return best and best[1:]


def band_index(y, x):
    """position inside the tile -> index inside its border band: the first HW rows, the last HW rows, then the 2 HW side values
    of every row between"""
    if y < HW:
        return y * B + x
    if y >= B - HW:
        return HW * B + (y - (B - HW)) * B + x
    return 2 * HW * B + (y - HW) * 2 * HW + (x if x < HW else HW + x - (B - HW))


BAND = B * B - (B - 2 * HW) ** 2                           # band values per species: 768


def brute_force(shape, elem_size):
    """[tiles_y, tiles_x, granules per tile] booleans: granule (species, band_index / values per granule) is local"""
    tiles_y, tiles_x = shape[0] // B, shape[1] // B
    rect = rectangles(tiles_y, tiles_x)
    gv = 2 if elem_size == 4 else 1                        # values per granule, x-adjacent
    bandu = BAND // gv
    out = np.zeros((tiles_y, tiles_x, 2 * bandu), dtype=bool)
    if rect is None:
        return out
    rx, rw, rh = rect
    xcd = lambda ty, tx: (ty // rh) * rx + tx // rw
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            for y in range(B):
                for x0 in range(0, B, gv):
                    if HW <= y < B - HW and HW <= x0 < B - HW:
                        continue                           # not in the band
                    local = True
                    for x in range(x0, x0 + gv):
                        for dy in (-1, 0, 1):
                            for dx in (-1, 0, 1):
                                if (dy, dx) == (0, 0):
                                    continue
                                # the window of tile (ty + dy, tx + dx) spans [-HW, B + HW) about its origin
                                if -HW <= y - B * dy < B + HW and -HW <= x - B * dx < B + HW:
                                    local &= xcd((ty + dy) % tiles_y, (tx + dx) % tiles_x) == xcd(ty, tx)
                    assert band_index(y, x0) % gv == 0
                    for sp in range(2):                    # both species travel alike
                        out[ty, tx, sp * bandu + band_index(y, x0) // gv] = local
    return out


def query_bits(shape, elem_size, options=None):
    """the library's answer, as brute_force's array"""
    tiles_y, tiles_x = shape[0] // B, shape[1] // B
    per_tile = 2 * BAND // (2 if elem_size == 4 else 1)
    n = tiles_y * tiles_x * per_tile // 32
    out = (ctypes.c_int * n)()
    opts = dict(options or {}, debug_handover_local=n)
    rc = _lib.lib().percnn_pi_debug_plan(0, 2, _lib.shape_arg(shape), elem_size, _lib.options_arg(opts), out)
    assert rc == 0
    words = np.array(out[:], dtype=np.int64).astype(np.uint32)
    bits = (words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1
    return bits.astype(bool).reshape(tiles_y, tiles_x, per_tile)


def query(shape, elem_size, options=None):
    """local granules per tile"""
    return query_bits(shape, elem_size, options).sum(axis=2)


# the shapes of the GPU test, the flagship, rectangles one tile high whose x-neighbours wrap onto themselves, an 8 x 8 tile grid
SHAPES = [(128, 128), (256, 128), (160, 160), (512, 512), (256, 64), (256, 256)]


@pytest.mark.parametrize("elem_size", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_local_granules_match_brute_force(shape, elem_size):
    want = brute_force(shape, elem_size)
    assert np.array_equal(query_bits(shape, elem_size), want)            # granule by granule
    assert not query(shape, elem_size, {"handover_local": 0}).any()
    assert not query(shape, elem_size, {"tile_xcd": 0}).any()           # identity map: nothing is local


def test_known_counts():
    per_tile = 2 * (B * B - (B - 2 * HW) ** 2) // 2        # 768 float32 granules of two values
    got = query((512, 512), 4)
    # 8 x 4 tiles per XCD: N/S pieces 3/4, E/W pieces 7/8, corner blocks 21/32 local -> 73/96 = 76 % on average
    assert got.sum() * 96 == 73 * per_tile * got.size
    assert (got[1:3, 1:7] == per_tile).all() and got.max() == per_tile and got.min() < per_tile
    assert rectangles(16, 16) == (2, 8, 4)
    assert np.array_equal(query((512, 512), 8), 2 * got)
    assert not query((160, 160), 4).any() and rectangles(5, 5) is None
    assert rectangles(4, 4) == (2, 2, 1) and rectangles(8, 2) == (1, 2, 1)        # rectangles one tile high
    assert 0 < query((128, 128), 4).min() and query((128, 128), 4).max() < per_tile


def test_refusals():
    out = (ctypes.c_int * 384)()
    f, q = _lib.lib().percnn_pi_debug_plan, b"debug_handover_local=384"
    assert f(0, 2, _lib.shape_arg((128, 128)), 4, q, out) == 0         # 16 tiles x 24 words fit exactly
    assert f(0, 2, _lib.shape_arg((100, 128)), 4, q, out) != 0         # not whole 32 x 32 tiles
    assert f(0, 3, _lib.shape_arg((32, 32, 32)), 4, q, out) != 0
    assert f(0, 2, _lib.shape_arg((128, 128)), 2, q, out) != 0
    assert f(0, 2, _lib.shape_arg((128, 128)), 4, q, None) != 0
    # the buffer's capacity travels with the key: one int short and nothing is written
    guard = (ctypes.c_int * 384)(*([-7] * 384))
    assert f(0, 2, _lib.shape_arg((128, 128)), 4, b"debug_handover_local=383", guard) != 0 and set(guard) == {-7}
    assert f(0, 2, _lib.shape_arg((128, 128)), 8, q, guard) != 0 and set(guard) == {-7}       # float64: 48 words per tile
    # ... so a caller that expects the plan's 15 words and passes the key by mistake is refused, not overrun
    with pytest.raises(RuntimeError):
        _lib.rollout_plan(0, (512, 512), 4, {"debug_handover_local": 1})
    with pytest.raises(RuntimeError):
        _lib.rollout_plan(0, (512, 512), 4, {"debug_handover_local": 15})
    assert _lib.rollout_plan(0, (128, 128), 4, {"debug_handover_local": 0})["tile"] is not None
    # a query of one call and one entry point, never a process-wide default
    assert _lib.lib().percnn_pi_set_option(b"debug_handover_local", 384) != 0
    four = (ctypes.c_int * 4)()
    assert _lib.lib().percnn_pi_debug_batch_plan(0, 2, _lib.shape_arg((128, 128)), 4, 1, q, four) != 0
