"""The plain-C oracle on a periodically tiled problem.

The operators are pointwise plus a periodic stencil.  A field that repeats a small tile (py, px[, pz]) whose extents divide the
grid's therefore maps, bit for bit, onto the tiling of the oracle's result on the tile alone -- forward, for the adjoint state,
over any number of steps -- and the parameter gradient of the grid is (number of tiles) x the tile's.  That makes the oracle
affordable at sizes where buffers pass 2^31 elements or 2^32 bytes: it runs on the tile, the device holds the grid.

A 32-bit slip moves an access by 2^31 or 2^32 bytes or elements.  With extents that are powers of two such a move lands on an
equivalent periodic position and the tiling hides it; ``wraps_are_visible`` is the precondition, on the reference alone, that it
does not."""
import numpy as np
import torch

import util

# elements per comparison chunk: the bool result of `ne` (1 byte each) is the only temporary of that size -- 1 GiB
CHUNK_ELEMS = 1 << 30
DISTANCES = (1 << 29, 1 << 30, 1 << 31, 1 << 32)          # elements; for float32 the first two are 2^31 and 2^32 bytes


def reps_of(shape, period):
    shape, period = tuple(int(s) for s in shape), tuple(int(p) for p in period)
    assert len(shape) == len(period) and all(s % p == 0 for s, p in zip(shape, period)), (shape, period)
    return tuple(s // p for s, p in zip(shape, period))


def tiles_of(shape, period):
    return int(np.prod(reps_of(shape, period)))


def tile_up(tile, shape, device=None, out=None):
    """tile [..., *p] (numpy or torch) -> device tensor [..., *shape] that repeats it over the trailing len(shape) axes
    (out: write there)"""
    t = torch.tensor(tile) if isinstance(tile, np.ndarray) else tile      # (a copy: references are read-only arrays)
    if device is not None:
        t = t.to(device)
    nd = len(shape)
    reps = reps_of(shape, t.shape[t.dim() - nd:])
    lead = tuple(t.shape[:t.dim() - nd])
    if out is None:
        out = torch.empty(lead + tuple(shape), dtype=t.dtype, device=t.device)
    assert tuple(out.shape) == lead + tuple(shape) and out.is_contiguous()
    inter = []
    for r, p in zip(reps, t.shape[t.dim() - nd:]):
        inter += [r, p]
    ov = out.view(lead + tuple(inter))                      # [..., ry, py, rx, px]: a view, nothing is copied twice
    tv = t.reshape(lead + tuple(x for p in t.shape[t.dim() - nd:] for x in (1, p)))
    ov.copy_(tv.expand_as(ov))
    return out


def _int_view(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def _first_true(ne):
    """index tuple of the first True of a bool tensor in C order, by one reduction per axis"""
    idx = []
    for _ in range(ne.dim()):
        v = ne if ne.dim() == 1 else ne.flatten(1).any(1)
        i = int(torch.nonzero(v)[0])
        idx.append(i)
        ne = ne[i]
    return tuple(idx)


def assert_is_tiling(dev, tile, ndim, what="tensor"):
    """dev [*lead, *S] on the device (S: the trailing ndim axes) is, bit for bit (NaN payloads included), the tiling of tile
    [*lead, *p].  Compared through a reshaped broadcast view in chunks of leading rows (and of periods along the first spatial
    axis where one row alone is too large): no temporary above CHUNK_ELEMS bytes.  Reports the first differing (lead..., point)."""
    t = torch.tensor(tile) if isinstance(tile, np.ndarray) else tile
    t = t.to(dev.device)
    assert dev.dtype == t.dtype and dev.is_contiguous(), (dev.dtype, t.dtype)
    assert dev.dim() == t.dim(), "tile and tensor must have the same number of axes"
    k = dev.dim() - int(ndim)
    lead, S, p = tuple(dev.shape[:k]), tuple(dev.shape[k:]), tuple(t.shape[k:])
    assert tuple(t.shape[:k]) == lead, (tuple(dev.shape), tuple(t.shape))
    reps = reps_of(S, p)
    L = int(np.prod(lead)) if lead else 1
    row = int(np.prod(S))
    inter = tuple(x for r, q in zip(reps, p) for x in (r, q))
    dv = _int_view(dev).view((L,) + inter)                  # [L, r0, p0, r1, p1, ...]
    tv = _int_view(t.contiguous()).view((L,) + tuple(x for q in p for x in (1, q)))
    rows = max(1, CHUNK_ELEMS // row)
    per0 = reps[0] if row <= CHUNK_ELEMS else max(1, CHUNK_ELEMS // (row // reps[0]))
    for l0 in range(0, L, rows):
        l1 = min(L, l0 + rows)
        for r0 in range(0, reps[0], per0):
            r1 = min(reps[0], r0 + per0)
            ne = dv[l0:l1, r0:r1] != tv[l0:l1]
            if bool(ne.any()):
                i = _first_true(ne)
                li = np.unravel_index(l0 + i[0], lead) if lead else ()
                point = tuple((i[1 + 2 * a] + (r0 if a == 0 else 0)) * p[a] + i[2 + 2 * a] for a in range(len(p)))
                got = dev[tuple(int(x) for x in li) + point].item()
                want = t[tuple(int(x) for x in li) + tuple(x % q for x, q in zip(point, p))].item()
                raise AssertionError(f"{what}: first difference from the tiled oracle at {tuple(int(x) for x in li)} + {point}: "
                                     f"got {got!r}, the tile holds {want!r}")
            del ne


def wraps_are_visible(tile_buf, layout, elem_size, samples=2000, seed=0, need=0.99):
    """The precondition of the tiling trick, on the reference alone.  tile_buf [*lead, *p]: the tile's version of a device
    buffer of shape `layout` = [*lead, *S].  For every distance D of DISTANCES (elements) and of 2^31, 2^32 bytes that fits
    inside the buffer: `samples` random element offsets o >= D; o and o - D are mapped through the layout onto the tile (lead
    indices as they are, points modulo the periods); the two values must differ in at least `need` of the samples -- a 32-bit
    wrap of an index or a byte offset by D then shows as wrong bits in almost every element it touches.
    -> {D: fraction}; the caller asserts that the dict is not empty where its buffer is meant to cross a threshold."""
    tile_buf = np.asarray(tile_buf)
    layout = tuple(int(x) for x in layout)
    assert tile_buf.ndim == len(layout)
    total = int(np.prod([int(x) for x in layout], dtype=object))
    mods = np.array(tile_buf.shape, dtype=np.int64)
    for n, q in zip(layout, tile_buf.shape):
        assert n % q == 0, (layout, tile_buf.shape)
    bits = np.ascontiguousarray(tile_buf).view(np.uint32 if tile_buf.dtype.itemsize == 4 else np.uint64)
    dists = sorted(set(DISTANCES) | {(1 << 31) // elem_size, (1 << 32) // elem_size})
    rs = np.random.RandomState(seed)
    out = {}
    for D in dists:
        if D >= total:
            continue
        o = D + (rs.random_sample(samples) * (total - D)).astype(np.int64)
        o = np.minimum(o, total - 1)
        a = bits[tuple(i % m for i, m in zip(np.unravel_index(o, layout), mods))]
        b = bits[tuple(i % m for i, m in zip(np.unravel_index(o - D, layout), mods))]
        out[D] = float(np.mean(a != b))
        assert out[D] >= need, (f"a shift by {D} elements ({D * elem_size} bytes) in a buffer {layout} tiled from "
                                f"{tile_buf.shape} changes only {100 * out[D]:.1f} % of the sampled values: the tiled "
                                f"oracle would not see a 32-bit wrap")
    return out


# ---- the oracle on the tile ----
def rollout_fwd(h0_tile, P, T):
    """[2,*p] -> [T+1,2,*p]"""
    return util.o_rollout_fwd(np.ascontiguousarray(h0_tile), P, T)


def rollout_bwd(traj_tile, g_tile, P, mask=None):
    """-> (dL/dh0 [2,*p], the tile's float64 gradient row); frames a mask switches off count as zero"""
    g = np.array(g_tile, copy=True)
    if mask is not None:
        g[[not m for m in mask]] = 0
    g0, pg = util.o_rollout_bwd(np.ascontiguousarray(traj_tile), g, P)
    return g0, np.asarray(pg, dtype=np.float64)


def step_fwd(h_tile, P):
    return util.o_step_fwd(np.ascontiguousarray(h_tile), P)


def step_bwd(h_tile, G_tile, inj_tile, P):
    gp, pg = util.o_step_bwd(np.ascontiguousarray(h_tile), np.ascontiguousarray(G_tile), inj_tile, P)
    return gp, np.asarray(pg, dtype=np.float64)
