"""No GPU: which values every tuning option accepts and refuses, pinned at the edges of its rule.

The library is driven through a per-call option string on percnn_pi_debug_plan, which touches no process default.  VALUES is
the record: per key the values that are accepted and the values that are refused (range: lo - 1, lo, hi, hi + 1; stepped
range: off-step values too; set: a non-member next to each member; boolean: anything goes).  It was written against the
strcmp ladder apply_option used to be and holds for the table that replaced it.  The keys of VALUES must be the keys the
source states -- a key added there without a row here fails test_every_key_of_the_source_has_a_row."""
import ctypes
import os
import re

import pytest

from percnn_amd import _lib

EINVAL = -1
ANY = ([0, 1, 2, -1, -2 ** 31, 2 ** 40], [])                 # boolean: stored as value != 0, nothing refused
M24, M22, M20 = 1 << 24, 1 << 22, 1 << 20

# key -> (accepted, refused)
VALUES = {
    "block": ([64, 128, 192, 256], [63, 65, 0, -64, 127, 129, 255, 257, 320]),
    "vec": ([0, 1], [-1, 2, 4]),
    "wgrad_blocks": ([1, 2, 1024, 2048], [0, -1, 2049, 4096]),
    "tile": ([0, 1, 2], [-1, 3]),
    "tile_k": ([2, 4, 8], [1, 3, 5, 7, 9, 0, 16]),
    "tile_nt": ([256, 512, 1024], [255, 257, 511, 513, 1023, 1025, 0, 128, 2048]),
    "stream3d": ([0, 1, 2], [-1, 3]),
    "tile_fuse": ([0, 1, 2], [-1, 3]),
    "bwd_cpl": ([1, 2, 16], [0, -1, 17]),
    "zc": ([1, 8, 1024], [0, -1, 1025]),
    "overlap": ANY,
    "overlap_chunk": ([1, 128, M20], [0, -1, M20 + 1]),
    "fuse_wgrad": ([0, 1, 2], [-1, 3]),
    "skip_wgrad": ANY,
    "tile_xcd": ANY,
    "handover_local": ANY,
    # N > 0 makes percnn_pi_debug_plan write N ints: tests/test_handover_local_cpu.py covers that with a buffer of the size
    "debug_handover_local": ([0], [-1, M24 + 1]),
    "tile_by": ([0, 8, 16, 32], [-1, 1, 7, 9, 15, 17, 31, 33, 64]),
    "slab_fused_put_adj": ANY,
    "peer_upb": ([256, 2048, 65536], [255, 0, -1, 65537]),
    "peer_upb_take": ([0, 256, 2048, 65536], [-1, 1, 255, 65537]),
    "tile_persist": ([0, 1, 2], [-1, 3]),
    "persist_handshake": ANY,
    "fwd_small_half": ([0, 1], [-1, 2]),
    "adj_small_half": ([0, 1], [-1, 2]),
    "adj_small_pause": ([-1, 0, 200], [-2, 201]),
    "fwd_small_pause": ([-1, 0, 200], [-2, 201]),
    "persist_small": ([0, 1, 2], [-1, 3]),
    "fwd_persist_per_cu": ([1, 2], [0, 3]),
    "fwd_persist_f64": ANY,
    "adj_persist_f64": ANY,
    "fwd_persist": ANY,
    "persist_split": ANY,
    "persist_timeout_ms": ([1, 2000, 600000], [0, -1, 600001]),
    "persist_first_timeout_ms": ([1, 100, 600000], [0, -1, 600001]),
    "tile_wide": ([0, 1, 2, 3], [-1, 4]),
    "fwd_blocks": ([0, 1, M24], [-1, M24 + 1]),
    "xcd_window": ([0, 8, 16, M24], [-1, -8, 1, 7, 9, 12, M24 - 1, M24 + 1, M24 + 8]),
    "block_small": ANY,
    "rz": ([0, 1, 2, 4], [-1, 3, 5, 8]),
    "l2_tile_kb": ([0, 128, 16384], [-1, 16385]),
    "l2_tile_min_kb": ([0, 1536, M22], [-1, M22 + 1]),
    "peer_wire_us": ([0, 1, 100000], [-1, 100001]),
    "slab_put_blocks": ([4, 8, 16, 256], [0, 3, 5, 6, -4, 255, 257, 260]),
    "slab_fused_put": ANY,
    "slab_local_index": ANY,
    "slab_wide_adjoint": ANY,
    "lane_x": ([-1, 0, 2, 3, 4, 5, 6, 7], [-2, 1, 8]),
    "brick3d": ([0, 1, 2], [-1, 3]),
    "res3d": ([0, 1, 2], [-1, 3]),
    "brick_rz": ([0, 1, 2, 4], [-1, 3, 5, 8]),
    "brick_xcd": ([0, 1, 2], [-1, 3]),
    "brick_xny": ([-1, 0, 1, 2, 4, 8], [-2, 3, 5, 6, 7, 9, 16]),
    "brick_wide": ANY,
    "brick_nt": ([0, 256, 512], [-1, 1, 255, 257, 511, 513, 1024]),
    "brick_wgs": ([0, 1, 16], [-1, 17]),
    "brick_wt": ANY,
    "lds_pad": ([0, 16, 32, 80 * 1024], [-1, -16, 1, 15, 17, 24, 80 * 1024 - 1, 80 * 1024 + 1, 80 * 1024 + 16]),
    # the two keys that are no field of Options
    "graph": ([0], [-1, 1, 2]),                                # reserved
    "persist_reset": ([0, 1, -1, 7], []),                      # re-arms the resident launches, whatever the value
}


def plan_rc(spec):
    """return code of a plan query of a 64 x 64 float32 polynomial block under the per-call option string"""
    out = (ctypes.c_int * 15)()
    return _lib.lib().percnn_pi_debug_plan(0, 2, _lib.shape_arg((64, 64)), 4, spec, out)


def test_rollout_plan_takes_the_option_string():
    assert _lib.rollout_plan(0, (64, 64), 4, "tile_k=4")["fwd"]
    with pytest.raises(RuntimeError):
        _lib.rollout_plan(0, (64, 64), 4, "tile_k=3")


def test_there_are_58_fields_and_two_commands():
    assert len(VALUES) == 60


@pytest.mark.parametrize("key", sorted(VALUES))
def test_accepted_and_refused_values(key):
    accepted, refused = VALUES[key]
    for v in accepted:
        assert plan_rc(f"{key}={v}".encode()) == 0, (key, v)
    for v in refused:
        assert plan_rc(f"{key}={v}".encode()) == EINVAL, (key, v)


def test_set_option_refuses_the_per_call_query_and_unknown_keys():
    L = _lib.lib()
    for v in (0, 1, 16):
        assert L.percnn_pi_set_option(b"debug_handover_local", v) == EINVAL
    assert L.percnn_pi_set_option(None, 1) == EINVAL
    assert L.percnn_pi_set_option(b"nonsense", 1) == EINVAL
    assert L.percnn_pi_set_option(b"", 1) == EINVAL
    assert L.percnn_pi_set_option(b"graph", 1) == EINVAL and L.percnn_pi_set_option(b"graph", 0) == 0
    assert L.percnn_pi_set_option(b"tile_k", 3) == EINVAL and L.percnn_pi_set_option(b"tile_k", 4) == 0     # (4: the default)


def test_parser_of_the_option_string():
    ok = [None, b"", b"tile_k=4", b"tile_k=4,skip_wgrad=1", b"tile_k=4,",            # a trailing comma ends the string
          b"tile_k= 4", b"tile_k=+4", b"tile_k=04", b"adj_small_pause=-1",          # the value is strtol's, base 10
          b"tile_k=2,tile_k=4"]
    bad = [b"nonsense=1", b"tile_k=3", b"tile_k", b"=4", b"tile_k=4;tile=0", b"tile_k=x",      # tests/test_host_logic.py's
           b"tile_k=", b"tile_k=,tile=0", b"tile_k=4,,tile=0", b"a=1,,b=2", b",tile_k=4", b",",
           b"tile_k=4 ", b"tile_k=4x", b"tile_k=0x4", b" tile_k=4", b"tile_k =4", b"TILE_K=4",
           b"tile_k=4,nonsense=1", b"tile_k=4,tile", b"tile_k=99999999999999999999",
           b"a" * 31 + b"=1",                                   # fits the key buffer, names nothing
           b"a" * 32 + b"=1", b"a" * 33 + b"=1", b"a" * 4096 + b"=1",     # 32 characters and more: refused unread
           b"tile_k" + b"x" * 26 + b"=4"]
    for spec in ok:
        assert plan_rc(spec) == 0, spec
    for spec in bad:
        assert plan_rc(spec) == EINVAL, spec
    # a refused string leaves the call without effect and never reaches the process defaults
    assert plan_rc(b"tile=0,tile_k=3") == EINVAL
    assert _lib.rollout_plan(0, (64, 64), 4) == _lib.rollout_plan(0, (64, 64), 4, "tile=1,tile_k=4")


def test_every_key_of_the_source_has_a_row():
    """the keys apply_option knows, read from the source: arms `strcmp(key, "...")` of a ladder and rows `PI_OPT(name, ...)` of
    the table, whichever the tree has"""
    found = set()
    for unit in ("pi_abi.hip", "pi_host.hip"):
        path = os.path.join(_lib.CSRC, unit)
        if os.path.exists(path):
            with open(path) as f:
                text = f.read()
            found |= set(re.findall(r'strcmp\(key, "(\w+)"\)', text)) | set(re.findall(r"^\s*PI_OPT\((\w+),", text, re.M))
    assert found == set(VALUES), (sorted(found - set(VALUES)), sorted(set(VALUES) - found))
