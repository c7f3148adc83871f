"""No GPU: the Python binding of the C ABI is derived from the prototypes of include/percnn_pi*.h (percnn_amd/_lib.py).  What
holds it: the symbols the built library defines are counted by another tool than the parser, one signature per row of the type
rule is stated here literally, the parser refuses what it has no row for, and the three structures that cross the ABI are laid
out as the C compiler lays them out."""
import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_int, c_int64, c_long, c_size_t, c_uint32, c_uint64, c_void_p

import pytest

from percnn_amd import _lib

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

# exported by timing builds for tools that type them themselves; declared in no header, hence not bound
DEBUG_SYMBOLS = {"percnn_pi_debug_stamps", "percnn_pi_debug_wave_stamps", "percnn_pi_s1_debug_stamps"}


def test_every_defined_symbol_is_declared_and_every_declared_one_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    defined = {word for word in out.split() if word.startswith("percnn_pi_")}
    # the three are compiled only into timing builds (-DPI_TILE_TIMING, -DPI_S1_TIMING): a library may define them, and nothing
    # else that no header declares
    assert defined - DEBUG_SYMBOLS == set(_lib.PROTOTYPES)
    assert not DEBUG_SYMBOLS & set(_lib.PROTOTYPES)
    assert _lib.EXPORTS == list(_lib.PROTOTYPES) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS) == 153
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


vp, cs, ci, cd, sz, i64, u64 = c_void_p, c_char_p, c_int, c_double, c_size_t, c_int64, c_uint64
ip, lp, i64p, u64p, vpp = POINTER(c_int), POINTER(c_long), POINTER(c_int64), POINTER(c_uint64), POINTER(c_void_p)
ANCHORS = {
    "percnn_pi_rollout_bwd_f32": (ci, [vp, vp, cs, vp, vp, vp, sz, vp, ci, ci, i64p, ci, vp]),
    "percnn_pi_pack_fwd_guard_f64": (ci, [POINTER(_lib.ParamPtrs), ci, ci, cd, cd, ci, ci, vp, cd, cd, vp, cd, vp]),
    "percnn_pi_peer_box_status": (ci, [vp, u64p, vp]),
    "percnn_pi_peer_box_alloc": (ci, [vpp, sz]),
    "percnn_pi_peer_exchange_f32": (ci, [vp, ci, i64p, ci, ci, POINTER(_lib.PeerRing), vp]),
    "percnn_pi_library_moments_f32": (ci, [vp, i64, i64, i64p, ci, ci, cd, cd, ci, c_uint32, u64, u64, vp, vp, vp, vp, vp, sz,
                                           vp]),
    "percnn_pi_set_option": (ci, [cs, c_long]),
    "percnn_pi_persist_status": (ci, [lp]),
    "percnn_pi_batch_rollout_bwd_obs_sqerr_f64": (ci, [vp, vp, cs, ip, cd, vp, vp, vp, vp, sz, vp, ci, ci, i64p, ci, ci, cs, vp]),
    "percnn_pi_slab_rollout_fwd_f64": (ci, [vp, vp, ci, ci, i64p, ci, ci, POINTER(_lib.HaloRing), ci, vp]),
    "percnn_pi_lib_rk4_ensemble_rollout_bwd_workspace_bytes": (sz, [i64p, ci, ci]),
    "percnn_pi_halo_ring_bytes": (sz, []),
}


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_anchor_signature(name):
    restype, argtypes = ANCHORS[name]
    got_res, got_args = _lib.PROTOTYPES[name]
    assert got_res is restype
    assert len(got_args) == len(argtypes)
    for k, (got, want) in enumerate(zip(got_args, argtypes)):
        assert got is want, (name, k, got, want)
    f = getattr(_lib.lib(), name)
    assert f.restype is restype and len(f.argtypes) == len(argtypes)
    assert all(got is want for got, want in zip(f.argtypes, argtypes))


def test_every_row_of_the_type_rule_has_an_anchor():
    used = {c for res, args in ANCHORS.values() for c in [res] + args}
    assert used == set(_lib.CTYPES.values())


def test_the_entry_points_that_had_no_argtypes_are_bound():
    lengths = {"percnn_pi_abi_version": 0, "percnn_pi_persist_fence": 1}
    for suf in ("f32", "f64"):
        lengths.update({f"percnn_pi_step_bwd_rows_{suf}": 12, f"percnn_pi_bwd_rows_finish_{suf}": 7,
                        f"percnn_pi_rollout_bwd_top_{suf}": 15})
    L = _lib.lib()
    for name, n in lengths.items():
        f = getattr(L, name)
        assert f.restype is c_int and f.argtypes is not None and len(f.argtypes) == n, name
    assert list(L.percnn_pi_persist_fence.argtypes) == [vp]
    assert list(L.percnn_pi_bwd_rows_finish_f32.argtypes) == [vp, sz, ci, ci, i64p, vp, vp]


@pytest.mark.parametrize("text, name", [("int percnn_pi_x(struct foo *p);", "percnn_pi_x"),
                                        ("float percnn_pi_y(int a);", "percnn_pi_y"),
                                        ("int percnn_pi_z(long long n);", "percnn_pi_z"),
                                        ("int percnn_pi_w(const void** p);", "percnn_pi_w"),
                                        ("int percnn_pi_v(char* out);", "percnn_pi_v"),
                                        ("int percnn_pi_u(int a[3]);", "percnn_pi_u")])
def test_the_parser_refuses_a_type_without_a_row(text, name):
    with pytest.raises(RuntimeError, match=rf"some_header\.h.*\b{name}\b"):
        _lib.parse_prototypes(text, "some_header.h")


def test_the_parser_reads_c_as_it_is_written():
    text = """
    #ifndef X
    #define PERCNN_PI_FAKE(a, b) \\
        percnn_pi_not_a_prototype(a, b);
    typedef struct percnn_pi_peer_ring { void* my_box; int (*send)(const void* buf, size_t count); } percnn_pi_peer_ring;
    /* int percnn_pi_commented_out(int a); */
    // int percnn_pi_commented_out_too(int a);
    int percnn_pi_a(const float *x, const float* y, const float * z, const float*w,   /* four ways to attach the star */
                    int n /* a comment, with a comma, inside the list */,
                    // and a line comment, with (parentheses);
                    void **out,
                    percnn_pi_peer_ring* ring);        /* trailing */
    size_t
    percnn_pi_b
        (void);
    int percnn_pi_c(int, const unsigned char*, long *);int percnn_pi_d(const int64_t*shape);
    #endif
    """
    assert _lib.parse_prototypes(text) == {
        "percnn_pi_a": (ci, [vp, vp, vp, vp, ci, vpp, POINTER(_lib.PeerRing)]),
        "percnn_pi_b": (sz, []),
        "percnn_pi_c": (ci, [ci, cs, lp]),
        "percnn_pi_d": (ci, [i64p]),
    }


STRUCTS = {     # C name -> (ctypes class, members in the order of include/percnn_pi.h)
    "percnn_pi_param_ptrs": (_lib.ParamPtrs, ["c", "w", "branch"]),
    "percnn_pi_peer_ring": (_lib.PeerRing, ["my_box", "prev_box", "next_box", "slot_bytes", "epoch", "timeout_ticks"]),
    "percnn_pi_halo_ring": (_lib.HaloRing, ["comm", "prev", "next", "dtype_f32", "dtype_f64", "group_start", "group_end", "send",
                                            "recv", "peer", "stage", "stage_bytes"]),
}


def test_structure_layouts_are_the_c_compilers(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "percnn_pi.h"', "int main(void) {"]
    for cname, (_, members) in STRUCTS.items():
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{m} %zu %zu\\n", offsetof({cname}, {m}), sizeof((({cname}*)0)->{m}));' for m in members]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", INCLUDE, "-o", str(exe), str(src)])
    c = {k: [int(x) for x in v] for k, *v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    for cname, (cls, members) in STRUCTS.items():
        assert [n for n, _ in cls._fields_] == members
        assert c[cname] == [ctypes.sizeof(cls)], cname
        for m in members:
            field = getattr(cls, m)
            assert c[f"{cname}.{m}"] == [field.offset, field.size], (cname, m)
    assert _lib.lib().percnn_pi_halo_ring_bytes() == ctypes.sizeof(_lib.HaloRing)


def test_abi_version_is_the_headers():
    with open(os.path.join(INCLUDE, "percnn_pi.h")) as f:
        macro = int(re.search(r"^#define PERCNN_PI_ABI_VERSION (\d+)", f.read(), flags=re.M).group(1))
    assert _lib.ABI_VERSION == macro == _lib.lib().percnn_pi_abi_version()


def test_missing_headers_say_where_they_were_looked_for(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "CSRC", str(tmp_path / "a" / "b"))
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / "include"))):
        _lib._read_headers()
