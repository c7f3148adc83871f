"""CPU: Stage-2 equation discovery -- library names, the row-class hash, STRidge on moments against STRidge on the explicit
matrix and against the reference's own result (tests/golden/stage2/stage2_burgers_32x32.npz, tools/make_golden_stage2.py), and the
C-ABI surface of the library moments (validation only, nothing is launched)."""
import ctypes
import math

import numpy as np
import pytest

from stage2_util import explicit_library, explicit_moments, explicit_stridge, explicit_train, fixture

SYMBOLS = ["percnn_pi_library_moments_workspace_bytes", "percnn_pi_library_moments_f32", "percnn_pi_library_moments_f64"]
TERMS = {"u": ["ones*lap_u", "u*u_x", "v*u_y"], "v": ["ones*lap_v", "u*v_x", "v*v_y"]}


def test_library_terms_are_the_reference_names():
    import percnn_amd
    assert percnn_amd.LIBRARY_TERMS == [str(s) for s in fixture()["names"]]
    assert len(percnn_amd.LIBRARY_TERMS) == 70


def test_row_class_reproduces_hand_computed_hashes():
    """mix32 of r + seed, worked out with plain integers: (r, seed) -> hash"""
    from percnn_amd import row_class
    known = [(0, 0, 0x00000000), (1, 0, 0x688990c0), (2, 0, 0xd1132181), (12345, 0, 0x912efcf7), (0xffffffff, 0, 0x6768824a),
             (0xffffffff, 1, 0x00000000), (7, 0xdeadbeef, 0xf27fcba3), (1000000, 42, 0x55e50e3d)]
    for r, seed, h in known:
        # the class changes exactly where a threshold passes the hash
        assert row_class(r, seed, h + 1, h + 1) == 0, (r, seed)
        assert row_class(r, seed, h, h + 1) == 1, (r, seed)
        assert row_class(r, seed, h, h) == 2, (r, seed)
    assert row_class(np.array([0, 1, 2, 12345]), 0, 1 << 32, 1 << 32).tolist() == [0, 0, 0, 0]           # no split
    assert row_class(np.array([1, 2, 12345]), 0, 0x688990c1, 0x912efcf8).tolist() == [0, 2, 1]
    # the reference's setting keeps about 20 % of the rows and trains on about 80 % of those
    c = row_class(np.arange(200000), 0, int(0.16 * 2 ** 32), int(0.2 * 2 ** 32))
    assert abs((c == 0).mean() - 0.16) < 0.004 and abs((c == 1).mean() - 0.04) < 0.002


@pytest.fixture(scope="module")
def problem():
    """the fixture trajectory's explicit library with the hash split of the reference's setting, and its moments"""
    from percnn_amd.discovery import REFERENCE_SPLIT, row_class, split_thresholds
    fx = fixture()
    seed, t_train, t_keep = split_thresholds(REFERENCE_SPLIT)
    assert (t_train, t_keep) == (int(round(0.16 * 2 ** 32)), int(round(0.2 * 2 ** 32)))
    theta, y, r = explicit_library(fx["traj"], float(fx["dx"]), float(fx["dt"]), "interior")
    cls = row_class(r, seed, t_train, t_keep)
    mom = explicit_moments(fx["traj"], float(fx["dx"]), float(fx["dt"]), "interior", seed, t_train, t_keep)
    return fx, theta, y, cls, mom


def test_explicit_library_is_the_reference_library(problem):
    """the float64 restatement against the reference's float32 convolutions (accumulated in float64): float32 rounding of
    the derivative columns, 6e-8 relative per entry, a few times that on the sums"""
    fx, theta, y, cls, mom = problem
    assert theta.shape[0] == int(fx["rows"]) == 19 * 28 * 28
    G, b = theta.T @ theta, theta.T @ y
    dg, dy = np.sqrt(np.diag(fx["G_ref"])), np.sqrt(fx["yy_ref"])
    assert (np.abs(G - fx["G_ref"]) <= 1e-5 * dg[:, None] * dg[None, :]).all()
    assert (np.abs(b - fx["b_ref"]) <= 1e-5 * dg[:, None] * dy[None, :]).all()


@pytest.mark.parametrize("species", ["u", "v"])
def test_stridge_on_moments_equals_stridge_on_the_matrix(problem, species):
    from percnn_amd import stridge
    fx, theta, y, cls, mom = problem
    s = "uv".index(species)
    scale = 1.0 / np.linalg.norm(theta[cls < 2], axis=0)
    X, Y = (theta * scale)[cls == 0], y[cls == 0, s]
    for tol in (0.5, 20.0, 60.0):
        for must_have in (5, 6):
            want = explicit_stridge(X, Y, 0.01, 40, tol, must_have)
            got = stridge(X.T @ X, X.T @ Y, 0.01, 40, tol, must_have)
            assert (got != 0).tolist() == (want != 0).tolist(), (tol, must_have)
            nz = want != 0
            assert (np.abs(got[nz] - want[nz]) <= 1e-8 * np.abs(want[nz])).all(), (tol, must_have)


@pytest.mark.parametrize("species", ["u", "v"])
def test_train_stridge_equals_the_matrix_version_and_the_reference(problem, species):
    """Against the reference's w_best the measured relative differences on this fixture are written below; the bound is 2e-3
    (the reference draws another random subsample / split and keeps a float32 copy of the normalised matrix).
    Measured here: u 3.4e-4, v 6.8e-4."""
    from percnn_amd import LIBRARY_TERMS, train_stridge
    from percnn_amd.discovery import DEFAULTS
    fx, theta, y, cls, mom = problem
    s = "uv".index(species)
    got = train_stridge(mom, species, **DEFAULTS[species])
    want = explicit_train(theta, y[:, s], cls, **DEFAULTS[species])
    names = [t for t, c in zip(LIBRARY_TERMS, got) if c != 0]
    assert names == TERMS[species]
    assert (got != 0).tolist() == (want != 0).tolist()
    nz = want != 0
    rel = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
    print(f"{species}: moments vs explicit matrix, relative {rel.max():.2e}")
    assert rel.max() <= 1e-8
    ref = fx["w_best_" + species]
    assert (got != 0).tolist() == (ref != 0).tolist()
    rel = np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])
    print(f"{species}: moments vs the reference's w_best, relative {rel.max():.2e}: {dict(zip(names, got[nz]))}")
    assert rel.max() <= 2e-3


def test_train_stridge_refuses_what_it_cannot_score(problem):
    from percnn_amd import train_stridge
    from percnn_amd.discovery import DEFAULTS
    fx, theta, y, cls, (G, b, yy, n) = problem
    with pytest.raises(ValueError, match="split"):
        train_stridge((G, b, yy, np.array([n[0], 0.0])), "u", **DEFAULTS["u"])
    with pytest.raises(ValueError, match="species"):
        train_stridge((G, b, yy, n), "w", **DEFAULTS["u"])
    with pytest.raises(ValueError, match="normalize"):
        train_stridge((G, b, yy, n), "u", normalize=0, **DEFAULTS["u"])


def test_discovery_symbols_are_declared_exported_and_bound():
    import os
    import percnn_amd
    from percnn_amd import _lib
    L = percnn_amd.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "percnn_pi_discovery.h")).read()
    for name in SYMBOLS:
        assert name + "(" in hdr
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert "pi_disc_abi.hip" in _lib.SOURCES and _lib.ABI_VERSION == 3
    for name in ("LIBRARY_TERMS", "row_class", "library_moments", "stridge", "train_stridge", "discover", "LibraryMoments"):
        assert getattr(percnn_amd, name) is getattr(percnn_amd.discovery, name)


def test_library_moments_argument_errors_do_not_need_a_gpu():
    """Validation before any launch (fake pointers): everything on the list of include/percnn_pi_discovery.h -> -1, a short
    workspace -> -2."""
    import percnn_amd
    L = percnn_amd.lib()
    two32 = 1 << 32
    shape = (ctypes.c_int64 * 2)(8, 8)
    wsb = L.percnn_pi_library_moments_workspace_bytes
    assert wsb(shape, 5, 1) > 0 and wsb(shape, 5, 3) >= wsb(shape, 5, 1)
    assert wsb(shape, 2, 1) == 0 and wsb(shape, 5, 0) == 0 and wsb(shape, 5, 65536) == 0 and wsb(None, 5, 1) == 0
    assert wsb((ctypes.c_int64 * 2)(4, 8), 5, 1) == 0 and wsb((ctypes.c_int64 * 2)(8, 4), 5, 1) == 0
    assert wsb((ctypes.c_int64 * 2)(1 << 15, 1 << 15), 4, 1) > 0 and wsb((ctypes.c_int64 * 2)(1 << 15, 1 << 15), 5, 1) == 0
    T, G, B, YY, N, WS = 1 << 20, 1 << 30, (1 << 30) + (1 << 20), (1 << 30) + (2 << 20), (1 << 30) + (3 << 20), 1 << 31
    big = 1 << 30
    for suf in ("f32", "f64"):
        f = getattr(L, f"percnn_pi_library_moments_{suf}")

        def call(traj=T, fs=128, ss=0, shape=shape, nframes=5, batch=1, dx=0.01, dt=2.5e-4, region=0, seed=0, t_train=two32,
                 t_keep=two32, G=G, b=B, yy=YY, n=N, ws=WS, ws_bytes=big):
            return f(traj, fs, ss, shape, nframes, batch, dx, dt, region, seed, t_train, t_keep, G, b, yy, n, ws, ws_bytes, None)

        # NULL pointers
        for kw in ({"traj": None}, {"G": None}, {"b": None}, {"yy": None}, {"n": None}, {"shape": None}):
            assert call(**kw) == -1, kw
        assert call(nframes=2) == -1 and call(nframes=0) == -1 and call(nframes=-1) == -1
        assert call(shape=(ctypes.c_int64 * 2)(4, 8)) == -1 and call(shape=(ctypes.c_int64 * 2)(8, 4)) == -1
        for batch in (0, -3, 65536, 70000):
            assert call(batch=batch) == -1, batch
        assert call(shape=(ctypes.c_int64 * 2)(1 << 15, 1 << 15), nframes=5, fs=1 << 31) == -1      # nframes*H*W > 2^32
        assert call(t_train=two32, t_keep=two32 - 1) == -1 and call(t_train=0, t_keep=two32 + 1) == -1
        for bad in (0.0, -0.01, math.inf, math.nan):
            assert call(dx=bad) == -1 and call(dt=bad) == -1, bad
        assert call(region=2) == -1 and call(region=-1) == -1
        assert call(fs=-128) == -1 and call(ss=-1, batch=2) == -1
        # outputs / workspace inside the trajectory: frames 0..4 of 128 elements each from T
        esz = 4 if suf == "f32" else 8
        inside = T + 4 * 128 * esz
        for kw in ({"G": inside}, {"b": inside}, {"yy": inside}, {"n": inside}, {"ws": inside}, {"G": T - 8}):
            assert call(**kw) == -1, kw
        # a short workspace
        need = wsb(shape, 5, 1)
        assert call(ws_bytes=need - 1) == -2 and call(ws=None) == -2 and call(ws_bytes=0) == -2
        assert call(batch=3, ss=1 << 16, ws_bytes=wsb(shape, 5, 3) - 1) == -2
