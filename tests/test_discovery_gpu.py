"""GPU: Stage-2 library moments (csrc/pi_disc.h) against a float64 numpy restatement with the hash row classes, and
``discover`` end to end on the reference's fixture and on a Stage-3 Burgers rollout."""
import numpy as np
import pytest
import torch

from stage2_util import explicit_moments, fixture

pytestmark = pytest.mark.gpu

SHAPES = [(5, 5), (6, 7), (13, 33), (32, 32), (20, 70)]           # (5, 5): one interior point per frame
FRAMES = [3, 4, 9]
SPLITS = [None, (3, 1.0, 0.8), (11, 0.2, 0.8)]
DX, DT = 1.0 / 100, 2.5e-4
TERMS = {"u": ["ones*lap_u", "u*u_x", "v*u_y"], "v": ["ones*lap_v", "u*v_x", "v*v_y"]}


def _check(got, ref, what):
    """DESIGN section 3's float64 reduction bar: |G_ij - ref| <= 1e-10 sqrt(G_ii G_jj); b and yy with yy in place of a diagonal"""
    G, b, yy, n = (t.cpu().numpy() for t in got)
    Gr, br, yr, nr = ref
    assert np.array_equal(n, nr), (what, n, nr)
    for c in (0, 1):
        dg, dy = np.sqrt(np.diag(Gr[c])), np.sqrt(yr[c])
        eg = np.abs(G[c] - Gr[c]) - 1e-10 * dg[:, None] * dg[None, :]
        assert (eg <= 0).all(), (what, c, "G", float(eg.max()))
        eb = np.abs(b[c] - br[c]) - 1e-10 * dg[:, None] * dy[None, :]
        assert (eb <= 0).all(), (what, c, "b", float(eb.max()))
        assert (np.abs(yy[c] - yr[c]) <= 1e-10 * yr[c]).all(), (what, c, "yy")
        assert np.array_equal(G[c], G[c].T), (what, c, "G is not bitwise symmetric")


@pytest.mark.parametrize("N", FRAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_match_float64_restatement(shape, N):
    """every (dtype, region, split, batch) of one grid and frame count; row counts include non-multiples of 4 and of 64"""
    import percnn_amd as pa
    from percnn_amd.discovery import split_thresholds
    H, W = shape
    rng = np.random.default_rng(1000 * H + 10 * W + N)
    for dtype in (torch.float32, torch.float64):
        host = torch.from_numpy(0.5 * rng.standard_normal((N, 4, 2, H, W))).to(dtype)
        dev = host.cuda()
        for region in ("interior", "periodic"):
            for split in SPLITS:
                seed, t_train, t_keep = split_thresholds(split)
                refs = [explicit_moments(host[:, 1 + s].numpy(), DX, DT, region, seed, t_train, t_keep) for s in range(3)]
                for B in (1, 3):
                    view = dev[:, 1:1 + B]                                         # [N, B, 2, H, W], not contiguous
                    what = (shape, N, str(dtype), region, split, B)
                    got = pa.library_moments(view, DX, DT, region=region, split=split)
                    assert got.G.shape == (B, 2, 70, 70) and got.b.shape == (B, 2, 70, 2)
                    assert got.yy.shape == (B, 2, 2) and got.n.shape == (B, 2)
                    again = pa.library_moments(view, DX, DT, region=region, split=split)
                    for a, b_ in zip(got, again):
                        assert torch.equal(a, b_), (what, "a repeated call differs")
                    for s in range(B):
                        _check([t[s] for t in got], refs[s], what + (s,))
                        single = pa.library_moments(dev[:, 1 + s], DX, DT, region=region, split=split)
                        assert single.G.shape == (2, 70, 70) and single.n.shape == (2,)
                        for a, b_ in zip(got, single):
                            assert torch.equal(a[s], b_), (what, s, "batched sample differs from the unbatched call")


def test_discover_on_the_reference_fixture():
    """the six reference terms and no others; coefficients within 2e-3 relative of the reference's own w_best
    (measured without a device, test_discovery_cpu.py: u 3.4e-4, v 6.8e-4)"""
    import percnn_amd as pa
    fx = fixture()
    names = [str(s) for s in fx["names"]]
    eqs = pa.discover(torch.from_numpy(fx["traj"]).cuda(), float(fx["dx"]), float(fx["dt"]))
    for sp in ("u", "v"):
        assert list(eqs[sp]) == TERMS[sp], eqs[sp]
        ref = fx["w_best_" + sp]
        for t, c in eqs[sp].items():
            r = ref[names.index(t)]
            print(sp, t, c, r, abs(c - r) / abs(r))
            assert abs(c - r) <= 2e-3 * abs(r), (sp, t, c, r)


def test_discover_recovers_the_stage3_burgers_cell():
    """40 explicit Euler steps of the Stage-3 cell use the library's own stencils, so the library fits the trajectory exactly up
    to conditioning: six terms, coefficients within 1e-4 relative of the cell's parameters"""
    import percnn_amd as pa
    cell = pa.Stage3BurgersCell().cuda()
    ys = torch.arange(32, dtype=torch.float64) / 32
    yy, xx = torch.meshgrid(ys, ys, indexing="ij")
    tp = 2 * np.pi
    u = torch.sin(tp * xx) * torch.cos(tp * yy) + 0.3 * torch.cos(2 * tp * xx + 0.5)
    v = torch.cos(tp * xx) * torch.sin(tp * yy) - 0.2 * torch.sin(tp * (xx + 2 * yy))
    with torch.no_grad():
        outs, _ = pa.RCNN(cell, step=40, effective_step=list(range(40)), init_state=torch.stack((u, v))[None].cuda())()
        traj = torch.cat(tuple(outs), 0)
    assert traj.shape == (41, 2, 32, 32) and traj.dtype == torch.float64 and traj.is_cuda
    eqs = pa.discover(traj, cell.dx, cell.dt, region="periodic")
    want = {sp: [float(getattr(cell, k + sp).detach()) for k in ("nu_", "C1_", "C2_")] for sp in ("u", "v")}
    for sp in ("u", "v"):
        assert list(eqs[sp]) == TERMS[sp], eqs[sp]
        for (t, c), r in zip(eqs[sp].items(), want[sp]):
            print(sp, t, c, r, abs(c - r) / abs(r))
            assert abs(c - r) <= 1e-4 * abs(r), (sp, t, c, r)


def test_refused_inputs_name_the_argument():
    import percnn_amd as pa
    ok = torch.zeros(4, 2, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="traj.*device"):
        pa.library_moments(ok.cpu(), DX, DT)
    with pytest.raises(ValueError, match="N >= 3"):
        pa.library_moments(ok[:2], DX, DT)
    with pytest.raises(ValueError, match="H, W >= 5"):
        pa.library_moments(torch.zeros(4, 2, 4, 8, device="cuda"), DX, DT)
    with pytest.raises(ValueError, match="2 channels"):
        pa.library_moments(torch.zeros(4, 3, 8, 8, device="cuda"), DX, DT)
    with pytest.raises(ValueError, match="region"):
        pa.library_moments(ok, DX, DT, region="padded")
    with pytest.raises(ValueError, match="stride-1"):
        pa.library_moments(torch.zeros(4, 2, 8, 16, device="cuda")[..., ::2], DX, DT)
    with pytest.raises(RuntimeError, match="invalid argument"):
        pa.library_moments(ok, 0.0, DT)
