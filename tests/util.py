"""Shared helpers for the test-suite (golden fixtures, error norms)."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fp32 tolerances (BASELINE.json: <= 1e-5 rel-L2 vs the reference path); fp64 runs are held to 1e-12.
TOL_TRAJ = {np.dtype("float32"): 1e-5, np.dtype("float64"): 1e-12}
TOL_GRAD = {np.dtype("float32"): 2e-5, np.dtype("float64"): 1e-10}


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def small_cases():
    fns = sorted(f for f in glob.glob(os.path.join(GOLDEN, "*.npz"))
                 if "_big_" not in f and "_biggrad_" not in f and "_longgrad" not in f and "harness" not in f and "stage3" not in f and "stage1" not in f
                 and "train_iter" not in f)
    assert fns, "golden fixtures missing"
    return fns


def case_id(fn):
    return os.path.basename(fn)[:-4]


def family(fn):
    return os.path.basename(fn).split("_")[0]


class Golden:
    def __init__(self, fn):
        self.fn = fn
        self.z = np.load(fn)
        self.family = family(fn)
        self.sd = {k[6:]: self.z[k] for k in self.z.files if k.startswith("param/")}
        self.h0 = self.z["h0"]                       # [1,2,*S]
        self.dtype = self.h0.dtype
        self.ndim = self.h0.ndim - 2
        self.hc = self.sd["Wh1_u.weight"].shape[0]
        self.steps = int(self.z["steps"])
        self.keep_t = [int(t) for t in self.z["keep_t"]]
        self.stride_t = int(self.z["stride_t"])
        self.dt = float(self.z["dt"])
        self.dx = float(self.z["dx"])
        self.mu_up = float(self.z["mu_up"])

    def traj(self, t):
        return self.z[f"traj/{t}"]

    def grads(self, loss):
        pre = f"grad_{loss}/"
        return {k[len(pre):]: self.z[k] for k in self.z.files if k.startswith(pre)}

    def oracle_cell(self):
        from oracle import restatement as R
        cell = {"gs2d": R.gs2d_cell, "gs3d": R.gs3d_cell, "lo2d": R.lo2d_cell}[self.family]()
        cell.load_state_dict({k: torch.tensor(v) for k, v in self.sd.items()})
        return cell

    def product_cell(self, device, reaction="poly"):
        import percnn_amd as pa
        cell = {"gs2d": pa.gs2d_cell, "gs3d": pa.gs3d_cell, "lo2d": pa.lo2d_cell}[self.family](reaction=reaction)
        cell.load_state_dict({k: torch.tensor(v) for k, v in self.sd.items()})
        return cell.to(device)

    def packed(self, reaction="factored"):
        """Parameter block for the plain-C oracle, coefficient computed as the reference does."""
        from oracle import pi_oracle as O
        cell = self.oracle_cell()
        cu, cv = [c.detach().numpy() for c in cell.coefficients()]
        if reaction == "poly":
            return O.pack_poly(self.sd, self.dt, cu, cv, self.dtype)
        return O.pack_params(self.sd, self.dt, cu, cv, self.dtype)

    def named_grads_from_packed(self, pg):
        """Packed gradient block -> reference parameter names (chain through sigmoid where needed)."""
        from oracle import pi_oracle as O
        G = O.unpack_grads(np.asarray(pg, dtype=np.float64), self.hc, self.ndim)
        out = {k: v for k, v in G.items() if not k.startswith("coef_")}
        if "CA" in self.sd:
            for n, c in (("CA", "coef_u"), ("CB", "coef_v")):
                s = 1.0 / (1.0 + np.exp(-self.sd[n].astype(np.float64)))
                out[n] = G[c] * self.mu_up * s * (1 - s)
        else:
            out["DA"], out["DB"] = G["coef_u"], G["coef_v"]
        return out


def data_loss(traj, stride_t, ndim):
    sl = (slice(0, -1, stride_t), slice(None)) + (slice(None, None, 4),) * ndim
    return ((traj[sl] - 0.5) ** 2).mean()


# ---- oracle dispatch on the block kind (36 entries = pre-contracted polynomial block, "hc = 0") ----
def hc_of(P):
    return 0 if len(P) == 36 else ((len(P) - 16) // 2 - 1) // 10


def o_step_fwd(h, P):
    from oracle import pi_oracle as O
    return O.poly_step_fwd(h, P) if len(P) == 36 else O.step_fwd(h, P, hc_of(P))


def o_step_bwd(h, G, inj, P):
    from oracle import pi_oracle as O
    return O.poly_step_bwd(h, G, inj, P) if len(P) == 36 else O.step_bwd(h, G, inj, P, hc_of(P))


def o_rollout_fwd(h0, P, T):
    from oracle import pi_oracle as O
    return O.poly_rollout_fwd(h0, P, T) if len(P) == 36 else O.rollout_fwd(h0, P, hc_of(P), T)


def o_rollout_bwd(traj, g, P):
    from oracle import pi_oracle as O
    return O.poly_rollout_bwd(traj, g, P) if len(P) == 36 else O.rollout_bwd(traj, g, P, hc_of(P))


def random_block(hc, ndim, dtype, seed, scale=0.5):
    """Random but well-conditioned parameter block (hc = 0: polynomial block of 36 entries)."""
    rs = np.random.RandomState(seed)
    n = 36 if hc == 0 else 16 + 2 * (10 * hc + 1)
    P = np.zeros(n, dtype=dtype)
    P[0] = 0.1
    P[1:3] = rs.uniform(0.01, 0.05, 2)
    P[3] = -2.0 * ndim * 1.25
    for a in range(ndim):
        P[4 + 4 * a:8 + 4 * a] = (-1 / 12, 4 / 3, 4 / 3, -1 / 12) + rs.uniform(-0.01, 0.01, 4)  # asymmetric on purpose
    P[16:] = rs.uniform(-scale, scale, n - 16)
    return P


# ---- batched / ensemble rollouts: the C-ABI through ctypes, and the plain-C oracle looped over the samples ----
def bits_equal(a, b):
    """bit-identical torch tensors (NaN payloads included)"""
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _suf(dt):
    return "f32" if dt == torch.float32 else "f64"


def _abi_stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _opt(options):
    from percnn_amd import _lib
    return _lib.options_arg(options)


def _rollout_bwd_abi(kind, traj, g, P, hc, shape, B, T, mask, options, g_h0):
    from percnn_amd import _lib
    L = _lib.lib()
    shape = tuple(int(s) for s in shape)
    if B is None:
        nbytes = L.percnn_pi_rollout_bwd_workspace_bytes(hc, len(shape), _lib.shape_arg(shape), T, traj.element_size())
    else:
        nbytes = getattr(L, f"percnn_pi_{kind}_rollout_bwd_workspace_bytes")(hc, len(shape), _lib.shape_arg(shape), B, T,
                                                                            traj.element_size())
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=traj.device)
    if g_h0 is None:
        g_h0 = torch.empty(((2,) if B is None else (B, 2)) + shape, dtype=traj.dtype, device=traj.device)
    pg = torch.zeros(tuple(P.shape), dtype=torch.float64, device=traj.device)
    if mask is not None and not isinstance(mask, bytes):
        mask = bytes(bytearray(1 if m else 0 for m in mask))
    if B is None:
        f = getattr(L, "percnn_pi_rollout_bwd_opt_" + _suf(traj.dtype))
        rc = f(traj.data_ptr(), g.data_ptr(), mask, g_h0.data_ptr(), pg.data_ptr(), ws.data_ptr(), ws.numel(), P.data_ptr(), hc,
               len(shape), _lib.shape_arg(shape), T, _opt(options), _abi_stream())
    else:
        f = getattr(L, f"percnn_pi_{kind}_rollout_bwd_" + _suf(traj.dtype))
        rc = f(traj.data_ptr(), g.data_ptr(), mask, g_h0.data_ptr(), pg.data_ptr(), ws.data_ptr(), ws.numel(), P.data_ptr(), hc,
               len(shape), _lib.shape_arg(shape), B, T, _opt(options), _abi_stream())
    assert rc == 0, f"percnn_pi_{kind}_rollout_bwd returned {rc}"
    torch.cuda.synchronize()
    return g_h0, pg


def batch_rollout_bwd(traj, g, P, hc, shape, B, T, mask=None, options=None, g_h0=None):
    """percnn_pi_batch_rollout_bwd_*: traj / g [T+1,B,2,*S], ONE block P -> (dL/dh0 [B,2,*S], dL/dP double[np]);
    B = None: the unbatched percnn_pi_rollout_bwd_opt_* on [T+1,2,*S]"""
    return _rollout_bwd_abi("batch", traj, g, P, hc, shape, B, T, mask, options, g_h0)


def ensemble_rollout_bwd(traj, g, P, hc, shape, B, T, mask=None, options=None, g_h0=None):
    """percnn_pi_ensemble_rollout_bwd_*: P [B,np] -> (dL/dh0 [B,2,*S], dL/dP double[B,np]); B = None: as batch_rollout_bwd"""
    return _rollout_bwd_abi("ensemble", traj, g, P, hc, shape, B, T, mask, options, g_h0)


def single_rollout_bwd(traj, g, P, hc, shape, T, mask=None, options=None):
    """percnn_pi_rollout_bwd_opt_* on one sample: traj / g [T+1,2,*S] -> (dL/dh0 [2,*S], dL/dP double[np])"""
    return _rollout_bwd_abi("single", traj, g, P, hc, shape, None, T, mask, options, None)


def _rollout_fwd_abi(kind, traj, P, hc, shape, B, T, options):
    """in place on traj [T+1,B,2,*S] (frame 0 = the initial states); takes any base pointer, which the operators do not"""
    from percnn_amd import _lib
    L = _lib.lib()
    f = getattr(L, f"percnn_pi_{kind}_rollout_fwd_" + _suf(traj.dtype))
    rc = f(traj.data_ptr(), P.data_ptr(), hc, len(shape), _lib.shape_arg(shape), B, T, _opt(options), _abi_stream())
    assert rc == 0, f"percnn_pi_{kind}_rollout_fwd returned {rc}"
    torch.cuda.synchronize()
    return traj


def batch_rollout_fwd_(traj, P, hc, shape, B, T, options=None):
    return _rollout_fwd_abi("batch", traj, P, hc, shape, B, T, options)


def ensemble_rollout_fwd_(traj, P, hc, shape, B, T, options=None):
    return _rollout_fwd_abi("ensemble", traj, P, hc, shape, B, T, options)


def _step_bwd_abi(kind, h, g_out, g_inject, P, hc, shape, B, options):
    from percnn_amd import _lib
    L = _lib.lib()
    shape = tuple(int(s) for s in shape)
    nbytes = getattr(L, f"percnn_pi_{kind}_bwd_workspace_bytes")(hc, len(shape), _lib.shape_arg(shape), B, h.element_size())
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=h.device)
    g_in = torch.empty_like(h)
    pg = torch.zeros(tuple(P.shape), dtype=torch.float64, device=h.device)
    f = getattr(L, f"percnn_pi_{kind}_step_bwd_" + _suf(h.dtype))
    rc = f(h.data_ptr(), g_out.data_ptr(), None if g_inject is None else g_inject.data_ptr(), g_in.data_ptr(), pg.data_ptr(),
           ws.data_ptr(), ws.numel(), P.data_ptr(), hc, len(shape), _lib.shape_arg(shape), B, _opt(options), _abi_stream())
    assert rc == 0, f"percnn_pi_{kind}_step_bwd returned {rc}"
    torch.cuda.synchronize()
    return g_in, pg


def batch_step_bwd(h, g_out, P, hc, shape, B, g_inject=None, options=None):
    """percnn_pi_batch_step_bwd_*: h / g_out / g_inject [B,2,*S], ONE block -> (dL/dh [B,2,*S], dL/dP double[np])"""
    return _step_bwd_abi("batch", h, g_out, g_inject, P, hc, shape, B, options)


def ensemble_step_bwd(h, g_out, P, hc, shape, B, g_inject=None, options=None):
    """percnn_pi_ensemble_step_bwd_*: P [B,np] -> (dL/dh [B,2,*S], dL/dP double[B,np])"""
    return _step_bwd_abi("ensemble", h, g_out, g_inject, P, hc, shape, B, options)


def ensemble_blocks(hc, ndim, dtype, B, seed, scale=0.1):
    """B distinct blocks: a seed of their own, and one of eight values of dt"""
    Ps = []
    for b in range(B):
        P = random_block(hc, ndim, dtype, seed + 17 * b + 1, scale=scale)
        P[0] = 0.1 * (1.0 + 0.125 * (b % 8))
        Ps.append(P)
    return np.stack(Ps)


def o_batch_reference(h0, P, T, g=None, mask=None):
    """The plain-C oracle looped over the samples.  h0 [B,2,*S]; P one block [np] (every sample) or [B,np]; g [T+1,B,2,*S]
    (frames a mask switches off count as zero, whatever they hold).
    -> (traj [T+1,B,2,*S], dL/dh0 [B,2,*S], per-sample gradient rows float64 [B,np]); the last two None without g.
    The shared-block path's gradient is rows.sum(0) in float64."""
    B = h0.shape[0]
    Pb = [P if P.ndim == 1 else P[b] for b in range(B)]
    traj = np.stack([o_rollout_fwd(np.ascontiguousarray(h0[b]), Pb[b], T) for b in range(B)], axis=1)
    if g is None:
        return traj, None, None
    g = np.array(g, copy=True)
    if mask is not None:
        g[[not m for m in mask]] = 0
    g0, rows = [], []
    for b in range(B):
        a, r = o_rollout_bwd(np.ascontiguousarray(traj[:, b]), np.ascontiguousarray(g[:, b]), Pb[b])
        g0.append(a)
        rows.append(np.asarray(r, dtype=np.float64))
    return traj, np.stack(g0), np.stack(rows)


def grad_err(got, want):
    """relative L2 of a parameter gradient against the oracle's (the measure of test_fuzz_gpu.py)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


# ---- cases of test_batch_fuzz_gpu.py / test_batch_dispatch_gpu.py (read without a GPU by test_batched_cpu.py) ----
# A case is a dict: id, shape, hc, dtype, B, T, mask (kind), options (dict or None), seed.
MASK_KINDS = ("none", "random", "top", "only0", "empty")
# bounds of test_fuzz_gpu.py for the same comparison (kernel reductions against the oracle's), relative L2
GRAD_TOL = {np.dtype("float32"): 1e-4, np.dtype("float64"): 1e-10}


def make_case(cid, shape, hc, dtype, B, T, mask="none", options=None, seed=None):
    return {"id": cid, "shape": tuple(int(s) for s in shape), "hc": int(hc), "dtype": np.dtype(dtype), "B": int(B), "T": int(T),
            "mask": mask, "options": dict(options) if options else None, "seed": int(cid if seed is None else seed)}


def batch_case_id(c):
    o = "" if not c["options"] else "-" + ",".join(f"{k}={v}" for k, v in c["options"].items())
    return (f"{c['id']}-{'x'.join(map(str, c['shape']))}-hc{c['hc']}-{c['dtype'].name}-B{c['B']}-T{c['T']}"
            f"{'' if c['mask'] == 'none' else '-' + c['mask']}{o}")


def make_mask(kind, T, rs):
    """-> list of T + 1 bools, or None (dense)"""
    if kind == "none":
        return None
    if kind == "random":
        return [bool(m) for m in rs.rand(T + 1) < 0.5]
    if kind == "top":                                   # the top frame carries no gradient: t_top < T (t_top = 0 when T = 1)
        m = [bool(x) for x in rs.rand(T + 1) < 0.6]
        m[T] = False
        if T >= 2:
            m[T - 1 - int(rs.randint(0, (T + 1) // 2))] = True
        return m
    if kind == "only0":
        return [t == 0 for t in range(T + 1)]
    if kind == "mod3":                                  # the mask of test_tile_variants_bitwise
        return [t % 3 == 0 for t in range(T + 1)]
    assert kind == "empty", kind
    return [False] * (T + 1)


def make_inputs(c):
    """Host arrays of a case, a function of the case alone: h0 [B,2,*S], the shared block P, the per-sample blocks Pe [B,np]
    (a seed and a dt of their own), dL/dtraj g [T+1,B,2,*S] and the mask."""
    rs = np.random.RandomState(1000 + c["seed"])
    shape, hc, dtype, B, T = c["shape"], c["hc"], c["dtype"].type, c["B"], c["T"]
    P = random_block(hc, len(shape), dtype, 50 + c["seed"], scale=0.3 if hc <= 8 else 0.15)
    Pe = ensemble_blocks(hc, len(shape), dtype, B, 50 + c["seed"])
    h0 = rs.uniform(0.1, 0.9, (B, 2) + shape).astype(dtype)
    g = rs.standard_normal((T + 1, B, 2) + shape).astype(dtype)
    return {"h0": h0, "P": P, "Pe": Pe, "g": g, "mask": make_mask(c["mask"], T, rs)}


def block_of(inp, path):
    return inp["P"] if path == "batch" else inp["Pe"]


def oracle(c, inp, path):
    """(traj, dL/dh0, gradient rows [B,np] float64) of one path"""
    return o_batch_reference(inp["h0"], block_of(inp, path), c["T"], inp["g"], inp["mask"])


def check_case(c, dev, refs=None, inp=None, tag=""):
    """Run a case on the device through the operators (forward) and the C-ABI (backward), both paths, and hold every sample to
    the oracle: trajectory and dL/dh0 bit-identical, gradients within GRAD_TOL, masked-out dL/dtraj frames poisoned with NaN
    and never read, two identical calls bit-identical.  refs: {path: oracle(...)} computed by the caller (reuse)."""
    import torch
    import percnn_amd as pa
    inp = make_inputs(c) if inp is None else inp
    shape, hc, B, T, mask, opts = c["shape"], c["hc"], c["B"], c["T"], inp["mask"], c["options"]
    h0 = torch.from_numpy(inp["h0"]).to(dev)
    gd = torch.from_numpy(inp["g"]).to(dev)
    if mask is not None and not all(mask):
        gd[[not m for m in mask]] = float("nan")        # masked-out frames must not be read
    tol = GRAD_TOL[c["dtype"]]
    for path in ("batch", "ensemble"):
        traj_o, g0_o, rows_o = refs[path] if refs else oracle(c, inp, path)
        assert np.isfinite(traj_o).all() and np.isfinite(g0_o).all() and np.isfinite(rows_o).all(), "ill-conditioned input"
        Pd = torch.from_numpy(block_of(inp, path)).to(dev)
        fwd = pa.pi_rollout_batched if path == "batch" else pa.pi_rollout_ensemble
        bwd = batch_rollout_bwd if path == "batch" else ensemble_rollout_bwd
        traj = fwd(h0, Pd, T, opts).contiguous()
        got = traj.cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[:, b], traj_o[:, b]), f"{tag}{path}: trajectory of sample {b}"
        assert torch.equal(fwd(h0, Pd, T, opts), traj), f"{tag}{path}: forward run to run"
        g0, pg = bwd(traj, gd, Pd, hc, shape, B, T, mask, opts)
        g0n, pgn = g0.cpu().numpy(), pg.cpu().numpy()
        assert np.isfinite(g0n).all() and np.isfinite(pgn).all(), f"{tag}{path}: a masked-out frame was read"
        for b in range(B):
            assert np.array_equal(g0n[b], g0_o[b]), f"{tag}{path}: dL/dh0 of sample {b}"
        if opts and opts.get("skip_wgrad"):
            pass                                        # state and adjoint only; the caller compares param_grad
        elif path == "batch":
            err = grad_err(pgn, rows_o.sum(0))
            print(f"{tag}batch gradient rel-L2 {err:.3g}")
            assert err < tol, f"{tag}batch: parameter gradient {err:.3g}"
        else:
            for b in range(B):
                err = grad_err(pgn[b], rows_o[b])
                print(f"{tag}ensemble row {b} rel-L2 {err:.3g}")
                assert err < tol, f"{tag}ensemble: gradient row {b} {err:.3g}"
        g0b, pgb = bwd(traj, gd, Pd, hc, shape, B, T, mask, opts)
        assert torch.equal(g0, g0b) and torch.equal(pg, pgb), f"{tag}{path}: backward run to run"
