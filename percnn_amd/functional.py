"""torch.autograd front-end of the HIP Pi-block kernels.

``pi_step`` / ``pi_rollout`` are what the drop-in modules (``percnn_amd.modules``) call in place
of the reference's per-step ATen sequence (``RCNNCell.forward`` -- DataDrivenModeling/2d_gs_rd/
train_2drd.py:105-121, 3d_gs_rd/train_3drd.py:123-139, ForwardSimulationOfPDEs/2d_lambda_omega/
percnn_LO_eqn.py:98-112) and its T-step loop (``RCNN.forward`` -- train_2drd.py:162-190).

Everything here is plumbing: tensors supply device memory and the current HIP stream; the math
runs in ``libpercnn_pi.so`` through the C-ABI of ``include/percnn_pi.h``.  CPU tensors are
rejected -- there is no fallback path.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib

_SUF = {torch.float32: "f32", torch.float64: "f64"}
_OFFS = (-2, -1, 1, 2)


def param_count(hc: int) -> int:
    return 16 + 2 * (10 * hc + 1)


# ------------------------------------------------------------------------------------------------
# parameter block (layout documented in include/percnn_pi.h)
# ------------------------------------------------------------------------------------------------
_index_cache: dict = {}


def _gather_index(hc: int, ndim: int, device) -> torch.Tensor:
    """Index into the flat concatenation [dt, coef_u, coef_v, W_laplace.weight(5^ndim),
    {Wh1.w, Wh1.b, Wh2.w, Wh2.b, Wh3.w, Wh3.b, Wh4.w, Wh4.b} for u then v] that yields the block."""
    key = (hc, ndim, str(device))
    if key in _index_cache:
        return _index_cache[key]
    nst = 5 ** ndim
    idx = [0] * param_count(hc)
    idx[0], idx[1], idx[2] = 0, 1, 2

    def lin(pos):
        r = 0
        for p in pos:
            r = r * 5 + p
        return 3 + r

    centre = [2] * ndim
    idx[3] = lin(centre)
    for a in range(3):
        for i, off in enumerate(_OFFS):
            if a < ndim:
                pos = list(centre)
                pos[a] += off
                idx[4 + 4 * a + i] = lin(pos)
            else:
                idx[4 + 4 * a + i] = lin(centre)   # unused slots (2D): any finite value
    per_species = 3 * (2 * hc + hc) + hc + 1
    for s in range(2):
        src = 3 + nst + s * per_species
        dst = 16 + s * (10 * hc + 1)
        for k in range(3):
            wsrc = src + k * 3 * hc
            for j in range(hc):
                idx[dst + 10 * j + 3 * k + 0] = wsrc + 2 * j
                idx[dst + 10 * j + 3 * k + 1] = wsrc + 2 * j + 1
                idx[dst + 10 * j + 3 * k + 2] = wsrc + 2 * hc + j
        w4 = src + 9 * hc
        for j in range(hc):
            idx[dst + 10 * j + 9] = w4 + j
        idx[dst + 10 * hc] = w4 + hc
    t = torch.tensor(idx, dtype=torch.long, device=device)
    _index_cache[key] = t
    return t


def pack_params(dt: torch.Tensor, coef_u: torch.Tensor, coef_v: torch.Tensor, w_laplace: torch.Tensor,
                branch: Sequence[torch.Tensor]) -> torch.Tensor:
    """Differentiable (cat + index_select) assembly of the parameter block on the device.

    ``branch`` = [Wh1_u.w, Wh1_u.b, Wh2_u.w, Wh2_u.b, Wh3_u.w, Wh3_u.b, Wh4_u.w, Wh4_u.b, (same for v)].
    Gradients flow back to every input through stock autograd, so e.g. dL/dCA falls out of
    ``coef_u = mu_up * sigmoid(CA)`` (train_2drd.py:115) without any kernel support.
    """
    hc = branch[0].shape[0]
    ndim = w_laplace.dim() - 2
    flat = torch.cat([dt.reshape(1), coef_u.reshape(1), coef_v.reshape(1), w_laplace.reshape(-1)]
                     + [b.reshape(-1) for b in branch])
    return flat.index_select(0, _gather_index(hc, ndim, flat.device))


# ------------------------------------------------------------------------------------------------
# the same assembly (+ contraction) in ONE launch: percnn_pi_pack_fwd/bwd_* (csrc/pi_contract.h)
# ------------------------------------------------------------------------------------------------
def _param_ptrs(tensors: Sequence[Optional[torch.Tensor]]):
    """tensors = [c_u, c_v, W_laplace.weight, Wh1_u.w, Wh1_u.b, ..., Wh4_v.b] (19) -> percnn_pi_param_ptrs"""
    pp = _lib.ParamPtrs()
    ptr = [None if t is None else t.data_ptr() for t in tensors]
    pp.c[0], pp.c[1], pp.w = ptr[0], ptr[1], ptr[2]
    for i in range(16):
        pp.branch[i] = ptr[3 + i]
    return pp


def _check_pack_inputs(tensors):
    if len(tensors) != 19:
        raise ValueError("pack_block expects [c_u, c_v, W_laplace.weight, 16 branch tensors]")
    t0 = tensors[2]
    if not t0.is_cuda:
        raise RuntimeError("percnn_amd: pack_block has no CPU path (use functional.pack_params)")
    for t in tensors:
        if t.device != t0.device or t.dtype != t0.dtype or not t.is_contiguous():
            raise ValueError("pack_block: tensors must be contiguous and share device and dtype")


def pack_fwd_hip(tensors, hc: int, ndim: int, dt: float, mu_up: float, sigmoid: bool, contract: bool, guard=None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """guard = (host_slot_address, seq, u_max, v_max): the launch also leaves the conditioning number A of the pre-contracted
    form and `seq` in the host-mapped slot (include/percnn_pi.h, percnn_pi_pack_fwd_guard_*); out: write into this block."""
    _check_pack_inputs(tensors)
    w = tensors[2]
    n = NPOLY if contract else param_count(hc)
    if out is None:
        out = torch.empty(n, dtype=w.dtype, device=w.device)
    elif out.numel() != n or out.dtype != w.dtype or out.device != w.device or not out.is_contiguous():
        raise ValueError("pack_fwd_hip: `out` does not fit this block")
    with torch.cuda.device(w.device):
        if guard is None:
            f = getattr(_lib.lib(), "percnn_pi_pack_fwd_" + _SUF[w.dtype])
            _lib.check(f(ctypes.byref(_param_ptrs(tensors)), hc, ndim, float(dt), float(mu_up), int(sigmoid), int(contract),
                         out.data_ptr(), _stream()), "pack_fwd")
        else:
            slot, seq, u_max, v_max = guard
            f = getattr(_lib.lib(), "percnn_pi_pack_fwd_guard_" + _SUF[w.dtype])
            _lib.check(f(ctypes.byref(_param_ptrs(tensors)), hc, ndim, float(dt), float(mu_up), int(sigmoid), int(contract),
                         out.data_ptr(), float(u_max), float(v_max), ctypes.c_void_p(slot), float(seq), _stream()),
                       "pack_fwd_guard")
    return out


class PolyGuard:
    """Host side of the conditioning guard of reaction='poly' (VERDICT r3 #2a; the rule is RCNNCell's docstring): every pack
    launch leaves A = |dt| max_s sum_m |c_m^s| phi_m(bound) / max(bound) and its sequence number in two host-mapped doubles;
    ``decide()`` reads them WITHOUT synchronising -- the value of the most recent pack that has completed, normally the previous
    training iteration's -- and flips the cell between the pre-contracted and the factored block with hysteresis."""

    def __init__(self, device):
        self.device = torch.device(device)
        p = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().percnn_pi_host_words_alloc(ctypes.byref(p), 16), "host_words_alloc")
        self.address = p.value
        self._view = (ctypes.c_double * 2).from_address(self.address)
        self.issued = 0                  # sequence number of the last pack launched with this slot
        self.seen = 0                    # ... of the last one whose A has been read
        self.A = None
        self.factored = False
        import weakref
        weakref.finalize(self, _lib.lib().percnn_pi_host_words_free, ctypes.c_void_p(self.address))

    def __deepcopy__(self, memo):
        """copy.deepcopy(cell) / pickling a cell: the copy gets a host slot of its own (the slot is process-local pinned
        memory, not data) and starts from this guard's decision"""
        g = PolyGuard(self.device)
        g.factored = self.factored
        return g

    def __reduce__(self):
        return (PolyGuard, (self.device,))

    def next_seq(self) -> int:
        self.issued += 1
        return self.issued

    def read(self):
        """-> (A, seq) of the latest completed pack, or (None, 0)"""
        s0 = self._view[1]
        a = self._view[0]
        s1 = self._view[1]
        if s0 != s1:                     # a launch wrote between the two reads: the next call sees it
            return self.A, self.seen
        if s1 > 0:
            self.A, self.seen = float(a), int(s1)
        return self.A, self.seen

    def decide(self, a_max: float) -> bool:
        """True: pack the factored block.  Switch up above a_max, back below a_max / 2."""
        A, _ = self.read()
        if A is not None:
            if not self.factored and A > a_max:
                self.factored = True
            elif self.factored and A < 0.5 * a_max:
                self.factored = False
        return self.factored


def pack_bwd_hip(tensors, g_block: torch.Tensor, hc: int, ndim: int, dt: float, mu_up: float, sigmoid: bool,
                 contract: bool, one_buffer: bool = False):
    """-> gradients of the 18 trainable tensors, in the order of ``tensors`` without W_laplace.weight.
    one_buffer: the gradients are views of ONE allocation (eager autograd path; outputs of a registered operator must
    not share storage, so ``torch.ops.percnn.pack_block_backward`` allocates them one by one)"""
    _check_pack_inputs(tensors)
    w = tensors[2]
    g_block = g_block.contiguous()
    if one_buffer:                   # 18 allocator round trips are a third of the host time of this call otherwise
        train = [t for i, t in enumerate(tensors) if i != 2]
        flat = torch.empty(sum(t.numel() for t in train), dtype=w.dtype, device=w.device)
        grads, o = [], 0
        for t in train:
            grads.append(flat[o:o + t.numel()].view(t.shape))
            o += t.numel()
    else:
        grads = [torch.empty_like(t) for i, t in enumerate(tensors) if i != 2]
    gptr = grads[:2] + [None] + grads[2:]
    f = getattr(_lib.lib(), "percnn_pi_pack_bwd_" + _SUF[w.dtype])
    with torch.cuda.device(w.device):
        _lib.check(f(ctypes.byref(_param_ptrs(tensors)), ctypes.byref(_param_ptrs(gptr)), hc, ndim, float(dt), float(mu_up),
                     int(sigmoid), int(contract), g_block.data_ptr(), _stream()), "pack_bwd")
    return grads


class PackBlockFunction(torch.autograd.Function):
    """Eager-mode front of the two pack kernels: ``apply(meta, guard, *tensors)`` with meta = (hc, ndim, dt, mu_up, sigmoid,
    contract), guard = None or pack_fwd_hip's guard tuple.  A plain autograd.Function on purpose -- measured on the MI355X box's host (tools/pack_time.py), per call
    without / with backward: stock tensor ops 86 / 550 us, the registered operator (torch.ops.percnn.pack_block, what
    torch.compile traces) 38 / 480-840 us, this 21 / 320 us: with one small launch each way the dispatcher's Python
    layers are what is left to pay."""

    @staticmethod
    def forward(ctx, meta, guard, acc, *tensors):
        """acc: None, or the native GradSink (``BlockState.sink``) whose workspace rows the per-step nodes of a reference-style
        loop leave their parameter-gradient sums in (csrc/torch_ext.cpp: cell_step) -- this node delivers them, once per
        backward pass.  The sink, not the BlockState: the state holds this node's output."""
        ctx.meta = meta
        ctx.acc = acc
        ctx.set_materialize_grads(False)
        # NOT save_for_backward: the block is cached by RCNNCell.param_block and shared by every step of an iteration, so
        # several backward() calls may run through this node (`out1 = cell(h1); out2 = cell(h2); out1.sum().backward();
        # out2.sum().backward()`) -- saved tensors would be freed by the first.  The parameters are leaves that
        # outlive the node; the in-place check save_for_backward would have made is done by hand.
        ctx.tensors = tensors
        ctx.versions = tuple(t._version for t in tensors)
        return pack_fwd_hip(tensors, *meta, guard=guard)

    @staticmethod
    def backward(ctx, g):
        if tuple(t._version for t in ctx.tensors) != ctx.versions:
            raise RuntimeError("percnn_amd: a parameter of the packed block was modified in place between the forward and "
                               "this backward pass (same rule as autograd's saved tensors)")
        if ctx.acc is not None:
            extra = _lib.torch_ext().take_block_grad(ctx.acc, ctx.tensors[2])  # the step nodes' sums of THIS pass (or None)
            if extra is not None:
                extra = extra[:NPOLY if ctx.meta[5] else param_count(ctx.meta[0])]   # (the accumulator is sized for either block kind)
                g = extra if g is None else g + extra
        if g is None:
            return (None,) * (3 + len(ctx.tensors))
        gr = pack_bwd_hip(ctx.tensors, g, *ctx.meta, one_buffer=True)
        return (None, None, None, gr[0], gr[1], None, *gr[2:])


# ------------------------------------------------------------------------------------------------
# pre-contracted ("poly") reaction: Wh4(Wh1(h)*Wh2(h)*Wh3(h)) as a cubic in (u, v)
# ------------------------------------------------------------------------------------------------
NPOLY = 36
NADV = 60            # advective polynomial block of the Stage-3 physics-based cells (hc = -1)
_MONO = {(0, 0): 0, (1, 0): 1, (0, 1): 2, (2, 0): 3, (1, 1): 4, (0, 2): 5, (3, 0): 6, (2, 1): 7, (1, 2): 8, (0, 3): 9}
_k_cache: dict = {}


def _contraction_tensor(device) -> torch.Tensor:
    """K[m,a,b,c] = 1 iff e_a*e_b*e_c == phi_m with e = (u, v, 1) and
    phi = (1, u, v, u^2, uv, v^2, u^3, u^2 v, u v^2, v^3)."""
    key = str(device)
    if key not in _k_cache:
        ex = [(1, 0), (0, 1), (0, 0)]
        K = torch.zeros(10, 3, 3, 3, dtype=torch.float64)
        for a in range(3):
            for b in range(3):
                for c in range(3):
                    e = (ex[a][0] + ex[b][0] + ex[c][0], ex[a][1] + ex[b][1] + ex[c][1])
                    K[_MONO[e], a, b, c] = 1.0
        e0 = torch.zeros(10, dtype=torch.float64)
        e0[0] = 1.0
        _k_cache[key] = (K.to(device), e0.to(device))
    return _k_cache[key]


def contract_fwd_hip(P: torch.Tensor) -> torch.Tensor:
    """one launch (csrc/pi_contract.h): factored block on a HIP device -> 36-entry polynomial block"""
    _require(P, "params")
    Q = torch.empty(NPOLY, dtype=P.dtype, device=P.device)
    f = getattr(_lib.lib(), "percnn_pi_contract_fwd_" + _SUF[P.dtype])
    with torch.cuda.device(P.device):
        _lib.check(f(P.data_ptr(), _hc_of(P), Q.data_ptr(), _stream()), "contract_fwd")
    return Q


def contract_bwd_hip(P: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    _require(P, "params"); _require(g, "g_poly", P.dtype)
    gP = torch.empty_like(P)
    f = getattr(_lib.lib(), "percnn_pi_contract_bwd_" + _SUF[P.dtype])
    with torch.cuda.device(P.device):
        _lib.check(f(P.data_ptr(), _hc_of(P), g.data_ptr(), gP.data_ptr(), _stream()), "contract_bwd")
    return gP


class _ContractFunction(torch.autograd.Function):
    """contract_block on CPU tensors (host-side tools, tests) with a hand-written chain rule in plain torch ops; HIP
    tensors go through the registered operator ``torch.ops.percnn.contract_block`` instead (one launch each way)."""

    @staticmethod
    def _factors(P):
        hc = _hc_of(P)
        B = P[16:].to(torch.float64).reshape(2, 10 * hc + 1)
        Wm = B[:, :10 * hc].reshape(2, hc, 10)
        L1, L2, L3, w4 = Wm[..., 0:3], Wm[..., 3:6], Wm[..., 6:9], Wm[..., 9]
        T12 = L1.unsqueeze(-1) * L2.unsqueeze(-2)                          # [2, hc, 3, 3]
        T = T12.unsqueeze(-1) * L3[:, :, None, None, :]                   # [2, hc, 3, 3, 3]
        return hc, B, L1, L2, L3, w4, T12, T

    @staticmethod
    def forward(ctx, P):
        K, _e0 = _contraction_tensor(P.device)
        hc, B, L1, L2, L3, w4, T12, T = _ContractFunction._factors(P)
        S = (T * w4[:, :, None, None, None]).sum(1).reshape(2, 27)        # sum over the hidden channels
        c = S @ K.reshape(10, 27).t()                                      # [2, 10]
        c[:, 0] += B[:, 10 * hc]
        ctx.save_for_backward(P)
        return torch.cat([P[:16], c.to(P.dtype).reshape(20)])

    @staticmethod
    def backward(ctx, g):
        (P,) = ctx.saved_tensors
        K, _e0 = _contraction_tensor(P.device)
        hc, B, L1, L2, L3, w4, T12, T = _ContractFunction._factors(P)
        gc = g[16:].to(torch.float64).reshape(2, 10)
        G = (gc @ K.reshape(10, 27)).reshape(2, 1, 3, 3, 3)
        gw4 = (T * G).sum((2, 3, 4))                                       # [2, hc]
        GW = G * w4[:, :, None, None, None]
        gL3 = (GW * T12.unsqueeze(-1)).sum((2, 3))
        gT12 = (GW * L3[:, :, None, None, :]).sum(4)
        gL1 = (gT12 * L2.unsqueeze(-2)).sum(3)
        gL2 = (gT12 * L1.unsqueeze(-1)).sum(2)
        gB = torch.cat([torch.cat([gL1, gL2, gL3, gw4.unsqueeze(-1)], -1).reshape(2, 10 * hc), gc[:, 0:1]], 1)
        return torch.cat([g[:16], gB.reshape(-1).to(P.dtype)])


def contract_block(P: torch.Tensor) -> torch.Tensor:
    """Factored parameter block -> pre-contracted polynomial block (36 entries, "hc = 0").

    The Hadamard product of the three 1x1 branches followed by the 1x1 aggregation
    (train_2drd.py:115-116) is the cubic  r(u,v) = sum_m c_m phi_m(u,v)  with
    c_m = sum_j Wh4[j] * sum_{abc} K[m,a,b,c] L1[j,a] L2[j,b] L3[j,c]  (+ Wh4.bias for m = 0),
    L_k[j] = (Wh_k.weight[j,0], Wh_k.weight[j,1], Wh_k.bias[j]) -- the same expansion the reference
    prints symbolically (train_3drd.py:442-468).  Evaluated in float64, rounded once to the compute
    dtype.  The backward is the exact multilinear chain rule dL/dc -> dL/dWh* (hand-written, float64)."""
    if P.is_cuda:
        return torch.ops.percnn.contract_block(P)
    return _ContractFunction.apply(P)


def check_star_stencil(w_laplace: torch.Tensor) -> None:
    """The kernels implement star stencils of radius 2 (what the reference ships: train_2drd.py:20-24,
    train_3drd.py:22-39).  Anything else is rejected loudly (host check, one sync)."""
    ndim = w_laplace.dim() - 2
    if ndim not in (2, 3) or tuple(w_laplace.shape) != (1, 1) + (5,) * ndim:
        raise ValueError(f"W_laplace.weight must be [1,1,{','.join(['5'] * ndim)}], got {tuple(w_laplace.shape)}")
    w = w_laplace.detach().reshape((5,) * ndim).cpu()
    mask = torch.zeros_like(w, dtype=torch.bool)
    centre = (2,) * ndim
    mask[centre] = True
    for a in range(ndim):
        for off in _OFFS:
            pos = list(centre)
            pos[a] += off
            mask[tuple(pos)] = True
    if bool((w[~mask] != 0).any()):
        raise ValueError("W_laplace.weight has non-zero entries off the radius-2 star; unsupported stencil")


# ------------------------------------------------------------------------------------------------
# raw calls
# ------------------------------------------------------------------------------------------------
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> ctypes.c_void_p:
    if _raw_stream is not None:                       # the current stream's handle without building a Stream object (~0.2 vs ~2 us)
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require(t: torch.Tensor, name: str, dtype=None) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"percnn_amd: {name} must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype not in _SUF:
        raise RuntimeError(f"percnn_amd: {name} must be float32 or float64, got {t.dtype}")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"percnn_amd: {name} has dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"percnn_amd: {name} must be contiguous")


def _hc_of(P: torch.Tensor) -> int:
    """hidden width encoded by the block length; 0 = pre-contracted polynomial block (36 entries)."""
    if P.dim() == 1 and P.numel() == NPOLY:
        return 0
    if P.dim() == 1 and P.numel() == NADV:
        return -1
    n = P.numel() - 16
    if P.dim() != 1 or n < 22 or n % 2 or (n // 2 - 1) % 10:
        raise RuntimeError(f"percnn_amd: parameter block has {P.numel()} entries; expected 16 + 2*(10*hc+1)")
    return (n // 2 - 1) // 10


def workspace(hc: int, shape: Sequence[int], dtype, device) -> torch.Tensor:
    nbytes = _lib.lib().percnn_pi_bwd_workspace_bytes(hc, len(shape), _lib.shape_arg(shape), dtype.itemsize)
    if nbytes == 0:
        raise RuntimeError("percnn_amd: invalid problem shape")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def rollout_workspace(hc: int, shape: Sequence[int], T: int, dtype, device) -> torch.Tensor:
    nbytes = _lib.lib().percnn_pi_rollout_bwd_workspace_bytes(hc, len(shape), _lib.shape_arg(shape), T,
                                                              dtype.itemsize)
    if nbytes == 0:
        raise RuntimeError("percnn_amd: invalid problem shape")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def rollout_fwd_(traj: torch.Tensor, P: torch.Tensor, options=None) -> torch.Tensor:
    """In place: traj[0] holds the initial state; frames 1..T are written.
    options: per-call tuning overrides (dict or "key=value,..."; keys of include/percnn_pi.h:percnn_pi_set_option)."""
    _require(traj, "traj"); _require(P, "params", traj.dtype)
    T = traj.shape[0] - 1
    shape = traj.shape[2:]
    f = getattr(_lib.lib(), "percnn_pi_rollout_fwd_opt_" + _SUF[traj.dtype])
    with torch.cuda.device(traj.device):
        _lib.check(f(traj.data_ptr(), P.data_ptr(), _hc_of(P), len(shape), _lib.shape_arg(shape), T,
                     _lib.options_arg(options), _stream()), "rollout_fwd")
    return traj


def rollout_bwd(traj: torch.Tensor, g_traj: torch.Tensor, P: torch.Tensor,
                frame_mask: Optional[Sequence[bool]] = None, ws: Optional[torch.Tensor] = None, options=None):
    """-> (dL/dh0 [2,*S], dL/dparams double[np]);  options: per-call tuning overrides (see rollout_fwd_)"""
    _require(traj, "traj"); _require(g_traj, "g_traj", traj.dtype); _require(P, "params", traj.dtype)
    T = traj.shape[0] - 1
    shape = traj.shape[2:]
    hc = _hc_of(P)
    g_h0 = torch.empty_like(traj[0])
    pg = torch.zeros(P.numel(), dtype=torch.float64, device=traj.device)
    if ws is None:
        ws = rollout_workspace(hc, shape, T, traj.dtype, traj.device)
    mask = None
    if frame_mask is not None:
        assert len(frame_mask) == T + 1
        mask = bytes(bytearray(1 if m else 0 for m in frame_mask))
    f = getattr(_lib.lib(), "percnn_pi_rollout_bwd_opt_" + _SUF[traj.dtype])
    with torch.cuda.device(traj.device):
        _lib.check(f(traj.data_ptr(), g_traj.data_ptr(), mask, g_h0.data_ptr(), pg.data_ptr(), ws.data_ptr(),
                     ws.numel(), P.data_ptr(), hc, len(shape), _lib.shape_arg(shape), T, _lib.options_arg(options),
                     _stream()), "rollout_bwd")
    return g_h0, pg


def _mask_bytes(frame_mask, n):
    if frame_mask is None:
        return None
    assert len(frame_mask) == n
    return bytes(bytearray(1 if m else 0 for m in frame_mask))


def traj_sqerr(traj: torch.Tensor, target: Optional[torch.Tensor] = None, frame_mask: Optional[Sequence[bool]] = None,
               scale: float = 1.0) -> torch.Tensor:
    """scale * sum over the frames with frame_mask[t] of sum_x (traj_t - target_t)^2 as a 0-dim tensor of traj's dtype, in one
    streaming pass (``percnn_pi_traj_sqerr_*``; target None = 0)."""
    _require(traj, "traj")
    if target is not None:
        _require(target, "target", traj.dtype)
        assert target.shape == traj.shape
    out = torch.empty((), dtype=traj.dtype, device=traj.device)
    ws = torch.empty(8192, dtype=torch.uint8, device=traj.device)
    shape = traj.shape[2:]
    f = getattr(_lib.lib(), "percnn_pi_traj_sqerr_" + _SUF[traj.dtype])
    with torch.cuda.device(traj.device):
        _lib.check(f(traj.data_ptr(), target.data_ptr() if target is not None else None, _mask_bytes(frame_mask, traj.shape[0]),
                     traj.shape[0], len(shape), _lib.shape_arg(shape), float(scale), out.data_ptr(), ws.data_ptr(), ws.numel(),
                     _stream()), "traj_sqerr")
    return out


def rollout_bwd_sqerr(traj: torch.Tensor, P: torch.Tensor, target: Optional[torch.Tensor] = None,
                      frame_mask: Optional[Sequence[bool]] = None, scale: float = 1.0,
                      dev_scale: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, options=None):
    """Backward of  L = (scale / 2) * sum_{t in mask} sum_x (traj_t - target_t)^2  (times the device scalar ``dev_scale``)
    WITHOUT a dL/dtraj buffer: the sweep forms  scale * (h_t - target_t)  from the state it reads anyway
    (``percnn_pi_rollout_bwd_sqerr_*``).  -> (dL/dh0 [2,*S], dL/dparams double[np]).  Block kinds without the in-kernel form
    (advective blocks) take the materialising route here."""
    _require(traj, "traj"); _require(P, "params", traj.dtype)
    if target is not None:
        _require(target, "target", traj.dtype)
        assert target.shape == traj.shape
    if dev_scale is not None:
        dev_scale = dev_scale.reshape(1).to(traj.dtype).contiguous()
    T = traj.shape[0] - 1
    shape = traj.shape[2:]
    hc = _hc_of(P)
    g_h0 = torch.empty_like(traj[0])
    pg = torch.zeros(P.numel(), dtype=torch.float64, device=traj.device)
    if ws is None:
        ws = rollout_workspace(hc, shape, T, traj.dtype, traj.device)
    f = getattr(_lib.lib(), "percnn_pi_rollout_bwd_sqerr_" + _SUF[traj.dtype])
    with torch.cuda.device(traj.device):
        rc = f(traj.data_ptr(), target.data_ptr() if target is not None else None, _mask_bytes(frame_mask, T + 1), float(scale),
               dev_scale.data_ptr() if dev_scale is not None else None, g_h0.data_ptr(), pg.data_ptr(), ws.data_ptr(),
               ws.numel(), P.data_ptr(), hc, len(shape), _lib.shape_arg(shape), T, _lib.options_arg(options), _stream())
    if rc == -1 and hc == -1:                                # advective block: materialise dL/dtraj, ordinary sweep
        g = traj if target is None else traj - target
        g = g * (float(scale) if dev_scale is None else float(scale) * dev_scale)
        return rollout_bwd(traj, g, P, frame_mask=frame_mask, ws=ws, options=options)
    _lib.check(rc, "rollout_bwd_sqerr")
    return g_h0, pg


class PiRolloutSqErrFunction(torch.autograd.Function):
    """Rollout + squared-error loss as ONE autograd node:  loss = weight * sum_{t in frames} sum_x (h_t -
    target_t)^2.  Forward = the fused rollout + one streaming reduction; backward = the sweep with the loss gradient formed
    in-kernel -- no dL/dtraj, 24 (32 with a target) instead of 32 + 2 x 8 bytes per point and step.  Returns (loss, traj);
    traj is not differentiable (inspection / validation only)."""

    @staticmethod
    def forward(ctx, h0, P, steps, target, frame_mask, weight, options):
        _check_state(h0)
        P = P.contiguous()
        traj = torch.empty((steps + 1,) + tuple(h0.shape[1:]), dtype=h0.dtype, device=h0.device)
        traj[0].copy_(h0[0])
        rollout_fwd_(traj, P, options=options)
        loss = traj_sqerr(traj, target, frame_mask, weight)
        ctx.save_for_backward(traj, P) if target is None else ctx.save_for_backward(traj, P, target)
        ctx.meta = (frame_mask, float(weight), options)
        ctx.mark_non_differentiable(traj)
        ctx.set_materialize_grads(False)
        return loss, traj

    @staticmethod
    def backward(ctx, g_loss, _g_traj):
        saved = ctx.saved_tensors
        traj, P = saved[0], saved[1]
        target = saved[2] if len(saved) > 2 else None
        frame_mask, weight, options = ctx.meta
        g_h0, pg = rollout_bwd_sqerr(traj, P, target, frame_mask, 2.0 * weight, g_loss, options=options)
        return g_h0[None], pg.to(P.dtype), None, None, None, None, None


def sqerr_selection(steps: int, frames: Optional[Sequence[int]], reduction: str, sample_numel: int, what: str = "pi_rollout_sqerr"):
    """Host arithmetic of the squared-error operators, no device involved: which of the steps + 1 frames the loss covers and
    the weight of one squared difference.  frames: indices into the frames (negative ones count from the end, duplicates
    count once; None = all).  -> (mask, weight): mask a list of steps + 1 bools, or None when every frame is selected;
    weight = 1 / (selected frames * sample_numel) for "mean" -- sample_numel = 2 * prod(S), the elements of ONE sample's
    frame -- and 1 for "sum".  An empty selection raises."""
    T1 = int(steps) + 1
    sel = sorted(set(int(t) % T1 for t in frames)) if frames is not None else list(range(T1))
    if not sel:
        raise ValueError(f"{what}: no frame selected")
    mask = None if len(sel) == T1 else [t in set(sel) for t in range(T1)]
    weight = {"mean": 1.0 / (len(sel) * int(sample_numel)), "sum": 1.0}[reduction]
    return mask, weight


def pi_rollout_sqerr(h0: torch.Tensor, P: torch.Tensor, steps: int, target: Optional[torch.Tensor] = None,
                     frames: Optional[Sequence[int]] = None, reduction: str = "mean", options=None):
    """-> (loss, traj detached): ``mse_loss(traj[frames], target[frames], reduction)`` of the T-step rollout from h0 (target
    None: ``(traj[frames] ** 2).mean()`` / ``.sum()``) as one autograd node.  frames: indices into the T+1 frames (default
    all); target: [T+1, 2, *S] (frames outside `frames` are never read)."""
    mask, weight = sqerr_selection(steps, frames, reduction, int(h0[0].numel()))
    if target is not None and tuple(target.shape) != (int(steps) + 1,) + tuple(h0.shape[1:]):
        raise ValueError("target must have the trajectory's shape [steps + 1, 2, *S]")
    return PiRolloutSqErrFunction.apply(h0, P, int(steps), target, mask, weight, options)


# ---- the same loss per sample of a batch (one block) / an ensemble (one block per sample): [B] losses, one autograd node ----
def _strides_arg(strides):
    return (ctypes.c_int * len(strides))(*[int(x) for x in strides])


def _check_target(target, traj, frame_mask, strides):
    """the target of a per-sample loss: of the trajectory's shape (strides None: dense) or compact in time and space"""
    if strides is not None:
        return _check_compact(target, traj, frame_mask, strides)
    if target is not None:
        _require(target, "target", traj.dtype)
        assert target.shape == traj.shape


def _traj_loss_samples(traj, target, frame_mask, strides, scale):
    """``traj_sqerr_batched`` (strides None) and ``traj_obs_sqerr_batched``: one streaming pass, one fixed-order sum per sample"""
    _require(traj, "traj")
    _check_target(target, traj, frame_mask, strides)
    B, shape = int(traj.shape[1]), traj.shape[3:]
    L = _lib.lib()
    nbytes = L.percnn_pi_batch_traj_sqerr_workspace_bytes(B)
    if nbytes == 0:
        raise RuntimeError(f"percnn_amd: invalid batch size {B}")
    out = torch.empty(B, dtype=traj.dtype, device=traj.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=traj.device)
    what = "batch_traj_sqerr" if strides is None else "batch_traj_obs_sqerr"
    lattice = () if strides is None else (_strides_arg(strides),)
    f = getattr(L, f"percnn_pi_{what}_" + _SUF[traj.dtype])
    with torch.cuda.device(traj.device):
        _lib.check(f(traj.data_ptr(), target.data_ptr() if target is not None else None, _mask_bytes(frame_mask, traj.shape[0]),
                     traj.shape[0], len(shape), _lib.shape_arg(shape), *lattice, B, float(scale), out.data_ptr(), ws.data_ptr(),
                     ws.numel(), _stream()), what)
    return out


def _rollout_bwd_loss_samples(traj, P, target, frame_mask, strides, scale, dev_scale, ws, options, g_h0, ensemble=None):
    """``rollout_bwd_sqerr_batched`` (strides None) and ``rollout_bwd_obs_sqerr_batched``: the batched / ensemble sweep with the
    loss gradient formed in-kernel."""
    _require(traj, "traj"); _require(P, "params", traj.dtype)
    _check_target(target, traj, frame_mask, strides)
    T, B, shape = traj.shape[0] - 1, int(traj.shape[1]), traj.shape[3:]
    if ensemble is None:
        ensemble = P.dim() == 2
    if strides is not None and P.dim() != (2 if ensemble else 1):    # (the dense form leaves a block of another rank to _hc_of)
        raise ValueError(f"{'one parameter block per sample [B,np]' if ensemble else 'one parameter block [np]'}, got {tuple(P.shape)}")
    kind = "ensemble" if ensemble else "batch"
    if ensemble and P.shape[0] != B:
        raise ValueError(f"one parameter block per sample: P [{B},np], got {tuple(P.shape)}")
    hc = _hc_of(P[0] if ensemble else P)
    if dev_scale is not None:
        dev_scale = dev_scale.reshape(B).to(traj.dtype).contiguous()
    L = _lib.lib()
    if g_h0 is None:
        g_h0 = torch.empty_like(traj[0])
    pg = torch.zeros(tuple(P.shape), dtype=torch.float64, device=traj.device)
    if ws is None:
        nbytes = getattr(L, f"percnn_pi_{kind}_rollout_bwd_workspace_bytes")(hc, len(shape), _lib.shape_arg(shape), B, T,
                                                                            traj.dtype.itemsize)
        if nbytes == 0:
            raise RuntimeError("percnn_amd: invalid problem shape, batch size or block kind")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=traj.device)
    what = f"{kind}_rollout_bwd_sqerr" if strides is None else f"{kind}_rollout_bwd_obs_sqerr"
    lattice = () if strides is None else (_strides_arg(strides),)
    f = getattr(L, f"percnn_pi_{what}_" + _SUF[traj.dtype])
    with torch.cuda.device(traj.device):
        _lib.check(f(traj.data_ptr(), target.data_ptr() if target is not None else None, _mask_bytes(frame_mask, T + 1), *lattice,
                     float(scale), dev_scale.data_ptr() if dev_scale is not None else None, g_h0.data_ptr(), pg.data_ptr(),
                     ws.data_ptr(), ws.numel(), P.data_ptr(), hc, len(shape), _lib.shape_arg(shape), B, T,
                     _lib.options_arg(options), _stream()), what)
    return g_h0, pg


def traj_sqerr_batched(traj: torch.Tensor, target: Optional[torch.Tensor] = None, frame_mask: Optional[Sequence[bool]] = None,
                       scale: float = 1.0) -> torch.Tensor:
    """traj / target [F,B,2,*S] -> [B] of traj's dtype: scale * sum over the frames with frame_mask[f] of sum_x (traj[f,b] -
    target[f,b])^2, one streaming pass and one fixed-order sum per sample (``percnn_pi_batch_traj_sqerr_*``; target None = 0)."""
    return _traj_loss_samples(traj, target, frame_mask, None, scale)


def rollout_bwd_sqerr_batched(traj: torch.Tensor, P: torch.Tensor, target: Optional[torch.Tensor] = None,
                              frame_mask: Optional[Sequence[bool]] = None, scale: float = 1.0,
                              dev_scale: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, options=None,
                              g_h0: Optional[torch.Tensor] = None):
    """Backward of the B losses  L_b = (scale / 2) * sum_{t in mask} sum_x (traj[t,b] - target[t,b])^2, each times its own
    factor ``dev_scale[b]`` (a [B] device tensor, None = 1), WITHOUT a dL/dtraj buffer (``percnn_pi_{batch,ensemble}_rollout_
    bwd_sqerr_*``).  traj / target [T+1,B,2,*S]; P [np]: one block -> (dL/dh0 [B,2,*S], double [np] summed over the samples);
    P [B,np]: one block per sample -> (dL/dh0, double [B,np])."""
    return _rollout_bwd_loss_samples(traj, P, target, frame_mask, None, scale, dev_scale, ws, options, g_h0)


class _PiRolloutLossSamplesFunction(torch.autograd.Function):
    """The node of ``PiRolloutSqErrBatchedFunction`` (strides None: dense) and ``PiRolloutObsSqErrBatchedFunction``."""

    @staticmethod
    def forward(ctx, h0, P, steps, target, frame_mask, strides, weight, options):
        _native()
        P = P.contiguous()
        op = torch.ops.percnn.pi_rollout_ensemble if P.dim() == 2 else torch.ops.percnn.pi_rollout_batched
        traj = op(h0, P, steps, _options_str(options))
        loss = _traj_loss_samples(traj, target, frame_mask, strides, weight)
        ctx.save_for_backward(traj, P) if target is None else ctx.save_for_backward(traj, P, target)
        ctx.meta = (frame_mask, strides, float(weight), options)
        ctx.mark_non_differentiable(traj)
        ctx.set_materialize_grads(False)
        return loss, traj

    @staticmethod
    def backward(ctx, g_loss, _g_traj):
        if g_loss is None:
            return None, None, None, None, None, None, None, None
        saved = ctx.saved_tensors
        traj, P = saved[0], saved[1]
        target = saved[2] if len(saved) > 2 else None
        frame_mask, strides, weight, options = ctx.meta
        g_h0, pg = _rollout_bwd_loss_samples(traj, P, target, frame_mask, strides, 2.0 * weight, g_loss.contiguous(), None,
                                             options, None)
        return g_h0, pg.to(P.dtype), None, None, None, None, None, None


class PiRolloutSqErrBatchedFunction(_PiRolloutLossSamplesFunction):
    """``PiRolloutSqErrFunction`` for B trajectories: loss[b] = weight * sum_{t in frames} sum_x (h_t[b] - target_t[b])^2, a
    [B] tensor, as ONE autograd node.  Forward = the batched (P [np]) or ensemble (P [B,np]) rollout + one streaming
    reduction per sample; backward = the sweep with the incoming [B] gradient as per-sample factors, the loss gradient formed
    in-kernel -- no dL/dtraj [T+1,B,2,*S], no host synchronisation.  Returns (loss, traj); traj is not differentiable."""

    @classmethod
    def apply(cls, h0, P, steps, target, frame_mask, weight, options):         # the dense form takes no strides
        return super().apply(h0, P, steps, target, frame_mask, None, weight, options)


def _pi_rollout_sqerr_samples(what, h0, P, steps, target, frames, reduction, options):
    if h0.dim() not in (4, 5) or h0.shape[1] != 2:
        raise ValueError(f"{what}: h0 must be [B,2,*S], got {tuple(h0.shape)}")
    mask, weight = sqerr_selection(steps, frames, reduction, int(h0[0].numel()), what)
    if target is not None:
        if tuple(target.shape) != (int(steps) + 1,) + tuple(h0.shape):
            raise ValueError("target must have the trajectory's shape [steps + 1, B, 2, *S]")
        target = target.detach()
    return PiRolloutSqErrBatchedFunction.apply(h0, P, int(steps), target, mask, weight, options)


def pi_rollout_sqerr_batched(h0: torch.Tensor, P: torch.Tensor, steps: int, target: Optional[torch.Tensor] = None,
                             frames: Optional[Sequence[int]] = None, reduction: str = "mean", options=None):
    """-> (loss [B], traj [T+1,B,2,*S] detached): ``loss[b] = mse_loss(traj[frames, b], target[frames, b], reduction)`` of the
    T-step rollouts from h0 [B,2,*S] with ONE block P [np] (target None: 0; the mean is over len(frames) * 2 * prod(S)), as
    one autograd node.  ``loss.mean().backward()``, ``.sum()`` or any weighting of the samples is the caller's line; the
    parameter gradient is the sum over the samples.  target gets no gradient."""
    if P.dim() != 1:
        raise ValueError(f"pi_rollout_sqerr_batched: one parameter block [np], got {tuple(P.shape)}")
    return _pi_rollout_sqerr_samples("pi_rollout_sqerr_batched", h0, P, steps, target, frames, reduction, options)


def pi_rollout_sqerr_ensemble(h0: torch.Tensor, P: torch.Tensor, steps: int, target: Optional[torch.Tensor] = None,
                              frames: Optional[Sequence[int]] = None, reduction: str = "mean", options=None):
    """``pi_rollout_sqerr_batched`` with one block per sample, P [B,np]: loss[b] is member b's loss, and row b of the [B,np]
    parameter gradient is the gradient of member b alone."""
    if P.dim() != 2 or P.shape[0] != h0.shape[0]:
        raise ValueError(f"pi_rollout_sqerr_ensemble: one parameter block per sample [B,np], got {tuple(P.shape)}")
    return _pi_rollout_sqerr_samples("pi_rollout_sqerr_ensemble", h0, P, steps, target, frames, reduction, options)


# ---- the per-sample loss on sparse observations: a sub-lattice of the selected frames against a compact target ----
def obs_selection(steps: int, t_idx: Sequence[int], strides, shape: Sequence[int], reduction: str = "mean",
                  what: str = "pi_rollout_obs_sqerr"):
    """Host arithmetic of the sparse-observation operators, no device involved.  t_idx: frame indices into the steps + 1
    frames, strictly increasing after negative ones are wrapped; strides: an int or one int >= 1 per axis of `shape`.
    -> (t_idx wrapped, mask, strides, Sc, weight): mask a list of steps + 1 bools (None when every frame is selected),
    Sc = ceil(S / s) per axis, weight = 1 / (len(t_idx) * 2 * prod(Sc)) for "mean" -- what ``F.mse_loss`` of one sample's
    slice divides by -- and 1 for "sum"."""
    T1 = int(steps) + 1
    sel = [int(t) % T1 for t in t_idx]
    if not sel:
        raise ValueError(f"{what}: no frame selected")
    if any(b <= a for a, b in zip(sel, sel[1:])):
        raise ValueError(f"{what}: t_idx must be strictly increasing, got {list(t_idx)}")
    if isinstance(strides, int):
        strides = (strides,) * len(shape)
    strides = tuple(int(x) for x in strides)
    if len(strides) != len(shape):
        raise ValueError(f"{what}: one stride per axis of {tuple(shape)}, got {strides}")
    if any(x < 1 for x in strides):
        raise ValueError(f"{what}: strides must be >= 1, got {strides}")
    Sc = tuple(-(-int(n) // x) for n, x in zip(shape, strides))
    mask = None if len(sel) == T1 else [t in set(sel) for t in range(T1)]
    numel = 2
    for n in Sc:
        numel *= n
    weight = {"mean": 1.0 / (len(sel) * numel), "sum": 1.0}[reduction]
    return sel, mask, strides, Sc, weight


def _check_compact(target, traj, frame_mask, strides):
    F, B, shape = traj.shape[0], int(traj.shape[1]), traj.shape[3:]
    n = F if frame_mask is None else sum(1 for m in frame_mask if m)
    if len(strides) != len(shape):
        raise ValueError(f"one stride per axis of {tuple(shape)}, got {tuple(strides)}")
    if target is not None:
        _require(target, "target", traj.dtype)
    if target is not None and all(int(x) >= 1 for x in strides):   # (a stride < 1 is the library's to refuse)
        want = (n, B, 2) + tuple(-(-int(s) // int(x)) for s, x in zip(shape, strides))
        if tuple(target.shape) != want:
            raise ValueError(f"compact target must be {want}, got {tuple(target.shape)}")


def traj_obs_sqerr_batched(traj: torch.Tensor, target: Optional[torch.Tensor] = None,
                           frame_mask: Optional[Sequence[bool]] = None, strides: Sequence[int] = (), scale: float = 1.0) -> torch.Tensor:
    """traj [F,B,2,*S], target [n,B,2,*Sc] compact in time and space (None = 0) -> [B] of traj's dtype: scale * sum over the
    frames with frame_mask[f] and the lattice points x_d % s_d == 0 of (traj - target)^2 (``percnn_pi_batch_traj_obs_sqerr_*``)."""
    return _traj_loss_samples(traj, target, frame_mask, strides, scale)


def rollout_bwd_obs_sqerr_batched(traj: torch.Tensor, P: torch.Tensor, target: Optional[torch.Tensor] = None,
                                  frame_mask: Optional[Sequence[bool]] = None, strides: Sequence[int] = (), scale: float = 1.0,
                                  dev_scale: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, options=None,
                                  g_h0: Optional[torch.Tensor] = None, ensemble: Optional[bool] = None):
    """``rollout_bwd_sqerr_batched`` for the loss on the lattice of the selected frames against the compact target
    [n,B,2,*Sc] (``percnn_pi_{batch,ensemble}_rollout_bwd_obs_sqerr_*``): no dL/dtraj, no scatter of the observed frames.
    ensemble: None = by the rank of P ([np] / [B,np]).  B = 1 runs the same launches with one sample."""
    return _rollout_bwd_loss_samples(traj, P, target, frame_mask, strides, scale, dev_scale, ws, options, g_h0, ensemble)


class PiRolloutObsSqErrBatchedFunction(_PiRolloutLossSamplesFunction):
    """``PiRolloutSqErrBatchedFunction`` on sparse observations: loss[b] = weight * sum_k sum over the lattice of
    (h_{t_k}[b] - target[k, b])^2, a [B] tensor, as ONE autograd node.  Forward = the batched (P [np]) or ensemble (P [B,np])
    rollout + one reduction per sample over the lattice; backward = the sweep with the incoming [B] gradient as per-sample
    factors, the loss gradient formed in-kernel at the lattice points -- no dL/dtraj [T+1,B,2,*S], no scatter, no host
    synchronisation.  Returns (loss, traj); traj is not differentiable."""


def _pi_rollout_obs_sqerr_samples(what, h0, P, steps, target, t_idx, strides, reduction, options):
    if h0.dim() not in (4, 5) or h0.shape[1] != 2:
        raise ValueError(f"{what}: h0 must be [B,2,*S], got {tuple(h0.shape)}")
    sel, mask, strides, Sc, weight = obs_selection(steps, t_idx, strides, tuple(h0.shape[2:]), reduction, what)
    if target is not None:
        if tuple(target.shape) != (len(sel), int(h0.shape[0]), 2) + Sc:
            raise ValueError(f"{what}: target must be [n, B, 2, *ceil(S / s)] = {(len(sel), int(h0.shape[0]), 2) + Sc}, "
                             f"got {tuple(target.shape)}")
        target = target.detach().contiguous()
    return PiRolloutObsSqErrBatchedFunction.apply(h0, P, int(steps), target, mask, strides, weight, options)


def pi_rollout_obs_sqerr_batched(h0: torch.Tensor, P: torch.Tensor, steps: int, target: Optional[torch.Tensor],
                                 t_idx: Sequence[int], strides, reduction: str = "mean", options=None):
    """-> (loss [B], traj [T+1,B,2,*S] detached): ``loss[b] = mse_loss(traj[t_idx][:, b, :, ::s_0, ::s_1(, ::s_2)],
    target[:, b], reduction)`` of the T-step rollouts from h0 [B,2,*S] with ONE block P [np], as one autograd node --
    the reference's data loss (``output[0:-1:20, :, ::4, ::4]`` against the coarse truth) for B trajectories at once.
    target: [len(t_idx), B, 2, *ceil(S / s)], compact in time and space (None: 0); t_idx strictly increasing (negative
    indices count from the end); strides an int or one per axis.  The parameter gradient is the sum over the samples;
    target gets no gradient."""
    if P.dim() != 1:
        raise ValueError(f"pi_rollout_obs_sqerr_batched: one parameter block [np], got {tuple(P.shape)}")
    return _pi_rollout_obs_sqerr_samples("pi_rollout_obs_sqerr_batched", h0, P, steps, target, t_idx, strides, reduction, options)


def pi_rollout_obs_sqerr_ensemble(h0: torch.Tensor, P: torch.Tensor, steps: int, target: Optional[torch.Tensor],
                                  t_idx: Sequence[int], strides, reduction: str = "mean", options=None):
    """``pi_rollout_obs_sqerr_batched`` with one block per sample, P [B,np]: loss[b] is member b's loss, and row b of the
    [B,np] parameter gradient is the gradient of member b alone."""
    if P.dim() != 2 or P.shape[0] != h0.shape[0]:
        raise ValueError(f"pi_rollout_obs_sqerr_ensemble: one parameter block per sample [B,np], got {tuple(P.shape)}")
    return _pi_rollout_obs_sqerr_samples("pi_rollout_obs_sqerr_ensemble", h0, P, steps, target, t_idx, strides, reduction, options)


def step_fwd(h: torch.Tensor, P: torch.Tensor, out: Optional[torch.Tensor] = None, slab: bool = False,
             halo: int = 2, skip: int = 0, planes: Optional[Sequence[int]] = None, options=None):
    """h: [2,*S] -> next state.  slab=True: h is a local slab [2, n0+2*halo, ...] (see include/percnn_pi.h);
    planes=(lo, hi): only those padded planes of the output are computed (communication overlap)."""
    _require(h, "h"); _require(P, "params", h.dtype)
    if out is None:
        out = torch.empty_like(h)
    _require(out, "out", h.dtype)
    shape = list(h.shape[1:])
    L = _lib.lib()
    with torch.cuda.device(h.device):
        if slab and planes is not None:
            shape[0] -= 2 * halo
            f = getattr(L, "percnn_pi_slab_step_fwd_range_" + _SUF[h.dtype])
            rc = f(h.data_ptr(), out.data_ptr(), P.data_ptr(), _hc_of(P), len(shape), _lib.shape_arg(shape), halo,
                   int(planes[0]), int(planes[1]), _stream())
        elif slab:
            shape[0] -= 2 * halo
            f = getattr(L, "percnn_pi_slab_step_fwd_" + _SUF[h.dtype])
            rc = f(h.data_ptr(), out.data_ptr(), P.data_ptr(), _hc_of(P), len(shape), _lib.shape_arg(shape), halo,
                   skip, _stream())
        else:
            f = getattr(L, "percnn_pi_step_fwd_opt_" + _SUF[h.dtype])
            rc = f(h.data_ptr(), out.data_ptr(), P.data_ptr(), _hc_of(P), len(shape), _lib.shape_arg(shape),
                   _lib.options_arg(options), _stream())
    _lib.check(rc, "step_fwd")
    return out


def step_bwd(h: torch.Tensor, g_out: torch.Tensor, P: torch.Tensor, g_inject: Optional[torch.Tensor] = None,
             g_in: Optional[torch.Tensor] = None, param_grad: Optional[torch.Tensor] = None, slab: bool = False,
             halo: int = 2, ws: Optional[torch.Tensor] = None, sweep_only: bool = False,
             planes: Optional[Sequence[int]] = None, no_reset: bool = False, no_finish: bool = False, options=None):
    """-> (dL/dh, param_grad double[np] (accumulated if given)).  sweep_only (slab): adjoint state and
    diffusion-coefficient gradients only; the branch gradients come from ``slab_wgrad`` afterwards.
    planes=(lo, hi) (slab): only those padded planes of dL/dh are computed; no_reset / no_finish: the launch shares
    its gradient sums with earlier / later launches of the same sweep through the workspace (include/percnn_pi.h)."""
    _require(h, "h"); _require(g_out, "g_out", h.dtype); _require(P, "params", h.dtype)
    if g_inject is not None:
        _require(g_inject, "g_inject", h.dtype)
    if g_in is None:
        g_in = torch.zeros_like(h) if slab else torch.empty_like(h)
    hc = _hc_of(P)
    if param_grad is None:
        param_grad = torch.zeros(P.numel(), dtype=torch.float64, device=h.device)
    shape = list(h.shape[1:])
    if slab:
        shape[0] -= 2 * halo
    if ws is None:
        ws = workspace(hc, shape, h.dtype, h.device)
    L = _lib.lib()
    inj = g_inject.data_ptr() if g_inject is not None else None
    with torch.cuda.device(h.device):
        flags = (1 if sweep_only else 0) | (2 if no_reset else 0) | (4 if no_finish else 0)
        if slab and (planes is not None or flags > 1):
            lo, hi = (int(planes[0]), int(planes[1])) if planes is not None else (halo, halo + shape[0])
            f = getattr(L, "percnn_pi_slab_step_bwd_range_" + _SUF[h.dtype])
            rc = f(h.data_ptr(), g_out.data_ptr(), inj, g_in.data_ptr(), param_grad.data_ptr(), ws.data_ptr(),
                   ws.numel(), P.data_ptr(), hc, len(shape), _lib.shape_arg(shape), halo, lo, hi, flags, _stream())
        elif slab:
            f = getattr(L, "percnn_pi_slab_step_bwd_" + _SUF[h.dtype])
            rc = f(h.data_ptr(), g_out.data_ptr(), inj, g_in.data_ptr(), param_grad.data_ptr(), ws.data_ptr(),
                   ws.numel(), P.data_ptr(), hc, len(shape), _lib.shape_arg(shape), halo, 1 if sweep_only else 0,
                   _stream())
        else:
            f = getattr(L, "percnn_pi_step_bwd_opt_" + _SUF[h.dtype])
            rc = f(h.data_ptr(), g_out.data_ptr(), inj, g_in.data_ptr(), param_grad.data_ptr(), ws.data_ptr(),
                   ws.numel(), P.data_ptr(), hc, len(shape), _lib.shape_arg(shape), _lib.options_arg(options), _stream())
    _lib.check(rc, "step_bwd")
    return g_in, param_grad


def slab_rollout_fwd_native_(traj: torch.Tensor, P: torch.Tensor, halo: int, ring, overlap: bool) -> torch.Tensor:
    """The whole T-step slab loop incl. halo exchanges in one C call (include/percnn_pi.h, native slab rollouts).
    ring: ctypes pointer to a ``_lib.HaloRing`` or None (single rank: periodic wrap by index inside the step launches).
    overlap: bool, or the C entry point's flag word (bit 0 faces first, bit 1 single-rank wrap by face copies)."""
    _require(traj, "traj"); _require(P, "params", traj.dtype)
    shape = list(traj.shape[2:])
    shape[0] -= 2 * halo
    f = getattr(_lib.lib(), "percnn_pi_slab_rollout_fwd_" + _SUF[traj.dtype])
    with torch.cuda.device(traj.device):
        _lib.check(f(traj.data_ptr(), P.data_ptr(), _hc_of(P), len(shape), _lib.shape_arg(shape), halo,
                     traj.shape[0] - 1, ring, int(overlap), _stream()), "slab_rollout_fwd")
    return traj


def slab_rollout_bwd_native(traj: torch.Tensor, g_traj: torch.Tensor, P: torch.Tensor, halo: int, ring, overlap: bool):
    """-> (adjoint trajectory [T+1, 2, n0+2*halo, ...] (frame 0 = dL/dh0, padded), LOCAL dL/dparams double[np])"""
    _require(traj, "traj"); _require(g_traj, "g_traj", traj.dtype); _require(P, "params", traj.dtype)
    shape = list(traj.shape[2:])
    shape[0] -= 2 * halo
    hc = _hc_of(P)
    adj = torch.empty_like(traj)
    pg = torch.zeros(P.numel(), dtype=torch.float64, device=traj.device)
    ws = workspace(hc, shape, traj.dtype, traj.device)
    f = getattr(_lib.lib(), "percnn_pi_slab_rollout_bwd_" + _SUF[traj.dtype])
    with torch.cuda.device(traj.device):
        _lib.check(f(traj.data_ptr(), g_traj.data_ptr(), adj.data_ptr(), pg.data_ptr(), ws.data_ptr(), ws.numel(),
                     P.data_ptr(), hc, len(shape), _lib.shape_arg(shape), halo, traj.shape[0] - 1, ring,
                     int(overlap), _stream()), "slab_rollout_bwd")
    return adj, pg


def slab_wgrad(traj: torch.Tensor, adj: torch.Tensor, P: torch.Tensor, halo: int, param_grad: torch.Tensor,
               ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Accumulate the branch-weight (or coefficient-moment) gradients of all steps of LOCAL padded
    trajectories [T+1, 2, n0+2*halo, ...] into ``param_grad`` -- one time-parallel reduction."""
    _require(traj, "traj"); _require(adj, "adj", traj.dtype); _require(P, "params", traj.dtype)
    T = traj.shape[0] - 1
    shape = list(traj.shape[2:])
    shape[0] -= 2 * halo
    hc = _hc_of(P)
    if ws is None:
        ws = workspace(hc, shape, traj.dtype, traj.device)
    f = getattr(_lib.lib(), "percnn_pi_slab_wgrad_" + _SUF[traj.dtype])
    with torch.cuda.device(traj.device):
        _lib.check(f(traj.data_ptr(), adj.data_ptr(), param_grad.data_ptr(), ws.data_ptr(), ws.numel(), P.data_ptr(),
                     hc, len(shape), _lib.shape_arg(shape), halo, T, _stream()), "slab_wgrad")
    return param_grad


# ------------------------------------------------------------------------------------------------
# autograd
# ------------------------------------------------------------------------------------------------
def _check_state(h: torch.Tensor) -> None:
    if h.dim() not in (4, 5) or h.shape[0] != 1 or h.shape[1] != 2:
        raise RuntimeError(f"percnn_amd: state must be [1,2,*S] (batch 1, two species), got {tuple(h.shape)}")


def _step_fwd_lean(h: torch.Tensor, P: torch.Tensor) -> torch.Tensor:
    """step_fwd for the per-step call of a reference-style loop: same checks, no context manager / option parsing when the
    tensors already live on the current device (the host side of a 100^2 step costs more than its 3 us kernel)."""
    _require(h, "h"); _require(P, "params", h.dtype)
    if h.device.index != torch.cuda.current_device():
        return step_fwd(h[0], P)[None]
    out = torch.empty_like(h)
    shape = h.shape[2:]
    f = getattr(_lib.lib(), "percnn_pi_step_fwd_opt_" + _SUF[h.dtype])
    _lib.check(f(h.data_ptr(), out.data_ptr(), P.data_ptr(), _hc_of(P), len(shape), _lib.shape_arg(shape), None, _stream()),
               "step_fwd")
    return out


class PiStepFunction(torch.autograd.Function):
    """One fused step: replaces the ~30 ATen launches of RCNNCell.forward."""

    @staticmethod
    def forward(ctx, h, P):
        _check_state(h)
        h = h.contiguous()
        P = P.contiguous()
        out = _step_fwd_lean(h, P)
        ctx.save_for_backward(h, P)
        return out

    @staticmethod
    def backward(ctx, g):
        h, P = ctx.saved_tensors
        g_in, pg = step_bwd(h[0], g.contiguous()[0], P)
        return g_in[None], pg.to(P.dtype)


class PiRolloutFunction(torch.autograd.Function):
    """T fused steps; returns the whole trajectory [T+1,2,*S] (frame 0 = h0), i.e. what the
    reference's callers build with torch.cat(tuple(outputs), dim=0) (train_2drd.py:394)."""

    @staticmethod
    def forward(ctx, h0, P, steps):
        _check_state(h0)
        P = P.contiguous()
        traj = torch.empty((steps + 1,) + tuple(h0.shape[1:]), dtype=h0.dtype, device=h0.device)
        traj[0].copy_(h0[0])
        rollout_fwd_(traj, P)
        ctx.save_for_backward(traj, P)
        return traj

    @staticmethod
    def backward(ctx, g_traj):
        traj, P = ctx.saved_tensors
        g_h0, pg = rollout_bwd(traj, g_traj.contiguous(), P)
        return g_h0[None], pg.to(P.dtype), None


def _dense_prefix_view(grads, traj):
    """The T+1 per-frame gradients as ONE view of traj's shape if they are consecutive slices of one buffer, else None."""
    T1 = traj.shape[0]
    g0 = grads[0]
    if any(g is None for g in grads) or not g0.is_contiguous() or g0.dtype != traj.dtype:
        return None
    step_bytes = traj[0].numel() * traj.element_size()
    base = g0.data_ptr()
    st = g0.untyped_storage()
    room = st.nbytes() - (base - st.data_ptr())
    if room < T1 * step_bytes:
        return None
    if not all(g.is_contiguous() and g.dtype == traj.dtype and g.data_ptr() == base + k * step_bytes
               and g.untyped_storage().data_ptr() == st.data_ptr() for k, g in enumerate(grads)):
        return None
    return torch.as_strided(g0, traj.shape, traj.stride(), g0.storage_offset())


def _assemble_frame_grads(grads, frames, traj):
    """dL/dtraj [T+1,R,2,*S] from the per-frame gradients [R,2,*S] autograd hands back.  ``frames`` = the dense list 0..T (what
    ``torch.cat(tuple(outputs))`` followed by any dense loss produces: CatBackward narrows its incoming gradient, so
    the per-frame gradients are consecutive slices of one buffer -> zero-copy view), optionally FOLLOWED by extra
    frames (``RCNN.forward`` returns ``second_last_state`` as one more output): extras without a gradient cost
    nothing, extras with one cost a single copy of the dense part.  Anything else: the frames that carry a gradient
    are copied and the rest is masked out of the sweep."""
    T1 = traj.shape[0]
    if len(frames) >= T1 and tuple(frames[:T1]) == tuple(range(T1)):
        view = _dense_prefix_view(grads[:T1], traj)
        if view is not None:
            extras = [(k, g) for k, g in zip(frames[T1:], grads[T1:]) if g is not None]
            if not extras:
                return view, None
            g_traj = view.clone()                              # autograd owns `view`: never accumulate into it
            for k, g in extras:
                g_traj[k].add_(g)
            return g_traj, None
    g_traj = torch.empty_like(traj)
    mask = [False] * T1
    for k, g in zip(frames, grads):
        if g is None:
            continue
        if mask[k]:
            g_traj[k].add_(g)
        else:
            g_traj[k].copy_(g)
            mask[k] = True
    return g_traj, mask


class Frame(torch.Tensor):
    """One [1,2,*S] frame of a rollout as ``RCNN.forward()`` hands it out: an ordinary tensor (every operation on it returns
    plain ``torch.Tensor``s) that remembers which trajectory buffer it is a view of, so that the reference's own next line --
    ``output = torch.cat(tuple(output), dim=0)`` (train_2drd.py:394, train_3drd.py:400, percnn_LO_eqn.py:367) -- returns
    that buffer (a slice of it for a run of consecutive steps) instead of copying the whole trajectory forward
    (2 GiB at 512^2 x 1000) and slicing its gradient apart again backward.  Anything else -- another order, another dim,
    frames of two rollouts, foreign tensors in the sequence, ``out=`` -- takes the stock ``torch.cat``."""

    _pi_index: int = -1
    _pi_stacked: Optional[torch.Tensor] = None

    # copies and pickles are plain tensors: a copy is no view of the trajectory buffer, and the link must not drag 2 GiB along
    def __deepcopy__(self, memo):
        return self.as_subclass(torch.Tensor).__deepcopy__(memo)

    def __reduce_ex__(self, proto):
        return self.as_subclass(torch.Tensor).__reduce_ex__(proto)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is torch.cat and args and "out" not in kwargs:
            view = _cat_of_frames(args[0], kwargs.get("dim", args[1] if len(args) > 1 else 0))
            if view is not None:
                return view
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


def _cat_of_frames(seq, dim) -> Optional[torch.Tensor]:
    """the view of the trajectory buffer that equals torch.cat(seq, dim), or None"""
    if not isinstance(seq, (tuple, list)) or len(seq) == 0 or type(seq[0]) is not Frame:
        return None
    st = seq[0]._pi_stacked
    if st is None or not isinstance(dim, int) or dim not in (0, -st.dim()):
        return None
    i0, n = seq[0]._pi_index, len(seq)
    if i0 < 0:
        return None
    # consecutive steps only: for every n-th step a strided view would be free forward, but its SliceBackward hands the sweep a
    # dense, mostly zero dL/dtraj where the stock cat's per-frame gradients let it mask the unobserved frames out
    for j, f in enumerate(seq):
        if type(f) is not Frame or f._pi_stacked is not st or f._pi_index != i0 + j:
            return None
    b = seq[0].shape[0]                                     # rows per frame: 1, or B of a batched rollout
    if i0 == 0 and n * b == st.shape[0]:
        return st                                           # every frame: the buffer itself, no node in between
    return st[i0 * b:(i0 + n) * b]


def link_frames(frames: Sequence[torch.Tensor], stacked: torch.Tensor) -> None:
    """tell the frames of one rollout (PiRolloutFramesFunction's outputs) which tensor torch.cat may return for them"""
    for f in frames:
        if type(f) is Frame:
            f._pi_stacked = stacked


def frame_outputs(ctx, buf: torch.Tensor, frames: Sequence[int]):
    """Forward half of the frame-list protocol every fused rollout node shares.  buf: the trajectory buffer [T+1,R,2,*S]
    (R = 1: one trajectory, R = B: a batch or an ensemble).  -> the requested frames ``buf[k]`` [R,2,*S] as ``Frame``s (what makes
    the caller's ``torch.cat(tuple(outputs))`` free) and, LAST, the buffer as [(T+1)*R,2,*S]: what that ``torch.cat`` is."""
    ctx.frames = tuple(int(k) for k in frames)
    ctx.set_materialize_grads(False)
    views = buf.unbind(0)                                   # all frame views in one call
    outs = []
    for k in ctx.frames:
        f = views[k].as_subclass(Frame)
        f._pi_index = k
        outs.append(f)
    return tuple(outs) + (buf.view((-1,) + tuple(buf.shape[2:])),)


def frame_grads(frames, grads, buf: torch.Tensor):
    """Backward half: ``grads`` = the gradients of ``frame_outputs``' outputs (one per frame, then the stacked one).
    -> None when nothing carries a gradient, else (dL/dtraj of buf's shape, contiguous; frame mask or None = every frame)."""
    g_stacked, grads = grads[-1], grads[:-1]
    per_frame = any(g is not None for g in grads)
    if g_stacked is None:
        return _assemble_frame_grads(grads, frames, buf) if per_frame else None
    if not per_frame:                                       # the loss was written on `outputs.stacked` alone: zero-copy
        return g_stacked.contiguous().view(buf.shape), None
    g_traj = g_stacked.clone(memory_format=torch.contiguous_format).view(buf.shape)
    for k, g in zip(frames, grads):                         # both: per-frame gradients on top of a copy of the stacked one
        if g is not None:
            g_traj[k].add_(g)
    return g_traj, None


class PiRolloutFramesFunction(torch.autograd.Function):
    """T fused steps, returned as the reference returns them: a tuple of [1,2,*S] frames (train_2drd.py:162-190
    appends every effective step to a Python list).  The frames are views of ONE trajectory buffer; the backward
    receives one gradient per frame and runs ONE fused rollout backward.  (Slicing an autograd tensor T+1 times
    instead would make autograd allocate and zero a full-trajectory gradient per slice: 1.4 s instead of 6 ms per
    iteration at 512^2 x 1000 -- measured.)  The LAST output is that buffer itself, [T+1,2,*S]: what the reference's callers
    build with ``torch.cat(tuple(outputs), dim=0)`` (train_2drd.py:394) without the 2 GiB copy and its CatBackward
    (``RCNN.forward()`` hands it out as ``outputs.stacked``)."""

    @staticmethod
    def forward(ctx, h0, P, steps, frames):
        _check_state(h0)
        P = P.contiguous()
        traj = torch.empty((steps + 1,) + tuple(h0.shape[1:]), dtype=h0.dtype, device=h0.device)
        traj[0].copy_(h0[0])
        rollout_fwd_(traj, P)
        ctx.save_for_backward(traj, P)
        return frame_outputs(ctx, traj.unsqueeze(1), frames)

    @staticmethod
    def backward(ctx, *grads):
        traj, P = ctx.saved_tensors
        routed = frame_grads(ctx.frames, grads, traj.unsqueeze(1))
        if routed is None:
            return None, None, None, None
        g_h0, pg = rollout_bwd(traj, routed[0].squeeze(1), P, frame_mask=routed[1])
        return g_h0[None], pg.to(P.dtype), None, None


def pi_rollout_frames(h0: torch.Tensor, P: torch.Tensor, steps: int, frames: Sequence[int], with_stacked: bool = False):
    out = PiRolloutFramesFunction.apply(h0, P, int(steps), tuple(frames))
    return out if with_stacked else out[:-1]


class PiRolloutBatchedFramesFunction(torch.autograd.Function):
    """``PiRolloutFramesFunction`` for a batched initial state [B,2,*S]: one ``torch.ops.percnn.pi_rollout_batched`` call (P [np]:
    one block) or ``pi_rollout_ensemble`` call (P [B,np]: one block per sample), the frames are [B,2,*S] views of its
    [T+1,B,2,*S] buffer, the LAST output is that buffer as [(T+1)*B,2,*S] -- what ``torch.cat(tuple(outputs), dim=0)`` of the
    batched frames is (train_2drd.py:394).  The backward runs ONE batched or ensemble rollout backward on the dense dL/dtraj
    (the operators take no frame mask: frames without a gradient are zero-filled); the parameter gradient has P's shape."""

    @staticmethod
    def forward(ctx, h0, P, steps, frames):
        _native()
        P = P.contiguous()
        op = torch.ops.percnn.pi_rollout_ensemble if P.dim() == 2 else torch.ops.percnn.pi_rollout_batched
        traj = op(h0, P, steps, "")
        ctx.save_for_backward(traj, P)
        return frame_outputs(ctx, traj, frames)

    @staticmethod
    def backward(ctx, *grads):
        traj, P = ctx.saved_tensors
        routed = frame_grads(ctx.frames, grads, traj)
        if routed is None:
            return None, None, None, None
        g_traj, mask = routed
        for k, used in enumerate(mask or ()):
            if not used:
                g_traj[k].zero_()
        op = torch.ops.percnn.pi_rollout_ensemble_backward if P.dim() == 2 else torch.ops.percnn.pi_rollout_batched_backward
        g_h0, pg = op(traj, P, g_traj, "")
        return g_h0, pg, None, None


PiRolloutEnsembleFramesFunction = PiRolloutBatchedFramesFunction    # (one node: the rank of P chooses the operator)


def pi_rollout_batched_frames(h0: torch.Tensor, P: torch.Tensor, steps: int, frames: Sequence[int], with_stacked: bool = False):
    out = PiRolloutBatchedFramesFunction.apply(h0, P, int(steps), tuple(frames))
    return out if with_stacked else out[:-1]


def pi_rollout_ensemble_frames(h0: torch.Tensor, P: torch.Tensor, steps: int, frames: Sequence[int], with_stacked: bool = False):
    out = PiRolloutEnsembleFramesFunction.apply(h0, P, int(steps), tuple(frames))
    return out if with_stacked else out[:-1]


def _progression(t_idx: Sequence[int]):
    """(start, step, n) if t_idx is an increasing arithmetic progression (what a slice of range(T+1) gives), else None"""
    n = len(t_idx)
    if n == 0:
        return None
    step = t_idx[1] - t_idx[0] if n > 1 else 1
    if step <= 0 or any(t_idx[i + 1] - t_idx[i] != step for i in range(n - 1)):
        return None
    return t_idx[0], step, n


def _observe(traj: torch.Tensor, t_idx: Sequence[int], sub) -> torch.Tensor:
    """traj[t_idx][:, :, ::s, ...] gathered with ONE strided copy when t_idx is a progression (no index tensor: building
    one is a pageable host-to-device copy that stalls the host)"""
    pr = _progression(t_idx)
    if pr is not None:
        t0, step, n = pr
        return traj[t0:t0 + (n - 1) * step + 1:step][(slice(None),) + sub].contiguous()
    idx = torch.tensor(t_idx, dtype=torch.long, device=traj.device)
    return traj.index_select(0, idx)[(slice(None),) + sub].contiguous()


def _scatter_observed(g_traj: torch.Tensor, t_idx: Sequence[int], sub, g_pred: torch.Tensor):
    """adjoint of _observe into an UNINITIALISED dL/dtraj buffer: only observed frames are written (zero + strided add,
    two launches for a progression); returns the frame mask for the sweep"""
    mask = [False] * g_traj.shape[0]
    pr = _progression(t_idx)
    if pr is not None:
        t0, step, n = pr
        view = g_traj[t0:t0 + (n - 1) * step + 1:step]
        view.zero_()
        view[(slice(None),) + sub].add_(g_pred)
        for t in t_idx:
            mask[t] = True
        return mask
    for i, t in enumerate(t_idx):
        if not mask[t]:
            g_traj[t].zero_()
            mask[t] = True
        g_traj[t][sub] += g_pred[i]
    return mask


class PiRolloutObserveFunction(torch.autograd.Function):
    """Rollout + observation operator in one autograd node: returns ``traj[t_idx][:, :, ::sx, ::sy(, ::sz)]`` -- what the
    reference's training loss looks at (``output[0:-1:20, :, ::4, ::4]``, train_2drd.py:397; ``[:-1:15, :, ::2, ::2, ::2]``,
    train_3drd.py:403).  Going through ``torch.cat(outputs)[...]`` instead makes autograd materialise a dense, almost
    entirely zero dL/dtraj (2 GB at 512^2 x 1000) that the sweep then streams; here the backward fills only the
    observed frames of an uninitialised buffer and masks every other frame out of the sweep."""

    @staticmethod
    def forward(ctx, h0, P, steps, t_idx, strides):
        _check_state(h0)
        P = P.contiguous()
        traj = torch.empty((steps + 1,) + tuple(h0.shape[1:]), dtype=h0.dtype, device=h0.device)
        traj[0].copy_(h0[0])
        rollout_fwd_(traj, P)
        ctx.save_for_backward(traj, P)
        ctx.t_idx = tuple(int(t) % (steps + 1) for t in t_idx)
        ctx.sub = (slice(None),) + tuple(slice(None, None, int(s)) for s in strides)
        pred = _observe(traj, ctx.t_idx, ctx.sub)
        ctx.mark_non_differentiable(traj)
        return pred, traj

    @staticmethod
    def backward(ctx, g_pred, _g_traj_unused):
        traj, P = ctx.saved_tensors
        g_traj = torch.empty_like(traj)                    # never initialised as a whole: unobserved frames are masked
        mask = _scatter_observed(g_traj, ctx.t_idx, ctx.sub, g_pred)
        g_h0, pg = rollout_bwd(traj, g_traj, P, frame_mask=mask)
        return g_h0[None], pg.to(P.dtype), None, None, None


def _options_str(options) -> str:
    b = _lib.options_arg(options)
    return b.decode() if b else ""


def pi_rollout_observe(h0: torch.Tensor, P: torch.Tensor, steps: int, t_idx: Sequence[int], strides: Sequence[int],
                       options=None):
    """-> (pred [len(t_idx), 2, ceil(S/stride)...], traj [steps+1, 2, *S] detached);  torch.ops.percnn.pi_rollout_observe"""
    pred, traj = torch.ops.percnn.pi_rollout_observe(h0, P, int(steps), [int(t) for t in t_idx],
                                                     [int(s) for s in strides], _options_str(options))
    return pred, traj.detach()


def _native():
    """torch.ops.percnn.{pi_step, pi_rollout}: loaded on first use if the package was imported before it was built"""
    from . import ops
    ops.load_native()
    return _lib.torch_ext()


def pi_step(h: torch.Tensor, P: torch.Tensor, options=None) -> torch.Tensor:
    """One fused Pi-block step: the registered operator ``torch.ops.percnn.pi_step`` (csrc/torch_ext.cpp: C++ implementation and
    C++ autograd node, no Python frame between the dispatcher and the C-ABI) -- what a ``torch.compile`` graph holds and what
    eager callers of this function get.  ``RCNNCell.forward`` -- the call a reference-style step loop makes T times per
    iteration -- goes through the library's eager entry points instead (``cell_step`` / ``step_nograd``, same kernels)."""
    _native()
    return torch.ops.percnn.pi_step(h, P, _options_str(options))


def pi_step_nograd(h: torch.Tensor, P: torch.Tensor) -> torch.Tensor:
    """One fused step without an autograd node (inference loops; the caller has checked that nothing records)."""
    return _native().step_nograd(h, P)


def pi_rollout(h0: torch.Tensor, P: torch.Tensor, steps: int, options=None) -> torch.Tensor:
    """T fused steps -> trajectory [T+1,2,*S] through ``torch.ops.percnn.pi_rollout``."""
    _native()
    return torch.ops.percnn.pi_rollout(h0, P, int(steps), _options_str(options))


def pi_step_batched(h: torch.Tensor, P: torch.Tensor, options=None) -> torch.Tensor:
    """One fused step of B independent states [B,2,*S] with ONE parameter block: ``torch.ops.percnn.pi_step_batched`` (batch as a
    grid dimension of the step kernels; sample b bit-identical to ``pi_step`` on that sample alone)."""
    _native()
    return torch.ops.percnn.pi_step_batched(h, P, _options_str(options))


def pi_rollout_batched(h0: torch.Tensor, P: torch.Tensor, steps: int, options=None) -> torch.Tensor:
    """T fused steps of B independent trajectories: h0 [B,2,*S] -> [T+1,B,2,*S] (frame-major; ``.flatten(0, 1)`` is the
    reference's ``torch.cat(tuple(outputs), dim=0)`` of batched frames) through ``torch.ops.percnn.pi_rollout_batched``;
    the parameter gradient is the sum over the samples."""
    _native()
    return torch.ops.percnn.pi_rollout_batched(h0, P, int(steps), _options_str(options))


def pi_step_ensemble(h: torch.Tensor, P: torch.Tensor, options=None) -> torch.Tensor:
    """One fused step of B independent states [B,2,*S], sample b with its own parameter block P[b] (P [B,np], blocks of one
    kind): ``torch.ops.percnn.pi_step_ensemble``; sample b bit-identical to ``pi_step(h[b:b+1], P[b])``."""
    _native()
    return torch.ops.percnn.pi_step_ensemble(h, P, _options_str(options))


def pi_rollout_ensemble(h0: torch.Tensor, P: torch.Tensor, steps: int, options=None) -> torch.Tensor:
    """T fused steps of B independent trajectories, sample b with its own block P[b]: h0 [B,2,*S], P [B,np] -> [T+1,B,2,*S]
    through ``torch.ops.percnn.pi_rollout_ensemble``.  The parameter gradient is [B,np], one row per sample."""
    _native()
    return torch.ops.percnn.pi_rollout_ensemble(h0, P, int(steps), _options_str(options))
