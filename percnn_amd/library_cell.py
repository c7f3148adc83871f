"""Stage-3 cell for ANY equation Stage-2 can return: the hand-over from ``discover()`` to fine-tuning.

The reference writes one ``fine_tuning_*.py`` per discovered equation (2D_Burgers_eqn/Stage-3, 2D_Lambda_Omega_eqn/stage-3);
``Stage3BurgersCell`` / ``Stage3LambdaOmegaCell`` are those two.  ``LibraryCell`` carries one coefficient per entry of the
70-term candidate library and species,

    next_s = h_s + dt * sum_k psi_k * sum_m C[s][m][k] * phi_m        phi: ``discovery._A``,  psi: ``discovery._B``

so ``pa.discover(traj, dx, dt)`` -> ``LibraryCell.from_equations(eqs, dx, dt)`` -> ``pa.RCNN(cell, ...)`` -> fine-tune works
for whatever came out.  One fused launch per step and per adjoint step (``csrc/pi_lib.h``, ``include/percnn_pi_library_cell.h``);
the 140 coefficient gradients are contractions on the float64 matrix cores.  float64, one [1,2,H,W] periodic state, dx = dy.
No CPU path: CPU tensors raise.

``integrator="rk4"`` takes the classical Runge-Kutta step of the reference cells' ``forward_rk4`` instead of the explicit Euler
step: four right-hand sides in one launch forward, one recompute launch and one launch per stage backward.

``LibraryEnsemble`` advances B cells in those same launches: sample b of a [B,2,H,W] state with member b's coefficients, what
batched ``discover()`` returns (``LibraryEnsemble.from_equations``).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .discovery import LIBRARY_TERMS, _A, _B
from .functional import _stream, _assemble_frame_grads, Frame

NCOEF = 140                              # PERCNN_PI_LIB_COEFS
INTEGRATORS = ("euler", "rk4")


def _entry(integrator: str, name: str):
    """the C entry point ``name`` of the step ``integrator`` takes"""
    if integrator not in INTEGRATORS:
        raise ValueError(f"LibraryCell: integrator must be one of {INTEGRATORS}, got {integrator!r}")
    return getattr(_lib.lib(), f"percnn_pi_lib_{'rk4_' if integrator == 'rk4' else ''}{name}")


def _check_state(t: torch.Tensor, name: str, lead) -> None:
    """[lead, 2, H, W] float64 on the device, contiguous, H and W >= 5 (``lead`` None: any leading extent)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"LibraryCell: {name} must be a tensor on the HIP device (there is no CPU path)")
    if t.dtype != torch.float64:
        raise TypeError(f"LibraryCell: {name} must be float64, got {t.dtype}")
    if t.dim() != 4 or t.shape[1] != 2 or (lead is not None and t.shape[0] != lead):
        want = "[1,2,H,W] (one trajectory; B samples go through LibraryEnsemble)" if lead == 1 else "[T+1,2,H,W]"
        raise ValueError(f"LibraryCell: {name} must be {want}, got {tuple(t.shape)}")
    if t.shape[2] < 5 or t.shape[3] < 5:
        raise ValueError(f"LibraryCell: {name} needs H, W >= 5 (radius-2 periodic stencils), got H = {t.shape[2]}, W = {t.shape[3]}")
    if not t.is_contiguous():
        raise ValueError(f"LibraryCell: {name} must be contiguous")


def _check_coef(C: torch.Tensor) -> None:
    if not isinstance(C, torch.Tensor) or not C.is_cuda:
        raise RuntimeError("LibraryCell: coef must be a tensor on the HIP device (there is no CPU path)")
    if C.dtype != torch.float64 or C.numel() != NCOEF or not C.is_contiguous():
        raise ValueError(f"LibraryCell: coef must be contiguous float64 [2,10,7], got {C.dtype} {tuple(C.shape)}")


def step_fwd(h: torch.Tensor, C: torch.Tensor, dx: float, dt: float, out: Optional[torch.Tensor] = None,
             integrator: str = "euler") -> torch.Tensor:
    """h: [1,2,H,W] -> the next state"""
    fn = _entry(integrator, "step_fwd_f64")
    _check_state(h, "h", 1)
    _check_coef(C)
    out = torch.empty_like(h) if out is None else out
    with torch.cuda.device(h.device):
        _lib.check(fn(h.data_ptr(), out.data_ptr(), C.data_ptr(), _lib.shape_arg(h.shape[2:]), float(dx), float(dt), _stream()),
                   "lib_step_fwd")
    return out


def rollout_fwd_(traj: torch.Tensor, C: torch.Tensor, dx: float, dt: float, integrator: str = "euler") -> torch.Tensor:
    """In place: traj[0] holds the initial state, frames 1..T are written.  traj: [T+1,2,H,W]."""
    fn = _entry(integrator, "rollout_fwd_f64")
    _check_state(traj, "traj", None)
    _check_coef(C)
    with torch.cuda.device(traj.device):
        _lib.check(fn(traj.data_ptr(), C.data_ptr(), _lib.shape_arg(traj.shape[2:]), traj.shape[0] - 1, float(dx), float(dt),
                      _stream()), "lib_rollout_fwd")
    return traj


def rollout_bwd(traj: torch.Tensor, g_traj: torch.Tensor, C: torch.Tensor, dx: float, dt: float, frame_mask=None,
                integrator: str = "euler"):
    """-> (dL/dh0 [2,H,W], dL/dC [2,10,7]: all 140 entries, whatever the support)"""
    ws_bytes, fn = _entry(integrator, "rollout_bwd_workspace_bytes"), _entry(integrator, "rollout_bwd_f64")
    _check_state(traj, "traj", None)
    _check_state(g_traj, "g_traj", traj.shape[0])
    if g_traj.shape != traj.shape:
        raise ValueError(f"LibraryCell: g_traj must have the trajectory's shape {tuple(traj.shape)}, got {tuple(g_traj.shape)}")
    _check_coef(C)
    T, shape = traj.shape[0] - 1, traj.shape[2:]
    ws = torch.empty(ws_bytes(_lib.shape_arg(shape), T), dtype=torch.uint8, device=traj.device)
    mask = None
    if frame_mask is not None:
        assert len(frame_mask) == T + 1
        mask = bytes(bytearray(1 if m else 0 for m in frame_mask))
    g_h0 = torch.empty_like(traj[0])
    gC = torch.empty((2, 10, 7), dtype=torch.float64, device=traj.device)
    with torch.cuda.device(traj.device):
        _lib.check(fn(traj.data_ptr(), g_traj.data_ptr(), mask, g_h0.data_ptr(), gC.data_ptr(), ws.data_ptr(), ws.numel(),
                      C.data_ptr(), _lib.shape_arg(shape), T, float(dx), float(dt), _stream()), "lib_rollout_bwd")
        ws.record_stream(torch.cuda.current_stream())
    return g_h0, gC


class LibraryRolloutFramesFunction(torch.autograd.Function):
    """T fused steps with the contract of ``stage1.Stage1RolloutFramesFunction``: the requested [1,2,H,W] frames are views of
    ONE trajectory buffer and outputs of ONE autograd node; the trajectory itself rides along as the last output."""

    @staticmethod
    def forward(ctx, h0, C, dx, dt, steps, frames, integrator="euler"):
        _check_state(h0, "h0", 1)
        C = C.contiguous()
        traj = torch.empty((steps + 1,) + tuple(h0.shape[1:]), dtype=torch.float64, device=h0.device)
        traj[0].copy_(h0[0])
        rollout_fwd_(traj, C, dx, dt, integrator=integrator)
        ctx.save_for_backward(traj, C)
        ctx.dx, ctx.dt, ctx.integrator = dx, dt, integrator
        ctx.frames = tuple(int(k) for k in frames)
        ctx.set_materialize_grads(False)
        views = traj.unsqueeze(1).unbind(0)
        outs = []
        for k in ctx.frames:                                # functional.Frame: the caller's torch.cat(tuple(output)) is a view
            f = views[k].as_subclass(Frame)
            f._pi_index = k
            outs.append(f)
        return tuple(outs) + (traj.view(traj.shape),)

    @staticmethod
    def backward(ctx, *grads):
        traj, C = ctx.saved_tensors
        g_stacked, grads = grads[-1], grads[:-1]
        if g_stacked is None and all(g is None for g in grads):
            return None, None, None, None, None, None, None
        if g_stacked is not None and all(g is None for g in grads):
            g_traj, mask = g_stacked.contiguous(), None
        elif g_stacked is None:
            g_traj, mask = _assemble_frame_grads(grads, ctx.frames, traj)
        else:
            g_traj, mask = g_stacked.clone(), None
            for k, g in zip(ctx.frames, grads):
                if g is not None:
                    g_traj[k].add_(g[0])
        g_h0, gC = rollout_bwd(traj, g_traj, C, ctx.dx, ctx.dt, frame_mask=mask, integrator=ctx.integrator)
        return g_h0[None], gC.reshape(C.shape), None, None, None, None, None


def _term_index(term: str) -> int:
    try:
        return LIBRARY_TERMS.index(term)
    except ValueError:
        raise ValueError(f"LibraryCell: unknown library term {term!r}; the terms are percnn_amd.LIBRARY_TERMS "
                         f"('<monomial>*<factor>', e.g. 'u*u_x', 'ones*lap_v')") from None


class LibraryCell(nn.Module):
    """Physics-based cell over the whole candidate library (module docstring).  ``coefficients``: a [2,10,7] array
    (``C[s][m][k]`` = coefficient of ``LIBRARY_TERMS[7m + k]`` in the equation of species s, physical units -- what
    ``discover()`` returns) .  ``support``: None = the entries that are non-zero now stay trainable, the others stay zero;
    ``"dense"`` = all 140 train; or a [2,10,7] mask.  ``integrator``: ``"euler"`` (the step the reference trains with) or
    ``"rk4"`` (its ``forward_rk4``) -- the step ``cell(h)``, ``rollout`` and ``rollout_frames`` take.
    ``cell(h) -> (ch, ch)`` like the other cells."""

    def __init__(self, coefficients, dx: float, dt: float, support=None, integrator: str = "euler"):
        super().__init__()
        if integrator not in INTEGRATORS:
            raise ValueError(f"LibraryCell: integrator must be one of {INTEGRATORS}, got {integrator!r}")
        self.integrator = integrator
        C = torch.as_tensor(np.asarray(coefficients.detach().cpu() if isinstance(coefficients, torch.Tensor) else coefficients,
                                       dtype=np.float64))
        if tuple(C.shape) != (2, 10, 7):
            raise ValueError(f"LibraryCell: coefficients must be [2,10,7] (species, monomial, factor), got {tuple(C.shape)}")
        if not (np.isfinite(dx) and np.isfinite(dt) and dx > 0 and dt > 0):
            raise ValueError(f"LibraryCell: dx and dt must be positive and finite, got dx = {dx}, dt = {dt}")
        self.coef = nn.Parameter(C.clone())
        if support is None:
            sup = C != 0
        elif isinstance(support, str):
            if support != "dense":
                raise ValueError(f"LibraryCell: support must be None, 'dense' or a [2,10,7] mask, got {support!r}")
            sup = torch.ones(2, 10, 7, dtype=torch.bool)
        else:
            sup = torch.as_tensor(np.asarray(support)) != 0
            if tuple(sup.shape) != (2, 10, 7):
                raise ValueError(f"LibraryCell: support must be [2,10,7], got {tuple(sup.shape)}")
        self.register_buffer("support", sup.to(torch.float64))
        self.dx = self.dy = float(dx)
        self.dt = float(dt)
        self.ndim, self.reaction = 2, "library"

    # ---- equations in, equations out ----------------------------------------------------------------------------------
    @classmethod
    def from_equations(cls, eqs: dict, dx: float, dt: float, support=None, integrator: str = "euler") -> "LibraryCell":
        """``eqs``: one dict as ``discover()`` returns it, ``{"u": {term: coefficient}, "v": {...}}``"""
        if not isinstance(eqs, dict) or set(eqs) - {"u", "v"}:
            raise ValueError(f"LibraryCell.from_equations: eqs must be {{'u': {{term: c}}, 'v': {{term: c}}}} (one sample of "
                             f"discover()), got keys {list(eqs) if isinstance(eqs, dict) else type(eqs).__name__}")
        C = np.zeros((2, 70))
        for s, sp in enumerate("uv"):
            for term, c in eqs.get(sp, {}).items():
                C[s, _term_index(term)] = float(c)
        return cls(C.reshape(2, 10, 7), dx, dt, support=support, integrator=integrator)

    def equations(self) -> dict:
        """the current parameters as ``discover()`` would return them (entries off the support or equal to zero left out)"""
        C = self.param_block().detach().cpu().numpy().reshape(2, 70)
        return {sp: {t: float(c) for t, c in zip(LIBRARY_TERMS, C[s]) if c != 0} for s, sp in enumerate("uv")}

    @classmethod
    def from_cell(cls, cell, integrator: str = "euler") -> "LibraryCell":
        """a ``Stage3BurgersCell`` or ``Stage3LambdaOmegaCell`` as the library cell of the same equation"""
        from .modules import Stage3BurgersCell, Stage3LambdaOmegaCell
        p = lambda n: float(getattr(cell, n).detach())
        if isinstance(cell, Stage3BurgersCell):
            eqs = {"u": {"ones*lap_u": p("nu_u"), "u*u_x": p("C1_u"), "v*u_y": p("C2_u")},
                   "v": {"ones*lap_v": p("nu_v"), "u*v_x": p("C1_v"), "v*v_y": p("C2_v")}}
        elif isinstance(cell, Stage3LambdaOmegaCell):
            cubic = ("u**3*ones", "u**2*v*ones", "u*v**2*ones", "v**3*ones")
            eqs = {"u": {"ones*lap_u": p("nu_u"), "u*ones": p("C1_u"), **{t: p(f"C{i + 2}_u") for i, t in enumerate(cubic)}},
                   "v": {"ones*lap_v": p("nu_v"), "v*ones": p("C1_v"), **{t: p(f"C{i + 2}_v") for i, t in enumerate(cubic)},
                         "u*ones": p("C6_v")}}
        else:
            raise TypeError(f"LibraryCell.from_cell: cell must be a Stage3BurgersCell or a Stage3LambdaOmegaCell, got "
                            f"{type(cell).__name__}")
        # a parameter that happens to be zero stays on the support: the support is the equation's form
        C, sup = np.zeros((2, 70)), np.zeros((2, 70))
        for s, sp in enumerate("uv"):
            for term, c in eqs[sp].items():
                C[s, _term_index(term)], sup[s, _term_index(term)] = c, 1.0
        out = cls(C.reshape(2, 10, 7), cell.dx, cell.dt, support=sup.reshape(2, 10, 7), integrator=integrator)
        return out.to(next(cell.parameters()).device)

    # ---- the cell ---------------------------------------------------------------------------------------------------------
    def param_block(self) -> torch.Tensor:
        """[2,10,7]: ``coef * support`` -- autograd leaves the entries off the support at zero gradient"""
        return self.coef * self.support

    def rollout(self, h0: torch.Tensor, steps: int) -> torch.Tensor:
        """-> [steps+1,2,H,W], frame 0 = h0"""
        return LibraryRolloutFramesFunction.apply(h0, self.param_block(), self.dx, self.dt, int(steps), (), self.integrator)[-1]

    def rollout_frames(self, h0: torch.Tensor, steps: int, frames: Sequence[int], with_stacked: bool = False):
        """hook used by ``percnn_amd.RCNN``: the requested frames as outputs of one autograd node (with_stacked: plus, last, the
        [steps+1,2,H,W] trajectory they are views of)"""
        out = LibraryRolloutFramesFunction.apply(h0, self.param_block(), self.dx, self.dt, int(steps), tuple(frames),
                                                 self.integrator)
        return out if with_stacked else out[:-1]

    def forward(self, h: torch.Tensor):
        ch = self.rollout(h, 1)[1:2]
        return ch, ch

    def forward_rk4(self, h: torch.Tensor):
        """One fused, differentiable Runge-Kutta step whatever ``self.integrator`` is (the reference method's name)"""
        ch = LibraryRolloutFramesFunction.apply(h, self.param_block(), self.dx, self.dt, 1, (), "rk4")[-1][1:2]
        return ch, ch

    def f_rhs(self, u, v):
        """The right-hand side on stock tensor operations ([1,1,H,W] or [H,W] fields, any device): ``(f_u, f_v)``"""
        d = self.dx

        def d1(f, ax):
            return ((torch.roll(f, 2, ax) - torch.roll(f, -2, ax)) + 8.0 * (torch.roll(f, -1, ax) - torch.roll(f, 1, ax))) / (12.0 * d)

        def lap(f):
            return ((-1.0 / 12.0) * ((torch.roll(f, 2, -2) + torch.roll(f, -2, -2)) + (torch.roll(f, 2, -1) + torch.roll(f, -2, -1)))
                    + (4.0 / 3.0) * ((torch.roll(f, 1, -2) + torch.roll(f, -1, -2)) + (torch.roll(f, 1, -1) + torch.roll(f, -1, -1)))
                    - 5.0 * f) / (d * d)

        u2, uv, v2 = u * u, u * v, v * v
        phi = [torch.ones_like(u), u, v, u2, uv, v2, u2 * u, u2 * v, u * v2, v2 * v]
        psi = [torch.ones_like(u), d1(u, -2), d1(u, -1), d1(v, -2), d1(v, -1), lap(u), lap(v)]
        C = self.param_block()
        out = []
        for s in range(2):
            rhs = 0.0
            for k in range(7):
                q = sum(C[s, m, k] * phi[m] for m in range(10))
                rhs = rhs + psi[k] * q
            out.append(rhs)
        return out[0], out[1]

    def init_hidden_tensor(self, prev_state):
        return prev_state.to(self.coef.device)


# ---- ensembles: B equations per launch -----------------------------------------------------------------------------------------
def _ens_entry(integrator: str, name: str):
    """the C entry point ``ensemble_<name>`` of the step ``integrator`` takes"""
    if integrator not in INTEGRATORS:
        raise ValueError(f"LibraryEnsemble: integrator must be one of {INTEGRATORS}, got {integrator!r}")
    return getattr(_lib.lib(), f"percnn_pi_lib_{'rk4_' if integrator == 'rk4' else ''}ensemble_{name}")


def _check_ens_state(t: torch.Tensor, name: str, traj: bool = False) -> None:
    """[B,2,H,W] (``traj``: [T+1,B,2,H,W]) float64 on the device, contiguous, H and W >= 5"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"LibraryEnsemble: {name} must be a tensor on the HIP device (there is no CPU path)")
    if t.dtype != torch.float64:
        raise TypeError(f"LibraryEnsemble: {name} must be float64, got {t.dtype}")
    if t.dim() != (5 if traj else 4) or t.shape[-3] != 2 or t.shape[-4] < 1:
        raise ValueError(f"LibraryEnsemble: {name} must be {'[T+1,B,2,H,W]' if traj else '[B,2,H,W]'} (2D, two species), "
                         f"got {tuple(t.shape)}")
    if t.shape[-2] < 5 or t.shape[-1] < 5:
        raise ValueError(f"LibraryEnsemble: {name} needs H, W >= 5 (radius-2 periodic stencils), got H = {t.shape[-2]}, "
                         f"W = {t.shape[-1]}")
    if not t.is_contiguous():
        raise ValueError(f"LibraryEnsemble: {name} must be contiguous")


def _check_ens_coef(C: torch.Tensor, B: int) -> None:
    if not isinstance(C, torch.Tensor) or not C.is_cuda:
        raise RuntimeError("LibraryEnsemble: coef must be a tensor on the HIP device (there is no CPU path)")
    if C.dtype != torch.float64 or C.dim() < 2 or C.shape[0] != B or C.numel() != B * NCOEF or not C.is_contiguous():
        raise ValueError(f"LibraryEnsemble: coef must be contiguous float64 [B,2,10,7] with B = {B} (one block per sample), got "
                         f"{C.dtype} {tuple(C.shape)}")


def ensemble_step_fwd(h: torch.Tensor, C: torch.Tensor, dx: float, dt: float, out: Optional[torch.Tensor] = None,
                      integrator: str = "euler") -> torch.Tensor:
    """h: [B,2,H,W], C: [B,2,10,7] -> the next states, sample b with block b"""
    fn = _ens_entry(integrator, "step_fwd_f64")
    _check_ens_state(h, "h")
    _check_ens_coef(C, h.shape[0])
    out = torch.empty_like(h) if out is None else out
    with torch.cuda.device(h.device):
        _lib.check(fn(h.data_ptr(), out.data_ptr(), C.data_ptr(), _lib.shape_arg(h.shape[2:]), h.shape[0], float(dx), float(dt),
                      _stream()), "lib_ensemble_step_fwd")
    return out


def ensemble_rollout_fwd_(traj: torch.Tensor, C: torch.Tensor, dx: float, dt: float, integrator: str = "euler") -> torch.Tensor:
    """In place: traj[0] holds the B initial states, frames 1..T are written.  traj: [T+1,B,2,H,W], C: [B,2,10,7]."""
    fn = _ens_entry(integrator, "rollout_fwd_f64")
    _check_ens_state(traj, "traj", traj=True)
    _check_ens_coef(C, traj.shape[1])
    with torch.cuda.device(traj.device):
        _lib.check(fn(traj.data_ptr(), C.data_ptr(), _lib.shape_arg(traj.shape[3:]), traj.shape[1], traj.shape[0] - 1, float(dx),
                      float(dt), _stream()), "lib_ensemble_rollout_fwd")
    return traj


def ensemble_rollout_bwd(traj: torch.Tensor, g_traj: torch.Tensor, C: torch.Tensor, dx: float, dt: float, frame_mask=None,
                         integrator: str = "euler"):
    """-> (dL/dh0 [B,2,H,W], dL/dC [B,2,10,7]: all 140 entries per member, whatever the supports)"""
    ws_bytes, fn = _ens_entry(integrator, "rollout_bwd_workspace_bytes"), _ens_entry(integrator, "rollout_bwd_f64")
    _check_ens_state(traj, "traj", traj=True)
    _check_ens_state(g_traj, "g_traj", traj=True)
    if g_traj.shape != traj.shape:
        raise ValueError(f"LibraryEnsemble: g_traj must have the trajectory's shape {tuple(traj.shape)}, got {tuple(g_traj.shape)}")
    T, B, shape = traj.shape[0] - 1, traj.shape[1], traj.shape[3:]
    _check_ens_coef(C, B)
    ws = torch.empty(ws_bytes(_lib.shape_arg(shape), B, T), dtype=torch.uint8, device=traj.device)
    mask = None
    if frame_mask is not None:
        assert len(frame_mask) == T + 1
        mask = bytes(bytearray(1 if m else 0 for m in frame_mask))
    g_h0 = torch.empty_like(traj[0])
    gC = torch.empty((B, 2, 10, 7), dtype=torch.float64, device=traj.device)
    with torch.cuda.device(traj.device):
        _lib.check(fn(traj.data_ptr(), g_traj.data_ptr(), mask, g_h0.data_ptr(), gC.data_ptr(), ws.data_ptr(), ws.numel(),
                      C.data_ptr(), _lib.shape_arg(shape), B, T, float(dx), float(dt), _stream()), "lib_ensemble_rollout_bwd")
        ws.record_stream(torch.cuda.current_stream())
    return g_h0, gC


class LibraryEnsembleRolloutFramesFunction(torch.autograd.Function):
    """``LibraryRolloutFramesFunction`` for B members with the conventions of ``functional.PiRolloutBatchedFramesFunction``: the
    requested frames are [B,2,H,W] views of ONE [T+1,B,2,H,W] buffer and outputs of ONE autograd node; the LAST output is that
    buffer as [(T+1)*B,2,H,W], what ``torch.cat(tuple(outputs), dim=0)`` of the frames is.  Frames without a gradient are masked
    out of the backward sweep."""

    @staticmethod
    def forward(ctx, h0, C, dx, dt, steps, frames, integrator="euler"):
        _check_ens_state(h0, "h0")
        C = C.contiguous()
        _check_ens_coef(C, h0.shape[0])
        traj = torch.empty((steps + 1,) + tuple(h0.shape), dtype=torch.float64, device=h0.device)
        traj[0].copy_(h0)
        ensemble_rollout_fwd_(traj, C, dx, dt, integrator=integrator)
        ctx.save_for_backward(traj, C)
        ctx.dx, ctx.dt, ctx.integrator = dx, dt, integrator
        ctx.frames = tuple(int(k) for k in frames)
        ctx.set_materialize_grads(False)
        views = traj.unbind(0)
        outs = []
        for k in ctx.frames:
            f = views[k].as_subclass(Frame)
            f._pi_index = k
            outs.append(f)
        return tuple(outs) + (traj.view((-1,) + tuple(traj.shape[2:])),)

    @staticmethod
    def backward(ctx, *grads):
        traj, C = ctx.saved_tensors
        g_stacked, grads = grads[-1], grads[:-1]
        if g_stacked is None and all(g is None for g in grads):
            return None, None, None, None, None, None, None
        mask = None
        if g_stacked is not None:
            g_traj = g_stacked.reshape(traj.shape)
            if any(g is not None for g in grads):
                g_traj = g_traj.clone()
                for k, g in zip(ctx.frames, grads):
                    if g is not None:
                        g_traj[k].add_(g)
        else:
            g_traj, mask = torch.empty_like(traj), [False] * traj.shape[0]
            for k, g in zip(ctx.frames, grads):
                if g is None:
                    continue
                if mask[k]:
                    g_traj[k].add_(g)
                else:
                    g_traj[k].copy_(g)
                    mask[k] = True
        g_h0, gC = ensemble_rollout_bwd(traj, g_traj.contiguous(), C, ctx.dx, ctx.dt, frame_mask=mask, integrator=ctx.integrator)
        return g_h0, gC.reshape(C.shape), None, None, None, None, None


class LibraryEnsemble(nn.Module):
    """B ``LibraryCell``s advanced side by side: sample b of a state [B,2,H,W] runs with member b's 140 coefficients in the
    launches of one trajectory (``csrc/pi_lib.h``: the sample index rides on ``blockIdx.z``) -- what batched ``discover()``
    returns, a parameter study, bootstrap splits, a seed ensemble of fine-tunes.  The members share ``dx``, ``dt``, the
    integrator and the device; their supports may differ.  ``state_dict`` keys are ``cells.<i>.coef`` / ``cells.<i>.support``.
    ``LibraryEnsemble([cell] * B)`` is B initial conditions of one equation: its one parameter receives the sum of the sample
    gradients.  Sample b's trajectory and gradients are bit for bit those of member b run alone.
    ``RCNN(ensemble, step, effective_step, init_state=[B,2,H,W])`` runs B trajectories with B == len(cells).
    Out of scope, refused by name: 3D, float32, a CPU path, per-member dx or dt."""

    def __init__(self, cells):
        super().__init__()
        cells = list(cells)
        if not cells:
            raise ValueError("LibraryEnsemble needs at least one cell")
        for c in cells:
            if not isinstance(c, LibraryCell):
                raise ValueError(f"LibraryEnsemble: {type(c).__name__} is not a LibraryCell (Pi-block cells go into CellEnsemble)")
        for what, get in (("dx", lambda c: c.dx), ("dt", lambda c: c.dt), ("integrator", lambda c: c.integrator),
                          ("device", lambda c: c.coef.device)):
            vals = {get(c) for c in cells}
            if len(vals) != 1:
                raise ValueError(f"LibraryEnsemble: members must share {what} (one launch advances all of them); got "
                                 f"{sorted(map(str, vals))}")
        self.cells = nn.ModuleList(cells)
        self.ndim, self.reaction = 2, "library"

    dx = property(lambda self: self.cells[0].dx)
    dy = property(lambda self: self.cells[0].dy)
    dt = property(lambda self: self.cells[0].dt)
    integrator = property(lambda self: self.cells[0].integrator)

    def __len__(self) -> int:
        return len(self.cells)

    @classmethod
    def from_equations(cls, eqs, dx: float, dt: float, support=None, integrator: str = "euler") -> "LibraryEnsemble":
        """``eqs``: the list of dicts batched ``discover()`` returns, one member per sample"""
        if not isinstance(eqs, (list, tuple)) or not eqs:
            raise ValueError(f"LibraryEnsemble.from_equations: eqs must be a non-empty list of equation dicts (what discover() "
                             f"returns for a batch), got {type(eqs).__name__}")
        return cls([LibraryCell.from_equations(e, dx, dt, support=support, integrator=integrator) for e in eqs])

    def equations(self) -> list:
        """the members' current equations, as batched ``discover()`` would return them"""
        return [c.equations() for c in self.cells]

    def param_block(self) -> torch.Tensor:
        """[B,2,10,7]: the members' ``coef * support`` stacked (differentiable back to each member)"""
        return torch.stack([c.param_block() for c in self.cells])

    def _check_h0(self, h0, name: str = "h0") -> None:
        _check_ens_state(h0, name)
        if h0.shape[0] != len(self.cells):
            raise ValueError(f"LibraryEnsemble: {name} must be [B,2,H,W] with B = len(cells) = {len(self.cells)} (sample b runs "
                             f"with member b), got {tuple(h0.shape)}")

    def rollout(self, h0: torch.Tensor, steps: int) -> torch.Tensor:
        """-> [steps+1,B,2,H,W], frame 0 = h0"""
        self._check_h0(h0)
        out = LibraryEnsembleRolloutFramesFunction.apply(h0, self.param_block(), self.dx, self.dt, int(steps), (), self.integrator)
        return out[-1].view((int(steps) + 1,) + tuple(h0.shape))

    def rollout_frames(self, h0: torch.Tensor, steps: int, frames: Sequence[int], with_stacked: bool = False):
        """hook used by ``percnn_amd.RCNN``: the requested [B,2,H,W] frames as outputs of one autograd node (with_stacked: plus,
        last, the [(steps+1)*B,2,H,W] buffer they are views of)"""
        self._check_h0(h0)
        out = LibraryEnsembleRolloutFramesFunction.apply(h0, self.param_block(), self.dx, self.dt, int(steps), tuple(frames),
                                                         self.integrator)
        return out if with_stacked else out[:-1]

    def forward(self, h: torch.Tensor):
        ch = self.rollout(h, 1)[1]
        return ch, ch

    def init_hidden_tensor(self, prev_state):
        return prev_state.to(self.cells[0].coef.device)
