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
from .functional import _stream, _mask_bytes, frame_outputs, frame_grads

NCOEF = 140                              # PERCNN_PI_LIB_COEFS
INTEGRATORS = ("euler", "rk4")


# ---- host path: one body per call; ``ens`` = the ensemble flavour (a sample axis B after the frame axis, one block per sample) --
_WHO = {False: "LibraryCell", True: "LibraryEnsemble"}
_WANT = {(False, False): "[1,2,H,W] (one trajectory; B samples go through LibraryEnsemble)", (False, True): "[T+1,2,H,W]",
         (True, False): "[B,2,H,W] (2D, two species)", (True, True): "[T+1,B,2,H,W] (2D, two species)"}


def _entry(integrator: str, name: str, ens: bool = False):
    """the C entry point ``[ensemble_]<name>`` of the step ``integrator`` takes"""
    if integrator not in INTEGRATORS:
        raise ValueError(f"{_WHO[ens]}: integrator must be one of {INTEGRATORS}, got {integrator!r}")
    return getattr(_lib.lib(), f"percnn_pi_lib_{'rk4_' if integrator == 'rk4' else ''}{'ensemble_' if ens else ''}{name}")


def _check_state(t: torch.Tensor, name: str, ens: bool, traj: bool = False) -> None:
    """[1,2,H,W] / [B,2,H,W] (``traj``: [T+1,2,H,W] / [T+1,B,2,H,W]) float64 on the device, contiguous, H and W >= 5"""
    who = _WHO[ens]
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be a tensor on the HIP device (there is no CPU path)")
    if t.dtype != torch.float64:
        raise TypeError(f"{who}: {name} must be float64, got {t.dtype}")
    if ens:
        ok = t.dim() == (5 if traj else 4) and t.shape[-3] == 2 and t.shape[-4] >= 1
    else:
        ok = t.dim() == 4 and t.shape[1] == 2 and (traj or t.shape[0] == 1)
    if not ok:
        raise ValueError(f"{who}: {name} must be {_WANT[ens, traj]}, got {tuple(t.shape)}")
    if t.shape[-2] < 5 or t.shape[-1] < 5:
        raise ValueError(f"{who}: {name} needs H, W >= 5 (radius-2 periodic stencils), got H = {t.shape[-2]}, W = {t.shape[-1]}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")


def _check_coef(C: torch.Tensor, B: Optional[int] = None) -> None:
    """[2,10,7], or with ``B`` (the ensemble flavour) [B,2,10,7]: float64 on the device, contiguous"""
    who = _WHO[B is not None]
    if not isinstance(C, torch.Tensor) or not C.is_cuda:
        raise RuntimeError(f"{who}: coef must be a tensor on the HIP device (there is no CPU path)")
    ok = C.dtype == torch.float64 and C.is_contiguous() and C.numel() == (1 if B is None else B) * NCOEF
    if not ok or (B is not None and (C.dim() < 2 or C.shape[0] != B)):
        want = "[2,10,7]" if B is None else f"[B,2,10,7] with B = {B} (one block per sample)"
        raise ValueError(f"{who}: coef must be contiguous float64 {want}, got {C.dtype} {tuple(C.shape)}")


def _step_fwd(ens, h, C, dx, dt, out, integrator):
    fn = _entry(integrator, "step_fwd_f64", ens)
    _check_state(h, "h", ens)
    B = (h.shape[0],) if ens else ()                        # (the single entry points take no B)
    _check_coef(C, *B)
    out = torch.empty_like(h) if out is None else out
    with torch.cuda.device(h.device):
        _lib.check(fn(h.data_ptr(), out.data_ptr(), C.data_ptr(), _lib.shape_arg(h.shape[2:]), *B, float(dx), float(dt), _stream()),
                   f"lib_{'ensemble_' if ens else ''}step_fwd")
    return out


def _rollout_fwd_(ens, traj, C, dx, dt, integrator):
    fn = _entry(integrator, "rollout_fwd_f64", ens)
    _check_state(traj, "traj", ens, traj=True)
    B = (traj.shape[1],) if ens else ()
    _check_coef(C, *B)
    with torch.cuda.device(traj.device):
        _lib.check(fn(traj.data_ptr(), C.data_ptr(), _lib.shape_arg(traj.shape[-2:]), *B, traj.shape[0] - 1, float(dx), float(dt),
                      _stream()), f"lib_{'ensemble_' if ens else ''}rollout_fwd")
    return traj


def _rollout_bwd(ens, traj, g_traj, C, dx, dt, frame_mask, integrator):
    ws_bytes, fn = _entry(integrator, "rollout_bwd_workspace_bytes", ens), _entry(integrator, "rollout_bwd_f64", ens)
    _check_state(traj, "traj", ens, traj=True)
    _check_state(g_traj, "g_traj", ens, traj=True)
    if g_traj.shape != traj.shape:
        raise ValueError(f"{_WHO[ens]}: g_traj must have the trajectory's shape {tuple(traj.shape)}, got {tuple(g_traj.shape)}")
    B = (traj.shape[1],) if ens else ()
    _check_coef(C, *B)
    T, shape = traj.shape[0] - 1, _lib.shape_arg(traj.shape[-2:])
    ws = torch.empty(ws_bytes(shape, *B, T), dtype=torch.uint8, device=traj.device)
    g_h0 = torch.empty_like(traj[0])
    gC = torch.empty(B + (2, 10, 7), dtype=torch.float64, device=traj.device)
    with torch.cuda.device(traj.device):
        _lib.check(fn(traj.data_ptr(), g_traj.data_ptr(), _mask_bytes(frame_mask, T + 1), g_h0.data_ptr(), gC.data_ptr(),
                      ws.data_ptr(), ws.numel(), C.data_ptr(), shape, *B, T, float(dx), float(dt), _stream()),
                   f"lib_{'ensemble_' if ens else ''}rollout_bwd")
        ws.record_stream(torch.cuda.current_stream())
    return g_h0, gC


def step_fwd(h: torch.Tensor, C: torch.Tensor, dx: float, dt: float, out: Optional[torch.Tensor] = None,
             integrator: str = "euler") -> torch.Tensor:
    """h: [1,2,H,W] -> the next state"""
    return _step_fwd(False, h, C, dx, dt, out, integrator)


def rollout_fwd_(traj: torch.Tensor, C: torch.Tensor, dx: float, dt: float, integrator: str = "euler") -> torch.Tensor:
    """In place: traj[0] holds the initial state, frames 1..T are written.  traj: [T+1,2,H,W]."""
    return _rollout_fwd_(False, traj, C, dx, dt, integrator)


def rollout_bwd(traj: torch.Tensor, g_traj: torch.Tensor, C: torch.Tensor, dx: float, dt: float, frame_mask=None,
                integrator: str = "euler"):
    """-> (dL/dh0 [2,H,W], dL/dC [2,10,7]: all 140 entries, whatever the support)"""
    return _rollout_bwd(False, traj, g_traj, C, dx, dt, frame_mask, integrator)


def ensemble_step_fwd(h: torch.Tensor, C: torch.Tensor, dx: float, dt: float, out: Optional[torch.Tensor] = None,
                      integrator: str = "euler") -> torch.Tensor:
    """h: [B,2,H,W], C: [B,2,10,7] -> the next states, sample b with block b"""
    return _step_fwd(True, h, C, dx, dt, out, integrator)


def ensemble_rollout_fwd_(traj: torch.Tensor, C: torch.Tensor, dx: float, dt: float, integrator: str = "euler") -> torch.Tensor:
    """In place: traj[0] holds the B initial states, frames 1..T are written.  traj: [T+1,B,2,H,W], C: [B,2,10,7]."""
    return _rollout_fwd_(True, traj, C, dx, dt, integrator)


def ensemble_rollout_bwd(traj: torch.Tensor, g_traj: torch.Tensor, C: torch.Tensor, dx: float, dt: float, frame_mask=None,
                         integrator: str = "euler"):
    """-> (dL/dh0 [B,2,H,W], dL/dC [B,2,10,7]: all 140 entries per member, whatever the supports)"""
    return _rollout_bwd(True, traj, g_traj, C, dx, dt, frame_mask, integrator)


class LibraryRolloutFramesFunction(torch.autograd.Function):
    """T fused steps with the contract of ``functional.PiRolloutFramesFunction`` / ``PiRolloutBatchedFramesFunction``: the
    requested frames are views of ONE trajectory buffer and outputs of ONE autograd node; the buffer itself rides along as the
    last output.  The rank of C chooses the flavour -- [2,10,7]: one trajectory, h0 and frames [1,2,H,W], last output
    [T+1,2,H,W]; [B,2,10,7]: B members, h0 and frames [B,2,H,W], last output [(T+1)*B,2,H,W].  Frames without a gradient are
    masked out of the backward sweep."""

    @staticmethod
    def forward(ctx, h0, C, dx, dt, steps, frames, integrator="euler"):
        ens = C.dim() == 4
        _check_state(h0, "h0", ens)
        C = C.contiguous()
        buf = torch.empty((steps + 1,) + tuple(h0.shape), dtype=torch.float64, device=h0.device)    # [T+1,R,2,H,W], R = 1 or B
        buf[0].copy_(h0)
        _rollout_fwd_(ens, buf if ens else buf.squeeze(1), C, dx, dt, integrator)
        ctx.save_for_backward(buf, C)
        ctx.dx, ctx.dt, ctx.integrator = dx, dt, integrator
        return frame_outputs(ctx, buf, frames)

    @staticmethod
    def backward(ctx, *grads):
        buf, C = ctx.saved_tensors
        routed = frame_grads(ctx.frames, grads, buf)
        if routed is None:
            return None, None, None, None, None, None, None
        ens = C.dim() == 4
        traj, g_traj = (buf, routed[0]) if ens else (buf.squeeze(1), routed[0].squeeze(1))
        g_h0, gC = _rollout_bwd(ens, traj, g_traj, C, ctx.dx, ctx.dt, routed[1], ctx.integrator)
        return g_h0.view(buf.shape[1:]), gC.reshape(C.shape), None, None, None, None, None


LibraryEnsembleRolloutFramesFunction = LibraryRolloutFramesFunction    # (one node: the rank of C chooses the entry points)


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
        _check_state(h0, name, True)
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
