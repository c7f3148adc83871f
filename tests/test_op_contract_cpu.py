"""CPU: what a user can observe of the twelve ``torch.ops.percnn.pi_*`` operators and of the per-sample loss front ends
WITHOUT a device -- schemas, the texts and the order of the argument checks, the shapes the fake implementations answer
with, and the ``ValueError`` texts the Python layer raises before any device call.  The three flavours (single, batched,
ensemble) share their host code; this file pins what each of them says."""
import pytest
import torch

FLAVOURS = ("", "_batched", "_ensemble")

SCHEMAS = {
    "pi_step": 'percnn::pi_step(Tensor h, Tensor params, str options="") -> Tensor',
    "pi_step_backward": 'percnn::pi_step_backward(Tensor h, Tensor params, Tensor g_out, str options="") -> (Tensor, Tensor)',
    "pi_rollout": 'percnn::pi_rollout(Tensor h0, Tensor params, SymInt steps, str options="") -> Tensor',
    "pi_rollout_backward":
        'percnn::pi_rollout_backward(Tensor traj, Tensor params, Tensor g_traj, str options="") -> (Tensor, Tensor)',
    "pi_step_batched": 'percnn::pi_step_batched(Tensor h, Tensor params, str options="") -> Tensor',
    "pi_step_batched_backward":
        'percnn::pi_step_batched_backward(Tensor h, Tensor params, Tensor g_out, str options="") -> (Tensor, Tensor)',
    "pi_rollout_batched": 'percnn::pi_rollout_batched(Tensor h0, Tensor params, SymInt steps, str options="") -> Tensor',
    "pi_rollout_batched_backward":
        'percnn::pi_rollout_batched_backward(Tensor traj, Tensor params, Tensor g_traj, str options="") -> (Tensor, Tensor)',
    "pi_step_ensemble": 'percnn::pi_step_ensemble(Tensor h, Tensor params, str options="") -> Tensor',
    "pi_step_ensemble_backward":
        'percnn::pi_step_ensemble_backward(Tensor h, Tensor params, Tensor g_out, str options="") -> (Tensor, Tensor)',
    "pi_rollout_ensemble": 'percnn::pi_rollout_ensemble(Tensor h0, Tensor params, SymInt steps, str options="") -> Tensor',
    "pi_rollout_ensemble_backward":
        'percnn::pi_rollout_ensemble_backward(Tensor traj, Tensor params, Tensor g_traj, str options="") -> (Tensor, Tensor)',
}


@pytest.fixture(scope="module")
def ns():
    from percnn_amd import ops
    ops.load_native()
    return torch.ops.percnn


def _state(fl, *spatial, **kw):
    return torch.zeros((1 if fl == "" else 2, 2) + (spatial or (8, 8)), **kw)


def _block(fl, n=36, **kw):
    return torch.zeros((2, n) if fl == "_ensemble" else (n,), **kw)


def _traj(fl, h, T1):
    return h.new_zeros((T1,) + tuple(h.shape[1:] if fl == "" else h.shape))


def _calls(ns, fl, h, P, steps=3):
    """(operator name, thunk, name of its state argument) of the four operators of one flavour"""
    traj = _traj(fl, h, steps + 1)
    return [(f"pi_step{fl}", lambda: getattr(ns, f"pi_step{fl}")(h, P), "h"),
            (f"pi_step{fl}_backward", lambda: getattr(ns, f"pi_step{fl}_backward")(h, P, h), "h"),
            (f"pi_rollout{fl}", lambda: getattr(ns, f"pi_rollout{fl}")(h, P, steps), "h0"),
            (f"pi_rollout{fl}_backward", lambda: getattr(ns, f"pi_rollout{fl}_backward")(traj, P, traj), "traj")]


def test_schemas_are_the_documented_ones(ns):
    assert len(SCHEMAS) == 12
    for name, schema in SCHEMAS.items():
        assert str(getattr(ns, name).default._schema) == schema


def test_dispatch_keys_of_every_operator(ns):
    for name in SCHEMAS:
        for key in ("CUDA", "CPU"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"percnn::{name}", key), (name, key)
        # the forward operators carry the C++ autograd formula, the backward operators none
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"percnn::{name}", "Autograd") == (not name.endswith("_backward"))


@pytest.mark.parametrize("fl", FLAVOURS)
def test_cpu_tensors_get_the_package_message_naming_the_state(ns, fl):
    for name, call, arg in _calls(ns, fl, _state(fl), _block(fl)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert f"percnn_amd: {arg} must live on a HIP device (got cpu); there is no CPU path" in str(e.value), name


@pytest.mark.parametrize("fl", FLAVOURS)
def test_cpu_tensors_under_autograd_get_the_same_message(ns, fl):
    h, P = _state(fl).requires_grad_(True), _block(fl).requires_grad_(True)
    for name, call, arg in _calls(ns, fl, h, P):
        with pytest.raises(RuntimeError) as e:
            call()
        assert f"percnn_amd: {arg} must live on a HIP device (got cpu); there is no CPU path" in str(e.value), name


@pytest.mark.parametrize("fl", FLAVOURS)
def test_wrong_state_shape_is_refused_before_the_device_check(ns, fl):
    if fl == "":
        bad = [torch.zeros(2, 2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8)]
        text = "percnn_amd: state must be [1,2,*S] (batch 1, two species), got "
    else:
        bad = [torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 8), torch.zeros(2, 2, 4, 4, 4, 4)]
        text = "percnn_amd: batched state must be [B,2,*S] (two species), got "
    for h in bad:
        for name, call, _ in _calls(ns, fl, h, _block(fl))[:3]:      # (the rollout backward looks at the device of traj first)
            with pytest.raises(RuntimeError) as e:
                call()
            assert text + str(list(h.shape)) in str(e.value), name


@pytest.mark.parametrize("fl", FLAVOURS)
def test_device_check_comes_before_steps_and_block_checks(ns, fl):
    """`steps must be >= 0`, the ensemble's [B,np] check and the block-length message all come after require(h):
    with CPU tensors the device message wins."""
    h = _state(fl)
    for P, steps in ((_block(fl), -1), (torch.zeros(3, 36), 3), (torch.zeros(37), 3)):
        with pytest.raises(RuntimeError, match="h0 must live on a HIP device"):
            getattr(ns, f"pi_rollout{fl}")(h, P, steps)
        with pytest.raises(RuntimeError, match="h must live on a HIP device"):
            getattr(ns, f"pi_step{fl}_backward")(h, P, h)


@pytest.mark.parametrize("spatial", [(8, 12), (4, 6, 8)], ids=["2d", "3d"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_fake_implementations_answer_with_the_operators_shapes(ns, fl, dtype, spatial):
    from torch._subclasses.fake_tensor import FakeTensorMode
    steps = 3
    with FakeTensorMode():
        h = _state(fl, *spatial, dtype=dtype, device="cuda")
        for n in (36, 16 + 2 * 21):
            P = _block(fl, n, dtype=dtype, device="cuda")
            traj_shape = (steps + 1,) + tuple(h.shape[1:] if fl == "" else h.shape)
            out = getattr(ns, f"pi_step{fl}")(h, P)
            g_in, pg = getattr(ns, f"pi_step{fl}_backward")(h, P, h)
            traj = getattr(ns, f"pi_rollout{fl}")(h, P, steps)
            g_h0, pg_r = getattr(ns, f"pi_rollout{fl}_backward")(traj, P, traj)
            assert out.shape == h.shape and g_in.shape == h.shape and g_h0.shape == h.shape
            assert tuple(traj.shape) == traj_shape
            assert pg.shape == P.shape and pg_r.shape == P.shape
            for t in (out, g_in, pg, traj, g_h0, pg_r):
                assert t.dtype == dtype and t.device.type == "cuda" and t.is_contiguous()
        # a non-contiguous state: the step answers contiguous
        hp = h.transpose(-1, -2)
        assert not hp.is_contiguous()
        P = _block(fl, dtype=dtype, device="cuda")
        assert getattr(ns, f"pi_step{fl}")(hp, P).is_contiguous()
        assert getattr(ns, f"pi_step{fl}_backward")(hp, P, hp)[0].is_contiguous()
        assert tuple(getattr(ns, f"pi_rollout{fl}")(h, P, 0).shape) == (1,) + traj_shape[1:]


def test_fake_ensemble_checks_blocks_against_the_batch(ns):
    from torch._subclasses.fake_tensor import FakeTensorMode
    text = "percnn_amd: ensemble parameter blocks must be [B,np] with B = 2, got (3, 36)"
    with FakeTensorMode():
        h = torch.empty(2, 2, 8, 8, device="cuda")
        traj = torch.empty(4, 2, 2, 8, 8, device="cuda")
        P = torch.empty(3, 36, device="cuda")
        for call in (lambda: ns.pi_step_ensemble(h, P), lambda: ns.pi_step_ensemble_backward(h, P, h),
                     lambda: ns.pi_rollout_ensemble(h, P, 3), lambda: ns.pi_rollout_ensemble_backward(traj, P, traj)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert text in str(e.value)
        # the batched and single fakes do not look at the block's rank
        assert ns.pi_step_batched(h, P).shape == h.shape
        assert ns.pi_rollout_batched_backward(traj, P, traj)[1].shape == (3, 36)


# ---- the Python layer: per-sample losses, refused before any device call ------------------------------------------------
def _msg(fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    return str(e.value)


def test_dense_loss_front_ends_value_errors():
    import percnn_amd.functional as F
    h0, P1, P2 = torch.zeros(2, 2, 8, 8), torch.zeros(36), torch.zeros(2, 36)
    tgt = torch.zeros(3, 2, 2, 8, 8)
    b, e = F.pi_rollout_sqerr_batched, F.pi_rollout_sqerr_ensemble
    # rank of P
    assert _msg(b, h0, P2, 2) == "pi_rollout_sqerr_batched: one parameter block [np], got (2, 36)"
    assert _msg(e, h0, P1, 2) == "pi_rollout_sqerr_ensemble: one parameter block per sample [B,np], got (36,)"
    assert _msg(e, h0, torch.zeros(3, 36), 2) == "pi_rollout_sqerr_ensemble: one parameter block per sample [B,np], got (3, 36)"
    # rank of h0
    assert _msg(b, h0[0], P1, 2) == "pi_rollout_sqerr_batched: h0 must be [B,2,*S], got (2, 8, 8)"
    assert _msg(e, h0[0], P2, 2) == "pi_rollout_sqerr_ensemble: h0 must be [B,2,*S], got (2, 8, 8)"
    assert _msg(b, torch.zeros(2, 3, 8, 8), P1, 2) == "pi_rollout_sqerr_batched: h0 must be [B,2,*S], got (2, 3, 8, 8)"
    # target
    for fn, P in ((b, P1), (e, P2)):
        assert _msg(fn, h0, P, 2, tgt[:2]) == "target must have the trajectory's shape [steps + 1, B, 2, *S]"
        assert _msg(fn, h0, P, 2, tgt[:, :1]) == "target must have the trajectory's shape [steps + 1, B, 2, *S]"
    # empty selection (checked before the target)
    assert _msg(b, h0, P1, 2, tgt[:2], frames=[]) == "pi_rollout_sqerr_batched: no frame selected"
    assert _msg(e, h0, P2, 2, None, frames=()) == "pi_rollout_sqerr_ensemble: no frame selected"
    # the rank of P is looked at first, h0 second
    assert _msg(b, h0[0], P2, 2, frames=[]) == "pi_rollout_sqerr_batched: one parameter block [np], got (2, 36)"
    assert _msg(b, h0[0], P1, 2, frames=[]) == "pi_rollout_sqerr_batched: h0 must be [B,2,*S], got (2, 8, 8)"


def test_observed_loss_front_ends_value_errors():
    import percnn_amd.functional as F
    h0, P1, P2 = torch.zeros(2, 2, 8, 8), torch.zeros(36), torch.zeros(2, 36)
    b, e = F.pi_rollout_obs_sqerr_batched, F.pi_rollout_obs_sqerr_ensemble
    assert _msg(b, h0, P2, 4, None, [0, 2], 2) == "pi_rollout_obs_sqerr_batched: one parameter block [np], got (2, 36)"
    assert _msg(e, h0, P1, 4, None, [0, 2], 2) == "pi_rollout_obs_sqerr_ensemble: one parameter block per sample [B,np], got (36,)"
    assert _msg(b, h0[0], P1, 4, None, [0, 2], 2) == "pi_rollout_obs_sqerr_batched: h0 must be [B,2,*S], got (2, 8, 8)"
    assert _msg(e, h0[0], P2, 4, None, [0, 2], 2) == "pi_rollout_obs_sqerr_ensemble: h0 must be [B,2,*S], got (2, 8, 8)"
    for fn, P, what in ((b, P1, "pi_rollout_obs_sqerr_batched"), (e, P2, "pi_rollout_obs_sqerr_ensemble")):
        assert (_msg(fn, h0, P, 4, torch.zeros(2, 2, 2, 8, 8), [0, 2], 2) ==
                f"{what}: target must be [n, B, 2, *ceil(S / s)] = (2, 2, 2, 4, 4), got (2, 2, 2, 8, 8)")
        assert (_msg(fn, h0, P, 4, torch.zeros(3, 2, 2, 2, 3), [0, 2, -1], (3, 3)) ==
                f"{what}: target must be [n, B, 2, *ceil(S / s)] = (3, 2, 2, 3, 3), got (3, 2, 2, 2, 3)")
        assert _msg(fn, h0, P, 4, None, [], 2) == f"{what}: no frame selected"
        assert _msg(fn, h0, P, 4, None, [2, 1], 2) == f"{what}: t_idx must be strictly increasing, got [2, 1]"
        assert _msg(fn, h0, P, 4, None, [0, 2], (2,)) == f"{what}: one stride per axis of (8, 8), got (2,)"
        assert _msg(fn, h0, P, 4, None, [0, 2], (2, 0)) == f"{what}: strides must be >= 1, got (2, 0)"


def test_obs_selection_texts_and_values():
    from percnn_amd.functional import obs_selection
    assert _msg(obs_selection, 4, [], 2, (8, 8)) == "pi_rollout_obs_sqerr: no frame selected"
    assert _msg(obs_selection, 4, [1, 1], 2, (8, 8)) == "pi_rollout_obs_sqerr: t_idx must be strictly increasing, got [1, 1]"
    assert _msg(obs_selection, 4, [0, -1, 2], 2, (8, 8)) == "pi_rollout_obs_sqerr: t_idx must be strictly increasing, got [0, -1, 2]"
    assert _msg(obs_selection, 4, [0], (2, 2, 2), (8, 8)) == "pi_rollout_obs_sqerr: one stride per axis of (8, 8), got (2, 2, 2)"
    assert _msg(obs_selection, 4, [0], (0, 2), (8, 8), "mean", "w") == "w: strides must be >= 1, got (0, 2)"
    sel, mask, strides, Sc, weight = obs_selection(4, [0, 2, -1], 3, (8, 10))
    assert (sel, mask, strides, Sc) == ([0, 2, 4], [True, False, True, False, True], (3, 3), (3, 4))
    assert weight == 1.0 / (3 * 2 * 3 * 4)
    assert obs_selection(1, [0, 1], (1, 2), (8, 10), "sum")[1:] == (None, (1, 2), (8, 5), 1.0)


def test_sweep_calls_refuse_a_block_of_the_wrong_rank_by_name():
    """``rollout_bwd_*_batched`` name their own ``ValueError``s; those for tensors off the device come first (``_require``)."""
    import percnn_amd.functional as F
    traj, P = torch.zeros(3, 2, 2, 8, 8), torch.zeros(2, 36)
    for fn in (F.traj_sqerr_batched, F.traj_obs_sqerr_batched):
        with pytest.raises(RuntimeError, match=r"percnn_amd: traj must live on a HIP device \(got cpu\); there is no CPU path"):
            fn(traj)
    for fn in (F.rollout_bwd_sqerr_batched, F.rollout_bwd_obs_sqerr_batched):
        with pytest.raises(RuntimeError, match=r"percnn_amd: traj must live on a HIP device \(got cpu\); there is no CPU path"):
            fn(traj, P)


def test_public_names_and_signatures_stay():
    import inspect
    import percnn_amd.functional as F
    sig = lambda f: str(inspect.signature(f)).replace("typing.", "")
    assert sig(F.traj_sqerr_batched) == (
        "(traj: 'torch.Tensor', target: 'Optional[torch.Tensor]' = None, frame_mask: 'Optional[Sequence[bool]]' = None, "
        "scale: 'float' = 1.0) -> 'torch.Tensor'")
    assert sig(F.traj_obs_sqerr_batched) == (
        "(traj: 'torch.Tensor', target: 'Optional[torch.Tensor]' = None, frame_mask: 'Optional[Sequence[bool]]' = None, "
        "strides: 'Sequence[int]' = (), scale: 'float' = 1.0) -> 'torch.Tensor'")
    assert sig(F.rollout_bwd_sqerr_batched) == (
        "(traj: 'torch.Tensor', P: 'torch.Tensor', target: 'Optional[torch.Tensor]' = None, "
        "frame_mask: 'Optional[Sequence[bool]]' = None, scale: 'float' = 1.0, dev_scale: 'Optional[torch.Tensor]' = None, "
        "ws: 'Optional[torch.Tensor]' = None, options=None, g_h0: 'Optional[torch.Tensor]' = None)")
    assert sig(F.rollout_bwd_obs_sqerr_batched) == (
        "(traj: 'torch.Tensor', P: 'torch.Tensor', target: 'Optional[torch.Tensor]' = None, "
        "frame_mask: 'Optional[Sequence[bool]]' = None, strides: 'Sequence[int]' = (), scale: 'float' = 1.0, "
        "dev_scale: 'Optional[torch.Tensor]' = None, ws: 'Optional[torch.Tensor]' = None, options=None, "
        "g_h0: 'Optional[torch.Tensor]' = None, ensemble: 'Optional[bool]' = None)")
    for name in ("pi_rollout_sqerr_batched", "pi_rollout_sqerr_ensemble"):
        assert sig(getattr(F, name)) == (
            "(h0: 'torch.Tensor', P: 'torch.Tensor', steps: 'int', target: 'Optional[torch.Tensor]' = None, "
            "frames: 'Optional[Sequence[int]]' = None, reduction: 'str' = 'mean', options=None)")
    for name in ("pi_rollout_obs_sqerr_batched", "pi_rollout_obs_sqerr_ensemble"):
        assert sig(getattr(F, name)) == (
            "(h0: 'torch.Tensor', P: 'torch.Tensor', steps: 'int', target: 'Optional[torch.Tensor]', t_idx: 'Sequence[int]', "
            "strides, reduction: 'str' = 'mean', options=None)")
    for name in ("pi_rollout_batched_frames", "pi_rollout_ensemble_frames"):
        assert sig(getattr(F, name)) == (
            "(h0: 'torch.Tensor', P: 'torch.Tensor', steps: 'int', frames: 'Sequence[int]', with_stacked: 'bool' = False)")
    for name in ("PiRolloutSqErrBatchedFunction", "PiRolloutObsSqErrBatchedFunction", "PiRolloutBatchedFramesFunction",
                 "PiRolloutEnsembleFramesFunction"):
        assert issubclass(getattr(F, name), torch.autograd.Function)
    for name in ("traj_sqerr_batched", "traj_obs_sqerr_batched", "rollout_bwd_sqerr_batched", "rollout_bwd_obs_sqerr_batched",
                 "pi_rollout_sqerr_batched", "pi_rollout_sqerr_ensemble", "pi_rollout_obs_sqerr_batched",
                 "pi_rollout_obs_sqerr_ensemble"):
        assert getattr(F, name).__doc__
