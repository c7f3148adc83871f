"""GPU: the argument checks of the twelve ``torch.ops.percnn.pi_*`` operators that need HIP tensors to be reached -- every
refusal here is raised before a launch of the package's kernels -- and, per operator, the shape / dtype / contiguity of what it
returns.  8x8 grids, B = 2, T = 2, both dtypes."""
import numpy as np
import pytest
import torch

from util import bits_equal, random_block

pytestmark = pytest.mark.gpu

FLAVOURS = ("", "_batched", "_ensemble")
DTYPES = [torch.float32, torch.float64]
B, T, S = 2, 2, (8, 8)


@pytest.fixture(scope="module")
def ns():
    from percnn_amd import ops
    ops.load_native()
    return torch.ops.percnn


def _np(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def _state(fl, dtype, dev, shape=S):
    rs = np.random.RandomState(3)
    return torch.from_numpy((0.2 + 0.3 * rs.rand(1 if fl == "" else B, 2, *shape)).astype(_np(dtype))).to(dev)


def _block(fl, dtype, dev, hc=0, ndim=2):
    if fl == "_ensemble":
        return torch.from_numpy(np.stack([random_block(hc, ndim, _np(dtype), 11 + b, scale=0.1) for b in range(B)])).to(dev)
    return torch.from_numpy(random_block(hc, ndim, _np(dtype), 11, scale=0.1)).to(dev)


def _zeros_block(fl, n, dtype, dev, rows=B):
    return torch.zeros((rows, n) if fl == "_ensemble" else (n,), dtype=dtype, device=dev)


def _traj_like(fl, h, T1=T + 1):
    return h.new_zeros((T1,) + tuple(h.shape[1:] if fl == "" else h.shape))


def _four(ns, fl, h, P, traj=None, g=None, g_traj=None):
    traj = _traj_like(fl, h) if traj is None else traj
    g = h if g is None else g
    g_traj = traj if g_traj is None else g_traj
    return [(f"pi_step{fl}", lambda: getattr(ns, f"pi_step{fl}")(h, P)),
            (f"pi_step{fl}_backward", lambda: getattr(ns, f"pi_step{fl}_backward")(h, P, g)),
            (f"pi_rollout{fl}", lambda: getattr(ns, f"pi_rollout{fl}")(h, P, T)),
            (f"pi_rollout{fl}_backward", lambda: getattr(ns, f"pi_rollout{fl}_backward")(traj, P, g_traj))]


def _raises(call, text, name=""):
    with pytest.raises(RuntimeError) as e:
        call()
    assert text in str(e.value), (name, str(e.value).splitlines()[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_ensemble_blocks_are_checked_against_the_batch(ns, hip_device, dtype):
    h = _state("_ensemble", dtype, hip_device)
    P = _zeros_block("_ensemble", 36, dtype, hip_device, rows=3)
    for name, call in _four(ns, "_ensemble", h, P):
        _raises(call, "percnn_amd: ensemble parameter blocks must be [B,np] with B = 2 (the state's batch size), got [3, 36]", name)
    for name, call in _four(ns, "_ensemble", h, P[0]):
        _raises(call, "percnn_amd: ensemble parameter blocks must be [B,np] with B = 2 (the state's batch size), got [36]", name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_advective_blocks_have_no_ensemble_path(ns, hip_device, dtype):
    h = _state("_ensemble", dtype, hip_device)
    for name, call in _four(ns, "_ensemble", h, _zeros_block("_ensemble", 60, dtype, hip_device)):
        _raises(call, "percnn_amd: the advective block has no ensemble path", name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_advective_block_is_refused_by_the_library(ns, hip_device, dtype):
    h = _state("_batched", dtype, hip_device)
    P = _zeros_block("_batched", 60, dtype, hip_device)
    calls = dict(_four(ns, "_batched", h, P))
    _raises(calls["pi_step_batched"], "percnn_amd: batch_step_fwd failed: invalid argument")
    _raises(calls["pi_rollout_batched"], "percnn_amd: batch_rollout_fwd failed: invalid argument")
    for name in ("pi_step_batched_backward", "pi_rollout_batched_backward"):
        _raises(calls[name], "percnn_amd: invalid batched problem (shape, batch size or block kind)", name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fl", FLAVOURS)
def test_malformed_block_length(ns, hip_device, fl, dtype):
    h = _state(fl, dtype, hip_device)
    for n in (37, 20):
        for name, call in _four(ns, fl, h, _zeros_block(fl, n, dtype, hip_device)):
            _raises(call, f"percnn_amd: parameter block has {n} entries; expected 16 + 2*(10*hc+1)", name)
    if fl != "_ensemble":                                    # a stack of blocks where one block belongs
        for name, call in _four(ns, fl, h, torch.zeros(2, 36, dtype=dtype, device=hip_device)):
            _raises(call, "percnn_amd: parameter block has 72 entries; expected 16 + 2*(10*hc+1)", name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fl", FLAVOURS)
def test_negative_steps_and_mismatched_dtypes(ns, hip_device, fl, dtype):
    h, P = _state(fl, dtype, hip_device), _block(fl, dtype, hip_device)
    _raises(lambda: getattr(ns, f"pi_rollout{fl}")(h, P, -1), "percnn_amd: steps must be >= 0")
    other = torch.float64 if dtype == torch.float32 else torch.float32
    names = {torch.float32: "Float", torch.float64: "Double"}
    for name, call in _four(ns, fl, h, P.to(other)):
        _raises(call, f"percnn_amd: params has dtype {names[other]}, expected {names[dtype]}", name)
    _raises(lambda: getattr(ns, f"pi_step{fl}_backward")(h, P, h.to(other)),
            f"percnn_amd: g_out has dtype {names[other]}, expected {names[dtype]}")
    traj = _traj_like(fl, h)
    _raises(lambda: getattr(ns, f"pi_rollout{fl}_backward")(traj, P, traj.to(other)),
            f"percnn_amd: g_traj has dtype {names[other]}, expected {names[dtype]}")
    _raises(lambda: getattr(ns, f"pi_step{fl}")(h, P.cpu()), "percnn_amd: params must live on a HIP device (got cpu); there is no CPU path")
    _raises(lambda: getattr(ns, f"pi_step{fl}_backward")(h, P, h.cpu()),
            "percnn_amd: g_out must live on a HIP device (got cpu); there is no CPU path")
    _raises(lambda: getattr(ns, f"pi_step{fl}")(h.to(torch.float16), P), "percnn_amd: h must be float32 or float64, got Half")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fl", FLAVOURS[1:])
def test_gradient_of_another_shape(ns, hip_device, fl, dtype):
    h, P = _state(fl, dtype, hip_device), _block(fl, dtype, hip_device)
    _raises(lambda: getattr(ns, f"pi_step{fl}_backward")(h, P, h[:1]),
            "percnn_amd: g_out must have the state's shape [2, 2, 8, 8], got [1, 2, 8, 8]")
    traj = _traj_like(fl, h)
    for g in (traj[:2], traj[:, :1], traj[..., :4]):
        _raises(lambda: getattr(ns, f"pi_rollout{fl}_backward")(traj, P, g), "percnn_amd: g_traj must have the trajectory's shape")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fl", FLAVOURS)
def test_rollout_backward_wants_a_contiguous_trajectory_of_its_flavours_rank(ns, hip_device, fl, dtype):
    h, P = _state(fl, dtype, hip_device), _block(fl, dtype, hip_device)
    wide = _traj_like(fl, _state(fl, dtype, hip_device, (8, 16)))
    strided = wide[..., ::2]
    assert strided.shape == _traj_like(fl, h).shape and not strided.is_contiguous()
    _raises(lambda: getattr(ns, f"pi_rollout{fl}_backward")(strided, P, strided.contiguous()), "percnn_amd: traj must be contiguous")
    if fl == "":
        bad = torch.zeros(T + 1, 3, 8, 8, dtype=dtype, device=hip_device)
        _raises(lambda: ns.pi_rollout_backward(bad, P, bad), "percnn_amd: traj must be [T+1,2,*S]")
    else:
        word = fl[1:]
        for bad in (torch.zeros(T + 1, 2, 8, 8, dtype=dtype, device=hip_device),
                    torch.zeros(T + 1, B, 3, 8, 8, dtype=dtype, device=hip_device)):
            _raises(lambda: getattr(ns, f"pi_rollout{fl}_backward")(bad, P, bad), f"percnn_amd: {word} traj must be [T+1,B,2,*S]")


def _check(t, shape, dtype, dev):
    assert tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_contiguous() and t.device == dev


@pytest.mark.parametrize("dtype,hc,shape", [(torch.float32, 0, (8, 8)), (torch.float64, 2, (8, 8)), (torch.float32, 2, (8, 8, 8))],
                         ids=["f32-poly-2d", "f64-hc2-2d", "f32-hc2-3d"])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_every_operator_answers_with_its_shapes_and_the_blocks_dtype(ns, hip_device, fl, dtype, hc, shape):
    dev = torch.device("cuda", torch.cuda.current_device())
    h, P = _state(fl, dtype, hip_device, shape), _block(fl, dtype, hip_device, hc, len(shape))
    step, step_bwd = getattr(ns, f"pi_step{fl}"), getattr(ns, f"pi_step{fl}_backward")
    roll, roll_bwd = getattr(ns, f"pi_rollout{fl}"), getattr(ns, f"pi_rollout{fl}_backward")
    traj_shape = (T + 1,) + tuple(h.shape[1:] if fl == "" else h.shape)

    out = step(h, P)
    _check(out, h.shape, dtype, dev)
    g = torch.ones_like(h)
    g_in, pg = step_bwd(h, P, g)
    _check(g_in, h.shape, dtype, dev)
    _check(pg, P.shape, P.dtype, dev)
    traj = roll(h, P, T)
    _check(traj, traj_shape, dtype, dev)
    assert bits_equal(traj[0], h[0] if fl == "" else h)
    assert bits_equal(traj[1], out[0] if fl == "" else out)
    gt = torch.ones_like(traj)
    g_h0, pg_r = roll_bwd(traj, P, gt)
    _check(g_h0, h.shape, dtype, dev)
    _check(pg_r, P.shape, P.dtype, dev)
    _check(roll(h, P, 0), (1,) + traj_shape[1:], dtype, dev)
    assert torch.isfinite(pg).all() and torch.isfinite(pg_r).all() and float(pg_r.abs().max()) > 0

    # non-contiguous inputs are taken (made contiguous inside), outputs are contiguous and the same bits
    hw = _state(fl, dtype, hip_device, shape[:-1] + (2 * shape[-1],))
    hs = hw[..., ::2]
    assert not hs.is_contiguous()
    _check(step(hs, P), h.shape, dtype, dev)
    assert bits_equal(step(hs, P), step(hs.contiguous(), P))
    assert bits_equal(step_bwd(hs, P, hs)[0], step_bwd(hs.contiguous(), P, hs.contiguous())[0])
    assert bits_equal(roll(hs, P, T), roll(hs.contiguous(), P, T))

    # the autograd formulas call the backward operators: same bits, gradient of the block in the block's shape and dtype
    h1, P1 = h.clone().requires_grad_(True), P.clone().requires_grad_(True)
    step(h1, P1).backward(g)
    assert bits_equal(h1.grad, g_in) and bits_equal(P1.grad, pg)
    _check(P1.grad, P.shape, P.dtype, dev)
    h2, P2 = h.clone().requires_grad_(True), P.clone().requires_grad_(True)
    roll(h2, P2, T, "").backward(gt)
    assert bits_equal(h2.grad, g_h0) and bits_equal(P2.grad, pg_r)
    # options travel to the backward operator
    h3 = h.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="failed: invalid argument"):
        roll(h3, P, T, "nonsense=1")
