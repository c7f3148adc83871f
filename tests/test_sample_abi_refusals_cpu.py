"""What the batched and the ensemble entry points of the C ABI refuse, and with which code, before anything is launched.

One table per flavour.  The two flavours validate differently on purpose (include/percnn_pi.h): the batched entries hand
batch == 1 to the unbatched entry before they look at anything else and refuse almost no aliases; the ensemble entries validate
first, delegate after, and refuse every output that lies on an input.  Every row returns before the first HIP call: the pointers
are made-up numbers.  A row that must be ACCEPTED shows it by reaching the workspace refusal (-2) with a 16-byte workspace, or
by returning 0 for a rollout of zero steps; an accepted batched step_fwd would launch, so its aliases have no row."""
import ctypes

import pytest

EINVAL, EWORKSPACE = -1, -2

# argument lists of the entry points, in call order (include/percnn_pi.h)
SIG = {
    "step_fwd": "h out P hc ndim shape batch options stream",
    "step_bwd": "h g_out g_inj g_in param_grad ws ws_bytes P hc ndim shape batch options stream",
    "rollout_fwd": "traj P hc ndim shape batch T options stream",
    "rollout_bwd": "traj g_traj mask g_h0 param_grad ws ws_bytes P hc ndim shape batch T options stream",
    "rollout_bwd_sqerr": "traj target mask scale dev g_h0 param_grad ws ws_bytes P hc ndim shape batch T options stream",
    "rollout_bwd_obs_sqerr": "traj target_c mask strides scale dev g_h0 param_grad ws ws_bytes P hc ndim shape batch T options stream",
    "traj_sqerr": "traj target mask nframes ndim shape batch scale out ws ws_bytes stream",
    "traj_obs_sqerr": "traj target_c mask nframes ndim shape strides batch scale out ws ws_bytes stream",
}
SWEEPS = ("rollout_bwd", "rollout_bwd_sqerr", "rollout_bwd_obs_sqerr")
BWD = ("step_bwd",) + SWEEPS
LOSS_VALUES = ("traj_sqerr", "traj_obs_sqerr")

SHAPE2 = (ctypes.c_int64 * 2)(8, 8)
SHAPE3 = (ctypes.c_int64 * 3)(8, 8, 8)


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


# A call that is in order except for its workspace of 16 bytes: every entry with a workspace answers -2, rollout_fwd runs zero
# steps and answers 0, and step_fwd has no such call (its rows each carry a refusal).  All pointers are 16-byte aligned.
BASE = dict(h=0x1000, out=0x2000, P=0x3000, g_out=0x4000, g_inj=0x5000, g_in=0x6000, param_grad=0x7000, ws=0x8000, ws_bytes=16,
            traj=0x9000, g_traj=0xA000, g_h0=0xB000, target=0xC000, target_c=0xD000, dev=0xE000, mask=None, strides=ints(2, 2),
            scale=0.5, hc=8, ndim=2, shape=SHAPE2, batch=2, T=0, nframes=3, options=None, stream=None)
ROOMY = dict(ws_bytes=1 << 40)                                 # (only ever together with a misaligned workspace)


def call(L, flavour, entry, suf, over):
    if entry in LOSS_VALUES:
        name = f"percnn_pi_batch_{entry}_{suf}"                  # the loss values have one flavour
    else:
        name = f"percnn_pi_{flavour}_{entry}_{suf}"
    args = dict(BASE, **over)
    return getattr(L, name)(*[args[k] for k in SIG[entry].split()])


def rows_common(ens):
    """Rows that read the same for both flavours."""
    r = []
    everything = tuple(SIG) if not ens else tuple(e for e in SIG if e not in LOSS_VALUES)
    for entry in everything:
        for batch in (0, -3, 65536, 70000):
            r.append((entry, dict(batch=batch), EINVAL))
        # a bad batch wins over everything behind it
        r.append((entry, dict(batch=0, ws=None), EINVAL))
    for entry in everything:
        if entry in LOSS_VALUES:
            continue
        r.append((entry, dict(options=b"nonsense=1"), EINVAL))
        r.append((entry, dict(options=b"tile_k=3"), EINVAL))
        r.append((entry, dict(ndim=4), EINVAL))
        r.append((entry, dict(shape=None), EINVAL))
        r.append((entry, dict(hc=65), EINVAL))
        r.append((entry, dict(P=None), EINVAL))
    # the largest batch is in order: the entries with a workspace get as far as refusing it
    for entry in BWD + (() if ens else LOSS_VALUES):
        r.append((entry, dict(batch=65535), EWORKSPACE))
    # the workspace: missing, too small (BASE), misaligned
    for entry in BWD + (() if ens else LOSS_VALUES):
        for batch in (1, 2, 4):
            r.append((entry, dict(batch=batch), EWORKSPACE))
            r.append((entry, dict(batch=batch, ws=None, **ROOMY), EWORKSPACE))
            r.append((entry, dict(batch=batch, ws=0x8004, **ROOMY), EWORKSPACE))
    for entry in BWD:
        r.append((entry, dict(ws=0x8008, **ROOMY), EWORKSPACE))   # 8-byte aligned is not enough for the adjoint frames
        r.append((entry, dict(param_grad=None), EINVAL))          # ... and a missing pointer comes before the small workspace
    # steps
    r.append(("step_fwd", dict(h=None), EINVAL))
    r.append(("step_fwd", dict(out=None), EINVAL))
    r.append(("step_fwd", dict(out=BASE["h"]), EINVAL))
    for batch in (1, 2):
        r.append(("step_fwd", dict(batch=batch, out=BASE["h"]), EINVAL))
        r.append(("step_bwd", dict(batch=batch, g_in=BASE["g_out"]), EINVAL))
        r.append(("step_bwd", dict(batch=batch, g_in=BASE["g_out"], ws=None), EINVAL))
    r.append(("step_bwd", dict(h=None), EINVAL))
    r.append(("step_bwd", dict(g_out=None), EINVAL))
    r.append(("step_bwd", dict(g_in=None), EINVAL))
    r.append(("step_bwd", dict(g_inj=None), EWORKSPACE))          # no injection: in order
    # rollouts
    r.append(("rollout_fwd", dict(), 0))
    r.append(("rollout_fwd", dict(batch=1), 0))
    r.append(("rollout_fwd", dict(hc=0, options=b"tile_k=4"), 0))
    r.append(("rollout_fwd", dict(traj=None), EINVAL))
    for entry in ("rollout_fwd",) + SWEEPS:
        for batch in (1, 2):
            r.append((entry, dict(batch=batch, T=-1), EINVAL))
    for entry in SWEEPS:
        r.append((entry, dict(traj=None), EINVAL))
        r.append((entry, dict(g_h0=None), EINVAL))
        r.append((entry, dict(T=5), EWORKSPACE))
    r.append(("rollout_bwd", dict(g_traj=None), EINVAL))
    for batch in (1, 2):
        r.append(("rollout_bwd_sqerr", dict(batch=batch, target=None), EWORKSPACE))   # no target: the loss is sum h^2, in order
    # loss forms: dL/dh0 and the gradients are written while the factors are read
    for entry in ("rollout_bwd_sqerr", "rollout_bwd_obs_sqerr"):
        r.append((entry, dict(g_h0=BASE["dev"]), EINVAL))
        r.append((entry, dict(param_grad=BASE["dev"]), EINVAL))
        r.append((entry, dict(dev=None), EWORKSPACE))
    # sparse observations: strides, the lattice, the compact target -- for one sample too, and before the workspace
    for batch in (1, 2):
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, strides=None), EINVAL))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, strides=None, ws=None), EINVAL))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, strides=ints(0, 1)), EINVAL))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, strides=ints(2, -1)), EINVAL))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, strides=ints(2, 0), ws=None), EINVAL))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, ndim=3, shape=SHAPE3, strides=ints(1, 2, 0)), EINVAL))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, ndim=3, shape=SHAPE3, strides=ints(1, 2, 3)), EWORKSPACE))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, g_h0=BASE["target_c"]), EINVAL))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, target_c=None), EWORKSPACE))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, strides=ints(1, 1)), EWORKSPACE))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, hc=-1), EINVAL))
        r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, hc=-1, strides=None), EINVAL))
    return r


def rows_batched():
    r = rows_common(False)
    # hc = -1: batch 1 is the unbatched call, which has the advective block; larger batches have none
    r.append(("step_fwd", dict(hc=-1, batch=2), EINVAL))
    r.append(("step_fwd", dict(hc=-1, batch=4, out=BASE["h"]), EINVAL))
    r.append(("step_bwd", dict(hc=-1, batch=1), EWORKSPACE))
    r.append(("step_bwd", dict(hc=-1, batch=2), EINVAL))
    r.append(("rollout_fwd", dict(hc=-1, batch=1), 0))
    r.append(("rollout_fwd", dict(hc=-1, batch=2), EINVAL))
    r.append(("rollout_bwd", dict(hc=-1, batch=1), EWORKSPACE))
    r.append(("rollout_bwd", dict(hc=-1, batch=2), EINVAL))
    r.append(("rollout_bwd_sqerr", dict(hc=-1, batch=1), EINVAL))       # the unbatched refusal: no loss form on that block
    r.append(("rollout_bwd_sqerr", dict(hc=-1, batch=2), EINVAL))
    # aliases the batched flavour does NOT refuse: the call gets as far as the workspace (or runs its zero steps)
    r.append(("rollout_fwd", dict(traj=BASE["P"]), 0))
    for batch in (1, 2):
        for other in ("h", "g_inj", "P"):
            r.append(("step_bwd", dict(batch=batch, g_in=BASE[other]), EWORKSPACE))
        for other in ("traj", "g_traj", "P"):
            r.append(("rollout_bwd", dict(batch=batch, g_h0=BASE[other]), EWORKSPACE))
    # ... except dL/dh0 on the trajectory, the target or the block in LOSS form, for more than one sample (one sample is the
    # unbatched call, which refuses none of them)
    for other in ("traj", "target", "P"):
        r.append(("rollout_bwd_sqerr", dict(g_h0=BASE[other]), EINVAL))
        r.append(("rollout_bwd_sqerr", dict(g_h0=BASE[other], ws=None), EINVAL))       # the alias first, then the workspace
        r.append(("rollout_bwd_sqerr", dict(batch=1, g_h0=BASE[other]), EWORKSPACE))
    r.append(("rollout_bwd_sqerr", dict(target=None, g_h0=BASE["traj"]), EINVAL))
    # the sparse form stays on the sample launches for one sample: its refusals are the batched ones there too
    for batch in (1, 2):
        for other in ("traj", "P"):
            r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, g_h0=BASE[other]), EINVAL))
            r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, g_h0=BASE[other], ws=None), EINVAL))
    # the loss values: the dense one hands one sample to the unbatched pass (which refuses no alias and never sees a lattice),
    # the sparse one does not
    for entry in LOSS_VALUES:
        r.append((entry, dict(traj=None), EINVAL))
        r.append((entry, dict(out=None), EINVAL))
        r.append((entry, dict(nframes=-1), EINVAL))
        r.append((entry, dict(ndim=4), EINVAL))
        r.append((entry, dict(shape=None), EINVAL))
        r.append((entry, dict(out=BASE["traj"]), EINVAL))
        r.append((entry, dict(out=BASE["traj"], ws=None), EINVAL))
        r.append((entry, dict(nframes=0), EWORKSPACE))
    r.append(("traj_sqerr", dict(out=BASE["target"]), EINVAL))
    r.append(("traj_sqerr", dict(target=None), EWORKSPACE))
    r.append(("traj_sqerr", dict(batch=1, out=BASE["traj"]), EWORKSPACE))
    r.append(("traj_sqerr", dict(batch=1, out=BASE["target"]), EWORKSPACE))
    r.append(("traj_sqerr", dict(batch=1, nframes=-1), EINVAL))
    r.append(("traj_obs_sqerr", dict(out=BASE["target_c"]), EINVAL))
    r.append(("traj_obs_sqerr", dict(target_c=None), EWORKSPACE))
    for batch in (1, 2):
        r.append(("traj_obs_sqerr", dict(batch=batch, out=BASE["traj"]), EINVAL))
        r.append(("traj_obs_sqerr", dict(batch=batch, out=BASE["target_c"]), EINVAL))
        r.append(("traj_obs_sqerr", dict(batch=batch, strides=None), EINVAL))
        r.append(("traj_obs_sqerr", dict(batch=batch, strides=ints(0, 1)), EINVAL))
        r.append(("traj_obs_sqerr", dict(batch=batch, strides=ints(1, -2), ws=None), EINVAL))   # the lattice first
        r.append(("traj_obs_sqerr", dict(batch=batch, ndim=3, shape=SHAPE3, strides=ints(3, 1, 0)), EINVAL))
        r.append(("traj_obs_sqerr", dict(batch=batch, strides=ints(1, 1)), EWORKSPACE))
    return r


def rows_ensemble():
    r = rows_common(True)
    # hc = -1 has no ensemble flavour, not even for one sample -- and that is checked before the pointers
    for entry in ("step_fwd", "step_bwd", "rollout_fwd") + SWEEPS:
        for batch in (1, 2):
            r.append((entry, dict(hc=-1, batch=batch), EINVAL))
    # every output on an input is refused, for one sample too (validate first, delegate after), and before the workspace
    for batch in (1, 2):
        r.append(("step_fwd", dict(batch=batch, out=BASE["P"]), EINVAL))
        r.append(("rollout_fwd", dict(batch=batch, traj=BASE["P"]), EINVAL))
        for other in ("h", "g_inj", "P"):
            r.append(("step_bwd", dict(batch=batch, g_in=BASE[other]), EINVAL))
            r.append(("step_bwd", dict(batch=batch, g_in=BASE[other], ws=None), EINVAL))
        for other in ("traj", "g_traj", "P"):
            r.append(("rollout_bwd", dict(batch=batch, g_h0=BASE[other]), EINVAL))
            r.append(("rollout_bwd", dict(batch=batch, g_h0=BASE[other], ws=None), EINVAL))
        for other in ("traj", "target", "P"):
            r.append(("rollout_bwd_sqerr", dict(batch=batch, g_h0=BASE[other]), EINVAL))
            r.append(("rollout_bwd_sqerr", dict(batch=batch, g_h0=BASE[other], ws=None), EINVAL))
        r.append(("rollout_bwd_sqerr", dict(batch=batch, target=None, g_h0=BASE["traj"]), EINVAL))
        for other in ("traj", "P"):
            r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, g_h0=BASE[other]), EINVAL))
            r.append(("rollout_bwd_obs_sqerr", dict(batch=batch, g_h0=BASE[other], ws=None), EINVAL))
        # the loss-form checks hold for one sample as well
        r.append(("rollout_bwd_sqerr", dict(batch=batch, g_h0=BASE["dev"]), EINVAL))
        r.append(("rollout_bwd_sqerr", dict(batch=batch, param_grad=BASE["dev"]), EINVAL))
    return r


@pytest.mark.parametrize("flavour,rows", [("batch", rows_batched()), ("ensemble", rows_ensemble())], ids=["batched", "ensemble"])
def test_sample_entry_points_refuse_before_any_launch(flavour, rows):
    import percnn_amd
    L = percnn_amd.lib()
    assert len(rows) > 150
    bad = []
    for suf in ("f32", "f64"):
        for entry, over, want in rows:
            got = call(L, flavour, entry, suf, over)
            if got != want:
                bad.append((flavour, entry, suf, {k: (v if isinstance(v, (int, bytes, type(None))) else list(v)) for k, v in over.items()},
                            "want", want, "got", got))
    assert not bad, "\n".join(map(str, bad))


def test_every_sample_entry_point_has_rows():
    for flavour, rows in (("batch", rows_batched()), ("ensemble", rows_ensemble())):
        seen = {e for e, _, _ in rows}
        want = set(SIG) if flavour == "batch" else set(SIG) - set(LOSS_VALUES)
        assert seen == want, (flavour, want - seen)
