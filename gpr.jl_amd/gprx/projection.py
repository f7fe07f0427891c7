"""Maximal-coordinate rollout physics on the MI355X (include/gprx.h gprx_projectv,
gprx_rollout_max).

`projectv` is GPR's projectv! (src/projections/implicitProjection.jl:80-107): the Newton projection
of a predicted twist (v, w per body) onto the mechanism's joint constraints, for many mechanism
states in one launch.  `predictdynamics` is examples/utils/predictdynamics.jl:7-22 for many test
trajectories in one launch: per step the G GPs' mean predictions at the current CState, getvw,
projectv! and updatestate!, all on the device.  `predictdynamics_rec` / `predictdynamics_md_rec` are
the same rollouts keeping the CState at the steps the caller names, in launches of bounded length
(gprx_rollout_max_rec, gprx_rollout_max_md_rec; examples/energy.jl's predictedstates).

Mechanisms are the experiments' (examples/utils/data/simulations.jl): P1 pendulum, P2 double
pendulum, CP cart-pole, FB four-bar (which the experiments project with regularizer=1e-10,
FBnoise.jl:43).  The constraint functions and the state update restate ConstrainedDynamics 0.7.4
(absent from the reference tree; oracle/projection_oracle.py documents what is restated and what
pins it).
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .batch import Context, GPBatch
from .rollout import MECH

NBODIES = {"P1": 1, "P2": 2, "CP": 2, "FB": 4}
REGULARIZER = {"P1": 0.0, "P2": 0.0, "CP": 0.0, "FB": 1e-10}  # the experiments' projectv! settings
DT = 0.01


def getvw(mu, vw_indices, nb: int) -> np.ndarray:
    """The experiments' getvw (e.g. P2noise.jl:46): mu_k at 1-based CState position vw_indices[k],
    zero elsewhere, returned as (..., 6 nb) = (v_1, w_1, ..., v_nb, w_nb)."""
    mu = np.asarray(mu, dtype=np.float64)
    c = np.zeros(mu.shape[:-1] + (13 * nb,))
    for k, i in enumerate(vw_indices):
        c[..., i - 1] = mu[..., k]
    c = c.reshape(mu.shape[:-1] + (nb, 13))
    return c[..., 7:13].reshape(mu.shape[:-1] + (6 * nb,))


def projectv(mech: str, cstates, vw_pred, regularizer: float | None = None, newton_iter: int = 100, eps: float = 1e-10,
             dt: float = DT, ctx: Context | None = None):
    """projectv!(vu, wu, mechanism; newtonIter, eps, regularizer) for T mechanism states.
    cstates (T, 13 nb): the mechanism's CState (setstates!); vw_pred (T, 6 nb): predicted (v, w) per
    body.  Returns (vw (T, 6 nb) projected, iterations (T,), status (T,): 1 = singular KKT matrix)."""
    if mech not in MECH:
        raise ValueError(f"Experiment {mech} not supported!")
    nb = NBODIES[mech]
    cs = np.ascontiguousarray(np.atleast_2d(cstates), dtype=np.float64)
    vw = np.ascontiguousarray(np.atleast_2d(vw_pred), dtype=np.float64)
    T = cs.shape[0]
    if cs.shape != (T, 13 * nb) or vw.shape != (T, 6 * nb):
        raise ValueError(f"cstates must be (T, {13 * nb}) and vw_pred (T, {6 * nb})")
    reg = REGULARIZER[mech] if regularizer is None else float(regularizer)
    ctx = ctx or _default_ctx()
    out = np.empty((T, 6 * nb))
    it = np.empty(T, dtype=np.int32)
    st = np.empty(T, dtype=np.int32)
    L.check(L.lib.gprx_projectv(ctx.h, MECH[mech], float(dt), T, L.dptr(cs), L.dptr(vw), reg, int(newton_iter), float(eps),
                                L.dptr(out), L.iptr(it), L.iptr(st)), ctx.h)
    return out, it, st


def vi_step(mech: str, cstates, regularizer: float | None = None, newton_iter: int = 100, eps: float = 1e-10,
            dt: float = DT, ctx: Context | None = None):
    """One variational-integrator step (ConstrainedDynamics newton! after setstates!, the MeanDynamics
    prior mean of src/mDynamics.jl:41-60) for T states on the device (k_vi_step, one wave each); the
    same contract as the host restatement gprx.vi.vi_step: cstates (T, 13 nb) -> (solution CStates
    (T, 13 nb) [x2, q2, v2, w2] per body, NaN rows for failed states; iterations (T,); status (T,):
    0 converged, 1 not converged, 2 failed)."""
    from . import vi

    if mech not in MECH:
        raise ValueError(f"Experiment {mech} not supported!")
    nb = NBODIES[mech]
    cs = np.ascontiguousarray(np.atleast_2d(cstates), dtype=np.float64)
    T = cs.shape[0]
    if cs.shape != (T, 13 * nb):
        raise ValueError(f"cstates must be (T, {13 * nb})")
    reg = vi.REGULARIZER[mech] if regularizer is None else float(regularizer)
    ctx = ctx or _default_ctx()
    out = np.empty((T, 13 * nb))
    it = np.empty(T, dtype=np.int32)
    st = np.empty(T, dtype=np.int32)
    L.check(L.lib.gprx_vi_step(ctx.h, MECH[mech], float(dt), T, L.dptr(cs), reg, int(newton_iter), float(eps),
                               L.dptr(out), L.iptr(it), L.iptr(st)), ctx.h)
    return out, it, st


def simulate(mech: str, start, steps: int, rec, mass=None, inertia=None, damp=None, regularizer: float | None = None,
             newton_iter: int = 100, eps: float = 1e-10, dt: float = DT, steps_per_launch: int = 0,
             ctx: Context | None = None):
    """simulate!(mechanism, steps dt, control!, record = true) of the reference's datasets
    (examples/utils/data/simulations.jl) for T trajectories, every step on the device (gprx_simulate,
    k_simulate: one wave per trajectory).  start (T, 13 nb) CStates; rec (T, R) or (R,) non-decreasing
    1-based storage indices in [1, steps + 1] (1 = the start, j = after j - 1 steps); mass (T, nb),
    inertia (T, nb, 3, 3), damp (T, nb, 6) = (c_v, c_w) per body, or their single-trajectory shapes for
    all; None: the nominal bodies / no friction (gprx.vi.vi_step documents the equations).  Returns
    (records (T, R, 13 nb), NaN after a failed step; status (T,): OR of the per-step statuses, 2 =
    a failed step ended the trajectory).  A solve that stagnates at the rounding floor ends with status 1
    (gprx.vi.vi_step's stall_stop)."""
    from . import vi

    if mech not in MECH:
        raise ValueError(f"Experiment {mech} not supported!")
    nb = NBODIES[mech]
    S = np.ascontiguousarray(np.atleast_2d(start), dtype=np.float64)
    T = S.shape[0]
    if S.shape != (T, 13 * nb):
        raise ValueError(f"start must be (T, {13 * nb})")
    rc = np.asarray(rec, dtype=np.int32)
    rc = np.ascontiguousarray(np.broadcast_to(rc, (T, rc.shape[-1])) if rc.ndim == 1 else rc)
    if rc.ndim != 2 or rc.shape[0] != T or rc.shape[1] < 1:
        raise ValueError("rec must be (T, R) or (R,), R >= 1")
    R = rc.shape[1]

    def per_traj(a, shape):
        if a is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (T,) + shape))

    m, J, c = per_traj(mass, (nb,)), per_traj(inertia, (nb, 3, 3)), per_traj(damp, (nb, 6))
    reg = vi.REGULARIZER[mech] if regularizer is None else float(regularizer)
    ctx = ctx or _default_ctx()
    out = np.empty((T, R, 13 * nb))
    st = np.empty(T, dtype=np.int32)
    L.check(L.lib.gprx_simulate(ctx.h, MECH[mech], float(dt), int(steps), T, L.dptr(S), L.dptr(m), L.dptr(J), L.dptr(c), reg,
                                int(newton_iter), float(eps), R, L.iptr(rc), int(steps_per_launch), L.dptr(out), L.iptr(st)),
            ctx.h)
    return out, st


def predictdynamics(mech: str, groups, start, steps: int, vw_indices, regularizer: float | None = None,
                    traj_group=None, dt: float = DT, ctx: Context | None = None):
    """predictdynamics(mechanism, gps, startobservation, steps, getvw; regularizer) for T
    trajectories.  groups: list of rollout groups, each a list of G GP references -- (GPBatch,
    slot) pairs or MeanZero GPEs -- factorised at their hyperparameters; start (T, 13 nb) CStates;
    vw_indices: the experiment's 1-based vwindices (output g's CState position).  Returns (final
    CStates (T, 13 nb), mean projection error per step (T,), status (T,))."""
    return _predictdynamics(mech, groups, start, steps, vw_indices, regularizer, traj_group, dt, ctx, md=False)[:3]


def _predictdynamics(mech, groups, start, steps, vw_indices, regularizer, traj_group, dt, ctx, md, vi_regularizer=None,
                     record=None):
    """predictdynamics (md False: MeanZero GPs) and predictdynamics_md: (final CStates, projection
    error, status, vi_status), the last None for MeanZero GPs.  record = (rec, steps_per_launch): the
    recorded forms, with the trajectory (T, R, 13 nb) ahead of the four."""
    from .rollout import _device_args, _record_args, _slot_ref, _slot_ref_md

    if mech not in MECH:
        raise ValueError(f"Experiment {mech} not supported!")
    nb = NBODIES[mech]
    S = np.ascontiguousarray(np.atleast_2d(start), dtype=np.float64)
    T = S.shape[0]
    if S.shape != (T, 13 * nb):
        raise ValueError(f"start must be (T, {13 * nb})")
    G = len(vw_indices)
    rc, traj, rtail = _record_args(record[0], T, steps, record[1], 13 * nb) if record else (None, None, ())
    pre = (traj,) if record else ()
    ref = (lambda g, k: _slot_ref_md(g, mech, "max", k)) if md else (lambda g, k: _slot_ref(g))
    batches, slots, tg, ctx = _device_args(groups, G, f"each group needs {G} GPs (one per vw index)", T, traj_group, ref, ctx)
    vwi = np.ascontiguousarray(vw_indices, dtype=np.int32)
    reg = REGULARIZER[mech] if regularizer is None else float(regularizer)
    out = np.empty((T, 13 * nb))
    pe = np.empty(T)
    st = np.empty(T, dtype=np.int32)
    head = (ctx.h, MECH[mech], float(dt), int(steps), reg)
    tail = (len(groups), batches, L.iptr(slots), G, L.iptr(vwi), T, L.iptr(tg), L.dptr(S), L.dptr(out), L.dptr(pe), L.iptr(st))
    if not md:
        fn = L.lib.gprx_rollout_max_rec if record else L.lib.gprx_rollout_max
        L.check(fn(*head, *tail, *rtail), ctx.h)
        return pre + (out, pe, st, None)
    from . import vi

    vreg = vi.REGULARIZER[mech] if vi_regularizer is None else float(vi_regularizer)
    vst = np.empty(T, dtype=np.int32)
    fn = L.lib.gprx_rollout_max_md_rec if record else L.lib.gprx_rollout_max_md
    L.check(fn(*head, vreg, *tail, L.iptr(vst), *rtail), ctx.h)
    return pre + (out, pe, st, vst)


def predictdynamics_md(mech: str, groups, start, steps: int, vw_indices, regularizer: float | None = None,
                       vi_regularizer: float | None = None, traj_group=None, dt: float = DT, ctx: Context | None = None):
    """predictdynamics with MeanDynamics GPs (predict_y = μ(obs) + k*ᵀα, src/mDynamics.jl:41-55) in one
    device launch (gprx_rollout_max_md): per step the G GP means plus getμ(vωindices) of one
    variational-integrator step at the current CState, then getvw, projectv! and updatestate!.
    Arguments as predictdynamics; the GPs are (GPBatch, slot) pairs factorised on y - μ(X) or GPEs
    that carry MeanDynamics(mech, g + 1, "max").  Returns (final CStates (T, 13 nb), mean projection
    error per step (T,), status (T,): 1 = singular projection, 2 = a failed physics step, the row is
    NaN; vi_status (T,): OR of the per-step vi_step statuses)."""
    return _predictdynamics(mech, groups, start, steps, vw_indices, regularizer, traj_group, dt, ctx, md=True,
                            vi_regularizer=vi_regularizer)


def predictdynamics_rec(mech: str, groups, start, steps: int, vw_indices, rec=None, regularizer: float | None = None,
                        traj_group=None, dt: float = DT, steps_per_launch: int = 0, ctx: Context | None = None):
    """predictdynamics that keeps the trajectory, in launches of at most steps_per_launch steps (0: the
    library's default; gprx_rollout_max_rec).  rec: None (every index, 1 .. steps + 1), (R,) for all
    trajectories or (T, R): non-decreasing 1-based storage indices, 1 = the start, j = the state after
    j - 1 steps.  Returns (trajectory (T, R, 13 nb): oldstates = CState(mechanism) of
    predictdynamics.jl:18 at each index, examples/energy.jl's predictedstates, NaN after a step that
    failed; then predictdynamics' three, bit for bit, whatever rec and steps_per_launch)."""
    return _predictdynamics(mech, groups, start, steps, vw_indices, regularizer, traj_group, dt, ctx, md=False,
                            record=(rec, steps_per_launch))[:4]


def predictdynamics_md_rec(mech: str, groups, start, steps: int, vw_indices, rec=None, regularizer: float | None = None,
                           vi_regularizer: float | None = None, traj_group=None, dt: float = DT, steps_per_launch: int = 0,
                           ctx: Context | None = None):
    """predictdynamics_md that keeps the trajectory (gprx_rollout_max_md_rec); rec and steps_per_launch
    as predictdynamics_rec's.  Returns (trajectory (T, R, 13 nb); then predictdynamics_md's four, bit
    for bit)."""
    return _predictdynamics(mech, groups, start, steps, vw_indices, regularizer, traj_group, dt, ctx, md=True,
                            vi_regularizer=vi_regularizer, record=(rec, steps_per_launch))


def _default_ctx():
    """The context of this process's device, in this order:
      * GPRX_DEVICE (an explicit device index);
      * torch's current device, when this process has already initialised torch's HIP runtime (a
        caller that chose a GPU with torch.cuda.set_device(k) keeps it; nothing is initialised here);
      * GPU LOCAL_RANK (mod the visible devices, as shard.init_ranks binds a rank; 0 without a
        launcher)."""
    import os
    import sys

    from .batch import default_context

    return default_context(default_device(int(L.lib.gprx_device_count()), os.environ, sys.modules.get("torch")))


def default_device(ndev: int, env, torch=None) -> int:
    """_default_ctx's device index (ndev visible devices, env a mapping, torch the imported module
    or None)."""
    n = max(1, int(ndev))
    if str(env.get("GPRX_DEVICE", "")).strip():
        return int(env["GPRX_DEVICE"]) % n
    if torch is not None and torch.cuda.is_initialized():
        return int(torch.cuda.current_device()) % n
    return int(env.get("LOCAL_RANK", "0") or 0) % n
