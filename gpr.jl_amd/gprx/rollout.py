"""Rollouts.  Minimal coordinates: predictdynamicsmin (examples/utils/predictdynamics.jl:30-102)
for many trajectories in one device launch (gprx_rollout_min, include/gprx.h).  Maximal
coordinates: predictdynamics (:7-22) with batched mean-only predictions per step and the physics
(projectv!, updatestate!) injected by the caller.

The reference calls `predict_y(gp, obs)[1][1]` once per GP per step per test trajectory
(predictdynamics.jl:44,58,75,90) -- G x steps x testsamples single-point predictions, each with
an O(N^2) variance it discards.  Here one workgroup per trajectory runs the whole step chain on
the MI355X, reading each GP's training inputs, alpha and kernel parameters from its batch slot.

Coordinates (startobservation layout, predictdynamics.jl:40,54,71,86):
    P1  (theta, omega)                       -> 1 GP  (omega)
    P2  (theta1, omega1, theta2, omega2)     -> 2 GPs (omega1, omega2), theta2 relative
    CP  (x, v, theta, omega)                 -> 2 GPs (v, omega)
    FB  (theta1, omega1, theta3, omega3)     -> 2 GPs (omega1, omega3)
GP inputs per step: that vector, or with usesin (sin q, cos q, qdot) for the angle coordinates.
rollout_min / predictdynamicsmin take MeanZero GPs; MeanDynamics GPs, whose mean is a physics solve per
step, roll out through rollout_min_md (gprx_rollout_min_md: the solve runs in the same launch).
rollout_min_rec / rollout_min_md_rec are the same rollouts keeping (q_old, qdot_old) at the steps the
caller names, in launches of bounded length (gprx_rollout_min_rec, gprx_rollout_min_md_rec).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from .batch import Context, GPBatch

MECH = {"P1": 1, "P2": 2, "CP": 3, "FB": 4}
NCOORD = {"P1": 1, "P2": 2, "CP": 2, "FB": 2}
ANGLE = {"P1": (True,), "P2": (True, True), "CP": (False, True), "FB": (True, True)}
DT = 0.01  # mechanism.Δt of the experiments (P2noise.jl(min):14)
# link lengths of the experiment mechanisms (examples/utils/simulations.jl:11,53-54,111; FB l = 1)
LENGTHS = {"P1": (1.0,), "P2": (1.0, 1.0), "CP": (0.5,), "FB": (1.0,)}


def input_dim(mech: str, usesin: bool) -> int:
    return sum(3 if (usesin and a) else 2 for a in ANGLE[mech])


def rollout_min(mech: str, groups, start, steps: int, usesin: bool = False, dt: float = DT,
                traj_group=None, ctx: Context | None = None) -> np.ndarray:
    """Run T rollouts.  groups: list of rollout groups, each a list of nc GP references -- a
    GPE or a (GPBatch, slot) pair -- for coordinates 1..nc.  start: (T, 2nc).  traj_group: (T,)
    group index per trajectory (default: all group 0).  Returns (T, 2nc) = (q_cur, qdot_last) per
    coordinate after `steps` steps."""
    return _rollout_min(mech, groups, start, steps, usesin, dt, traj_group, ctx, md=False)[0]


def _device_args(groups, n: int, what: str, T: int, traj_group, ref, ctx):
    """What the device rollouts share: the GP references of `groups` (n per group, GP k of a group
    resolved by ref(g, k)) as the C calls take them, and the (T,) group index per trajectory.
    Returns (batches, slots, traj_group, ctx); the arrays must outlive the call."""
    tg = np.zeros(T, dtype=np.int32) if traj_group is None else np.ascontiguousarray(traj_group, dtype=np.int32)
    if tg.shape != (T,):
        raise ValueError("traj_group must have one entry per trajectory")
    refs = []
    for grp in groups:
        if len(grp) != n:
            raise ValueError(what)
        refs += [ref(g, k) for k, g in enumerate(grp)]
    batches = (C.c_void_p * len(refs))(*[b.h.value for b, _ in refs])
    slots = np.ascontiguousarray([s for _, s in refs], dtype=np.int32)
    return batches, slots, tg, ctx or refs[0][0].ctx


def record_indices(rec, T: int, steps: int) -> np.ndarray:
    """The storage indices of a recorded rollout as the C calls take them, (T, R) int32: rec None
    (every index, 1 .. steps + 1), (R,) shared by all trajectories, or (T, R).  1-based, as
    gprx_simulate's: 1 is the start, j the state after j - 1 steps.  ValueError for a wrong shape, an
    index outside [1, steps + 1] or a decreasing row."""
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    if rec is None:
        rec = np.arange(1, steps + 2)
    rc = np.asarray(rec)
    if rc.size == 0:
        rc = rc.astype(np.int32)
    if rc.dtype.kind not in "iu":
        raise ValueError("rec must hold integers")
    if rc.ndim == 1:
        rc = np.broadcast_to(rc, (T, rc.shape[0]))
    if rc.ndim != 2 or rc.shape[0] != T:
        raise ValueError("rec must be None, (R,) or (T, R)")
    if rc.size and (rc.min() < 1 or rc.max() > steps + 1):
        raise ValueError(f"rec indices must lie in [1, steps + 1] = [1, {steps + 1}]")
    if np.any(np.diff(rc, axis=1) < 0):
        raise ValueError("rec must be non-decreasing per trajectory")
    return np.ascontiguousarray(rc, dtype=np.int32)


def _record_args(rec, T: int, steps: int, steps_per_launch: int, width: int):
    """(rec (T, R) int32, traj (T, R, width), the C calls' (R, rec, steps_per_launch, traj))."""
    if int(steps_per_launch) < 0:
        raise ValueError("steps_per_launch must be >= 1, or 0 for the default")
    rc = record_indices(rec, T, steps)
    R = rc.shape[1]
    traj = np.empty((T, R, width))
    return rc, traj, (R, L.iptr(rc) if R else None, int(steps_per_launch), L.dptr(traj) if R else None)


def _rollout_min(mech, groups, start, steps, usesin, dt, traj_group, ctx, md, vi_regularizer=None, record=None):
    """rollout_min (md False: MeanZero GPs) and rollout_min_md: (final, status, vi_status), the last
    two None for MeanZero GPs.  record = (rec, steps_per_launch): the recorded forms, with the
    trajectory (T, R, 2nc) ahead of the three."""
    if mech not in MECH:
        raise ValueError(f"Experiment {mech} not supported!")  # predictdynamics.jl:35
    nc = NCOORD[mech]
    start = np.ascontiguousarray(start, dtype=np.float64)
    if start.ndim == 1:
        start = start[None, :]
    T = start.shape[0]
    if start.shape != (T, 2 * nc):
        raise ValueError(f"start must be (T, {2 * nc})")
    variant = "min_sin" if usesin else "min"
    rc, traj, rtail = _record_args(record[0], T, steps, record[1], 2 * nc) if record else (None, None, ())
    pre = (traj,) if record else ()
    ref = (lambda g, k: _slot_ref_md(g, mech, variant, k)) if md else (lambda g, k: _slot_ref(g))
    batches, slots, tg, ctx = _device_args(groups, nc, f"{mech} rollouts use {nc} GP(s) per group", T, traj_group, ref, ctx)
    out = np.empty((T, 2 * nc), dtype=np.float64)
    head = (ctx.h, MECH[mech], 1 if usesin else 0, float(dt), int(steps))
    tail = (len(groups), batches, L.iptr(slots), T, L.iptr(tg), L.dptr(start), L.dptr(out))
    if not md:
        fn = L.lib.gprx_rollout_min_rec if record else L.lib.gprx_rollout_min
        L.check(fn(*head, *tail, *rtail), ctx.h)
        return pre + (out, None, None)
    from . import vi

    reg = vi.REGULARIZER[mech] if vi_regularizer is None else float(vi_regularizer)
    st = np.empty(T, dtype=np.int32)
    vst = np.empty(T, dtype=np.int32)
    fn = L.lib.gprx_rollout_min_md_rec if record else L.lib.gprx_rollout_min_md
    L.check(fn(*head, reg, *tail, L.iptr(st), L.iptr(vst), *rtail), ctx.h)
    return pre + (out, st, vst)


def _slot_ref(g):
    if isinstance(g, tuple):
        b, s = g
        if not isinstance(b, GPBatch):
            raise TypeError("a GP reference is a GPE or a (GPBatch, slot) pair")
        return b, int(s)
    from .gp import MeanZero  # GPE
    if not isinstance(g.mean, MeanZero):
        raise NotImplementedError("device rollouts need MeanZero GPs (MeanDynamics solves physics per step: "
                                  "predictdynamics_md / rollout_min_md)")
    return g._batch, 0


def _slot_ref_md(g, mech: str, variant: str, k: int):
    """GP k (0-based) of a MeanDynamics rollout group: a (GPBatch, slot) pair factorised on
    y - μ(X), or a GPE whose mean is MeanDynamics(mech, k + 1, variant)."""
    if isinstance(g, tuple):
        return _slot_ref(g)
    from .gp import MeanDynamics
    if not isinstance(g.mean, MeanDynamics):
        raise NotImplementedError("MeanDynamics rollouts need MeanDynamics GPs (MeanZero GPs roll out through "
                                  "predictdynamics / rollout_min)")
    m = g.mean
    if (m.mech, m.variant, m.mu_id) != (mech, variant, k + 1):
        raise ValueError(f"GP {k} of a {mech} {variant} group needs MeanDynamics({mech!r}, {k + 1}, {variant!r}), "
                         f"not ({m.mech!r}, {m.mu_id}, {m.variant!r})")
    return g._batch, 0


def rollout_min_md(mech: str, groups, start, steps: int, usesin: bool = False, dt: float = DT,
                   vi_regularizer: float | None = None, traj_group=None, ctx: Context | None = None):
    """rollout_min with MeanDynamics GPs (predict_y = μ(obs) + k*ᵀα, src/mDynamics.jl:41-55) in one
    device launch (gprx_rollout_min_md): per step the GP means at the features plus the rates of one
    variational-integrator step at the experiments' xtransform of the features.  groups as
    rollout_min's, of (GPBatch, slot) pairs factorised on y - μ(X) or GPEs that carry
    MeanDynamics(mech, g + 1, "min" / "min_sin").  Returns (final (T, 2nc), status (T,): 2 = a failed
    physics step, the row is NaN; vi_status (T,): OR of the per-step vi_step statuses)."""
    return _rollout_min(mech, groups, start, steps, usesin, dt, traj_group, ctx, md=True, vi_regularizer=vi_regularizer)


def rollout_min_rec(mech: str, groups, start, steps: int, rec=None, usesin: bool = False, dt: float = DT,
                    traj_group=None, steps_per_launch: int = 0, ctx: Context | None = None):
    """rollout_min that keeps the trajectory, in launches of at most steps_per_launch steps (0: the
    library's default; gprx_rollout_min_rec).  rec: None (every index, 1 .. steps + 1), (R,) for all
    trajectories or (T, R): non-decreasing 1-based storage indices, 1 = the start, j = after j - 1
    steps.  Returns (trajectory (T, R, 2nc): (q_old, qdot_old) per coordinate at each index; final
    (T, 2nc), bit for bit rollout_min's, whatever rec and steps_per_launch)."""
    return _rollout_min(mech, groups, start, steps, usesin, dt, traj_group, ctx, md=False, record=(rec, steps_per_launch))[:2]


def rollout_min_md_rec(mech: str, groups, start, steps: int, rec=None, usesin: bool = False, dt: float = DT,
                       vi_regularizer: float | None = None, traj_group=None, steps_per_launch: int = 0,
                       ctx: Context | None = None):
    """rollout_min_md that keeps the trajectory (gprx_rollout_min_md_rec); rec and steps_per_launch as
    rollout_min_rec's.  Returns (trajectory (T, R, 2nc), NaN after a failed physics step; final, status,
    vi_status as rollout_min_md's, bit for bit)."""
    return _rollout_min(mech, groups, start, steps, usesin, dt, traj_group, ctx, md=True, vi_regularizer=vi_regularizer,
                        record=(rec, steps_per_launch))


def _rotx_q(th):
    return [math.cos(th / 2), math.sin(th / 2), 0.0, 0.0]  # q2vec(UnitQuaternion(RotX(θ)))


def final_cstate(mech: str, q, lengths=None) -> np.ndarray:
    """The CState predictdynamicsmin returns, built from the final coordinates q (velocities zero):
    P1 predictdynamics.jl:48-49, P2 :63-66, CP :80-81, FB :95-101."""
    ls = LENGTHS[mech] if lengths is None else tuple(lengths)
    z6 = [0.0] * 6
    if mech == "P1":
        (th,), (l,) = q, ls
        return np.array([0.0, 0.5 * l * math.sin(th), -0.5 * l * math.cos(th)] + _rotx_q(th) + z6)
    if mech == "P2":
        (t1, t2), (l1, l2) = q, ls
        x1 = [0.0, 0.5 * l1 * math.sin(t1), -0.5 * l1 * math.cos(t1)]
        x2 = [0.0, l1 * math.sin(t1) + 0.5 * l2 * math.sin(t1 + t2), -l1 * math.cos(t1) - 0.5 * l2 * math.cos(t1 + t2)]
        return np.array(x1 + _rotx_q(t1) + z6 + x2 + _rotx_q(t1 + t2) + z6)
    if mech == "CP":
        (x, th), (l,) = q, ls
        return np.array([0.0, x, 0.0, 1.0] + [0.0] * 10 + [0.5 * l * math.sin(th) + x, -0.5 * l * math.cos(th)]
                        + _rotx_q(th) + z6)
    if mech == "FB":
        (t1, t2), (l,) = q, ls
        x1 = [0.0, 0.5 * math.sin(t1) * l, -0.5 * math.cos(t1) * l]
        x2 = [0.0, math.sin(t1) * l + 0.5 * math.sin(t2) * l, -math.cos(t1) * l - 0.5 * math.cos(t2) * l]
        x3 = [0.0, 0.5 * math.sin(t2) * l, -0.5 * math.cos(t2) * l]
        x4 = [0.0, math.sin(t2) * l + 0.5 * math.sin(t1) * l, -math.cos(t2) * l - 0.5 * math.cos(t1) * l]
        q1, q2 = _rotx_q(t1), _rotx_q(t2)
        return np.array(x1 + q1 + z6 + x2 + q2 + z6 + x3 + q2 + z6 + x4 + q1 + z6)
    raise ValueError(f"Experiment {mech} not supported!")


def predictdynamicsmin(mech: str, gps, startobservation, steps: int, usesin: bool = False,
                       dt: float = DT, lengths=None) -> np.ndarray:
    """predictdynamicsmin(mechanism, etype, gps, startobservation, steps; usesin) for one start
    observation (predictdynamics.jl:30-36): returns the predicted CState after `steps` steps."""
    fin = rollout_min(mech, [list(gps)], np.asarray(startobservation, dtype=np.float64)[None, :], steps, usesin, dt)
    return final_cstate(mech, fin[0, 0::2], lengths)


def predictdynamicsmin_batch(mech: str, gps, startobservations, steps: int, usesin: bool = False,
                             dt: float = DT, lengths=None) -> np.ndarray:
    """The experiments' test loop `for i in 1:length(xtest_old) predictdynamicsmin(...)`
    (e.g. P2noise.jl(min):73-76) in one launch: (T, 13 nbodies) predicted CStates."""
    fin = rollout_min(mech, [list(gps)], startobservations, steps, usesin, dt)
    return np.stack([final_cstate(mech, f[0::2], lengths) for f in fin])


def predictdynamics(gps, startobservations, steps: int, getvw, advance, prior_mean=None):
    """predictdynamics(mechanism, gps, startobservation, steps, getvω) for T maximal-coordinate
    trajectories at once (examples/utils/predictdynamics.jl:7-22).

    Per step the G GPs predict the next-step velocities at all T current CStates in ONE mean-only
    device evaluation (no variance: the reference discards it), instead of G x T single-point
    predict_y calls.  The physics stays on the host and is injected:
      gps               a GPBatch whose G slots share the training states (one trial's outputs,
                        CPnoise.jl:37-43), or a list of GPEs
      startobservations (T, d) CStates
      getvw(mu)         mu (G,) -> (vcurr, wcurr)             (the experiment's getvω)
      advance(s, v, w)  one trajectory's state (d,), predicted v, w -> (next state (d,), projection
                        error)  -- projectv! + updatestate! in the reference (ConstrainedDynamics)
      prior_mean        optional callable (d, T) -> (G, T) prior means added to the GP means for a
                        GPBatch (a GPE adds its own mean)
    Returns (final states (T, d), mean projection error per trajectory (T,))."""
    S = np.array(startobservations, dtype=np.float64)
    if S.ndim == 1:
        S = S[None, :]
    T = S.shape[0]
    err = np.zeros(T)
    for _ in range(steps):
        obs = np.ascontiguousarray(S.T)  # (d, T)
        if isinstance(gps, GPBatch):
            gps.set_test(obs)
            mu, _ = gps.predict(variance=False)  # (G, T)
            if prior_mean is not None:
                mu = mu + np.asarray(prior_mean(obs))
        else:
            mu = np.stack([g.predict_y_mean(obs) for g in gps])
        for t in range(T):
            v, w = getvw(mu[:, t])
            S[t], e = advance(S[t], v, w)
            err[t] += e
    return S, err / max(steps, 1)
