"""Test-side helper: the variational-integrator step with per-trajectory bodies and an external force
(gprx_simulate's step, gprx/vi.py vi_step(m=, J=, damp=)) held to the 70-digit truth of
oracle/hp_physics.py.  _Step is subclassed, not edited: the bodies are replaced and the residual's
dynamics rows lose F (translational) and 2 tau (rotational), both constant during the solve.

cases(mech): the two cases per mechanism of tests/golden/hp_sim_<mech>.npz --
  nominal   one generator state, nominal bodies, no friction
  extreme   another, dm and dJ at their +-10% extremes (alternating from body to body) and the friction
            at its largest draw (simdata.FRICTION_SCALE)
fp64 evaluations of a case (evaluations()): "lapack" -- the extended vi.vi_step as it stands -- and
"rev" -- the same with the bodies in reverse order (hp_physics' rev construction).  E is their errors'
geometric mean, A = max(|s_start|inf, |s|inf), the bound hp_oracle.bound(E, A, k) with k of
tests/golden/hp_phys_<mech>.npz.  Nothing here is fitted to the device.
"""
from __future__ import annotations

import pathlib

import mpmath
import numpy as np

from oracle import hp_oracle as H
from oracle import hp_physics as HP

mp = mpmath.mp
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
VI = HP.VI
FRICTION_MAX = {"P1": [1.0], "P2": [2.0, 0.5], "CP": [1.0, 0.5], "FB": [2.0, 0.5, 2.0, 0.5]}
CASES = ("nominal", "extreme")
DT = 0.01


class SimStep(HP._Step):
    """hp_physics._Step with the bodies (m, J) and the force of control! at the current velocities."""

    def __init__(self, mech, cstate, dt, h, m, J, damp, torque_factor=2):
        super().__init__(mech, cstate, dt, h)
        P = self.P
        self.m = HP._mpv(m)
        self.J = [[HP._mpv(Jb[i]) for i in range(3)] for Jb in np.asarray(J, dtype=np.float64)]
        self.mom1 = []
        for b in range(P.nb):  # (sq1 I - [w1 x]) J w1 with the new inertia
            w1 = P.w1[b]
            Jw = [sum((self.J[b][i][k] * w1[k] for k in range(3)), mp.mpf(0)) for i in range(3)]
            sq1 = mp.sqrt(4 / (P.dt * P.dt) - sum((t * t for t in w1), mp.mpf(0)))
            cr = (w1[1] * Jw[2] - w1[2] * Jw[1], w1[2] * Jw[0] - w1[0] * Jw[2], w1[0] * Jw[1] - w1[1] * Jw[0])
            self.mom1.append([sq1 * Jw[i] - cr[i] for i in range(3)])
        c = np.asarray(damp, dtype=np.float64).reshape(P.nb, 6)
        self.ext = []
        for b in range(P.nb):
            self.ext += [-(mp.mpf(float(c[b, k])) * P.v1[b][k]) for k in range(3)]                          # F = -c_v o v1
            self.ext += [torque_factor * -(mp.mpf(float(c[b, 3 + k])) * P.w1[b][k]) for k in range(3)]  # 2 tau

    def residual(self, s, lam):
        f = super().residual(s, lam)
        for j in range(6 * self.P.nb):
            f[j] = f[j] - self.ext[j]
        return f


def truth(mech, cstate, dt, s64, m, J, damp):
    """hp_physics.truth_vi for the parametrised step (the four-bar: the limit of the regularised
    iteration from the documented start, as there)."""
    nb = HP.nbodies(mech)
    with mp.workdps(HP.DPS):
        S = SimStep(mech, cstate, dt, mp.mpf(HP.HSTEP), m, J, damp)
        start = HP._twist_of(cstate, nb) if mech == "FB" else s64
        s, _, k, nf, nds = S.iterate(HP._mpv(start), [mp.mpf(0)] * S.P.nd, HP.REG[mech], 60, mp.mpf(HP.STOP), mp.mpf(HP.HSTEP))
        if not (nf < mp.mpf(HP.STOP) and nds < mp.mpf(HP.STOP)):
            raise RuntimeError(f"high-precision step did not converge: |f| {mp.nstr(nf, 3)}, |ds| {mp.nstr(nds, 3)}")
        out = HP._f64(s)
    A = max(float(np.max(np.abs(HP._twist_of(cstate, nb)))), float(np.max(np.abs(out))))
    return dict(s=out, A=A, steps=k)


def _reversed_name(mech):
    """Registers the mechanism with its bodies in reverse order in the test's own copy of gprx/vi.py."""
    name = mech + "_rev"
    if name not in VI.MECHANISMS:
        M = VI.MECHANISMS[mech]
        nb = M["nb"]
        r = lambda b: 0 if b == 0 else nb + 1 - b  # noqa: E731
        VI.MECHANISMS[name] = dict(nb=nb, m=list(M["m"])[::-1], J=list(M["J"])[::-1],
                                   joints=[(k, r(a), r(b), pa, pb, ax) for k, a, b, pa, pb, ax in M["joints"]])
        VI.REGULARIZER[name] = VI.REGULARIZER[mech]
    return name


def evaluations(mech, cstate, dt, m, J, damp):
    """{name: (twist (6 nb), iterations, status)} of the fp64 CPU evaluations."""
    nb = HP.nbodies(mech)
    cs = np.asarray(cstate, dtype=np.float64)
    with HP.quiet():
        sol, it, st = VI.vi_step(mech, cs[None], dt, m=m, J=J, damp=damp)
        rev = lambda a: np.ascontiguousarray(np.asarray(a)[::-1])  # noqa: E731
        rs, rit, rst = VI.vi_step(_reversed_name(mech), rev(cs.reshape(nb, 13)).reshape(1, -1), dt, m=rev(m), J=rev(J),
                                  damp=rev(np.asarray(damp).reshape(nb, 6)))
    back = HP._twist_of(rs[0], nb).reshape(nb, 6)[::-1].reshape(-1).copy()
    return {"lapack": (HP._twist_of(sol[0], nb), int(it[0]), int(st[0])), "rev": (back, int(rit[0]), int(rst[0]))}


def half_torque(damp):
    """The seeded fault: the torque enters the rotational row as tau instead of 2 tau (c_w halved:
    2 (c_w / 2) w = c_w w exactly)."""
    d = np.array(damp, dtype=np.float64).copy()
    d[..., 3:6] *= 0.5
    return d


def cases(mech):
    """[(name, cstate (13 nb), m (nb,), J (nb, 3, 3), damp (nb, 6))]."""
    D = HP._load_gprx("data")
    nb = HP.nbodies(mech)
    out = []
    for ci, name in enumerate(CASES):
        rng = np.random.default_rng(7000 + 10 * HP.MECHS.index(mech) + ci)
        cs = D._cstates(mech, D._sample_minimal(mech, 1, rng))[:, 0].copy()
        if name == "nominal":
            m, J = VI.body_params(mech)
            damp = VI.friction_damp(mech)
        else:
            sgn = np.array([1.0 if b % 2 == 0 else -1.0 for b in range(nb)])
            m, J = VI.body_params(mech, 1 + 0.1 * sgn, 1 - 0.1 * sgn)
            damp = VI.friction_damp(mech, FRICTION_MAX[mech])
        out.append((name, cs, m, J, damp))
    return out


def error_scale(ev, tr):
    errs = np.array([float(np.max(np.abs(ev[v][0] - tr))) for v in ("lapack", "rev")])
    return H.geomean(errs), errs


def load(mech):
    return dict(np.load(GOLDEN / f"hp_sim_{mech}.npz"))


def k_of(mech):
    return float(np.load(GOLDEN / f"hp_phys_{mech}.npz")["k"])
