"""HIGH-PRECISION ORACLE of the rollout physics -- test infrastructure only (imported by tests/ and
tests/golden/make_golden_hp_physics.py; never by the product path).

The two Newton solves of gprx_projection.hip (k_project / project<NW>, k_vi_step / vi_newton) held
to a truth that shares no derivative and no LU code with them or with their fp64 restatements:

truth_projectv()  the KKT point of  min |s - s_u|^2  s.t.  g(x3(s), q3(s)) = 0
                  (oracle/projection_oracle.py's docstring): s - s_u + G(s)^T lambda = 0, g = 0.
truth_vi()        the root of the variational-integrator step's system (gprx/vi.py's docstring):
                  the dynamics rows with Gpos = dg/d(x, phi) fixed at pose 2, and g(x3, q3) = 0.
Both are written from those equations in mpmath arithmetic (DPS = 70 working digits, so that the
1e-40 stopping rule and the differences below have room; at least the 50 the GP truth uses).  Only
the constraint FUNCTION g(x, q) is stated; every derivative (G = dg/ds, Gpos, the step's Newton
matrix) is a central difference of the high-precision function with step H = 1e-25 (truncation
~H^2 = 1e-50, cancellation 10^-DPS / H = 1e-45).  Newton starts from an fp64 solution and stops when
|f| and |ds| are below 1e-40; the result is rounded to fp64 once.
  * projectv's Newton matrix is projectv!'s own, [I G^T; G 0] with the numerically differentiated
    G: it leaves out lambda . d2g/ds2, so the iteration converges linearly (a factor ~1e-3 per step,
    a dozen steps), to the same fixed point -- the residual alone decides that.  Differentiating
    the residual's G^T lambda term once more would cost 6 nb times as many evaluations for nothing.
  * the step's matrix is the full numerical Jacobian of its residual (the lambda columns, in which
    the residual is linear, are written down: -Gpos^T).
  * the four-bar's loop constraints are redundant: the experiments' regulariser 1e-10 stands in the
    Newton matrix only (as on the device and in the restatements), the residual has no such term,
    so projectv's fixed point is the unregularised KKT point's twist; the multipliers are not
    unique and only the twists (v, w) are compared.  The four-bar's STEP has no unique root at all
    (truth_vi says why): its truth is the limit of the regularised iteration from the documented
    start, which is what newton! computes.
iterate_projectv() / iterate_vi()  the k-th iterate of the two documented iterations from their
                  documented start, in the same arithmetic: the truth for newton_iter = 1, 2.

variants_projectv() / variants_vi()  the legitimate fp64 evaluations:
    "lapack"  oracle.projection_oracle.projectv / gprx.vi.vi_step as they stand (LAPACK getrf)
    "dgetf2"  the same Newton loop over a numpy restatement of the device's LU order: dgetf2
              right-looking, first maximal pivot, reciprocal scaling, dgetrs' substitutions
    "qr"      the loop over a Householder QR solve (no LU at all); for the fixtures' converged records
              it runs to eps = 0 (qr_eps), 100 iterations -- what the iteration converges to, not
              where eps stops it
    "rev"     "lapack" with the bodies (and so the unknowns and the columns of G) in reverse order
    `fault` seeds one subtle defect into "dgetf2" (FAULTS; tests/test_hp_physics_oracle.py).
bound: hp_oracle.bound(E, A, k) = k max(E, eps A).  E: the geometric mean over the variants of
their largest twist error against the truth, per mechanism and case; A = max(|s_start|inf, |s|inf),
one rounding of the largest operand of the last s - ds; k the largest variant ratio over all
fixtures, a power of two >= 4.  All fixed from the CPU variants when the fixtures are generated.
"""
from __future__ import annotations

import contextlib
import importlib.util
import pathlib
import sys

import mpmath
import numpy as np
import scipy.linalg as sla

from oracle import hp_oracle as H
from oracle import projection_oracle as PO

mp = mpmath.mp
DPS = 70
HSTEP = "1e-25"
STOP = "1e-40"
VARIANTS = ("lapack", "dgetf2", "qr", "rev")
MECHS = ("P1", "P2", "CP", "FB")
REG = {"P1": 0.0, "P2": 0.0, "CP": 0.0, "FB": 1e-10}
# name -> what it does; seeded into the "dgetf2" variant of both solves
FAULTS = {
    "pb_scaled_1e-9": "the first joint offset pb times (1 + 1e-9)",
    "q3_halfdt_1e-10": "q3's dt/2 times (1 + 1e-10)",
    "gravity_9.80665": "standard gravity 9.80665 for the experiments' 9.81 (the step only)",
    "x3_from_xc": "x3 = xc + v dt instead of xk + v dt",
    "wbar_drops_ww": "the last body's wbar(w) = (sqrt(4/dt^2), w), w.w dropped",
    # the first three scaled down until the fixed 1e-9 bounds of test_projection.py / test_vi_device.py
    # accept them (tests/test_hp_physics_oracle.py: the gap these fixtures close)
    "pb_scaled_1e-12": "the first joint offset pb times (1 + 1e-12)",
    "q3_halfdt_1e-12": "q3's dt/2 times (1 + 1e-12)",
    "gravity_1e-9": "gravity 9.81 (1 + 1e-9) (the step only)",
}
_PB = {"pb_scaled_1e-9": 1e-9, "pb_scaled_1e-12": 1e-12}
_Q3 = {"q3_halfdt_1e-10": 1e-10, "q3_halfdt_1e-12": 1e-12}
_GRAV = {"gravity_9.80665": 9.80665, "gravity_1e-9": 9.81 * (1.0 + 1e-9)}


def _load_gprx(name):
    """gprx/<name>.py by file path (numpy only): the library need not be built."""
    key = f"_hp_physics_gprx_{name}"
    if key not in sys.modules:
        path = pathlib.Path(__file__).resolve().parents[1] / "gpr.jl_amd" / "gprx" / f"{name}.py"
        spec = importlib.util.spec_from_file_location(key, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[key] = mod
        spec.loader.exec_module(mod)
    return sys.modules[key]


VI = _load_gprx("vi")


class Singular(Exception):
    pass


# ---- the mechanisms ----------------------------------------------------------------------------
def joints_of(mech: str):
    """The flat sub-joint list (kind, a, b, pa, pb, axis); the projection's and the step's agree."""
    j = [s for eqc in PO.mechanism(mech)["eqcs"] for s in eqc]
    jv = VI.MECHANISMS[mech]["joints"]
    assert len(j) == len(jv) and all(a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
                                     and np.array_equal(a[5], b[5]) for a, b in zip(j, jv))
    return j


def nbodies(mech: str) -> int:
    return PO.mechanism(mech)["nb"]


# ---- high-precision pieces: only the constraint function and the x3 / q3 maps --------------------
def _mpv(a):
    return [mp.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def _f64(a):
    return np.array([float(v) for v in a], dtype=np.float64)


def _qmul(p, q):
    return (p[0] * q[0] - (p[1] * q[1] + p[2] * q[2] + p[3] * q[3]),
            p[0] * q[1] + q[0] * p[1] + (p[2] * q[3] - p[3] * q[2]),
            p[0] * q[2] + q[0] * p[2] + (p[3] * q[1] - p[1] * q[3]),
            p[0] * q[3] + q[0] * p[3] + (p[1] * q[2] - p[2] * q[1]))


def _qconj(q):
    return (q[0], -q[1], -q[2], -q[3])


def _rot(q, p):
    """R(q) p = (q0^2 - |qv|^2) p + 2 qv (qv.p) + 2 q0 qv x p."""
    c = q[0] * q[0] - (q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    d = q[1] * p[0] + q[2] * p[1] + q[3] * p[2]
    cr = (q[2] * p[2] - q[3] * p[1], q[3] * p[0] - q[1] * p[2], q[1] * p[1] - q[2] * p[0])
    return [c * p[k] + 2 * q[1 + k] * d + 2 * q[0] * cr[k] for k in range(3)]


def _step_q(q, w, dt):
    """q * wbar(w) * dt / 2, wbar(w) = (sqrt(4/dt^2 - w.w), w)."""
    wb = (mp.sqrt(4 / (dt * dt) - (w[0] * w[0] + w[1] * w[1] + w[2] * w[2])), w[0], w[1], w[2])
    return tuple(c * dt / 2 for c in _qmul(q, wb))


def _g(joints, x, q):
    """g at the poses x[b], q[b] (b 0-based; parent 0 is the origin)."""
    out = []
    for kind, a, b, pa, pb, axis in joints:
        xa, qa = ([mp.mpf(0)] * 3, (mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0))) if a == 0 else (x[a - 1], q[a - 1])
        xb, qb = x[b - 1], q[b - 1]
        if kind[0] == "T":
            r = _rot(qb, _mpv(pb))
            e = _rot(_qconj(qa), [xb[k] + r[k] - xa[k] for k in range(3)])
            e = [e[k] - mp.mpf(float(pa[k])) for k in range(3)]
        else:
            e = _qmul(_qconj(qa), qb)[1:]
        for row in PO.cmat(kind, axis):
            out.append(sum((mp.mpf(float(row[k])) * e[k] for k in range(3)), mp.mpf(0)))
    return out


def _norm(v):
    return mp.sqrt(sum((t * t for t in v), mp.mpf(0)))


def _solve(F, f):
    return list(mp.lu_solve(mp.matrix(F), mp.matrix(f)))  # mpmath's own elimination


class _Pose:
    """The discrete pose (x2, q2) of a CState in high precision, and g at the next pose of a twist."""

    def __init__(self, mech, cstate, dt):
        self.joints, self.nb = joints_of(mech), nbodies(mech)
        self.dt = mp.mpf(float(dt))
        c = np.asarray(cstate, dtype=np.float64).reshape(self.nb, 13)
        self.x1, self.q1 = [_mpv(c[b, 0:3]) for b in range(self.nb)], [tuple(_mpv(c[b, 3:7])) for b in range(self.nb)]
        self.v1, self.w1 = [_mpv(c[b, 7:10]) for b in range(self.nb)], [_mpv(c[b, 10:13]) for b in range(self.nb)]
        self.x2 = [[self.x1[b][k] + self.v1[b][k] * self.dt for k in range(3)] for b in range(self.nb)]
        self.q2 = [_step_q(self.q1[b], self.w1[b], self.dt) for b in range(self.nb)]
        self.nd = len(_g(self.joints, self.x2, self.q2))

    def g3(self, s):
        x3 = [[self.x2[b][k] + s[6 * b + k] * self.dt for k in range(3)] for b in range(self.nb)]
        q3 = [_step_q(self.q2[b], s[6 * b + 3:6 * b + 6], self.dt) for b in range(self.nb)]
        return _g(self.joints, x3, q3)

    def dg3(self, s, h):
        """G = dg/ds (nd x 6 nb) by central differences."""
        cols = []
        for j in range(6 * self.nb):
            sp, sm = list(s), list(s)
            sp[j], sm[j] = s[j] + h, s[j] - h
            gp, gm = self.g3(sp), self.g3(sm)
            cols.append([(a - b) / (2 * h) for a, b in zip(gp, gm)])
        return [[cols[j][r] for j in range(6 * self.nb)] for r in range(self.nd)]

    def gpos(self, h):
        """Gpos = dg/d(x_1, phi_1, ...) at pose 2, phi: q -> q * (1, phi), by central differences."""
        cols = []
        for b in range(self.nb):
            for k in range(6):
                res = []
                for sgn in (1, -1):
                    x, q = [list(v) for v in self.x2], list(self.q2)
                    if k < 3:
                        x[b][k] = x[b][k] + sgn * h
                    else:
                        ph = [mp.mpf(0)] * 3
                        ph[k - 3] = sgn * h
                        q[b] = _qmul(q[b], (mp.mpf(1), ph[0], ph[1], ph[2]))
                    res.append(_g(self.joints, x, q))
                cols.append([(a - c) / (2 * h) for a, c in zip(*res)])
        return [[cols[j][r] for j in range(6 * self.nb)] for r in range(self.nd)]


# ---- projectv! -------------------------------------------------------------------------------------
def _pj_residual(P, su, s, lam, G):
    n6 = 6 * P.nb
    top = [s[j] - su[j] + sum((G[r][j] * lam[r] for r in range(P.nd)), mp.mpf(0)) for j in range(n6)]
    return top + P.g3(s)


def _pj_iterate(P, su, s, lam, reg, steps, stop, h):
    """projectv!'s iteration z <- z - [I + reg, G^T; G, reg] \\ f(z) with G and f at z, for `steps`
    steps or until |f| and |ds| < stop.  Returns s, lam, the steps taken, the last |f| and |ds|."""
    n6, nd = 6 * P.nb, P.nd
    n = n6 + nd
    reg = mp.mpf(float(reg))
    nf = nds = mp.inf
    k = 0
    while k < steps:
        G = P.dg3(s, h)
        f = _pj_residual(P, su, s, lam, G)
        nf = _norm(f)
        if stop is not None and nf < stop and nds < stop:
            break
        F = [[mp.mpf(0)] * n for _ in range(n)]
        for i in range(n):
            F[i][i] = (1 if i < n6 else 0) + reg
        for r in range(nd):
            for j in range(n6):
                F[n6 + r][j] = F[j][n6 + r] = G[r][j]
        ds = _solve(F, f)
        s = [a - b for a, b in zip(s, ds[:n6])]
        lam = [a - b for a, b in zip(lam, ds[n6:])]
        nds = _norm(ds[:n6])  # the twist's step: the four-bar's multipliers are not unique
        k += 1
    return s, lam, k, nf, nds


def truth_projectv(mech, cstate, su, dt, s64, reg=None):
    """The KKT point next to the fp64 solution s64.  Returns dict(s: fp64 (6 nb), A, steps, f, ds)."""
    with mp.workdps(DPS):
        P = _Pose(mech, cstate, dt)
        s, lam, k, nf, nds = _pj_iterate(P, _mpv(su), _mpv(s64), [mp.mpf(0)] * P.nd, REG[mech] if reg is None else reg,
                                         200, mp.mpf(STOP), mp.mpf(HSTEP))
        if not (nf < mp.mpf(STOP) and nds < mp.mpf(STOP)):
            raise RuntimeError(f"high-precision projectv did not converge: |f| {mp.nstr(nf, 3)}, |ds| {mp.nstr(nds, 3)}")
        out = _f64(s)
    A = max(float(np.max(np.abs(su))), float(np.max(np.abs(out))))
    return dict(s=out, A=A, steps=k, f=float(nf), ds=float(nds), _s=s, _lam=lam)


def iterate_projectv(mech, cstate, su, dt, steps, reg=None):
    """The twist after `steps` steps of projectv!'s iteration from (s_u, lambda = 0)."""
    with mp.workdps(DPS):
        P = _Pose(mech, cstate, dt)
        s, _, k, _, _ = _pj_iterate(P, _mpv(su), _mpv(su), [mp.mpf(0)] * P.nd, REG[mech] if reg is None else reg, steps,
                                    None, mp.mpf(HSTEP))
        assert k == steps
        out = _f64(s)
    return dict(s=out, A=max(float(np.max(np.abs(su))), float(np.max(np.abs(out)))))


def kkt_defect(mech, cstate, su, dt, tr):
    """(|g|, |s - s_u + G^T lambda|) of a truth_projectv record's unrounded point, re-evaluated at
    80 digits with another difference step."""
    with mp.workdps(80):
        P = _Pose(mech, cstate, dt)
        f = _pj_residual(P, _mpv(su), tr["_s"], tr["_lam"], P.dg3(tr["_s"], mp.mpf("1e-30")))
        n6 = 6 * P.nb
        return float(_norm(f[n6:])), float(_norm(f[:n6]))


# ---- the variational-integrator step ---------------------------------------------------------------
class _Step:
    def __init__(self, mech, cstate, dt, h):
        self.P = P = _Pose(mech, cstate, dt)
        M = VI.MECHANISMS[mech]
        self.m = _mpv(M["m"])
        self.J = [[_mpv(Jb[i]) for i in range(3)] for Jb in M["J"]]
        self.grav = mp.mpf(float(VI.GRAV))
        self.G = P.gpos(h)
        self.mom1 = []
        for b in range(P.nb):
            w1 = P.w1[b]
            Jw = [sum((self.J[b][i][k] * w1[k] for k in range(3)), mp.mpf(0)) for i in range(3)]
            sq1 = mp.sqrt(4 / (P.dt * P.dt) - sum((t * t for t in w1), mp.mpf(0)))
            cr = (w1[1] * Jw[2] - w1[2] * Jw[1], w1[2] * Jw[0] - w1[0] * Jw[2], w1[0] * Jw[1] - w1[1] * Jw[0])
            self.mom1.append([sq1 * Jw[i] - cr[i] for i in range(3)])

    def residual(self, s, lam):
        P = self.P
        d = []
        for b in range(P.nb):
            v2, w2 = s[6 * b:6 * b + 3], s[6 * b + 3:6 * b + 6]
            for c in range(3):
                d.append(self.m[b] * ((v2[c] - P.v1[b][c]) / P.dt + (self.grav if c == 2 else 0)))
            Jw = [sum((self.J[b][i][k] * w2[k] for k in range(3)), mp.mpf(0)) for i in range(3)]
            sq2 = mp.sqrt(4 / (P.dt * P.dt) - sum((t * t for t in w2), mp.mpf(0)))
            cr = (w2[1] * Jw[2] - w2[2] * Jw[1], w2[2] * Jw[0] - w2[0] * Jw[2], w2[0] * Jw[1] - w2[1] * Jw[0])
            for i in range(3):
                d.append(sq2 * Jw[i] + cr[i] - self.mom1[b][i])
        for j in range(6 * P.nb):
            d[j] = d[j] - sum((self.G[r][j] * lam[r] for r in range(P.nd)), mp.mpf(0))
        return d + P.g3(s)

    def iterate(self, s, lam, reg, steps, stop, h):
        P = self.P
        n6, nd = 6 * P.nb, P.nd
        n = n6 + nd
        reg = mp.mpf(float(reg))
        nf = nds = mp.inf
        k = 0
        while k < steps:
            f = self.residual(s, lam)
            nf = _norm(f)
            if stop is not None and nf < stop and nds < stop:
                break
            F = [[mp.mpf(0)] * n for _ in range(n)]
            for j in range(n6):
                sp, sm = list(s), list(s)
                sp[j], sm[j] = s[j] + h, s[j] - h
                fp, fm = self.residual(sp, lam), self.residual(sm, lam)
                for i in range(n):
                    F[i][j] = (fp[i] - fm[i]) / (2 * h)
            for r in range(nd):
                for j in range(n6):
                    F[j][n6 + r] = -self.G[r][j]
                F[n6 + r][n6 + r] = -reg
            ds = _solve(F, f)
            s = [a - b for a, b in zip(s, ds[:n6])]
            lam = [a - b for a, b in zip(lam, ds[n6:])]
            nds = _norm(ds[:n6])
            k += 1
        return s, lam, k, nf, nds


def _twist_of(cstate, nb):
    return np.asarray(cstate, dtype=np.float64).reshape(nb, 13)[:, 7:13].reshape(-1).copy()


def truth_vi(mech, cstate, dt, s64, reg=None):
    """The step's root next to the fp64 solution twist s64 (6 nb: v2, w2 per body).
    The four-bar is the exception.  Its pose 2 = x1 + v1 dt lies off the constraint manifold (by
    (w dt)^2 / 2 for a generator state), where Gpos has full rank 24 while g(x3, q3) = 0 holds only 22
    independent equations: every twist on the constraint manifold is a root with some lambda, and
    which of them newton! reaches is decided by the regularised iteration's path.  Its truth is
    therefore the limit of that iteration from the documented start (the current velocities,
    lambda = 0) in high precision, not the root nearest to one fp64 answer."""
    with mp.workdps(DPS):
        S = _Step(mech, cstate, dt, mp.mpf(HSTEP))
        start = _twist_of(cstate, S.P.nb) if mech == "FB" else s64
        s, lam, k, nf, nds = S.iterate(_mpv(start), [mp.mpf(0)] * S.P.nd, REG[mech] if reg is None else reg, 60,
                                       mp.mpf(STOP), mp.mpf(HSTEP))
        if not (nf < mp.mpf(STOP) and nds < mp.mpf(STOP)):
            raise RuntimeError(f"high-precision step did not converge: |f| {mp.nstr(nf, 3)}, |ds| {mp.nstr(nds, 3)}")
        out = _f64(s)
    A = max(float(np.max(np.abs(_twist_of(cstate, S.P.nb)))), float(np.max(np.abs(out))))
    return dict(s=out, A=A, steps=k, f=float(nf), ds=float(nds), _s=s, _lam=lam)


def iterate_vi(mech, cstate, dt, steps, reg=None):
    """The twist after `steps` Newton steps from the current velocities and lambda = 0."""
    nb = nbodies(mech)
    s0 = _twist_of(cstate, nb)
    with mp.workdps(DPS):
        S = _Step(mech, cstate, dt, mp.mpf(HSTEP))
        s, _, k, _, _ = S.iterate(_mpv(s0), [mp.mpf(0)] * S.P.nd, REG[mech] if reg is None else reg, steps, None,
                                  mp.mpf(HSTEP))
        assert k == steps
        out = _f64(s)
    return dict(s=out, A=max(float(np.max(np.abs(s0))), float(np.max(np.abs(out)))))


def root_defect(mech, cstate, dt, tr):
    """(|g|, |dynamics rows|) of a truth_vi record's unrounded point at 80 digits, Gpos by another
    difference step."""
    with mp.workdps(80):
        S = _Step(mech, cstate, dt, mp.mpf("1e-30"))
        f = S.residual(tr["_s"], tr["_lam"])
        n6 = 6 * S.P.nb
        return float(_norm(f[n6:])), float(_norm(f[:n6]))


# ---- fp64 variants -------------------------------------------------------------------------------------
DBL_MIN = float(np.finfo(np.float64).tiny)


def solve_lapack(F, f):
    return sla.lu_solve(sla.lu_factor(F, check_finite=False), f, check_finite=False)


def solve_dgetf2(F, f):
    """The device's lu_solve: dgetf2 (right-looking, first maximal |pivot|, reciprocal scaling unless
    the pivot is subnormal, rank-1 update) and dgetrs' unit-lower / upper substitutions, which skip
    a zero right-hand-side entry.  Raises Singular on an exactly zero pivot."""
    A, b = np.array(F, dtype=np.float64), np.array(f, dtype=np.float64)
    n = len(b)
    singular = False
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            b[[k, p]] = b[[p, k]]
        akk = A[k, k]
        if akk == 0.0:
            singular = True
        elif k < n - 1:
            A[k + 1:, k] = A[k + 1:, k] * (1.0 / akk) if abs(akk) >= DBL_MIN else A[k + 1:, k] / akk
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(A[k + 1:, k], A[k, k + 1:])
    if singular:
        raise Singular
    for k in range(n):
        if b[k] != 0.0:
            b[k + 1:] = b[k + 1:] - b[k] * A[k + 1:, k]
    for k in range(n - 1, -1, -1):
        if b[k] != 0.0:
            b[k] = b[k] / A[k, k]
            b[:k] = b[:k] - b[k] * A[:k, k]
    return b


def solve_qr(F, f):
    Q, R = np.linalg.qr(F)
    return sla.solve_triangular(R, Q.T @ f, check_finite=False)


def _faulty_state(fault, nb):
    class St(PO.State):
        def x3(self, b):
            return (self.xc[b] if fault == "x3_from_xc" else self.xk[b]) + self.vsol[b] * self.dt

        def q3(self, b):
            w = self.wsol[b]
            if fault == "wbar_drops_ww" and b == nb - 1:
                return PO.qmul(self.qk[b], np.concatenate([[np.sqrt(4.0 / self.dt ** 2)], w])) * self.dt / 2.0
            return PO.wbar_step(self.qk[b], w, self.dt) * (1.0 + _Q3.get(fault, 0.0))

    return St


def _faulty_joints(joints, fault):
    """joints with the first non-zero pb scaled, for the pb faults."""
    out, done = [], False
    for kind, a, b, pa, pb, axis in joints:
        if fault in _PB and not done and any(pb):
            pb, done = tuple(np.asarray(pb) * (1.0 + _PB[fault])), True
        out.append((kind, a, b, pa, pb, axis))
    return out


def projectv_loop(mech, cstate, su, dt, reg, iters, eps, solve, fault=None):
    """projection_oracle.projectv's loop over `solve`: (s (6 nb), iterations, the iterates)."""
    m = PO.mechanism(mech)
    nb = m["nb"]
    if fault in _PB:
        m = dict(nb=nb, eqcs=[_faulty_joints([s for eqc in m["eqcs"] for s in eqc], fault)])  # the same rows, one list
    st = (_faulty_state(fault, nb) if fault else PO.State)(cstate, nb, dt)
    nd, n6 = PO.ndims(m), 6 * nb
    F = np.zeros((n6 + nd, n6 + nd))
    F[np.arange(n6), np.arange(n6)] = 1.0
    F = F + np.eye(n6 + nd) * reg
    s = np.zeros(n6 + nd)
    s[:n6] = su
    PO._set_solution(st, s)

    def f(s):
        return np.concatenate([-su + s[:n6] + F[n6:, :n6].T @ s[n6:], PO.constraints(m, st)])

    it, path = 0, []
    for it in range(1, iters + 1):
        G = PO.jacobian(m, st)
        F[n6:, :n6] = G
        F[:n6, n6:] = G.T
        ds = solve(F, f(s))
        s = s - ds
        PO._set_solution(st, s)
        path.append(s[:n6].copy())
        if np.linalg.norm(f(s)) < eps and np.linalg.norm(ds) < eps:
            break
    return s[:n6].copy(), it, path


def _reverse_mech(m):
    nb = m["nb"]
    r = lambda b: 0 if b == 0 else nb + 1 - b  # noqa: E731
    return dict(nb=nb, eqcs=[[(k, r(a), r(b), pa, pb, ax) for k, a, b, pa, pb, ax in eqc] for eqc in m["eqcs"]])


def _rev_rows(a, nb):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(nb, -1)[::-1]).reshape(-1)


def variants_projectv(mech, cstate, su, dt, iters=100, eps=1e-10, fault=None, reg=None, qr_eps=None):
    """{name: (s (6 nb), iterations)}.  qr_eps: the "qr" variant's own eps (None: `eps`); the
    fixtures' converged records pass 0, so that "qr" runs all `iters` iterations.  With `fault`, only
    the seeded "dgetf2"."""
    reg = REG[mech] if reg is None else reg
    nb = nbodies(mech)
    cs, su = np.asarray(cstate, dtype=np.float64), np.asarray(su, dtype=np.float64)
    if fault is not None:
        assert fault in FAULTS
        return {"dgetf2": projectv_loop(mech, cs, su, dt, reg, iters, eps, solve_dgetf2, fault)[:2]}
    m = PO.mechanism(mech)

    def po(mm, c, u):
        v, w, it = PO.projectv(mm, PO.State(c, nb, dt), list(u.reshape(nb, 6)[:, :3]), list(u.reshape(nb, 6)[:, 3:]),
                               newton_iter=iters, eps=eps, regularizer=reg)
        return np.concatenate([np.concatenate([v[b], w[b]]) for b in range(nb)]), it

    out = {"lapack": po(m, cs, su) if iters > 0 else (su.copy(), 0),
           "dgetf2": projectv_loop(mech, cs, su, dt, reg, iters, eps, solve_dgetf2)[:2],
           "qr": projectv_loop(mech, cs, su, dt, reg, iters, eps if qr_eps is None else qr_eps, solve_qr)[:2]}
    s, it = po(_reverse_mech(m), _rev_rows(cs, nb), _rev_rows(su, nb)) if iters > 0 else (su.copy(), 0)
    out["rev"] = (_rev_rows(s, nb), it)
    return out


def vi_loop(mech, cstate, dt, reg, iters, eps, solve, fault=None, order=None):
    """gprx.vi.vi_step's Newton loop for one state over `solve` (the same pieces: jac_phi, constraints,
    step_q, _dphi_dw; the dynamics block as vi.py writes it).  order: a permutation of the bodies.
    Returns (s (6 nb: v2, w2 per body), iterations, status, the iterates); status as vi_step's."""
    M = VI.MECHANISMS[mech]
    nb = M["nb"]
    joints = _faulty_joints(M["joints"], fault)
    m, J = np.asarray(M["m"], dtype=np.float64), np.stack(M["J"])
    c = np.asarray(cstate, dtype=np.float64).reshape(1, nb, 13)
    if order is not None:
        r = {0: 0, **{old + 1: new + 1 for new, old in enumerate(order)}}
        joints = [(k, r[a], r[b], pa, pb, ax) for k, a, b, pa, pb, ax in joints]
        c, m, J = c[:, order], m[list(order)], J[list(order)]
    mech_d = dict(nb=nb, joints=joints)
    grav = _GRAV.get(fault, VI.GRAV)
    x1, q1, v1, w1 = c[..., 0:3], c[..., 3:7], c[..., 7:10], c[..., 10:13]
    x2, q2 = x1 + v1 * dt, VI.step_q(q1, w1, dt)
    n6 = 6 * nb
    Gpos = VI.jac_phi(mech_d, x2, q2)[0]
    nd = Gpos.shape[0]
    Jw1 = np.einsum("bij,tbj->tbi", J, w1)
    sq1 = np.sqrt(4.0 / dt ** 2 - np.sum(w1 * w1, axis=-1))
    mom1 = sq1[..., None] * Jw1 - np.cross(w1, Jw1)

    def q3_of(w2):
        q3 = VI.step_q(q2, w2, dt) * (1.0 + _Q3.get(fault, 0.0))
        if fault == "wbar_drops_ww":
            wb = np.concatenate([[np.sqrt(4.0 / dt ** 2)], w2[0, nb - 1]])
            q3[0, nb - 1] = VI.qmul(q2[0, nb - 1], wb) * (dt / 2.0)
        return q3

    def residual(v2, w2, lam):
        Jw2 = np.einsum("bij,tbj->tbi", J, w2)
        sq2 = np.sqrt(4.0 / dt ** 2 - np.sum(w2 * w2, axis=-1))
        dT = m[None, :, None] * ((v2 - v1) / dt + np.array([0.0, 0.0, grav]))
        dR = sq2[..., None] * Jw2 + np.cross(w2, Jw2) - mom1
        d = np.concatenate([dT, dR], axis=-1).reshape(n6) - Gpos.T @ lam
        x3 = (x1 if fault == "x3_from_xc" else x2) + v2 * dt
        q3 = q3_of(w2)
        return np.concatenate([d, VI.constraints(mech_d, x3, q3)[0]]), Jw2, sq2, x3, q3

    v2, w2, lam = v1.copy(), w1.copy(), np.zeros(nd)
    it, status, path = 0, 1, []

    def twist():
        s = np.concatenate([v2[0], w2[0]], axis=-1)  # (nb, 6)
        if order is not None:
            back = np.empty_like(s)
            back[list(order)] = s
            s = back
        return s.reshape(-1).copy()

    for k in range(1, iters + 1):
        f, Jw2, sq2, x3, q3 = residual(v2, w2, lam)
        F = np.zeros((n6 + nd, n6 + nd))
        for b in range(nb):
            o = 6 * b
            wb = w2[0, b]
            F[o:o + 3, o:o + 3] = np.eye(3) * (m[b] / dt)
            F[o + 3:o + 6, o + 3:o + 6] = (sq2[0, b] * J[b] + VI.skew(wb) @ J[b] - VI.skew(Jw2[0, b])
                                           - np.outer(Jw2[0, b], wb) / sq2[0, b])
        F[:n6, n6:] = -Gpos.T
        Gphi3 = VI.jac_phi(mech_d, x3, q3)[0]
        for b in range(nb):
            o = 6 * b
            F[n6:, o:o + 3] = Gphi3[:, o:o + 3] * dt
            F[n6:, o + 3:o + 6] = Gphi3[:, o + 3:o + 6] @ VI._dphi_dw(q2[:, b], q3[:, b], w2[:, b], dt)[0]
        if reg:
            F[n6:, n6:] -= reg * np.eye(nd)
        if not (np.all(np.isfinite(F)) and np.all(np.isfinite(f))):
            status = 2
            break
        try:
            ds = solve(F, f)
        except (Singular, np.linalg.LinAlgError):
            status = 2
            break
        if not np.all(np.isfinite(ds)):
            status = 2
            break
        v2 = v2 - ds[:n6].reshape(1, nb, 6)[..., 0:3]
        w2 = w2 - ds[:n6].reshape(1, nb, 6)[..., 3:6]
        lam = lam - ds[n6:]
        it = k
        path.append(twist())
        if np.linalg.norm(residual(v2, w2, lam)[0]) < eps and np.linalg.norm(ds) < eps:
            status = 0
            break
    return twist(), it, status, path


def variants_vi(mech, cstate, dt, iters=100, eps=1e-10, fault=None, reg=None, qr_eps=None):
    """{name: (s (6 nb), iterations, status)}, as variants_projectv."""
    reg = REG[mech] if reg is None else reg
    nb = nbodies(mech)
    cs = np.asarray(cstate, dtype=np.float64)
    if fault is not None:
        assert fault in FAULTS
        return {"dgetf2": vi_loop(mech, cs, dt, reg, iters, eps, solve_dgetf2, fault)[:3]}
    assert reg == VI.REGULARIZER[mech]
    sol, it, st = VI.vi_step(mech, cs[None], dt, eps, iters)
    return {"lapack": (_twist_of(sol[0], nb), int(it[0]), int(st[0])),
            "dgetf2": vi_loop(mech, cs, dt, reg, iters, eps, solve_dgetf2)[:3],
            "qr": vi_loop(mech, cs, dt, reg, iters, eps if qr_eps is None else qr_eps, solve_qr)[:3],
            "rev": vi_loop(mech, cs, dt, reg, iters, eps, solve_lapack, order=tuple(range(nb))[::-1])[:3]}


# ---- bounds ------------------------------------------------------------------------------------------
def error_scale(results, truth):
    """(E, the variants' largest errors) of {name: (s, ...)} against a truth twist."""
    errs = np.array([float(np.max(np.abs(results[v][0] - truth))) for v in VARIANTS])
    return H.geomean(errs), errs


def ratio(err, E, A):
    return H.ratio(err, E, H.EPS * A)


@contextlib.contextmanager
def quiet():
    with np.errstate(invalid="ignore", divide="ignore"):
        yield
