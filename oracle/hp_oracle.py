"""HIGH-PRECISION ORACLE -- test infrastructure only (imported by tests/ and tests/golden/make_golden_hp.py;
never by the product path).

truth()    the exact-GP quantities of gp_oracle.py's docstrings (update_cK!, update_mll!, update_dmll!,
           predict_f with and without full_cov), written from those formulas in 50-digit mpmath
           arithmetic ("mp") or in x87 extended precision ("ld", np.longdouble, eps 2^-63, for the sizes
           where mpmath is too slow), and rounded to fp64 once.  It forms exact differences, so it does
           not depend on the distance mode.  With every scalar output q it returns A_q, the sum of the
           absolute values of the terms of q's last reduction: eps A_q is what rounding that one sum in
           fp64 can cost, the floor of every bound.
variants() the legitimate fp64 evaluations of the same quantities in one distance mode:
           "lapack"   gp_oracle's lml and predict_f per target (fit's pieces; fit itself is asserted
                      bit-equal on the first target) plus the K** - V^T V of those pieces
           "explicit" Cholesky and L^-1 formed explicitly over 64-row tiles along the device's
                      recursion (h = n / 2), alpha = L^-T (L^-1 y), K^-1 = L^-T L^-1, V = L^-1 K*
           "staged"   "explicit" over the Gram and cross-covariance as the device forms them (DESIGN.md
                      section 2): coordinates pre-scaled by sqrt(il2/2) in direct mode, sf2 folded into
                      a table exp -- another rounding of K, which the first two share
           "lapack_rev", "staged_rev"  the same two over the training points in reverse order: a
                      scalar such as the LML is one draw of the rounding per variant, and three
                      variants that share K or the factorisation under-sample it (DESIGN.md section 2;
                      tests/test_hp_oracle.py measures the spread over point orders).  These two
                      because they share neither K's rounding nor the factorisation; "explicit"
                      shares the first with "lapack" and the second with "staged"
           `fault` seeds one subtle defect into "explicit" (FAULTS; tests/test_hp_oracle.py).
bound()    k max(E_q, eps A_q): E_q is the geometric mean over the variants of max |variant - truth|, k
           the largest ratio of a variant's error to max(E_q, eps A_q) over all fixtures (a power of two,
           >= 4), both fixed when the fixtures are generated from the CPU variants alone.  The gradient
           is also held per component, to k_grad max(E_grad[p], eps A_q[p]) formed the same way.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as O

EPS = O.EPS
TILE = 64
QUANTITIES = ("mll", "grad", "alpha", "mu", "var", "cov")
FAULTS = ("kinv_drop_last", "v_skip_col16", "ard_scale_1e-9", "k_entry_1e3ulp", "alpha_rows_short")


# ---- arithmetic backends ------------------------------------------------------------------------
class _MP:
    name = "mp"

    def __init__(self):
        import mpmath

        self.m = mpmath
        self._mpf = np.frompyfunc(mpmath.mpf, 1, 1)
        self.exp = np.frompyfunc(mpmath.exp, 1, 1)
        self.log = np.frompyfunc(mpmath.log, 1, 1)
        self.sqrt = np.frompyfunc(mpmath.sqrt, 1, 1)
        self._flt = np.frompyfunc(float, 1, 1)

    def arr(self, a):
        return self._mpf(np.asarray(a, dtype=np.float64))

    def zeros(self, shape):
        z = np.empty(shape, dtype=object)
        z[...] = self.m.mpf(0)
        return z

    def log2pi(self):
        return self.m.log(2 * self.m.pi)

    def f64(self, a):
        return np.asarray(self._flt(a), dtype=np.float64)


class _LD:
    name = "ld"
    exp, log, sqrt = staticmethod(np.exp), staticmethod(np.log), staticmethod(np.sqrt)

    def arr(self, a):
        return np.asarray(a, dtype=np.float64).astype(np.longdouble)

    def zeros(self, shape):
        return np.zeros(shape, dtype=np.longdouble)

    def log2pi(self):
        return np.longdouble("1.83787706640934548356065947281123527972")

    def f64(self, a):
        return np.asarray(a, dtype=np.longdouble).astype(np.float64)


def _dot(a, b):
    """a @ b that also holds for an empty contraction of object arrays."""
    if a.shape[-1] == 0:
        return 0
    return a @ b


def _truth(be, X, Y, theta, Xs, want_cov):
    X64, Xs64 = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    d, N = X64.shape
    M = Xs64.shape[1]
    X, Xs, Y, th = be.arr(X64), be.arr(Xs64), be.arr(np.atleast_2d(Y)), be.arr(theta)
    G = Y.shape[0]
    il2, sf2, sn2 = be.exp(-2 * th[1:d + 1]), be.exp(2 * th[d + 1]), be.exp(2 * th[0])
    noise = sn2 + be.arr(EPS)

    def sq(A, B):  # (d, NA, NB) exact squared differences
        t = A[:, :, None] - B[:, None, :]
        return t * t

    def kern(Dst):  # sf2 exp(-sum_p D_p il2_p / 2)
        r = be.zeros(Dst.shape[1:])
        for p in range(d):
            r = r + Dst[p] * il2[p]
        return sf2 * be.exp(-r / 2)

    D = sq(X, X)
    Kf = kern(D)
    K = Kf.copy()
    ix = np.arange(N)
    K[ix, ix] = K[ix, ix] + noise
    # K = L L^T, column by column; Z = L^-1 by forward substitution on I
    L = be.zeros((N, N))
    for j in range(N):
        L[j, j] = be.sqrt(K[j, j] - _dot(L[j, :j], L[j, :j]))
        if j + 1 < N:
            L[j + 1:, j] = (K[j + 1:, j] - _dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    Z = be.zeros((N, N))
    for i in range(N):
        e = be.zeros(N)
        e[i] = e[i] + 1
        Z[i] = (e - _dot(L[i, :i], Z[:i])) / L[i, i]
    Kinv = Z.T @ Z
    # alpha and V by substitution (L T = [Y^T K*], L^T alpha = T_y), not through Z: the explicit
    # inverse would put cond(K) eps_backend |alpha| of unstructured error into mu
    Ks = kern(sq(X, Xs))  # N x M
    T = be.zeros((N, G + M))
    R = np.concatenate([Y.T, Ks], axis=1)
    for i in range(N):
        T[i] = (R[i] - _dot(L[i, :i], T[:i])) / L[i, i]
    Al = be.zeros((N, G))
    for i in range(N - 1, -1, -1):
        Al[i] = (T[i, :G] - _dot(L[i + 1:, i], Al[i + 1:])) / L[i, i]
    V = T[:, G:]
    logs = be.log(L[ix, ix])
    out = {k: [] for k in ("mll", "grad", "alpha", "mu", "A_mll", "A_grad", "A_grad_exp", "A_alpha", "A_mu")}
    Df = D.reshape(d, N * N)
    x2 = X * X
    for g in range(G):
        y = Y[g]
        a = Al[:, g]
        out["alpha"].append(a)
        out["A_alpha"].append(np.abs(Kinv) @ np.abs(y))
        out["mll"].append(-(y @ a + 2 * np.sum(logs) + be.log2pi() * N) / 2)
        out["A_mll"].append((np.sum(np.abs(y * a)) + 2 * np.sum(np.abs(logs)) + be.log2pi() * N) / 2)
        W = np.outer(a, a) - Kinv
        WK = W * Kf
        aWK = np.abs(WK)
        gr, Ag, Ae = be.zeros(d + 2), be.zeros(d + 2), be.zeros(d + 2)
        gr[0], Ag[0] = sn2 * np.sum(W[ix, ix]), sn2 * np.sum(np.abs(W[ix, ix]))
        gr[1:d + 1] = (Df @ WK.reshape(-1)) * il2 / 2
        Ag[1:d + 1] = (Df @ aWK.reshape(-1)) * il2 / 2
        gr[d + 1], Ag[d + 1] = np.sum(WK), np.sum(aWK)
        # the expanded form's operands: a^2 + b^2 (+ 2|ab| <= a^2 + b^2) in place of (a - b)^2
        Ae[1:d + 1] = (x2 @ np.sum(aWK, axis=1)) * 2 * il2 / 2
        Ae[0], Ae[d + 1] = Ag[0], Ag[d + 1]
        out["grad"].append(gr)
        out["A_grad"].append(Ag)
        out["A_grad_exp"].append(Ae)
        out["mu"].append(Ks.T @ a)
        out["A_mu"].append(np.abs(Ks).T @ np.abs(a))
    res = {k: be.f64(np.stack(v)) for k, v in out.items()}
    kss = sf2 + be.zeros(M)  # r(x*, x*) = 0 exactly
    vv = np.sum(V * V, axis=0)
    res["var"], res["A_var"] = be.f64(kss - vv), be.f64(kss + vv)
    if want_cov:
        Kss = kern(sq(Xs, Xs))
        res["cov"] = be.f64(Kss - V.T @ V)
        res["A_cov"] = be.f64(np.abs(Kss) + np.abs(V).T @ np.abs(V))
    return res


def truth(X, Y, theta, Xs, backend: str = "mp", want_cov: bool = True):
    """X (d, N), Y (G, N) targets sharing X and theta (one factorisation), Xs (d, M).  Returns fp64
    arrays mll (G), grad (G, d+2), alpha (G, N), mu (G, M), var (M, unclamped), cov (M, M), and A_<q>
    of the same shapes (A_grad_exp: the gradient's with the expanded distance form's operands)."""
    if backend == "mp":
        be = _MP()
        with be.m.workdps(50):
            return _truth(be, X, Y, theta, Xs, want_cov)
    return _truth(_LD(), X, Y, theta, Xs, want_cov)


# ---- fp64 variants ------------------------------------------------------------------------------
def _cross(X, theta, Xs, mode):
    il2, sf2, _, _ = O.kernel_params(theta, X.shape[0])
    Ks = sf2 * np.exp(-O.weighted_r(O.dist_stack(X, Xs, mode), il2) * 0.5)
    Kss = sf2 * np.exp(-O.weighted_r(O.dist_stack(Xs, Xs, mode), il2) * 0.5)
    return Ks, Kss


def _exp_table(x, sf2):
    """sf2 exp(x) for x <= 0 as the device's Gram and cross-covariance kernels form it (DESIGN.md
    section 2, "Not bit-parity with Distances.jl"): x = (64 m + j) ln2/64 + r by Cody-Waite, e^r - 1
    by a degree-5 Taylor polynomial, sf2 2^(j/64) from a 64-entry (hi, lo) table with sf2 folded in,
    one rounding of the sum.  numpy has no fma: the products round once more, far below eps."""
    ld = np.longdouble
    c = np.log(ld(2)) / 64
    m, e = np.frexp(np.float64(c))
    c_hi = float(np.ldexp(np.rint(np.ldexp(m, 32)), e - 32))  # 32 significant bits: n c_hi is exact
    c_lo = float(c - ld(c_hi))
    t = np.exp2(np.arange(64, dtype=ld) / 64)
    hi = t.astype(np.float64)
    lo = (t - hi).astype(np.float64)
    th = sf2 * hi
    tl = (ld(sf2) * hi.astype(ld) - th.astype(ld)).astype(np.float64) + sf2 * lo
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(np.maximum(x, -800.0) * float(1 / c))
    r = (x - n * c_hi) - n * c_lo
    q = r * (1.0 + r * (0.5 + r * (1.0 / 6 + r * (1.0 / 24 + r * (1.0 / 120)))))
    j = np.mod(n, 64).astype(np.int64)
    v = np.ldexp(th[j] + (th[j] * q + tl[j]), ((n - j) / 64).astype(np.int64))
    return np.where(x < -745.0, 0.0, v)


def _staged_kernel(XA, XB, theta, mode):
    """The noise-free covariance in the device's formulation: direct mode stages the coordinates
    pre-scaled by sqrt(il2_p / 2) and sums r/2 = sum_p (a - b)^2; expanded mode sums the oracle's r;
    both end in the table exp."""
    il2, sf2, _, _ = O.kernel_params(theta, XA.shape[0])
    if mode == O.DIST_EXPANDED:
        return _exp_table(-O.weighted_r(O.dist_stack(XA, XB, mode), il2) * 0.5, sf2)
    s = np.sqrt(0.5 * il2)[:, None]
    A, B = XA * s, XB * s
    r = np.zeros((XA.shape[1], XB.shape[1]))
    for p in range(XA.shape[0]):
        t = A[p][:, None] - B[p][None, :]
        r = r + t * t
    return _exp_table(-r, sf2)


def _lapack(X, Y, theta, Xs, mode, D, pin=True):
    """gp_oracle's own path per target (lml and predict_f, the pieces of fit, over the shared
    distance stack D; fit itself on the first target, which must agree bit for bit)."""
    res = {k: [] for k in ("mll", "grad", "alpha", "mu")}
    for y in Y:
        m, g, aux = O.lml(X, y, theta, mode, want_grad=True, D=D)
        mu, var = O.predict_f(X, theta, aux["alpha"], aux["U"], Xs, mode)
        for k, v in (("mll", m), ("grad", g), ("alpha", aux["alpha"]), ("mu", mu)):
            res[k].append(v)
    res = {k: np.stack(v) for k, v in res.items()}
    if pin:
        f = O.fit(X, Y[0], theta, Xs, mode)
        assert all(np.array_equal(f[k], res[k][0]) for k in res) and np.array_equal(f["var"], var)
    Ks, Kss = _cross(X, theta, Xs, mode)
    V = sla.solve_triangular(aux["U"], Ks, trans="T", lower=False)
    res["var"] = np.diag(Kss) - np.sum(V * V, axis=0)
    res["cov"] = Kss - V.T @ V
    assert np.array_equal(np.maximum(res["var"], 0.0), var)
    return res


def _factor_tiles(A, Li, o, n):
    """In place over tiles [o, o + n): A's lower triangle becomes L, Li becomes L^-1; the recursion
    of the device (top half h = n / 2, TRSM by the explicit inverse, SYRK, bottom half, L^-1's
    off-diagonal block -L22^-1 L21 L11^-1)."""
    N = A.shape[0]
    if n == 1:
        s = slice(o * TILE, min((o + 1) * TILE, N))
        A[s, s] = np.linalg.cholesky(A[s, s])
        Li[s, s] = sla.solve_triangular(A[s, s], np.eye(s.stop - s.start), lower=True)
        return
    h = n // 2
    t, b = slice(o * TILE, (o + h) * TILE), slice((o + h) * TILE, min((o + n) * TILE, N))
    _factor_tiles(A, Li, o, h)
    A[b, t] = A[b, t] @ Li[t, t].T
    A[b, b] = A[b, b] - A[b, t] @ A[b, t].T
    _factor_tiles(A, Li, o + h, n - h)
    Li[b, t] = -(Li[b, b] @ (A[b, t] @ Li[t, t]))


def _explicit(X, Y, theta, Xs, mode, D, fault=None, staged=False):
    d, N = X.shape
    il2, sf2, sn2, noise = O.kernel_params(theta, d)
    w = il2.copy()
    pv = int(np.argmax(np.var(X, axis=1)))  # a coordinate that varies
    if fault == "ard_scale_1e-9":
        w[pv] = w[pv] * (1.0 + 1e-9)
    Kf = _staged_kernel(X, X, theta, mode) if staged else sf2 * np.exp(-O.weighted_r(D, w) * 0.5)
    K = Kf.copy()
    ix = np.arange(N)
    K[ix, ix] = K[ix, ix] + noise
    if fault == "k_entry_1e3ulp":
        i, j = N - 1, N // 3
        K[i, j] = K[j, i] = K[i, j] * (1.0 + 1e3 * EPS)
    A, Li = K.copy(), np.zeros((N, N))
    try:
        _factor_tiles(A, Li, 0, -(-N // TILE))
    except np.linalg.LinAlgError as e:
        raise O.NotPosDef(0) from e
    Li = np.tril(Li)
    Kinv = Li.T @ Li
    r0 = TILE * ((N - 1) // TILE)  # first row of the last tile
    if fault == "kinv_drop_last":  # one row of the last tile loses its k = N-1 term
        Kinv[r0] = Kinv[r0] - Li[N - 1, r0] * Li[N - 1]
    if staged:
        Ks, Kss = _staged_kernel(X, Xs, theta, mode), _staged_kernel(Xs, Xs, theta, mode)
    else:
        Ks, Kss = _cross(X, theta, Xs, mode)
    V = Li @ Ks
    if fault == "v_skip_col16":  # rows r0..r0+15: the 16-wide block ending at column r0-1 skips it
        rows = slice(r0, min(r0 + 16, N))
        V[rows] = V[rows] - Li[rows, r0 - 1:r0] @ Ks[r0 - 1:r0]
    logdet = 2.0 * np.sum(np.log(np.diag(A)))
    Df = D.reshape(d, N * N)
    res = {k: [] for k in ("mll", "grad", "alpha", "mu")}
    for y in Y:
        t = Li @ y
        a = Li.T @ t
        if fault == "alpha_rows_short":  # the first tile's columns stop one row early
            a[:TILE] = a[:TILE] - Li[N - 1, :TILE] * t[N - 1]
        W = np.outer(a, a) - Kinv
        WK = W * Kf
        g = np.empty(d + 2)
        g[0] = sn2 * np.trace(W)
        g[1:d + 1] = 0.5 * (Df @ WK.reshape(-1)) * il2
        g[d + 1] = np.sum(WK)
        res["mll"].append(-(float(y @ a) + logdet + O.LOG2PI * N) / 2.0)
        res["grad"].append(g)
        res["alpha"].append(a)
        res["mu"].append(Ks.T @ a)
    res = {k: np.stack(v) for k, v in res.items()}
    res["var"] = np.diag(Kss) - np.sum(V * V, axis=0)
    res["cov"] = Kss - V.T @ V
    return res


def variants(X, Y, theta, Xs, mode, fault=None, D=None):
    """{name: results} of the fp64 evaluations in `mode`; Y (G, N).  With `fault`, only the seeded
    "explicit" one."""
    X, Xs, theta = (np.asarray(v, dtype=np.float64) for v in (X, Xs, theta))
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    if D is None:  # the callers that loop over theta pass the stack, which depends on X and mode only
        D = O.dist_stack(X, X, mode)
    if fault is not None:
        assert fault in FAULTS and X.shape[1] > 2 * TILE
        return {"explicit": _explicit(X, Y, theta, Xs, mode, D, fault)}
    Xr, Yr, Dr = np.ascontiguousarray(X[:, ::-1]), np.ascontiguousarray(Y[:, ::-1]), np.ascontiguousarray(D[:, ::-1, ::-1])

    def back(res):  # results for the reversed point order, alpha in the caller's order
        res["alpha"] = np.ascontiguousarray(res["alpha"][:, ::-1])
        return res

    return {"lapack": _lapack(X, Y, theta, Xs, mode, D), "explicit": _explicit(X, Y, theta, Xs, mode, D),
            "staged": _explicit(X, Y, theta, Xs, mode, D, staged=True),
            "lapack_rev": back(_lapack(Xr, Yr, theta, Xs, mode, Dr, pin=False)),
            "staged_rev": back(_explicit(Xr, Yr, theta, Xs, mode, Dr, staged=True))}


# ---- bounds -------------------------------------------------------------------------------------
def floor_of(tr, q, mode):
    """A_q of a truth record for the bound's floor; in expanded mode the gradient components whose
    truth is exactly zero (constant coordinates) take the expanded form's operands."""
    A = tr["A_" + q]
    if q == "grad" and mode == O.DIST_EXPANDED:
        A = np.where(tr["grad"] == 0.0, tr["A_grad_exp"], A)
    return A


def bound(E, A, k):
    return k * np.maximum(E, EPS * np.asarray(A))


def ratio(err, E, floor):
    """Largest err / max(E, floor), elementwise; 0 / 0 counts as 0 and err > 0 over 0 as inf."""
    err = np.asarray(err, dtype=np.float64)
    den = np.broadcast_to(np.maximum(E, floor), err.shape)
    return float(np.max(np.divide(err, den, out=np.where(err > 0, np.inf, 0.0), where=den > 0)))


def geomean(errs):
    errs = [float(e) for e in errs]
    return 0.0 if min(errs) == 0.0 else math.exp(sum(math.log(e) for e in errs) / len(errs))
