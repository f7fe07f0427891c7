"""Regenerates tests/golden/cvfold_*.npz: the high-precision truth of k-fold cross-validation
(predict_CVfold / logp_CVfold; Rasmussen & Williams 5.4.2 in block form), E_q from five fp64 CPU
variants and A_q.  CPU only, byte-identical on every run.

    python tests/golden/make_golden_cvfold.py [-j PROCS] [--only NAME ...]

Inputs (X, Y, thetas) are those of tests/golden/hp_<case>.npz; f_cp_520 and g_nonpd_p1 carry theirs in
loo_<case>.npz.  A fixture stores fold layouts, truths, E, A and k only.  A fixture's slots are its
(theta, target) pairs p = t G + g, as in the hp and loo fixtures.

For a fold V of m points, Q = [K^-1]_VV, a = alpha_V, K = Kf + (exp(2 log sn) + eps) I, alpha = K^-1 y:
    Q = C C^T,  w = C^-1 a,  mu_V = y_V - C^-T w,  var_i = sum_k (C^-1)_ki^2,
    logp_V = -|w|^2 / 2 + sum_i log C_ii - m log(2 pi) / 2,   logp = sum_V logp_V.
layouts    per case (layouts()): fold_of is (1, N), shared by the slots, or (P, N), one row per pair.
truth      50-digit mpmath for N <= 130 and x87 extended precision above (the backends of
           oracle/hp_oracle.py): exact differences in the distances, Cholesky, L^-1 by substitution,
           K^-1 = L^-T L^-1, then the formulas above with a Cholesky of Q; rounded to fp64 once.
variants   per distance mode, in fp64:
           "refit"       the definition: F refits on the points outside the fold (gp_oracle's Gram and
                         dpotrf), the joint predictive Gaussian at the fold's points, variance + noise,
                         its log density by a Cholesky of the predictive covariance.  A fold of all
                         points: the prior.
           "lapack"      the closed form from gp_oracle.lml's U: K^-1 = U^-1 U^-T, LAPACK Cholesky of Q
           "lapack_rev"  the same over the points in reverse order
           "staged"      the device's pipeline: the Gram as the device forms it, factorised and inverted
                         over 64-row tiles (hp_oracle._factor_tiles), L^-T's rows in fold order, Q as
                         their product, a right-looking Cholesky in 16-column steps, w by substitution
                         along with it, C^-1 column by column
           "staged_rev"  the same over the points in reverse order
E[layout][mode, theta, q]  the geometric mean over the five variants of max |variant - truth|,
           q in (mu, var, logp_fold, logp), with one stated exception (refit_left_out): where the
           complement of a fold holds at most one point, "refit" has no factorisation behind what it
           returns for that fold and its answer is no draw of the closed forms' rounding.
             no point left (one fold of every point): "refit" returns the prior, mean exactly 0 and
               variance K_ii, while every closed form has to cancel y - K alpha: its mu and var stay
               out of the mean (four variants; E_mu = 0 at N = 1, where the others are exact too).
             one point left (folds of 1 and N - 1 points): "refit" factors a 1 x 1 matrix and returns
               var to 5e-15 where the closed forms reach 6e-13 .. 1e-11: its var stays out.  Its mu
               stays in (every variant is below 4.7 with all five).
           Its logp_fold and logp stay in everywhere.  The generator prints E with and without "refit"
           wherever the exception applies, so the widening is on record per case.
A_q        the absolute sum of q's last reduction: sum_V |logp_V| for logp; |w|^2 / 2 + sum |log C_ii| +
           m log(2 pi) / 2 for logp_fold; |y_i| + |(Q^-1 a)_i|, the terms of its last subtraction, for mu
           (at N = 1 the truth is the prior mean, 0, and "refit" returns exactly 0, so E_mu is 0 there
           while every closed form rounds y - Q^-1 a to about eps |y|); |truth| for var.
k          8, read from hp_a_p2_1.npz.  Bound: |x - truth| <= k max(E_q, eps A_q).  The rungs of LEFT_OUT
           are left out of their case, in every layout (theta_index names the rungs kept); every
           layout is stored.  The generator fails if a variant exceeds k at a rung kept, if more than
           one rung of a case is listed, or if none is kept.
identities in the truth's precision, checked here: singleton folds against loo_<case>.npz, one fold of
           all points against hp_<case>.npz's mll (IDENT_RTOL of the quantity's A).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import math
import pathlib
import sys

import numpy as np
import scipy.linalg as sla

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(HERE))

from oracle import gp_oracle as O  # noqa: E402
from oracle import hp_oracle as H  # noqa: E402

QUANTITIES = ("mu", "var", "logp_fold", "logp")
VARIANTS = ("refit", "lapack", "lapack_rev", "staged", "staged_rev")
FAULTS = ("fold_order", "var_without_noise", "logdet_sign", "drop_last_fold")
CASES = ("a_p2_1", "a_p2_5", "a_p2_64", "a_p2_65", "b_cp_130", "b_p1_130", "b_fb_130", "e_d1", "c_cp_320", "f_cp_520",
         "g_nonpd_p1")
STORED = ("f_cp_520", "g_nonpd_p1")  # inputs in loo_<case>.npz
# theta rungs left out of a case, by index into its thetas, at most one per case: a fixed, reviewed
# list, only where a CPU variant itself exceeds k.  b_p1_130 at log sigma_n = -6
# (cond(K) = 7e11), the rung the LOO fixtures drop: a variant lies at 8.5 to 10.3 max(E_q, eps A_q) in
# every layout.  The generator fails if a variant exceeds k at anything kept.
LEFT_OUT = {"b_p1_130": (2,)}
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
IDENT_RTOL = 1e-13
CBS = 16  # the device's columns per Cholesky step


def case_inputs(name):
    """X (d, N), Y (G, N), thetas (T, d + 2)."""
    with np.load(HERE / (f"loo_{name}.npz" if name in STORED else f"hp_{name}.npz")) as z:
        return z["X"].copy(), z["Y"].copy(), np.atleast_2d(z["thetas"].copy())


def layouts(name, N, P):
    """{layout: fold_of (1, N) or (P, N)}; F = the largest id + 1."""
    i = np.arange(N)
    one = lambda a: np.asarray(a, dtype=np.int64)[None, :]  # noqa: E731
    if name == "a_p2_1":
        return {"one": one([0])}
    if name == "a_p2_5":
        return {"singletons": one(i), "odd_even": one(i % 2)}
    if name in ("a_p2_64", "a_p2_65"):
        return {"all": one(0 * i), "one_rest": one(np.minimum(i, 1)), "mod3": one(i % 3)}
    if name.startswith("b_"):
        straddle = np.where(i < 30, i, np.where(i < 95, 30, i - 64))  # a fold of 65 over packed positions 30..94
        out = {"c21": one(i // 21), "mod7": one(i % 7), "straddle65": one(straddle), "all": one(0 * i)}
        if name == "b_cp_130":  # an empty fold in the middle (id 3); a layout per slot
            out["empty_mid"] = one(np.where(i // 21 < 3, i // 21, i // 21 + 1))
            out["per_slot"] = np.stack([i // 21 if p % 2 == 0 else (i + p) % 7 for p in range(P)]).astype(np.int64)
        return out
    if name == "e_d1":
        return {"mod2": one(i % 2)}
    if name == "c_cp_320":
        return {"c20": one(i // 20), "t64_128_128": one(np.where(i < 64, 0, np.where(i < 192, 1, 2)))}
    if name == "f_cp_520":
        return {"all": one(0 * i), "mod25": one(i % 25)}
    if name == "g_nonpd_p1":
        return {"mod4": one(i % 4)}
    raise KeyError(name)


def nfolds(fo):
    return int(fo.max()) + 1


def backend_of(N):
    return "mp" if N <= 130 else "ld"


# ---- truth --------------------------------------------------------------------------------------
def _chol(be, A):
    n = A.shape[0]
    L = be.zeros((n, n))
    for j in range(n):
        L[j, j] = be.sqrt(A[j, j] - H._dot(L[j, :j], L[j, :j]))
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - H._dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    return L


def _linv(be, L):
    n = L.shape[0]
    Z = be.zeros((n, n))
    for i in range(n):
        e = be.zeros(n)
        e[i] = e[i] + 1
        Z[i] = (e - H._dot(L[i, :i], Z[:i])) / L[i, i]
    return Z


def _truth(be, X, Y, theta, lay, t):
    X64 = np.asarray(X, dtype=np.float64)
    d, N = X64.shape
    X, Y, th = be.arr(X64), be.arr(np.atleast_2d(Y)), be.arr(theta)
    G = Y.shape[0]
    il2, sf2, sn2 = be.exp(-2 * th[1:d + 1]), be.exp(2 * th[d + 1]), be.exp(2 * th[0])
    r = be.zeros((N, N))
    for p in range(d):
        dx = X[p][:, None] - X[p][None, :]
        r = r + dx * dx * il2[p]
    K = sf2 * be.exp(-r / 2)
    ix = np.arange(N)
    K[ix, ix] = K[ix, ix] + (sn2 + be.arr(H.EPS))
    Z = _linv(be, _chol(be, K))
    Ki = Z.T @ Z
    al = (Ki @ Y.T).T  # (G, N)
    out = {}
    for name, fo in lay.items():
        F = nfolds(fo)
        mu, var, A_mu = be.zeros((G, N)), be.zeros((G, N)), be.zeros((G, N))
        lpf, A_lpf = be.zeros((G, F)), be.zeros((G, F))
        done = {}
        for g in range(G):
            row = row_of(fo, t, g, G)
            for f in range(F):
                V = np.where(row == f)[0]
                if not len(V):
                    continue
                key = (f, V.tobytes())
                if key not in done:
                    C = _chol(be, Ki[np.ix_(V, V)])
                    done[key] = (C, _linv(be, C))
                C, Xi = done[key]
                w = Xi @ al[g, V]
                rr = Xi.T @ w
                mu[g, V], A_mu[g, V] = Y[g, V] - rr, abs(Y[g, V]) + abs(rr)
                var[g, V] = np.sum(Xi * Xi, axis=0)
                ld = be.log(np.diag(C))
                half = (w @ w) / 2
                lpf[g, f] = -half + np.sum(ld) - len(V) * be.log2pi() / 2
                A_lpf[g, f] = half + np.sum(abs(ld)) + len(V) * be.log2pi() / 2
        res = dict(mu=mu, var=var, logp_fold=lpf, logp=np.sum(lpf, axis=1), A_mu=A_mu, A_logp_fold=A_lpf,
                   A_logp=np.sum(abs(lpf), axis=1))
        out[name] = {k: be.f64(v) for k, v in res.items()}
    return out


def row_of(fo, t, g, G):
    """The layout row of the pair (t, g)."""
    return fo[(t * G + g) % fo.shape[0]] if fo.shape[0] > 1 else fo[0]


# ---- fp64 variants ------------------------------------------------------------------------------
def _closed_fold(Q, a, y, fault=None):
    """(mu, var, logp_V) of one fold from Q and a = alpha_V by LAPACK."""
    C = np.linalg.cholesky(Q)
    if fault == "fold_order":
        a = a[::-1]
    w = sla.solve_triangular(C, a, lower=True)
    Xi = sla.solve_triangular(C, np.eye(len(a)), lower=True)
    ld = np.sum(np.log(np.diag(C)))
    if fault == "logdet_sign":
        ld = -ld
    return y - Xi.T @ w, np.sum(Xi * Xi, axis=0), (-0.5 * (w @ w) + ld) - len(a) * HALF_LOG_2PI


def _assemble(Y, fo_rows, F, per_fold, fault=None):
    G, N = Y.shape
    mu, var, lpf = np.zeros((G, N)), np.zeros((G, N)), np.zeros((G, F))
    for g in range(G):
        for f in range(F):
            V = np.where(fo_rows[g] == f)[0]
            if len(V):
                mu[g, V], var[g, V], lpf[g, f] = per_fold(g, V)
    last = F - 1 if fault == "drop_last_fold" else F
    return dict(mu=mu, var=var, logp_fold=lpf, logp=np.sum(lpf[:, :last], axis=1))


def _lapack(X, Y, theta, mode, rows, F, fault=None):
    al, U = [], None
    for y in Y:
        _, _, aux = O.lml(X, y, theta, mode)
        U = aux["U"]
        al.append(aux["alpha"])
    Ui = sla.solve_triangular(U, np.eye(U.shape[0]), lower=False)
    Ki = Ui @ Ui.T
    return _assemble(Y, rows, F, lambda g, V: _closed_fold(Ki[np.ix_(V, V)], al[g][V], Y[g, V], fault), fault)


def _refit(X, Y, theta, mode, rows, F, fault=None):
    d, N = X.shape
    _, _, _, noise = O.kernel_params(theta, d)
    K, Kf, _ = O.gram(X, theta, mode)
    memo = {}

    def per_fold(g, V):
        key = V.tobytes()
        if key not in memo:
            keep = np.setdiff1d(np.arange(N), V)
            S = K[np.ix_(V, V)].copy()
            if len(keep):
                U = O.cholesky_upper(np.ascontiguousarray(K[np.ix_(keep, keep)]))
                Ks = Kf[np.ix_(keep, V)]
                Vw = sla.solve_triangular(U, Ks, trans="T", lower=False)
                S = S - Vw.T @ Vw
            else:
                U, Ks = None, None
            memo[key] = (keep, U, Ks, S, np.linalg.cholesky(S))
        keep, U, Ks, S, Lc = memo[key]
        m = Ks.T @ sla.cho_solve((U, False), Y[g, keep]) if U is not None else np.zeros(len(V))
        z = sla.solve_triangular(Lc, Y[g, V] - m, lower=True)
        v = np.diag(S) - (noise if fault == "var_without_noise" else 0.0)
        return m, v, (-0.5 * (z @ z) - np.sum(np.log(np.diag(Lc)))) - len(V) * HALF_LOG_2PI

    return _assemble(Y, rows, F, per_fold, fault)


def _chol_steps(Q, a):
    """The device's right-looking Cholesky in CBS-column steps, the right-hand side as one more row."""
    A, w, m = np.tril(Q).copy(), a.copy(), len(a)
    for k0 in range(0, m, CBS):
        k1 = min(k0 + CBS, m)
        A[k0:k1, k0:k1] = np.linalg.cholesky(A[k0:k1, k0:k1] + np.tril(A[k0:k1, k0:k1], -1).T)
        D = A[k0:k1, k0:k1]
        w[k0:k1] = sla.solve_triangular(D, w[k0:k1], lower=True)
        if k1 < m:
            A[k1:, k0:k1] = sla.solve_triangular(D, A[k1:, k0:k1].T, lower=True).T
            w[k1:] = w[k1:] - A[k1:, k0:k1] @ w[k0:k1]
            A[k1:, k1:] = A[k1:, k1:] - np.tril(A[k1:, k0:k1] @ A[k1:, k0:k1].T)
    return A, w


def _staged(X, Y, theta, mode, rows, F, fault=None):
    N = X.shape[1]
    _, _, _, noise = O.kernel_params(theta, X.shape[0])
    A = H._staged_kernel(X, X, theta, mode)
    ix = np.arange(N)
    A[ix, ix] = A[ix, ix] + noise
    Li = np.zeros((N, N))
    H._factor_tiles(A, Li, 0, -(-N // H.TILE))
    Li = np.tril(Li)
    Mt = Li.T
    al = [Li.T @ (Li @ y) for y in Y]

    def per_fold(g, V):
        P = Mt[V]  # the fold's rows of L^-T, in packed order (V ascending)
        C, w = _chol_steps(P @ P.T, al[g][V])
        Xi = sla.solve_triangular(C, np.eye(len(V)), lower=True)
        r = sla.solve_triangular(C, w, lower=True, trans="T")
        return Y[g, V] - r, np.sum(Xi * Xi, axis=0), (np.sum(np.log(np.diag(C))) - 0.5 * (w @ w)) - len(V) * HALF_LOG_2PI

    return _assemble(Y, rows, F, per_fold, fault)


def _rev(f, X, Y, theta, mode, rows, F):
    r = f(np.ascontiguousarray(X[:, ::-1]), np.ascontiguousarray(Y[:, ::-1]), theta, mode, [row[::-1] for row in rows], F)
    return {k: (np.ascontiguousarray(v[..., ::-1]) if k in ("mu", "var") else v) for k, v in r.items()}


def variants(X, Y, theta, mode, fo, t):
    G = Y.shape[0]
    rows, F = [row_of(fo, t, g, G) for g in range(G)], nfolds(fo)
    return {"refit": _refit(X, Y, theta, mode, rows, F), "lapack": _lapack(X, Y, theta, mode, rows, F),
            "lapack_rev": _rev(_lapack, X, Y, theta, mode, rows, F), "staged": _staged(X, Y, theta, mode, rows, F),
            "staged_rev": _rev(_staged, X, Y, theta, mode, rows, F)}


def faulty(X, Y, theta, mode, fo, t, fault):
    """One variant with a seeded fault (tests/test_cvfold_host.py): the bound must refuse it."""
    G = Y.shape[0]
    rows, F = [row_of(fo, t, g, G) for g in range(G)], nfolds(fo)
    return (_refit if fault == "var_without_noise" else _lapack)(X, Y, theta, mode, rows, F, fault=fault)


def floors(tr):
    """A_q per quantity of one truth record (see the module docstring)."""
    return dict(mu=tr["A_mu"], var=np.abs(tr["var"]), logp_fold=tr["A_logp_fold"], logp=tr["A_logp"])


def worst_ratio(res, tr, E, mode, t):
    """The largest |res - truth| / max(E_q, eps A_q) over the quantities, for rung t of a layout's record."""
    A = floors({k: v[t] for k, v in tr.items()})
    return max(H.ratio(np.abs(res[q] - tr[q][t]), E[mode, t, qi], H.EPS * A[q]) for qi, q in enumerate(QUANTITIES))


# ---- assembly -----------------------------------------------------------------------------------
def solve(job):
    name, ti = job
    X, Y, thetas = case_inputs(name)
    lay = layouts(name, X.shape[1], len(thetas) * Y.shape[0])
    tr = _truth_of(X, Y, thetas[ti], lay, ti)
    var = {ln: {mode: variants(X, Y, thetas[ti], mode, fo, ti) for mode in (0, 1)} for ln, fo in lay.items()}
    return name, ti, tr, var


def _truth_of(X, Y, theta, lay, t):
    if backend_of(X.shape[1]) == "mp":
        be = H._MP()
        with be.m.workdps(50):
            return _truth(be, X, Y, theta, lay, t)
    return _truth(H._LD(), X, Y, theta, lay, t)


def kept(name, T):
    """The theta rungs of a case that are kept (LEFT_OUT)."""
    assert len(LEFT_OUT.get(name, ())) <= 1, f"{name}: at most one rung may be left out"
    return [t for t in range(T) if t not in LEFT_OUT.get(name, ())]


def refit_left_out(fo):
    """The quantities whose E leaves "refit" out for the layout fo (see the module docstring): by the
    smallest number of points outside a fold, 0 -> mu and var, 1 -> var, more -> none."""
    N = fo.shape[1]
    left = min(N - int(np.max(np.bincount(row))) for row in fo)
    return ("mu", "var") if left == 0 else (("var",) if left == 1 else ())


def assemble(name, parts, k):
    X, Y, thetas = case_inputs(name)
    T, G = len(thetas), Y.shape[0]
    lay = layouts(name, X.shape[1], T * G)
    fx = dict(case=np.array(name), backend=np.array(backend_of(X.shape[1])), quantities=np.array(QUANTITIES),
              variant_names=np.array(VARIANTS), k=np.array(k))
    worst_all, over, names = 0.0, [], []
    for ln, fo in lay.items():
        tr = {q: np.stack([parts[t][0][ln][q] for t in range(T)]) for q in QUANTITIES + ("A_mu", "A_logp_fold", "A_logp")}
        E = np.zeros((2, T, len(QUANTITIES)))
        out_q = refit_left_out(fo)
        for mode in (0, 1):
            for t in range(T):
                for qi, q in enumerate(QUANTITIES):
                    err = {vn: np.max(np.abs(parts[t][1][ln][mode][vn][q] - tr[q][t])) for vn in VARIANTS}
                    E[mode, t, qi] = H.geomean([e for vn, e in err.items() if not (vn == "refit" and q in out_q)])
                    if q in out_q:
                        print(f"  {name} {ln} theta {t} mode {mode} E_{q}: {E[mode, t, qi]:.3e} without refit, "
                              f"{H.geomean(list(err.values())):.3e} with all five", flush=True)
        keep = kept(name, T)
        for mode in (0, 1):
            for t in range(T):
                worst = max(worst_ratio(parts[t][1][ln][mode][vn], tr, E, mode, t) for vn in VARIANTS)
                print(f"  {name} {ln} theta {t} mode {mode}: largest variant ratio {worst:.2f}", flush=True)
                if t in keep:
                    worst_all = max(worst_all, worst)
                    if worst > k:
                        over.append(f"{name} {ln} theta {t} mode {mode}: a variant at {worst:.2f} > k")
        names.append(ln)
        fx[f"{ln}.fold_of"] = fo.astype(np.int16)
        fx[f"{ln}.theta_index"] = np.array(keep, dtype=np.int64)
        for q, v in tr.items():
            fx[f"{ln}.{q}"] = v[keep]
        fx[f"{ln}.E"] = E[:, keep]
    assert keep, f"{name}: a whole case may not be left out"
    fx["layouts"] = np.array(names)
    return fx, worst_all, over


def check_identities(name, fx):
    lays = list(fx["layouts"])
    if ("all" in lays or "one" in lays) and name not in STORED:
        ln = "all" if "all" in lays else "one"
        with np.load(HERE / (f"hp_{name}.npz")) as z:
            mll = z["mll"][fx[f"{ln}.theta_index"]]
        err = np.max(np.abs(fx[f"{ln}.logp"] - mll) / fx[f"{ln}.A_logp_fold"][..., 0])
        print(f"  {name}: one fold against the hp mll: {err:.2e} of A")
        assert err <= IDENT_RTOL
    if "singletons" in lays:
        with np.load(HERE / f"loo_{name}.npz") as z:
            assert np.array_equal(z["theta_index"], fx["singletons.theta_index"])
            for q, lq in (("mu", "mu"), ("logp_fold", "logp_i"), ("logp", "logp")):
                A = np.abs(z[lq]) if q != "logp" else z["A_logp"]
                err = np.max(np.abs(fx[f"singletons.{q}"] - z[lq]) / np.maximum(A, 1e-300))
                print(f"  {name}: singleton folds against the loo truth, {q}: {err:.2e} of A")
                assert err <= IDENT_RTOL
            err = np.max(np.abs(fx["singletons.var"] - z["var"][:, None, :]) / z["var"][:, None, :])
            assert err <= IDENT_RTOL


def main():
    sys.path.insert(0, str(HERE))
    from make_golden_hp import save_npz

    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--parts", default=None, help="a file that keeps the solved jobs between runs")
    a = ap.parse_args()
    names = [n for n in CASES if a.only is None or n in a.only]
    with np.load(HERE / "hp_a_p2_1.npz") as z:
        k = float(z["k"])
    jobs = [(n, ti) for n in names for ti in range(len(case_inputs(n)[2]))]
    jobs.sort(key=lambda j: -case_inputs(j[0])[0].shape[1])
    parts = {}
    if a.parts and pathlib.Path(a.parts).exists():  # the solved jobs of an earlier run (not committed)
        import pickle

        parts = pickle.loads(pathlib.Path(a.parts).read_bytes())
        jobs = [j for j in jobs if j[1] not in parts.get(j[0], {})]
    with cf.ProcessPoolExecutor(a.j) as ex:
        for name, ti, tr, var in ex.map(solve, jobs):
            parts.setdefault(name, {})[ti] = (tr, var)
            print(f"{name} theta {ti} done", flush=True)
    if a.parts:
        import pickle

        pathlib.Path(a.parts).write_bytes(pickle.dumps(parts))
    over = []
    for name in names:
        fx, worst, ov = assemble(name, parts[name], k)
        over += ov
        print(f"{name}: largest variant ratio at what is kept {worst:.2f} (k = {k})")
        check_identities(name, fx)
        save_npz(HERE / f"cvfold_{name}.npz", fx)
    assert not over, "review LEFT_OUT:\n" + "\n".join(over)


if __name__ == "__main__":
    main()
