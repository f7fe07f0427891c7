"""Regenerates tests/golden/loo_*.npz: the high-precision truth of the leave-one-out predictions
(predict_LOO / logp_LOO; Rasmussen & Williams 5.10-5.12), the errors of five fp64 CPU variants against
it, E_q and A_q.  CPU only, byte-identical on every run.

    python tests/golden/make_golden_loo.py [-j PROCS] [--only NAME ...]

Inputs (X, Y, thetas) come from the existing tests/golden/hp_<case>.npz, of which a fixture stores
only the name; the one new input set, f_cp_520 (CP, N = 520: nt = 9 > BLK_TILES, a split node), is
gprx.data.make_trial("CP", 520, seed = 7) with hp_d_cp_512's theta ladder and is stored with its X, Y
and thetas, as is g_nonpd_p1 (nonpd_p1.npz's inputs at log sigma_n = -2).  A fixture's slots are its (theta, target) pairs, as in the hp fixtures.

With K = Kf + (exp(2 log sn) + eps) I, kinv_i = [K^-1]_ii and alpha = K^-1 y:
    var_i = 1 / kinv_i,  mu_i = y_i - alpha_i / kinv_i,
    logp_i = log(kinv_i) / 2 - alpha_i^2 / (2 kinv_i) - log(2 pi) / 2,  logp = sum_i logp_i.
truth      these in 50-digit mpmath for N <= 130 and in x87 extended precision above (the backends of
           oracle/hp_oracle.py), exact differences in the distances, Cholesky, L^-1 by substitution,
           kinv as column sums of squares, alpha by two substitutions; rounded to fp64 once.  The
           generator prints float80 against mpmath once, on b_cp_130.
variants   per distance mode, in fp64:
           "lapack"      the closed form from gp_oracle.lml's U (kinv = row sums of squares of U^-1) and alpha
           "lapack_rev"  the same over the points in reverse order
           "brute"       N refits on the other N - 1 points: gp_oracle.lml for U and alpha (the further
                         targets' alpha by lml's own cho_solve on that U), predict_f at the point left
                         out, variance + noise, the Gaussian log density.  N = 1: the prior, mean 0 and
                         variance sf2 + sn2 + eps.
           "staged"      the closed form over the Gram as the device forms it (hp_oracle._staged_kernel),
                         factorised and inverted over 64-row tiles (hp_oracle._factor_tiles)
           "staged_rev"  the same over the points in reverse order
           Stored as d_<variant>_<q> = variant - truth in float32 (a committed file stays below 1 MiB).
E[mode, theta, q]  the geometric mean over the five variants of max |variant - truth|
A_<q>      the absolute sum of q's last reduction: sum_i |logp_i| for logp (stored as A_logp) and |truth|
           elementwise for mu, var and logp_i.  Only where E_mu = 0 does mu take the terms of its last
           subtraction instead, |y_i| + |alpha_i / kinv_i| (stored as A_mu): at N = 1 the truth is the
           prior mean, exactly 0, and "brute" returns exactly 0, so E_mu = 0, while every closed form, on
           the CPU as on the device, rounds y - alpha / kinv to about eps |y|; a floor of eps |mu| = 0
           would refuse the fixture's own variants.  This holds for a_p2_1 alone.
k          8, the factor every hp_*.npz carries; it is read from hp_a_p2_1.npz, not fitted here.  The
           generator prints the largest ratio of a variant's error to max(E_q, eps A_q) per case;
           the rungs of the fixed list LEFT_OUT are left out of their case (theta_index names the
           rungs kept), the generator fails if a variant exceeds k at any rung kept, and
           tests/test_loo_host.py asserts the same of what is stored.
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
from make_golden_hp import load_data, save_npz  # noqa: E402

QUANTITIES = ("mu", "var", "logp_i", "logp")
VARIANTS = ("lapack", "lapack_rev", "brute", "staged", "staged_rev")
HP_CASES = ("a_p2_1", "a_p2_5", "a_p2_64", "a_p2_65", "b_cp_130", "b_p1_130", "b_fb_130", "e_d1", "c_cp_320", "d_cp_500")
NEW_CASE = "f_cp_520"
# the inputs of tests/golden/nonpd_p1.npz (P1, N = 40, nearly duplicated points) at log sigma_n = -2:
# the good neighbour of the failing slot in tests/test_loo.py
NONPD_CASE = "g_nonpd_p1"
STORED = (NEW_CASE, NONPD_CASE)  # fixtures that carry their X, Y and thetas
CASES = HP_CASES + STORED
# theta rungs left out of a case, by index into its thetas: a fixed, reviewed list.  b_p1_130 at
# log sigma_n = -6: "staged"'s logp lies at 16.9 max(E_q, eps A_q) in direct mode (the scalar is one
# draw of the rounding per variant, cond(K) = 7e11), so the rung does not suit k = 8; the issue's
# rule is to change the case, not k.  The generator fails if any rung it keeps exceeds k.
LEFT_OUT = {"b_p1_130": (2,)}
B32 = ("c_cp_320", "d_cp_500", NEW_CASE)  # also run in 32 slots (k_node8 / the 4-tile leaves)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def case_inputs(name):
    """X (d, N), Y (G, N), thetas (T, d + 2)."""
    if name == NEW_CASE:
        tr = load_data().make_trial("CP", 520, 1, seed=7)
        with np.load(HERE / "hp_d_cp_512.npz") as z:
            thetas = z["thetas"].copy()
        return np.ascontiguousarray(tr["X"]), np.ascontiguousarray(tr["Y"]), thetas
    if name == NONPD_CASE:
        with np.load(HERE / "nonpd_p1.npz") as z:
            th = z["theta"].copy()
            th[0] = -2.0
            return z["X"].copy(), z["Y"].copy(), th[None, :]
    with np.load(HERE / f"hp_{name}.npz") as z:
        return z["X"].copy(), z["Y"].copy(), z["thetas"].copy()


def backend_of(N):
    return "mp" if N <= 130 else "ld"


# ---- truth --------------------------------------------------------------------------------------
def _truth(be, X, Y, theta):
    X64 = np.asarray(X, dtype=np.float64)
    d, N = X64.shape
    X, Y, th = be.arr(X64), be.arr(np.atleast_2d(Y)), be.arr(theta)
    il2, sf2, sn2 = be.exp(-2 * th[1:d + 1]), be.exp(2 * th[d + 1]), be.exp(2 * th[0])
    r = be.zeros((N, N))
    for p in range(d):
        t = X[p][:, None] - X[p][None, :]
        r = r + t * t * il2[p]
    K = sf2 * be.exp(-r / 2)
    ix = np.arange(N)
    K[ix, ix] = K[ix, ix] + (sn2 + be.arr(H.EPS))
    L = be.zeros((N, N))
    for j in range(N):
        L[j, j] = be.sqrt(K[j, j] - H._dot(L[j, :j], L[j, :j]))
        if j + 1 < N:
            L[j + 1:, j] = (K[j + 1:, j] - H._dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    Z = be.zeros((N, N))  # L^-1 by forward substitution on I
    for i in range(N):
        e = be.zeros(N)
        e[i] = e[i] + 1
        Z[i] = (e - H._dot(L[i, :i], Z[:i])) / L[i, i]
    kinv = np.sum(Z * Z, axis=0)
    G = Y.shape[0]
    T = be.zeros((N, G))
    for i in range(N):
        T[i] = (Y.T[i] - H._dot(L[i, :i], T[:i])) / L[i, i]
    Al = be.zeros((N, G))
    for i in range(N - 1, -1, -1):
        Al[i] = (T[i] - H._dot(L[i + 1:, i], Al[i + 1:])) / L[i, i]
    al = Al.T  # (G, N)
    var = 1 / kinv
    mu = Y - al * var
    lpi = be.log(kinv) / 2 - al * al * var / 2 - be.log2pi() / 2
    res = dict(mu=mu, var=var, logp_i=lpi, logp=np.sum(lpi, axis=1), A_logp=np.sum(np.abs(lpi), axis=1),
               A_mu=np.abs(Y) + np.abs(al * var))
    return {k: be.f64(v) for k, v in res.items()}


def truth(X, Y, theta, backend):
    if backend == "mp":
        be = H._MP()
        with be.m.workdps(50):
            return _truth(be, X, Y, theta)
    return _truth(H._LD(), X, Y, theta)


# ---- fp64 variants ------------------------------------------------------------------------------
def _closed(Y, kinv, alpha):
    """mu (G, N), var (N), logp_i (G, N), logp (G) from kinv (N) and alpha (G, N), fp64."""
    var = 1.0 / kinv
    lpi = 0.5 * np.log(kinv) - 0.5 * alpha * alpha / kinv - HALF_LOG_2PI
    return dict(mu=Y - alpha / kinv, var=var, logp_i=lpi, logp=np.sum(lpi, axis=1))


def _lapack(X, Y, theta, mode):
    al, U = [], None
    for y in Y:
        _, _, aux = O.lml(X, y, theta, mode)
        U = aux["U"]
        al.append(aux["alpha"])
    Ui = sla.solve_triangular(U, np.eye(U.shape[0]), lower=False)
    return _closed(Y, np.sum(Ui * Ui, axis=1), np.stack(al))


def _staged(X, Y, theta, mode):
    N = X.shape[1]
    _, _, _, noise = O.kernel_params(theta, X.shape[0])
    A = H._staged_kernel(X, X, theta, mode)
    ix = np.arange(N)
    A[ix, ix] = A[ix, ix] + noise
    Li = np.zeros((N, N))
    H._factor_tiles(A, Li, 0, -(-N // H.TILE))
    Li = np.tril(Li)
    return _closed(Y, np.sum(Li * Li, axis=0), np.stack([Li.T @ (Li @ y) for y in Y]))


def _brute(X, Y, theta, mode):
    d, N = X.shape
    G = Y.shape[0]
    _, sf2, _, noise = O.kernel_params(theta, d)
    mu, var = np.empty((G, N)), np.empty(N)
    if N == 1:
        mu[:], var[:] = 0.0, sf2 + noise
    else:
        D = O.dist_stack(X, X, mode)
        for i in range(N):
            keep = np.r_[0:i, i + 1:N]
            Xk, Dk = np.ascontiguousarray(X[:, keep]), np.ascontiguousarray(D[:, keep][:, :, keep])
            _, _, aux = O.lml(Xk, Y[0, keep], theta, mode, D=Dk)
            for g in range(G):
                a = aux["alpha"] if g == 0 else sla.cho_solve((aux["U"], False), Y[g, keep])
                m, v = O.predict_f(Xk, theta, a, aux["U"], X[:, i:i + 1], mode)
                mu[g, i], var[i] = m[0], v[0] + noise
    lpi = -0.5 * np.log(var) - 0.5 * (Y - mu) ** 2 / var - HALF_LOG_2PI
    return dict(mu=mu, var=var, logp_i=lpi, logp=np.sum(lpi, axis=1))


def _rev(f, X, Y, theta, mode):
    r = f(np.ascontiguousarray(X[:, ::-1]), np.ascontiguousarray(Y[:, ::-1]), theta, mode)
    return {k: (v if k == "logp" else np.ascontiguousarray(v[..., ::-1])) for k, v in r.items()}


def variants(X, Y, theta, mode):
    return {"lapack": _lapack(X, Y, theta, mode), "lapack_rev": _rev(_lapack, X, Y, theta, mode),
            "brute": _brute(X, Y, theta, mode), "staged": _staged(X, Y, theta, mode),
            "staged_rev": _rev(_staged, X, Y, theta, mode)}


def floors(tr, E_mu):
    """A_q per quantity of one truth record; mu's is |mu| unless E_mu == 0 (see the module docstring)."""
    return dict(mu=np.abs(tr["mu"]) if E_mu > 0 else tr["A_mu"], var=np.abs(tr["var"]), logp_i=np.abs(tr["logp_i"]),
                logp=tr["A_logp"])


# ---- assembly -----------------------------------------------------------------------------------
def solve(job):
    name, ti = job
    X, Y, thetas = case_inputs(name)
    tr = truth(X, Y, thetas[ti], backend_of(X.shape[1]))
    return name, ti, tr, {mode: variants(X, Y, thetas[ti], mode) for mode in (0, 1)}


def assemble(name, parts, k):
    X, Y, thetas = case_inputs(name)
    T = len(thetas)
    fx = dict(case=np.array(name), backend=np.array(backend_of(X.shape[1])), quantities=np.array(QUANTITIES),
              variant_names=np.array(VARIANTS), k=np.array(k),
              B=np.array((0, 32) if name in B32 else (0,), dtype=np.int64))
    if name in STORED:
        fx.update(X=X, Y=Y, thetas=thetas)
    for q in QUANTITIES + ("A_logp", "A_mu"):
        fx[q] = np.stack([parts[t][0][q] for t in range(T)])
    E = np.zeros((2, T, len(QUANTITIES)))
    worst = 0.0
    for vn in VARIANTS:
        for q in QUANTITIES:
            fx[f"d_{vn}_{q}"] = np.stack([np.stack([parts[t][1][mode][vn][q] - parts[t][0][q] for t in range(T)])
                                          for mode in (0, 1)]).astype(np.float32)
    for mode in (0, 1):
        for t in range(T):
            for qi, q in enumerate(QUANTITIES):
                errs = [np.abs(fx[f"d_{vn}_{q}"][mode, t].astype(np.float64)) for vn in VARIANTS]
                E[mode, t, qi] = H.geomean([np.max(e) for e in errs])
                A = floors(parts[t][0], E[mode, t, 0])
                worst = max(worst, max(H.ratio(e, E[mode, t, qi], H.EPS * A[q]) for e in errs))
    fx["E"] = E
    return fx, worst


def prune(fx):
    """Takes the rungs of LEFT_OUT out of a case's arrays and fails if a CPU variant exceeds
    k max(E_q, eps A_q) at any rung kept, in either mode.  theta_index: the rungs kept, as indices into
    the case's thetas."""
    k, T = float(fx["k"]), fx["E"].shape[1]
    keep = [t for t in range(T) if t not in LEFT_OUT.get(str(fx["case"]), ())]
    for t in keep:
        for mode in (0, 1):
            A = floors({q: fx[q][t] for q in ("mu", "A_mu", "var", "logp_i", "A_logp")}, fx["E"][mode, t, 0])
            worst = max(H.ratio(np.abs(fx[f"d_{vn}_{q}"][mode, t].astype(np.float64)), fx["E"][mode, t, qi], H.EPS * A[q])
                        for qi, q in enumerate(QUANTITIES) for vn in VARIANTS)
            assert worst <= k, f"{fx['case']} theta {t} mode {mode}: a variant at {worst:.2f} > k; review LEFT_OUT"
    out = dict(fx)
    for key in QUANTITIES + ("A_logp", "A_mu"):
        out[key] = fx[key][keep]
    for key in [n for n in fx if n.startswith("d_")] + ["E"]:
        out[key] = fx[key][:, keep]
    out["theta_index"] = np.array(keep, dtype=np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    names = [n for n in CASES if a.only is None or n in a.only]
    with np.load(HERE / "hp_a_p2_1.npz") as z:
        k = float(z["k"])
    if a.only is None or "b_cp_130" in a.only:
        X, Y, thetas = case_inputs("b_cp_130")
        mp, ld = truth(X, Y, thetas[0], "mp"), truth(X, Y, thetas[0], "ld")
        print("float80 against mpmath at b_cp_130 theta 0: " + ", ".join(
            f"{q} {np.max(np.abs(mp[q] - ld[q])):.2e} (max |truth| {np.max(np.abs(mp[q])):.2e})" for q in QUANTITIES), flush=True)
    jobs = [(n, ti) for n in names for ti in range(len(case_inputs(n)[2]))]
    jobs.sort(key=lambda j: -case_inputs(j[0])[0].shape[1])
    parts = {}
    with cf.ProcessPoolExecutor(a.j) as ex:
        for name, ti, tr, var in ex.map(solve, jobs):
            parts.setdefault(name, {})[ti] = (tr, var)
            print(f"{name} theta {ti} done", flush=True)
    for name in names:
        fx, worst = assemble(name, parts[name], k)
        print(f"{name}: largest variant ratio {worst:.2f} (k = {k})")
        save_npz(HERE / f"loo_{name}.npz", prune(fx))


if __name__ == "__main__":
    main()
