"""Regenerates tests/golden/loograd_*.npz: the high-precision truth of the leave-one-out log predictive
probability and of its gradient with respect to theta = [log sn, log ell_1..d, log sf] (dlogpdθ_LOO;
Rasmussen & Williams 5.13), the errors of five fp64 CPU variants against it, E, E_grad, A_grad, k and
k_comp.  CPU only, byte-identical on every run.

    python tests/golden/make_golden_loo_grad.py [-j PROCS] [--only NAME ...]

Inputs (X, Y, thetas) come by name from tests/golden/hp_<case>.npz, and those of f_cp_520 and of
g_nonpd_p1 (nonpd_p1.npz's inputs at log sigma_n = -2: the good neighbour of the failing slot in
tests/test_loo_grad.py) from loo_<case>.npz; a fixture stores only the name.  A fixture's slots are its (theta, target) pairs.

With K = Kf + (exp(2 log sn) + eps) I, q_i = [K^-1]_ii, alpha = K^-1 y:
    logp = sum_i [log(q_i)/2 - alpha_i^2/(2 q_i) - log(2 pi)/2]
    c_i = (1/q_i + alpha_i^2/q_i^2)/2,  r_i = alpha_i/q_i,  beta = K^-1 r,  C = diag(c)
    dlogp = sum_kl dK_kl W'_kl,   W' = (beta alpha^T + alpha beta^T)/2 - K^-1 C K^-1       (the contraction)
    dK/dlog sn = 2 sn2 I,  dK/dlog ell_p = Kf o (x_p - x_p')^2/ell_p^2,  dK/dlog sf = 2 Kf
truth      logp and grad by the contraction, in 50-digit mpmath for N <= 130 and in x87 extended precision
           above (the backends of oracle/hp_oracle.py): exact differences in the distances, Cholesky, L^-1
           by substitution, K^-1 = L^-T L^-1, alpha by two substitutions; rounded to fp64 once.  On a_p2_5
           and e_d1 the generator also evaluates 5.13 parameter by parameter,
               dlogp/dtheta_j = sum_i [alpha_i (Z_j alpha)_i - (1 + alpha_i^2/q_i) (Z_j K^-1)_ii / 2] / q_i,
               Z_j = K^-1 dK/dtheta_j,
           and a central difference of the high-precision logp (h = 1e-12 at 50 digits), and asserts that
           both agree with the contraction (1e-40 and 1e-15 of the gradient's largest component).
variants   per distance mode, in fp64:
           "lapack"      gp_oracle.lml's U (K^-1 = U^-1 U^-T) and alpha, the contraction
           "lapack_rev"  the same over the points in reverse order
           "r513"        5.13 parameter by parameter with cho_solve on that U
           "staged"      the Gram as the device forms it (hp_oracle._staged_kernel), factorised and
                         inverted over 64-row tiles (hp_oracle._factor_tiles), the contraction
           "staged_rev"  the same over the points in reverse order
           Stored as d_<variant> = variant's grad - truth, (2, T, G, d + 2).
E[mode, theta]          the geometric mean over the five variants of their largest |grad - truth| (over
                        targets and components)
E_grad[mode, theta, p]  the same per component (largest over the targets)
A_grad[theta, g, p]     sum_kl |dK_kl W'_kl|, the absolute sum of the component's contraction.  In expanded
                        mode a component whose truth is exactly 0 (a constant coordinate) takes the expanded
                        distance form's operands, A_grad_exp (a^2 + b^2 in place of (a - b)^2), as
                        hp_oracle.floor_of does for the marginal likelihood's gradient.
k          8, the factor every hp_*.npz carries; read from hp_a_p2_1.npz, never fitted here.
k_comp     make_golden_hp.py's rule for k_grad, from the CPU variants alone: the largest ratio, over every
           case, theta kept, mode, variant, target and component, of a component's error to
           max(E_grad[p], eps A[p]), rounded up to a power of two and at least 4.  A full run computes and
           stores it; with --only it is read from loograd_a_p2_1.npz and the generator fails if a case
           written exceeds it.
The generator prints the largest ratio of a variant's error to max(E, eps A) per case; the rungs of the
fixed list LEFT_OUT are left out of their case (theta_index names the rungs kept), and the
generator fails if a variant exceeds k at any rung kept.
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
from make_golden_hp import save_npz  # noqa: E402

VARIANTS = ("lapack", "lapack_rev", "r513", "staged", "staged_rev")
HP_CASES = ("a_p2_1", "a_p2_5", "a_p2_64", "a_p2_65", "b_cp_130", "b_p1_130", "b_fb_130", "e_d1", "c_cp_320", "d_cp_500")
LOO_CASE = "f_cp_520"  # inputs stored in loo_f_cp_520.npz
NONPD_CASE = "g_nonpd_p1"  # ... in loo_g_nonpd_p1.npz
CASES = HP_CASES + (LOO_CASE, NONPD_CASE)
CHECKED = ("a_p2_5", "e_d1")  # 5.13 parameter by parameter and the central difference, in high precision
# theta rungs left out of a case, by index into its thetas, with the measured ratio beside each: a fixed,
# reviewed list (at most one rung per case, never a log sigma_n = -2 rung).
#   b_p1_130 rung 2 (log sigma_n = -6, cond(K) = 7e11): a variant at 12.19 max(E, eps A) in direct mode
#   (2.55 in expanded mode), the rung make_golden_loo.py leaves out too; k is not changed to suit it.
LEFT_OUT = {"b_p1_130": (2,)}
B32 = ("c_cp_320", "d_cp_500", LOO_CASE)  # also run in 32 slots
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def case_inputs(name):
    """X (d, N), Y (G, N), thetas (T, d + 2)."""
    fn = HERE / (f"loo_{name}.npz" if name in (LOO_CASE, NONPD_CASE) else f"hp_{name}.npz")
    with np.load(fn) as z:
        return z["X"].copy(), np.atleast_2d(z["Y"]).copy(), z["thetas"].copy()


def backend_of(N):
    return "mp" if N <= 130 else "ld"


# ---- truth --------------------------------------------------------------------------------------
def _state(be, X, Y, th):
    """Kf, K^-1, alpha (G, N) and logp (G) in the backend's arithmetic; X, Y, th already in it."""
    d, N = X.shape
    il2, sf2, sn2 = be.exp(-2 * th[1:d + 1]), be.exp(2 * th[d + 1]), be.exp(2 * th[0])
    t = X[:, :, None] - X[:, None, :]
    D = t * t
    r = be.zeros((N, N))
    for p in range(d):
        r = r + D[p] * il2[p]
    Kf = sf2 * be.exp(-r / 2)
    K = Kf.copy()
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
    Kinv = Z.T @ Z
    G = Y.shape[0]
    T = be.zeros((N, G))
    for i in range(N):
        T[i] = (Y.T[i] - H._dot(L[i, :i], T[:i])) / L[i, i]
    Al = be.zeros((N, G))
    for i in range(N - 1, -1, -1):
        Al[i] = (T[i] - H._dot(L[i + 1:, i], Al[i + 1:])) / L[i, i]
    al = Al.T
    q = Kinv[ix, ix]
    lpi = be.log(q) / 2 - al * al / q / 2 - be.log2pi() / 2
    return dict(D=D, Kf=Kf, Kinv=Kinv, al=al, q=q, logp=np.sum(lpi, axis=1), il2=il2, sf2=sf2, sn2=sn2)


def _truth(be, X64, Y64, theta, check):
    d, N = X64.shape
    X, Y, th = be.arr(X64), be.arr(Y64), be.arr(theta)
    s = _state(be, X, Y, th)
    D, Kf, Kinv, q, il2, sn2 = s["D"], s["Kf"], s["Kinv"], s["q"], s["il2"], s["sn2"]
    ix = np.arange(N)
    Df = D.reshape(d, N * N)
    x2 = X * X
    out = {k: [] for k in ("grad", "A_grad", "A_grad_exp")}
    for g in range(Y.shape[0]):
        a = s["al"][g]
        c = (1 / q + a * a / (q * q)) / 2
        r = a / q
        b = Kinv @ r
        W = (np.outer(b, a) + np.outer(a, b)) / 2 - (Kinv * c[None, :]) @ Kinv
        WK = W * Kf
        aWK = np.abs(WK)
        gr, Ag, Ae = be.zeros(d + 2), be.zeros(d + 2), be.zeros(d + 2)
        gr[0], Ag[0] = 2 * sn2 * np.sum(W[ix, ix]), 2 * sn2 * np.sum(np.abs(W[ix, ix]))
        gr[1:d + 1] = (Df @ WK.reshape(-1)) * il2
        Ag[1:d + 1] = (Df @ aWK.reshape(-1)) * il2
        gr[d + 1], Ag[d + 1] = 2 * np.sum(WK), 2 * np.sum(aWK)
        Ae[1:d + 1] = (x2 @ np.sum(aWK, axis=1)) * 2 * il2
        Ae[0], Ae[d + 1] = Ag[0], Ag[d + 1]
        if check:  # 5.13 parameter by parameter, and a central difference of logp
            dKs = [2 * sn2 * np.eye(N, dtype=object)] + [Kf * D[p] * il2[p] for p in range(d)] + [2 * Kf]
            scale = max(abs(v) for v in gr)
            for j, dK in enumerate(dKs):
                Zj = Kinv @ dK
                g513 = np.sum((a * (Zj @ a) - (1 + a * a / q) * np.sum(Zj * Kinv.T, axis=1) / 2) / q)
                assert abs(g513 - gr[j]) <= be.arr(1e-40) * scale, ("5.13 against the contraction", j, g513, gr[j])
                h = be.arr(1e-12)
                e = be.zeros(d + 2)
                e[j] = e[j] + h
                fd = (_state(be, X, Y[g:g + 1], th + e)["logp"][0] - _state(be, X, Y[g:g + 1], th - e)["logp"][0]) / (2 * h)
                assert abs(fd - gr[j]) <= be.arr(1e-15) * scale, ("central difference against the contraction", j, fd, gr[j])
        for k, v in (("grad", gr), ("A_grad", Ag), ("A_grad_exp", Ae)):
            out[k].append(v)
    res = {k: be.f64(np.stack(v)) for k, v in out.items()}
    res["logp"] = be.f64(s["logp"])
    return res


def truth(X, Y, theta, backend, check=False):
    if backend == "mp":
        be = H._MP()
        with be.m.workdps(50):
            return _truth(be, X, Y, theta, check)
    assert not check
    return _truth(H._LD(), X, Y, theta, False)


# ---- fp64 variants ------------------------------------------------------------------------------
def _contract(Kinv, alpha, Kf, D, theta):
    """grad (G, d + 2) by the contraction, fp64."""
    d, N = D.shape[0], D.shape[1]
    il2, _, sn2, _ = O.kernel_params(theta, d)
    q = np.diag(Kinv).copy()
    Df = D.reshape(d, N * N)
    out = []
    for a in alpha:
        c = 0.5 * (1.0 / q + a * a / (q * q))
        b = Kinv @ (a / q)
        W = 0.5 * (np.outer(b, a) + np.outer(a, b)) - (Kinv * c[None, :]) @ Kinv
        WK = W * Kf
        g = np.empty(d + 2)
        g[0] = 2.0 * sn2 * np.trace(W)
        g[1:d + 1] = (Df @ WK.reshape(-1)) * il2
        g[d + 1] = 2.0 * np.sum(WK)
        out.append(g)
    return np.stack(out)


def _lapack_parts(X, Y, theta, mode):
    al, U = [], None
    for y in Y:
        _, _, aux = O.lml(X, y, theta, mode)
        U = aux["U"]
        al.append(aux["alpha"])
    _, Kf, D = O.gram(X, theta, mode)
    return U, np.stack(al), Kf, D


def _lapack(X, Y, theta, mode):
    U, al, Kf, D = _lapack_parts(X, Y, theta, mode)
    Ui = sla.solve_triangular(U, np.eye(U.shape[0]), lower=False)
    return _contract(Ui @ Ui.T, al, Kf, D, theta)


def _r513(X, Y, theta, mode):
    U, al, Kf, D = _lapack_parts(X, Y, theta, mode)
    d, N = X.shape
    il2, _, sn2, _ = O.kernel_params(theta, d)
    Kinv = sla.cho_solve((U, False), np.eye(N))
    q = np.diag(Kinv).copy()
    dKs = [2.0 * sn2 * np.eye(N)] + [Kf * D[p] * il2[p] for p in range(d)] + [2.0 * Kf]
    g = np.empty((len(Y), d + 2))
    for j, dK in enumerate(dKs):
        Zj = sla.cho_solve((U, False), dK)
        zk = np.sum(Zj * Kinv.T, axis=1)  # diag(Z_j K^-1)
        for gi, a in enumerate(al):
            g[gi, j] = np.sum((a * (Zj @ a) - 0.5 * (1.0 + a * a / q) * zk) / q)
    return g


def _staged(X, Y, theta, mode):
    N = X.shape[1]
    _, _, _, noise = O.kernel_params(theta, X.shape[0])
    Kf = H._staged_kernel(X, X, theta, mode)
    A = Kf.copy()
    ix = np.arange(N)
    A[ix, ix] = A[ix, ix] + noise
    Li = np.zeros((N, N))
    H._factor_tiles(A, Li, 0, -(-N // H.TILE))
    Li = np.tril(Li)
    return _contract(Li.T @ Li, np.stack([Li.T @ (Li @ y) for y in Y]), Kf, O.dist_stack(X, X, mode), theta)


def _rev(f, X, Y, theta, mode):  # the gradient does not depend on the order of the points
    return f(np.ascontiguousarray(X[:, ::-1]), np.ascontiguousarray(Y[:, ::-1]), theta, mode)


def variants(X, Y, theta, mode):
    return {"lapack": _lapack(X, Y, theta, mode), "lapack_rev": _rev(_lapack, X, Y, theta, mode),
            "r513": _r513(X, Y, theta, mode), "staged": _staged(X, Y, theta, mode),
            "staged_rev": _rev(_staged, X, Y, theta, mode)}


def floor_of(grad, A_grad, A_grad_exp, mode):
    """A per component; in expanded mode the components whose truth is exactly 0 take A_grad_exp."""
    return np.where(grad == 0.0, A_grad_exp, A_grad) if mode == O.DIST_EXPANDED else A_grad


# ---- assembly -----------------------------------------------------------------------------------
def solve(job):
    name, ti = job
    X, Y, thetas = case_inputs(name)
    tr = truth(X, Y, thetas[ti], backend_of(X.shape[1]), check=name in CHECKED)
    return name, ti, tr, {mode: variants(X, Y, thetas[ti], mode) for mode in (0, 1)}


def assemble(name, parts, k):
    """Fixture arrays of a case, its largest variant ratio on the vector and per component."""
    X, Y, thetas = case_inputs(name)
    T, d = len(thetas), X.shape[0]
    fx = dict(case=np.array(name), backend=np.array(backend_of(X.shape[1])), variant_names=np.array(VARIANTS), k=np.array(k),
              B=np.array((0, 32) if name in B32 else (0,), dtype=np.int64))
    for q in ("logp", "grad", "A_grad", "A_grad_exp"):
        fx[q] = np.stack([parts[t][0][q] for t in range(T)])
    for vn in VARIANTS:
        fx[f"d_{vn}"] = np.stack([np.stack([parts[t][1][mode][vn] - parts[t][0]["grad"] for t in range(T)]) for mode in (0, 1)])
    E, Eg = np.zeros((2, T)), np.zeros((2, T, d + 2))
    worst, worst_c = np.zeros((2, T)), np.zeros((2, T))
    for mode in (0, 1):
        for t in range(T):
            errs = [np.abs(fx[f"d_{vn}"][mode, t]) for vn in VARIANTS]
            floor = H.EPS * floor_of(fx["grad"][t], fx["A_grad"][t], fx["A_grad_exp"][t], mode)
            E[mode, t] = H.geomean([np.max(e) for e in errs])
            Eg[mode, t] = [H.geomean([np.max(e[:, p]) for e in errs]) for p in range(d + 2)]
            worst[mode, t] = max(H.ratio(e, E[mode, t], floor) for e in errs)
            worst_c[mode, t] = max(H.ratio(e, Eg[mode, t], floor) for e in errs)
    fx["E"], fx["E_grad"] = E, Eg
    return fx, worst, worst_c


def prune(fx, worst, worst_c):
    """Takes the rungs of LEFT_OUT out of a case's arrays and fails if a CPU variant exceeds
    k max(E, eps A) at any rung kept, in either mode.  theta_index: the rungs kept.  Returns the arrays
    and the largest per-component ratio over the rungs kept."""
    name, k, T = str(fx["case"]), float(fx["k"]), fx["E"].shape[1]
    keep = [t for t in range(T) if t not in LEFT_OUT.get(name, ())]
    for t in keep:
        assert np.max(worst[:, t]) <= k, f"{name} theta {t}: a variant at {np.max(worst[:, t]):.2f} > k; review LEFT_OUT"
    out = dict(fx)
    for key in ("logp", "grad", "A_grad", "A_grad_exp"):
        out[key] = fx[key][keep]
    for key in [n for n in fx if n.startswith("d_")] + ["E", "E_grad"]:
        out[key] = fx[key][:, keep]
    out["theta_index"] = np.array(keep, dtype=np.int64)
    return out, float(np.max(worst_c[:, keep]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8, help="worker processes (1: in this process)")
    ap.add_argument("--only", nargs="*", default=None, help="write only these cases (k_comp is then read from loograd_a_p2_1.npz)")
    ap.add_argument("--out", default=str(HERE), help="directory the fixtures are written to")
    a = ap.parse_args(argv)
    names = [n for n in CASES if a.only is None or n in a.only]
    with np.load(HERE / "hp_a_p2_1.npz") as z:
        k = float(z["k"])
    jobs = [(n, ti) for n in names for ti in range(len(case_inputs(n)[2]))]

    def cost(j):
        X, Y, _ = case_inputs(j[0])
        return -(X.shape[1] ** 3) * (1 if backend_of(X.shape[1]) == "ld" else 40 * Y.shape[0])

    jobs.sort(key=cost)
    parts = {}
    with cf.ProcessPoolExecutor(a.j) if a.j > 1 else cf.ThreadPoolExecutor(1) as ex:
        for name, ti, tr, var in ex.map(solve, jobs):
            parts.setdefault(name, {})[ti] = (tr, var)
            print(f"{name} theta {ti} done", flush=True)
    out, worst_c = {}, 0.0
    for name in names:
        fx, worst, wc = assemble(name, parts[name], k)
        print(f"{name}: largest variant ratio per rung (mode 0; mode 1) {np.round(worst, 2).tolist()} (k = {k}), "
              f"of a component to its own E {np.round(wc, 2).tolist()}")
        out[name], wck = prune(fx, worst, wc)
        worst_c = max(worst_c, wck)
    if a.only is None:
        k_comp = max(4.0, 2.0 ** math.ceil(math.log2(worst_c)))
        print(f"largest per-component ratio {worst_c:.3f} -> k_comp = {k_comp}")
    else:
        with np.load(HERE / "loograd_a_p2_1.npz") as z:
            k_comp = float(z["k_comp"])
        assert worst_c <= k_comp, f"a component at {worst_c:.2f} > k_comp = {k_comp}: run without --only"
    for name, fx in out.items():
        fx["k_comp"] = np.array(k_comp)
        save_npz(pathlib.Path(a.out) / f"loograd_{name}.npz", fx)


if __name__ == "__main__":
    main()
