"""Regenerates tests/golden/hp_*.npz: inputs, the high-precision truth (oracle/hp_oracle.py), the
errors of the fp64 CPU variants against it, E_q (for the gradient per component: E_grad), A_q, k and
cond(K).  Byte-identical on every run.

    python tests/golden/make_golden_hp.py [-j PROCS] [--only NAME ...]

Cases (tests/test_hp_parity.py runs each at the batch sizes in "B"; 0 stands for one slot per
(theta, target)).  N <= 130 uses mpmath at 50 digits, N >= 256 np.longdouble (validated against
mpmath at N = 130 by tests/test_hp_oracle.py):
  a  P2 d=26, N = 1, 5, 33, 64, 65    single and partial tile, two tiles; N = 33 is the case the CPU
                                      suite regenerates
  b  P2, FB (d=52), CP, P1 (d=13)     N = 130: three tiles, asymmetric recursion; P2 and CP also fill 32
                                      slots
  c  P2, CP at N = 256, 320           fused leaves of 4, and of 2 and 3 tiles, 32 slots
  d  P2, CP at N = 512, 500           the one-launch 8-tile node, 500 pads the last tile
  e  d = 1, 16, 17, 33, 64            slot 0 of test_input_dimension_extremes' random inputs (both
                                      slots' targets), N = 130, M = 9
theta is gprx/theta_config.json's; the CP and P1 cases carry the noise ladder log sigma_n = -2, -5, -6:
a case holds at most three theta, dpotrf succeeds in both distance modes down to -6 on every one of
them (a rung is dropped where it does not), and -4 lies between rungs that are kept.  With M >= 4 test column 0 is a training
point, column 2 repeats column 1 and the last column lies 60 length scales away.
k is the largest ratio, over every case, theta, mode, quantity and variant, of a variant's error to
max(E_q, eps A_q), rounded up to a power of two and at least 4; it is computed over all cases
(also with --only) and stored in each file.  The gradient is held twice: to k and its E_q, the largest
error over components and targets, as every other quantity; and per component to k_grad and E_grad,
the same two figures formed for each component alone, so that a component far below g[0] is held to
its own scale.  One draw per component is noisier than the largest of d + 2, hence its own k_grad.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import importlib.util
import io
import math
import pathlib
import sys
import zipfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO))

from oracle import gp_oracle as O  # noqa: E402
from oracle import hp_oracle as H  # noqa: E402

LADDER = (-2.0, -5.0, -6.0)
VARIANTS = ("lapack", "explicit", "staged", "lapack_rev", "staged_rev")
COV_MAX_M = 17


def load_data():
    """gprx/data.py by file path: the library need not be built."""
    spec = importlib.util.spec_from_file_location("gprx_data", REPO / "gpr.jl_amd" / "gprx" / "data.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trial(name, mech, N, M, key, B, ladder=False):
    return dict(name=name, kind="trial", mech=mech, N=N, M=M, key=key, B=B, ladder=ladder)


CASES = [
    _trial("a_p2_1", "P2", 1, 1, 2, (0,)),
    _trial("a_p2_5", "P2", 5, 17, 4, (0,)),
    _trial("a_p2_33", "P2", 33, 5, 32, (0,)),
    _trial("a_p2_64", "P2", 64, 17, 64, (0,)),
    _trial("a_p2_65", "P2", 65, 100, 64, (0,)),
    _trial("b_p2_130", "P2", 130, 17, 128, (0, 32)),
    _trial("b_fb_130", "FB", 130, 17, 128, (0,)),
    _trial("b_cp_130", "CP", 130, 100, 128, (0, 32), ladder=True),
    _trial("b_p1_130", "P1", 130, 17, 128, (0,), ladder=True),
    _trial("c_p2_256", "P2", 256, 1, 256, (32,)),
    _trial("c_cp_256", "CP", 256, 17, 256, (32,), ladder=True),
    _trial("c_p2_320", "P2", 320, 100, 256, (32,)),
    _trial("c_cp_320", "CP", 320, 17, 256, (32,), ladder=True),
    _trial("d_p2_512", "P2", 512, 17, 512, (32,)),
    _trial("d_cp_512", "CP", 512, 100, 512, (32,), ladder=True),
    _trial("d_p2_500", "P2", 500, 100, 512, (32,)),
    _trial("d_cp_500", "CP", 500, 17, 512, (32,), ladder=True),
] + [dict(name=f"e_d{d}", kind="dim", d=d, N=130, M=9, B=(0,), ladder=False) for d in (1, 16, 17, 33, 64)]


def case_inputs(c):
    """X (d, N), Y (G, N), Xs (d, M), thetas (T, d + 2)."""
    if c["kind"] == "dim":
        d, N, M, B = c["d"], c["N"], c["M"], 2
        rng = np.random.default_rng(100 + d)
        X = rng.standard_normal((B, d, N))
        Xs = rng.standard_normal((B, d, M))
        Y = np.stack([np.sin(X[s].sum(axis=0)) + 0.05 * rng.standard_normal(N) for s in range(B)])
        th = np.stack([np.concatenate([[-2.0], np.log(np.full(d, 1.5 * np.sqrt(d)) * (1 + 0.1 * rng.random(d))), [0.1]])
                       for _ in range(B)])
        X, Xs, thetas = X[0], Xs[0].copy(), th[:1]
    else:
        data = load_data()
        tr = data.make_trial(c["mech"], c["N"], c["M"], seed=7)
        X, Y, Xs = tr["X"], tr["Y"], tr["Xs"].copy()
        th = data.theta0(c["mech"], c["key"])
        rungs = []
        for ls in (LADDER if c["ladder"] else LADDER[:1]):
            t = th.copy()
            t[0] = ls
            try:
                for mode in (0, 1):
                    O.cholesky_upper(O.gram(X, t, mode)[0])
                rungs.append(t)
            except O.NotPosDef:
                print(f"{c['name']}: rung log sigma_n = {ls} dropped (dpotrf fails)")
        thetas = np.stack(rungs)
    M = Xs.shape[1]
    if M >= 4:
        Xs[:, 0] = X[:, X.shape[1] // 2]
        Xs[:, 2] = Xs[:, 1]
        Xs[:, M - 1] = X[:, 0] + 60.0 * np.exp(thetas[0][1:-1])
    return np.ascontiguousarray(X), np.ascontiguousarray(Y), np.ascontiguousarray(Xs), thetas


def backend_of(c):
    return "mp" if c["N"] <= 130 else "ld"


def solve(job):
    """One (case, theta): the truth and each variant's results."""
    ci, ti = job
    c = CASES[ci]
    X, Y, Xs, thetas = case_inputs(c)
    tr = H.truth(X, Y, thetas[ti], Xs, backend_of(c), want_cov=Xs.shape[1] <= COV_MAX_M)
    var = {mode: H.variants(X, Y, thetas[ti], Xs, mode) for mode in (0, 1)}
    cond = float(np.linalg.cond(O.gram(X, thetas[ti], 1)[0]))
    return ci, ti, tr, var, cond


def assemble(c, parts):
    """Fixture arrays of a case from its per-theta parts, and its largest variant ratio."""
    X, Y, Xs, thetas = case_inputs(c)
    T = len(thetas)
    fx = dict(X=X, Y=Y, Xs=Xs, thetas=thetas, B=np.array(c["B"], dtype=np.int64), backend=np.array(backend_of(c)),
              variant_names=np.array(VARIANTS), quantities=np.array(H.QUANTITIES),
              cond=np.array([parts[t][3] for t in range(T)]))
    keys = [k for k in parts[0][1]]
    for k in keys:
        fx[k] = np.stack([parts[t][1][k] for t in range(T)])
    nq = len(H.QUANTITIES)
    verr = np.full((2, len(VARIANTS), T, nq), np.nan)
    E = np.full((2, T, nq), np.nan)
    Eg = np.zeros((2, T, X.shape[0] + 2))  # the gradient's E per component (largest over the targets)
    worst, worst_g = 0.0, 0.0
    for t in range(T):
        tr = parts[t][1]
        for mode in (0, 1):
            res = parts[t][2][mode]
            for qi, q in enumerate(H.QUANTITIES):
                if q not in tr:
                    continue
                errs = [np.abs(res[vn][q] - tr[q]) for vn in VARIANTS]
                verr[mode, :, t, qi] = [np.max(e) for e in errs]
                E[mode, t, qi] = H.geomean(verr[mode, :, t, qi])
                floor = H.EPS * H.floor_of(tr, q, mode)
                worst = max(worst, max(H.ratio(e, E[mode, t, qi], floor) for e in errs))
                if q == "grad":
                    Eg[mode, t] = [H.geomean([np.max(e[:, p]) for e in errs]) for p in range(Eg.shape[2])]
                    worst_g = max(worst_g, max(H.ratio(e, Eg[mode, t], floor) for e in errs))
    fx["verr"], fx["E"], fx["E_grad"] = verr, E, Eg
    return fx, worst, worst_g


def save_npz(path, arrays):
    """np.savez's layout with a fixed timestamp, so that regeneration is byte-identical."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--only", nargs="*", default=None, help="write only these cases (k still spans all)")
    a = ap.parse_args()
    jobs = [(ci, ti) for ci, c in enumerate(CASES) for ti in range(len(case_inputs(c)[3]))]
    jobs.sort(key=lambda j: -(CASES[j[0]]["N"] if backend_of(CASES[j[0]]) == "ld" else 10 * CASES[j[0]]["N"]
                              * CASES[j[0]].get("d", 26)))
    parts = {}
    with cf.ProcessPoolExecutor(a.j) as ex:
        for ci, ti, tr, var, cond in ex.map(solve, jobs):
            parts.setdefault(ci, {})[ti] = (None, tr, var, cond)
            print(f"{CASES[ci]['name']} theta {ti}: cond {cond:.2e}", flush=True)
    out, worst, worst_g = {}, 0.0, 0.0
    for ci, c in enumerate(CASES):
        out[c["name"]], w, wg = assemble(c, parts[ci])
        print(f"{c['name']}: largest variant ratio {w:.2f}, of a gradient component to its own E {wg:.2f}")
        worst, worst_g = max(worst, w), max(worst_g, wg)
    k, kg = (max(4.0, 2.0 ** math.ceil(math.log2(w))) for w in (worst, worst_g))
    print(f"largest ratio {worst:.3f} -> k = {k}; per gradient component {worst_g:.3f} -> k_grad = {kg}")
    for name, fx in out.items():
        if a.only is None or name in a.only:
            fx["k"], fx["k_grad"] = np.array(k), np.array(kg)
            save_npz(HERE / f"hp_{name}.npz", fx)


if __name__ == "__main__":
    main()
