"""cv_pack / cv_kinv / cv_fold / cv_final from gprx_ctx_kernel_stats (profiling on) at the bench shape
(P2, B = 240, N = 2048, d = 26) for two fold layouts, (a) 98 trajectory folds of at most 21 points and
(b) 8 folds of 256 points, next to loo_kinv of the same run (the route that forms all of K^-1), and one
cvfold() call with F = 98 against 98 refits of the same batch through set_train / run / predict.
RUNS runs per layout, each a fresh context and batch: one evaluation, WARM cvfold and loo_grad calls,
stats reset, then REPS calls of each.  Prints one line per kernel and run, then the median run; `--out
FILE` also writes the text there (profiles/cvfold_kernel_stats.txt).

    python scratch/cvfold_kernel_stats.py [--out FILE] [--no-refit]
"""
import argparse
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1] / "gpr.jl_amd"))
import gprx  # noqa: E402

RUNS, WARM, REPS = 3, 3, 10
KERNELS = ("cv_pack", "cv_kinv", "cv_fold", "cv_final", "loo_kinv", "loo_diag")
B, D, N = 240, 26, 2048


def inputs():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((D, N))
    Y = np.sin(X.sum(axis=0))[None, :] + 0.05 * rng.standard_normal((B, N))
    th = np.concatenate([[-2.0], np.log(np.full(D, 1.5 * np.sqrt(D))), [0.1]])
    return X, Y, th


def one_run(fold_of):
    X, Y, th = inputs()
    c = gprx.Context(0)
    c.set_profiling(True)
    b = gprx.GPBatch(B, D, N, 0, ctx=c)
    try:
        b.set_train(X, Y)
        b.set_folds(fold_of)
        assert np.all(b.run(th, grad=False)["status"] == 0)
        for _ in range(WARM):
            cv = b.cvfold()
            b.loo_grad()
        assert np.all(cv["status"] == 0) and np.all(np.isfinite(cv["logp"]))
        c.reset_stats()
        b.run(th, grad=False)
        for _ in range(REPS):
            b.cvfold()
            b.loo_grad()
        out = {}
        for k in KERNELS:
            s = c.kernel_stats(k)
            n = max(s["launches"], 1)
            out[k] = (s["launches"], s["ms"] / n, s["bytes"] / n, s["flops"] / n)
        return out
    finally:
        b.close()
        c.close()


def refit_comparison(fold_of, lines):
    """One cvfold() call (F folds) against F refits without the fold, alternating, on one context."""
    X, Y, th = inputs()
    F = int(fold_of.max()) + 1
    sizes = np.bincount(fold_of, minlength=F)
    c = gprx.Context(0)
    full = gprx.GPBatch(B, D, N, 0, ctx=c)
    full.set_train(X, Y)
    full.set_folds(fold_of)
    full.run(th, grad=False)
    full.cvfold()
    red = {int(m): gprx.GPBatch(B, D, N - int(m), int(m), ctx=c) for m in np.unique(sizes)}
    try:
        for rep in range(2):
            t0 = time.perf_counter()
            full.run(th, grad=False)
            cv = full.cvfold()
            t_cv = time.perf_counter() - t0
            t0 = time.perf_counter()
            worst = 0.0
            for f in range(F):
                keep, V = fold_of != f, fold_of == f
                rb = red[int(sizes[f])]
                rb.set_train(X[:, keep], Y[:, keep])
                rb.set_test(X[:, V])
                rb.run(th, grad=False)
                mu, _ = rb.predict()
                worst = max(worst, float(np.max(np.abs(mu - cv["mu"][:, V]))))
            t_re = time.perf_counter() - t0
            lines.append(f"  refit comparison, pass {rep}: run + cvfold() {t_cv * 1e3:.1f} ms; {F} refits (set_train, run, predict) "
                         f"{t_re * 1e3:.1f} ms; ratio {t_re / t_cv:.1f}; largest |mu_refit - mu_cvfold| {worst:.2e}")
    finally:
        full.close()
        for rb in red.values():
            rb.close()
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-refit", action="store_true")
    a = ap.parse_args()
    i = np.arange(N)
    lines = [f"python scratch/cvfold_kernel_stats.py: profiling on, gprx_ctx_kernel_stats; P2 bench shape B={B} d={D} N={N}; per "
             f"layout {RUNS} runs, each {WARM} warm-up cvfold + loo_grad calls, then 1 evaluation + {REPS} calls of each; ms, "
             "algorithmic bytes and flops per launch"]
    for label, fo in (("(a) 98 trajectory folds of <= 21 points", (i // 21).astype(np.int32)),
                      ("(b) 8 folds of 256 points", (i // 256).astype(np.int32))):
        runs = [one_run(fo) for _ in range(RUNS)]
        lines.append(label)
        for k in KERNELS:
            ms = [r[k][1] for r in runs]
            by, fl = runs[0][k][2], runs[0][k][3]
            med = float(np.median(ms))
            lines.append(f"  {k:9s} launches/run {runs[0][k][0]:3d}  ms/launch runs " + " ".join(f"{v:.4f}" for v in ms)
                         + f"  median {med:.4f}  {by / med / 1e9:.3f} TB/s  {fl / med / 1e9:.2f} TF/s")
    if not a.no_refit:
        refit_comparison((i // 21).astype(np.int32), lines)
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(txt + "\n")


if __name__ == "__main__":
    main()
