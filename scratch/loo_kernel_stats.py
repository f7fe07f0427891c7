"""loo_diag / loo_final from gprx_ctx_kernel_stats (profiling on) at the bench shape (P2, B = 240,
N = 2048) and at CP B = 1014, N = 512, next to the same context's alpha and pred_final entries.
RUNS runs per shape, each a fresh context and batch: one evaluation, WARM leave-one-out calls, stats
reset, one evaluation and REPS leave-one-out calls.  Prints one line per kernel and run, then the
median run; `--out FILE` also writes the text there (profiles/loo_kernel_stats.txt).

    python scratch/loo_kernel_stats.py [--out FILE]
"""
import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1] / "gpr.jl_amd"))
import gprx  # noqa: E402

RUNS, WARM, REPS = 3, 5, 30
KERNELS = ("loo_diag", "loo_final", "alpha", "pred_final")


def one_run(B, d, N, M):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((d, N))
    Y = np.sin(X.sum(axis=0))[None, :] + 0.05 * rng.standard_normal((B, N))
    th = np.concatenate([[-2.0], np.log(np.full(d, 1.5 * np.sqrt(d))), [0.1]])
    c = gprx.Context(0)
    c.set_profiling(True)
    b = gprx.GPBatch(B, d, N, M, ctx=c)
    try:
        b.set_train(X, Y)
        b.set_test(rng.standard_normal((d, M)))
        assert np.all(b.run(th, grad=True, predict=True)["status"] == 0)
        for _ in range(WARM):
            lo = b.loo()
        assert np.all(np.isfinite(lo["logp"]))
        c.reset_stats()
        b.run(th, grad=True, predict=True)
        for _ in range(REPS):
            b.loo()
        out = {}
        for k in KERNELS:
            s = c.kernel_stats(k)
            n = max(s["launches"], 1)
            out[k] = (s["launches"], s["ms"] / n, s["bytes"] / n)
        return out
    finally:
        b.close()
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"python scratch/loo_kernel_stats.py: profiling on, gprx_ctx_kernel_stats; per shape {RUNS} runs, each {WARM} warm-up "
             f"loo calls, then 1 evaluation + {REPS} loo calls; ms and bytes per launch, TB/s = algorithmic bytes / time"]
    for label, B, d, N, M in (("P2 bench shape", 240, 26, 2048, 100), ("CP", 1014, 26, 512, 100)):
        runs = [one_run(B, d, N, M) for _ in range(RUNS)]
        lines.append(f"{label}: B={B} d={d} N={N} M={M}")
        for k in KERNELS:
            ms = [r[k][1] for r in runs]
            by = runs[0][k][2]
            med = float(np.median(ms))
            lines.append(f"  {k:10s} launches/run {runs[0][k][0]:3d}  ms/launch runs " + " ".join(f"{v:.4f}" for v in ms)
                         + f"  median {med:.4f}  bytes/launch {by:.4e}  {by / med / 1e9:.3f} TB/s")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(txt + "\n")


if __name__ == "__main__":
    main()
