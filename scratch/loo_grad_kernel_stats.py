"""loo_kinv / loo_beta / loo_grad / loo_grad_final from gprx_ctx_kernel_stats (profiling on) at the bench
shape (P2, B = 240, N = 2048) and at CP B = 1014, N = 512, next to the same run's lauum_grad (the same
MFMA core over N^3/3 flops: the yardstick) and loo_diag.  RUNS runs per shape, each a fresh context and
batch: one evaluation with gradient, WARM loo_grad calls, stats reset, one evaluation with gradient and
REPS loo_grad calls.  Prints one line per kernel, then the MFMA rates; `--out FILE` also writes the text
there (profiles/loo_grad_kernel_stats.txt).  TF/s counts the GEMM flops only: N^3/3 for loo_kinv and
lauum_grad, N^3 for loo_grad (N = Npad).

    python scratch/loo_grad_kernel_stats.py [--out FILE]
"""
import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1] / "gpr.jl_amd"))
import gprx  # noqa: E402

RUNS, WARM, REPS = 3, 3, 10
KERNELS = ("loo_diag", "loo_kinv", "loo_beta", "loo_grad", "loo_grad_final", "lauum_grad")
GEMM = {"loo_kinv": 1.0 / 3.0, "loo_grad": 1.0, "lauum_grad": 1.0 / 3.0}  # flops / Npad^3 per slot


def one_run(B, d, N):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((d, N))
    Y = np.sin(X.sum(axis=0))[None, :] + 0.05 * rng.standard_normal((B, N))
    th = np.concatenate([[-2.0], np.log(np.full(d, 1.5 * np.sqrt(d))), [0.1]])
    c = gprx.Context(0)
    c.set_profiling(True)
    b = gprx.GPBatch(B, d, N, 0, ctx=c)
    try:
        b.set_train(X, Y)
        assert np.all(b.run(th, grad=True)["status"] == 0)
        for _ in range(WARM):
            lg = b.loo_grad()
        assert np.all(np.isfinite(lg["grad"]))
        c.reset_stats()
        b.run(th, grad=True)
        for _ in range(REPS):
            b.loo_grad()
        out = {}
        for k in KERNELS:
            s = c.kernel_stats(k)
            out[k] = (s["launches"], s["ms"] / max(s["launches"], 1))
        return out
    finally:
        b.close()
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"python scratch/loo_grad_kernel_stats.py: profiling on, gprx_ctx_kernel_stats; per shape {RUNS} runs, each {WARM} "
             f"warm-up loo_grad calls, then 1 evaluation with gradient + {REPS} loo_grad calls; ms per launch, "
             "TF/s = B Npad^3 (1/3 | 1) flops / time"]
    for label, B, d, N in (("P2 bench shape", 240, 26, 2048), ("CP", 1014, 26, 512)):
        runs = [one_run(B, d, N) for _ in range(RUNS)]
        Np = -(-N // 64) * 64
        lines.append(f"{label}: B={B} d={d} N={N}")
        for k in KERNELS:
            ms = [r[k][1] for r in runs]
            med = float(np.median(ms))
            rate = f"  {B * GEMM[k] * Np ** 3 / med / 1e9:.2f} TF/s" if k in GEMM else ""
            lines.append(f"  {k:14s} launches/run {runs[0][k][0]:3d}  ms/launch runs " + " ".join(f"{v:.4f}" for v in ms)
                         + f"  median {med:.4f}{rate}")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(txt + "\n")


if __name__ == "__main__":
    main()
