"""Kernel times of the joint-covariance path at the headline shape (P2, B = 240, N = 2048, d = 26,
M = 100) through the library's own profiling timers (HIP events around each launch):
pred_var (the existing per-point variance GEMM, the yardstick: the same N^2 M product in the same
run) against pred_whiten, pred_cov, cov_chol and cov_sample (S = 16 draws).  Two warm-up rounds,
then REPEATS rounds, each timed on its own; the median and the range per kernel.

    python scratch/pred_cov_perf.py [B] > profiles/pred_cov_perf.txt
"""
import pathlib
import statistics
import sys

REPO = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "gpr.jl_amd")]
import numpy as np  # noqa: E402

import gprx  # noqa: E402
from gprx import data  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 240
N, M, S, WARM, REPEATS = 2048, 100, 16, 2, 7
KERNELS = ["pred_cross", "pred_var", "pred_whiten", "pred_cov", "cov_chol", "cov_sample"]

trs = [data.make_trial("P2", N, M, seed=data.trial_seed("P2", t)) for t in range((B + 5) // 6)]
X = np.stack([trs[s // 6]["X"] for s in range(B)])
Y = np.stack([trs[s // 6]["Y"][s % 6] for s in range(B)])
Xs = np.stack([trs[s // 6]["Xs"] for s in range(B)])
th = np.tile(data.theta0("P2", N), (B, 1))
Z = np.random.default_rng(0).standard_normal((S, M))

ctx = gprx.Context(0)
b = gprx.GPBatch(B, 26, N, M, ctx=ctx)
b.set_train(X, Y)
b.set_test(Xs)
r = b.run(th, grad=False)
assert np.all(r["status"] == 0)
ctx.set_profiling(True)
rows = {k: [] for k in KERNELS}
for it in range(WARM + REPEATS):
    ctx.reset_stats()
    b.predict()            # pred_cross, pred_var, pred_final
    _, jit = b.sample(Z)   # pred_cross, pred_final, pred_whiten, pred_cov, cov_chol, cov_sample
    if it >= WARM:
        for k in KERNELS:
            st = ctx.kernel_stats(k)
            rows[k].append((st["ms"] / st["launches"], st["flops"] / st["launches"], st["bytes"] / st["launches"]))
print(f"P2 B={B} N={N} d=26 M={M} S={S}: per-launch kernel time, median of {REPEATS} (after {WARM} warm-up rounds)")
print(f"jitter: {int(np.sum(jit == 0))} slots at 0, max {np.max(jit):.3e}")
print(f"{'kernel':12s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'TFLOP/s':>8s} {'GB/s':>8s}")
for k in KERNELS:
    ms = [v[0] for v in rows[k]]
    med = statistics.median(ms)
    print(f"{k:12s} {med:10.3f} {min(ms):8.3f} {max(ms):8.3f} {rows[k][0][1] / med / 1e9:8.2f} {rows[k][0][2] / med / 1e6:8.1f}")
wv = statistics.median(v[0] for v in rows["pred_whiten"]) / statistics.median(v[0] for v in rows["pred_var"])
print(f"pred_whiten / pred_var = {wv:.2f}")
b.close()
ctx.close()
