"""Records tests/golden/node8_parent.npz: what one build of the library computes, with default
options, on the four batches of tests/test_gpu.py::test_node8_matches_recorded_results -- LML,
gradient, mean, variance, status and failing pivot of every slot, for that test to compare bit for bit.

Run once on an MI355X against the library to record (a variant build is selected with GPRX_LIB):

    GPRX_LIB=/path/to/libgprx.so python tests/golden/make_golden_node8.py [--out FILE]

The recorded build is commit 58cbc88, the last that also carried a 4-wave form of k_node8; the file
is the proof that its removal left k_node8 and everything around it bit-identical, and the anchor a
later change of the leaf re-records deliberately.

Cases (N, B, mechanism): every one takes the fused 8-tile node (B >= 32, N >= 512).  Slot 3 has a NaN
point 100 (fails in a top leaf at pivot 101), slot B - 2 a NaN point 300 (fails in a bottom leaf at
pivot 301).  N = 1024 and 2048 have nodes an ancestor's SYRK updated (read from S); N = 500 pads the
last tile.  Every slot has its own theta (theta0 + 0.05 N(0, 1)) and M = 40 test points.

Only the outputs are stored (the inputs are megabytes and come from gprx.data, numpy only), with a
SHA-256 of the bytes of X, Y, Xs and theta per case: a host on which the generator rounds differently
shows as other inputs, not as other results.
"""
from __future__ import annotations

import argparse
import hashlib
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parents[1]

CASES = [(512, 64, "CP"), (1024, 40, "P2"), (500, 36, "P2"), (2048, 32, "P2")]
OUTPUTS = ("mll", "grad", "mu", "var", "status", "info")
M = 40


def make_case(N: int, B: int, mech: str):
    """X (B, 26, N), Y (B, N), Xs (B, 26, M), theta (B, 28) of one case."""
    from gprx import data

    G = 26 if mech == "CP" else 6
    trs = [data.make_trial(mech, N, M, seed=data.trial_seed(mech, 60 + t)) for t in range(B // G + 1)]
    X = np.stack([trs[s // G]["X"] for s in range(B)])
    Y = np.stack([(trs[s // G]["Xcurr"] if mech == "CP" else trs[s // G]["Y"])[s % G] for s in range(B)])
    Xs = np.stack([trs[s // G]["Xs"] for s in range(B)])
    X[3][:, 100] = np.nan
    X[B - 2][:, 300] = np.nan
    rng = np.random.default_rng(N + B)
    th0 = data.theta0(mech, 512)
    T = np.stack([th0 + 0.05 * rng.standard_normal(th0.shape[0]) for _ in range(B)])
    return X, Y, Xs, T


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_case(gprx, ctx, X, Y, Xs, T, runs: int = 2) -> list:
    """The batch evaluated `runs` times (gradient and prediction); one result dict per run."""
    B, d, N = X.shape
    b = gprx.GPBatch(B, d, N, Xs.shape[2], ctx=ctx)
    try:
        b.set_train(X, Y)
        b.set_test(Xs)
        return [b.run(T, grad=True, predict=True) for _ in range(runs)]
    finally:
        b.close()


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def key(N: int, B: int, mech: str, name: str) -> str:
    return f"{mech}.n{N}.b{B}.{name}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(HERE / "node8_parent.npz"))
    args = ap.parse_args()
    for p in (REPO, REPO / "gpr.jl_amd"):
        sys.path.insert(0, str(p))
    import gprx

    g = {}
    ctx = gprx.Context(0)
    for N, B, mech in CASES:
        X, Y, Xs, T = make_case(N, B, mech)
        r1, r2 = run_case(gprx, ctx, X, Y, Xs, T)
        for name in OUTPUTS:  # a reference is reproducible, and fails where the case says
            if not same_bits(r1[name], r2[name]):
                sys.exit(f"NOT REPRODUCIBLE: {key(N, B, mech, name)}")
            g[key(N, B, mech, name)] = np.asarray(r1[name])
        bad = np.nonzero(r1["status"])[0].tolist()
        if bad != [3, B - 2] or r1["info"][[3, B - 2]].tolist() != [101, 301]:
            sys.exit(f"NOT THE EXPECTED FAILURES: {(N, B, mech)} {bad} {r1['info'][bad]}")
        g[key(N, B, mech, "sha256")] = np.array(digest(X, Y, Xs, T))
        print((N, B, mech), g[key(N, B, mech, "sha256")], "mll[0]", float(r1["mll"][0]).hex())
    ctx.close()
    np.savez_compressed(args.out, **g)
    print("wrote", args.out, pathlib.Path(args.out).stat().st_size, "bytes,", len(g), "arrays")


if __name__ == "__main__":
    main()
