"""Records tests/golden/rollouts_parent.npz: the four device rollouts (gprx_rollout_min,
gprx_rollout_min_md, gprx_rollout_max, gprx_rollout_max_md) as one build of the library computes
them, with their inputs, for tests/test_rollout_recorded.py to compare bit for bit.

Run once on an MI355X against the library to record (a variant build is selected with GPRX_LIB):

    GPRX_LIB=/path/to/libgprx.so python tests/golden/make_golden_rollouts.py [--out FILE]

Cases: every mechanism, both distance modes, the minimal form with and without the (sin, cos)
features; T = 3 trajectories in two rollout groups (traj_group = [0, 1, 0]) over 3 steps, so the
two-deep reduction buffer of the minimal kernel is reused.  N = 48 (less than one 256-thread stride),
300 (a second stride partly filled; in the minimal kernel's 4 x 256 loop the masked points) and, for
the minimal form, 1100 (a second pass of that loop).

Inputs: the generator's trial 5 (the four-bar's maximal form: trial 7, as tests/test_md_rollout.py)
with X and Y rounded to multiples of 2^-9 and stored as int16 -- the rollouts need a well-conditioned
fit, not physical data, and the fixture stays small.  The training set of N points is the first N
columns of the largest one.  One batch holds both groups: the same X and Y, the second group at
theta + 0.05.  The MeanDynamics entry points run on the same factorisation (their GPs add the
physics mean to whatever the fit gives).  The starts are the trial's test states, unrounded.
"""
from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parents[1]

MECHS = ("P1", "P2", "CP", "FB")
FORMS = ("max", "min", "min_sin")
SIZES = {"max": (48, 300), "min": (48, 300, 1100), "min_sin": (48, 300, 1100)}
MAX_TRIAL = {"P1": 5, "P2": 5, "CP": 5, "FB": 7}
T, STEPS = 3, 3
TRAJ_GROUP = np.array([0, 1, 0], dtype=np.int32)
SCALE = 512.0  # X and Y are multiples of 1 / SCALE
CASES = [(mech, form, N) for form in FORMS for mech in MECHS for N in SIZES[form]]


def make_inputs() -> dict:
    """The fixture's input arrays, from gprx.data (numpy only)."""
    from gprx import data

    def q(a):
        r = np.round(a * SCALE)
        assert np.max(np.abs(r)) < 2 ** 15
        return r.astype(np.int16)

    g = {}
    for mech in MECHS:
        for form in FORMS:
            N = max(SIZES[form])
            if form == "max":
                tr = data.make_trial(mech, N, T, seed=data.trial_seed(mech, MAX_TRIAL[mech]))
                th, start = data.theta0(mech, 64), tr["Xs"].T.copy()
            else:
                usesin = form == "min_sin"
                tr = data.make_trial_min(mech, N, T, seed=data.trial_seed(mech, 5), usesin=usesin)
                th, start = data.theta0_min(mech, 64, usesin), tr["start"].copy()
            g[f"{form}.{mech}.X"] = q(tr["X"])
            g[f"{form}.{mech}.Y"] = q(tr["Y"])
            g[f"{form}.{mech}.theta"] = np.stack([th, th + 0.05])
            g[f"{form}.{mech}.start"] = start
    return g


def run_case(ctx, g, mech: str, form: str, N: int, mode: int) -> dict:
    """Fits the case's two groups on the device in distance mode `mode` and runs both entry points of
    its coordinate form.  Returns {"<entry>.<output>": array}."""
    import gprx
    from gprx import data
    from gprx.projection import predictdynamics, predictdynamics_md
    from gprx.rollout import rollout_min, rollout_min_md

    ctx.set_dist_mode(mode)
    X = g[f"{form}.{mech}.X"][:, :N] / SCALE
    Y = g[f"{form}.{mech}.Y"][:, :N] / SCALE
    theta, start = g[f"{form}.{mech}.theta"], g[f"{form}.{mech}.start"]
    G = Y.shape[0]
    b = gprx.GPBatch(2 * G, X.shape[0], N, 0, ctx=ctx)
    b.set_train(X, np.concatenate([Y, Y]))
    st = b.run(np.repeat(theta, G, axis=0), grad=False)["status"]
    assert np.all(st == 0), st
    groups = [[(b, k * G + j) for j in range(G)] for k in range(2)]
    kw = dict(traj_group=TRAJ_GROUP, ctx=ctx)
    if form == "max":
        vwi = data.VW_INDICES[mech]
        res = {"rollout_max": predictdynamics(mech, groups, start, STEPS, vwi, **kw),
               "rollout_max_md": predictdynamics_md(mech, groups, start, STEPS, vwi, **kw)}
        names = ("out", "perr", "status", "vi_status")
    else:
        usesin = form == "min_sin"
        res = {"rollout_min": (rollout_min(mech, groups, start, STEPS, usesin, **kw),),
               "rollout_min_md": rollout_min_md(mech, groups, start, STEPS, usesin, **kw)}
        names = ("out", "status", "vi_status")
    b.close()
    return {f"{entry}.{name}": a for entry, arrays in res.items() for name, a in zip(names, arrays)}


def key(mech: str, form: str, N: int, mode: int, name: str) -> str:
    return f"{form}.{mech}.n{N}.m{mode}.{name}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(HERE / "rollouts_parent.npz"))
    args = ap.parse_args()
    for p in (REPO, REPO / "gpr.jl_amd"):
        sys.path.insert(0, str(p))
    import gprx

    g = make_inputs()
    ctx = gprx.Context(0)
    bad = []  # a reference has clean results: all finite, nothing singular, no failed physics step
    for mech, form, N in CASES:
        for mode in (0, 1):
            for name, a in run_case(ctx, g, mech, form, N, mode).items():
                if (not np.all(np.isfinite(a)) or (name.endswith(".status") and np.any(a))
                        or (name.endswith("vi_status") and np.any(a & 2))):
                    bad.append((mech, form, N, mode, name, a))
                g[key(mech, form, N, mode, name)] = a
    ctx.close()
    for b in bad:
        print("NOT CLEAN:", *b)
    if bad:
        sys.exit(1)
    np.savez_compressed(args.out, **g)
    print("wrote", args.out, pathlib.Path(args.out).stat().st_size, "bytes,", len(g), "arrays")


if __name__ == "__main__":
    main()
