"""Recorded rollouts: per-step times at the largest shapes (for the steps_per_launch default) and the
overhead against the one-launch entry points at the sweep's rollout shape.  Device-event kernel times
(gprx_ctx_kernel_stats), warmed up, alternating forms, 5 repeats; prints one line per shape and writes the
JSON to the path given as the first argument (default profiles/rollout_rec.json)."""
import json
import pathlib
import sys
import time

import numpy as np

REPO = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "gpr.jl_amd")]
import gprx  # noqa: E402
from gprx import data, mdynamics  # noqa: E402
from gprx.projection import predictdynamics, predictdynamics_md, predictdynamics_md_rec, predictdynamics_rec  # noqa: E402
from gprx.rollout import rollout_min, rollout_min_md, rollout_min_md_rec, rollout_min_rec  # noqa: E402

ctx = gprx.Context(0)
ctx.set_profiling(True)
OUT = {}
REP = 5


def stat(name, f):
    ctx.reset_stats()
    t0 = time.perf_counter()
    f()
    wall = time.perf_counter() - t0
    k = ctx.kernel_stats(name)
    return k["ms"], k["launches"], wall * 1e3


def fit(mech, form, N, T, md):
    seed = data.trial_seed(mech, 7 if (mech == "FB" and form == "max") else 5)
    if form == "max":
        tr = data.make_trial(mech, N, T, seed=seed)
        th, start = data.theta0(mech, N), tr["Xs"].T.copy()
        mu = mdynamics.mean_max(mech, tr["X"], ctx=ctx) if md else 0.0
    else:
        us = form == "min_sin"
        tr = data.make_trial_min(mech, N, T, seed=seed, usesin=us)
        th, start = data.theta0_min(mech, N, us), tr["start"].copy()
        mu = mdynamics.mean_min(mech, tr["X"], us, ctx=ctx) if md else 0.0
    Y = tr["Y"] - mu
    G = Y.shape[0]
    b = gprx.GPBatch(G, tr["X"].shape[0], N, 0, ctx=ctx)
    b.set_train(tr["X"], Y)
    assert np.all(b.run(np.tile(th, (G, 1)), grad=False)["status"] == 0)
    return b, [[(b, g) for g in range(G)]], start


def forms(mech, form, md, groups, start, steps):
    """{label: (stat name, callable)}: one launch; recorded with every index, one launch; recorded R = 0."""
    none = np.empty(0, dtype=np.int32)
    if form == "max":
        vwi = data.VW_INDICES[mech]
        one, rec = (predictdynamics_md, predictdynamics_md_rec) if md else (predictdynamics, predictdynamics_rec)
        n1, n2 = ("rollout_max_md", "rollout_max_md_rec") if md else ("rollout_max", "rollout_max_rec")
        return {"one": (n1, lambda: one(mech, groups, start, steps, vwi, ctx=ctx)),
                "rec_all": (n2, lambda: rec(mech, groups, start, steps, vwi, None, steps_per_launch=steps, ctx=ctx)),
                "rec_none": (n2, lambda: rec(mech, groups, start, steps, vwi, none, steps_per_launch=steps, ctx=ctx)),
                "rec_all_spl1": (n2, lambda: rec(mech, groups, start, steps, vwi, None, steps_per_launch=1, ctx=ctx))}
    us = form == "min_sin"
    one, rec = (rollout_min_md, rollout_min_md_rec) if md else (rollout_min, rollout_min_rec)
    n1, n2 = ("rollout_min_md", "rollout_min_md_rec") if md else ("rollout", "rollout_rec")
    return {"one": (n1, lambda: one(mech, groups, start, steps, us, ctx=ctx)),
            "rec_all": (n2, lambda: rec(mech, groups, start, steps, None, us, steps_per_launch=steps, ctx=ctx)),
            "rec_none": (n2, lambda: rec(mech, groups, start, steps, none, us, steps_per_launch=steps, ctx=ctx)),
            "rec_all_spl1": (n2, lambda: rec(mech, groups, start, steps, None, us, steps_per_launch=1, ctx=ctx))}


def measure(tag, mech, form, md, N, T, steps):
    b, groups, start = fit(mech, form, N, T, md)
    fs = forms(mech, form, md, groups, start, steps)
    for _, f in fs.values():
        f()  # warm up
    ms = {k: [] for k in fs}
    wall = {k: [] for k in fs}
    for _ in range(REP):
        for k, (name, f) in fs.items():
            m, n, w = stat(name, f)
            ms[k].append(m)
            wall[k].append(w)
    b.close()
    r = {k: dict(kernel_ms_min=min(v), kernel_ms_med=float(np.median(v)), kernel_ms_max=max(v), wall_ms_med=float(np.median(wall[k])),
                 per_step_ms=float(np.median(v)) / steps) for k, v in ms.items()}
    OUT[tag] = dict(mech=mech, form=form, md=md, N=N, T=T, steps=steps, **r)
    print(tag, json.dumps(OUT[tag]), flush=True)


# ---- the per-step times behind the default: the largest shapes
for T in (100, 3200):
    measure(f"big.max_md.T{T}", "FB", "max", True, 512, T, 20)
    measure(f"big.max.T{T}", "FB", "max", False, 512, T, 20)
    measure(f"big.min_md.T{T}", "FB", "min_sin", True, 512, T, 20)
    measure(f"big.min.T{T}", "FB", "min_sin", False, 512, T, 20)
# ---- overhead at the sweep's rollout shape: T = 100, 20 steps, N = 512, each mechanism's G
for mech in ("P1", "P2", "CP"):
    for md in (False, True):
        measure(f"sweep.max{'_md' if md else ''}.{mech}", mech, "max", md, 512, 100, 20)
        measure(f"sweep.min{'_md' if md else ''}.{mech}", mech, "min_sin", md, 512, 100, 20)
ctx.close()
pathlib.Path(sys.argv[1] if len(sys.argv) > 1 else REPO / "profiles" / "rollout_rec.json").write_text(json.dumps(OUT, indent=1))
