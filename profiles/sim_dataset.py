"""Measures gprx_simulate on the reference's dataset workload (dataset simulation)
and prints what profiles/sim_dataset.txt holds:

    python profiles/sim_dataset.py [MECH ...] > profiles/sim_dataset.txt

Per mechanism: one pass over a dataset's 200 trajectories x 19 999 steps at dtsim = 1e-4 with the dataset's
own dm, dJ and friction (statuses, how many trajectories are still running along the way), the whole
generate_dataset call, and for P2 and FB the same 2000 steps with nominal bodies by gprx_simulate and by a
host loop over gprx_vi_step (the route that existed before), and one launch of the default length.
"""
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "gpr.jl_amd")]
import numpy as np  # noqa: E402

import gprx  # noqa: E402
from gprx import projection, simdata, vi  # noqa: E402


def say(*a):
    print(*a, flush=True)


def main(mechs):
    ctx = gprx.Context(0)
    cfg = simdata.default_config()
    say("# one MI355X; dtsim 1e-4, eps 1e-10, newton_iter 100, steps_per_launch default; wall seconds of whole calls")
    say("# statuses: trajectories ending with status 0 / 1 / 2 (OR over their steps; 1: newton!'s test not met, 2: failed)")
    for mech in mechs:
        reg = simdata.regularizer(mech, cfg)
        rng = np.random.default_rng(0)
        par = simdata.draw_parameters(mech, cfg, rng)
        kinds = ["exp1"] * 50 + ["exp2"] * 50 + ["exptest"] * 100
        S = np.concatenate([simdata.initial_cstate(mech, simdata.draw_start(mech, k, rng)) for k in kinds])
        m, J = vi.body_params(mech, par["dm"], par["dJ"])
        c = vi.friction_damp(mech, par["friction"])
        rec = [1, 2001, 5001, 10001, 15001, 20000]
        projection.simulate(mech, S, 16, [17], m, J, c, regularizer=reg, dt=1e-4, ctx=ctx)  # warm
        t0 = time.perf_counter()
        o, st = projection.simulate(mech, S, 19999, rec, m, J, c, regularizer=reg, dt=1e-4, ctx=ctx)
        t = time.perf_counter() - t0
        alive = [int(np.sum(np.all(np.isfinite(o[:, r]), axis=1))) for r in range(len(rec))]
        say(f"{mech} one pass, 200 trajectories x 19 999 steps, regularizer {reg:g}: {t:.1f} s = {200 * 19999 / t:.3g} steps/s; "
            f"statuses {np.bincount(st, minlength=3).tolist()}; running at indices {rec}: {alive}")
        t0 = time.perf_counter()
        try:
            if mech == "FB":
                raise RuntimeError("not run: generate_dataset refuses the four-bar")
            ds = simdata.generate_dataset(mech, 0, cfg, ctx=ctx)
            fin = bool(all(np.all(np.isfinite(ds[k])) for k in ("train_old", "train_curr", "test_old", "test_future")))
            say(f"{mech} generate_dataset: {time.perf_counter() - t0:.1f} s; rows {ds['train_old'].shape[0]} + {ds['test_old'].shape[0]}, "
                f"all finite: {fin}")
        except RuntimeError as e:
            say(f"{mech} generate_dataset: RuntimeError after {time.perf_counter() - t0:.1f} s: {e}")
        if mech not in ("P2", "FB"):
            continue
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            projection.simulate(mech, S, 16, [17], regularizer=reg, dt=1e-4, ctx=ctx)
            ts.append(time.perf_counter() - t0)
        say(f"{mech} one launch, 16 steps x 200 trajectories: {min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f} ms (call wall time, 3 runs)")
        t0 = time.perf_counter()
        o, st = projection.simulate(mech, S, 2000, [2001], regularizer=reg, dt=1e-4, ctx=ctx)
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        cur, flags = S, np.zeros(len(S), dtype=np.int32)
        for _ in range(2000):
            cur, _, s1 = projection.vi_step(mech, cur, regularizer=reg, dt=1e-4, ctx=ctx)
            flags |= s1
        t_step = time.perf_counter() - t0
        both = np.all(np.isfinite(cur), axis=1) & np.all(np.isfinite(o[:, 0]), axis=1)
        say(f"{mech} 200 trajectories x 2000 steps, nominal bodies: gprx_simulate {t_dev:.2f} s, statuses {np.bincount(st, minlength=3).tolist()}; "
            f"host loop over gprx_vi_step {t_step:.2f} s ({t_step / t_dev:.2f}x), failed {int(np.sum((flags & 2) != 0))}; "
            f"finite in both {int(both.sum())}, same failures {bool(np.array_equal((flags & 2) != 0, st == 2))}, "
            f"largest |difference| over them {float(np.max(np.abs(cur[both] - o[both, 0]))) if both.any() else float('nan'):.2e}")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:] or ["P1", "P2", "CP", "FB"])
