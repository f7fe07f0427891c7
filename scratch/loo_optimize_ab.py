"""A/B of the leave-one-out optimiser: the parent's host loop (optim.optimize_batch(objective="loo"),
every slot evaluated in every round) against the device call (GPBatch.optimize(objective="loo"), finished
slots masked), on identical inputs, alternating on one card; and bench.py from both trees, alternating,
with its dumped outputs compared bit for bit.

    python scratch/loo_optimize_ab.py --parent DIR [--out profiles/loo_optimize_ab.txt] [--reps 3]

DIR: a checkout of the parent commit with its library built (make -C DIR/gpr.jl_amd).  Every
measurement runs in a fresh child process that imports gprx from one of the two trees; a child warms
its shapes up with one untimed call, then times `--calls` calls, each ending in the library's own
stream synchronisation.  Cases:
  bench   the bench's optimiser-leg shape: P2, N = 2048, d = 26, B = 48, max_evals = 30, the start jitter
          of test_device_optimize_bench_shape_bit_identical
  search  one CP search group: search.run_search_group("CP_MAX", 512, range(39), objective="loo")
The masked-work ratio (sum over rounds of active slots / (B x rounds)) comes from the host loop's trace."""
import argparse
import hashlib
import json
import os
import pathlib
import subprocess
import sys
import time

HERE = pathlib.Path(__file__).resolve().parents[1]


def child(case: str, side: str, calls: int):
    import numpy as np

    import gprx
    from gprx import data, optim, search
    from gprx.optim import LBFGS, Options

    ctx = gprx.Context(0)
    out = {"case": case, "side": side, "tree": str(pathlib.Path(gprx.__file__).resolve().parents[2])}
    digest = hashlib.sha256()
    if case == "bench":
        B, N = 48, 2048
        trs = [data.make_trial("P2", N, 0, seed=data.trial_seed("P2", 20 + t)) for t in range(B // 6)]
        X = np.stack([trs[s // 6]["X"] for s in range(B)])
        Y = np.stack([trs[s // 6]["Y"][s % 6] for s in range(B)])
        th0 = data.theta0("P2", 2048)
        rng = np.random.default_rng(11)
        amp = np.where(np.arange(B) % 5 == 0, 0.6, 0.05)
        T = np.stack([th0 + amp[s] * rng.standard_normal(th0.shape[0]) for s in range(B)])
        b = gprx.GPBatch(B, 26, N, 0, ctx=ctx)
        b.set_train(X, Y)
        o = Options(max_evals=30)

        def call(opts, trace=None):
            if side == "host":
                return optim.optimize_batch(b, T, LBFGS(), opts, trace=trace, objective="loo")
            return b.optimize(T, LBFGS(), opts, refit=False, objective="loo")

        call(Options(max_evals=2))  # warm-up: code objects, graphs, scratch
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            res, rounds = call(o)
            ts.append(time.perf_counter() - t0)
        if side == "host":  # the activity pattern, from the host loop's own trace (untimed call)
            tr = []
            call(o, tr)
            act = np.stack(tr)[:, :, 0]
            out.update(active_slot_rounds=int(act.sum()), slot_rounds=int(act.size))
        for r in res:
            digest.update(np.asarray(r.minimizer, dtype=np.float64).tobytes())
            digest.update(np.float64(r.minimum).tobytes())
        out.update(seconds=ts, rounds=int(rounds), B=B, f_calls=int(sum(r.f_calls for r in res)))
    else:
        traces = []
        if side == "host":  # record the rounds' activity without touching the host loop
            inner = optim.optimize_batch

            def recording(batch, theta0, method=None, options=None, trace=None, objective="mll"):
                tr = []
                r = inner(batch, theta0, method, options, trace=tr, objective=objective)
                traces.append(np.stack(tr)[:, :, 0])
                return r

            optim.optimize_batch = recording

        def call(evals):
            return search.run_search_group("CP_MAX", 512, range(39), ctx, 8, 5, evals, objective="loo")

        call(2)
        traces.clear()
        ts, topt = [], []
        for _ in range(calls):
            t0 = time.perf_counter()
            r = call(30)
            ts.append(time.perf_counter() - t0)
            topt.append(float(r["t_opt"]))
        if traces:
            per = traces[:len(traces) // calls]  # the batches of one call
            out.update(active_slot_rounds=int(sum(a.sum() for a in per)), slot_rounds=int(sum(a.size for a in per)))
        for k in ("theta", "mll", "kstep_mse"):
            digest.update(np.ascontiguousarray(r[k], dtype=np.float64).tobytes())
        out.update(seconds=ts, seconds_optimise=topt, rounds=r["rounds"] if isinstance(r["rounds"], int) else list(r["rounds"]),
                   slots=int(r["slots"]), batches=int(r["batches"]))
    out["digest"] = digest.hexdigest()[:16]
    print("AB " + json.dumps(out), flush=True)
    ctx.close()


def run_child(tree: pathlib.Path, case: str, side: str, calls: int, limit: int):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tree), str(tree / "gpr.jl_amd")]))
    r = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), "--child", case, side, "--calls", str(calls)],
                       env=env, capture_output=True, text=True, timeout=limit, cwd=str(tree))
    if r.returncode != 0:
        raise SystemExit(f"{case}/{side} in {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("AB ")][-1][3:])


def run_bench(tree: pathlib.Path, dump: pathlib.Path, limit: int):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=limit, cwd=str(tree))
    if r.returncode != 0:
        raise SystemExit(f"bench.py in {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("CASE", "SIDE"))
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--parent", type=pathlib.Path)
    ap.add_argument("--out", type=pathlib.Path, default=HERE / "profiles" / "loo_optimize_ab.txt")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dumps", type=pathlib.Path, default=HERE / "bench_out")
    ap.add_argument("--skip-bench", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.calls)
    if a.parent is None:
        ap.error("--parent DIR is required")
    import numpy as np

    parent = a.parent.resolve()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")  # kept current: a cut run leaves what it measured

    say("Leave-one-out optimiser: parent's host loop (A) against the device call (B), alternating on one MI355X.")
    say("A = optim.optimize_batch(objective='loo') in the parent's tree; B = GPBatch.optimize(objective='loo') here.")
    say(f"Each entry: one fresh process, one warm-up call, {a.calls} timed calls (seconds, host clock; every call ends synchronised).")
    for case, what in (("bench", "P2, N = 2048, d = 26, B = 48, max_evals = 30 (refit left out on both sides)"),
                       ("search", "search.run_search_group('CP_MAX', 512, range(39), ctx, 8, 5, 30, objective='loo'): whole call / optimiser part")):
        say()
        say(f"== {case}: {what}")
        res = {"host": [], "device": []}
        for rep in range(a.reps):
            for side, tree in (("host", parent), ("device", HERE)):
                r = run_child(tree, case, side, a.calls, 900)
                res[side].append(r)
                extra = f"  optimise {' '.join(f'{t:.3f}' for t in r['seconds_optimise'])}" if "seconds_optimise" in r else ""
                say(f"  rep {rep} {'A host  ' if side == 'host' else 'B device'}  {' '.join(f'{t:.3f}' for t in r['seconds'])}{extra}"
                    f"  rounds {r['rounds']}  digest {r['digest']}")
        h, d = res["host"], res["device"]
        key = "seconds_optimise" if case == "search" else "seconds"
        th, td = np.array([r[key] for r in h]).ravel(), np.array([r[key] for r in d]).ravel()
        say(f"  A {key}: median {np.median(th):.3f}  min {th.min():.3f}  max {th.max():.3f}")
        say(f"  B {key}: median {np.median(td):.3f}  min {td.min():.3f}  max {td.max():.3f}   A/B of medians {np.median(th) / np.median(td):.2f}")
        say(f"  results identical (digest of the minimisers and minima / of theta, mll, kstep_mse): "
            f"{len({r['digest'] for r in h + d}) == 1}")
        say(f"  active slot-rounds {h[0]['active_slot_rounds']} of {h[0]['slot_rounds']} = B x rounds "
            f"(ratio {h[0]['active_slot_rounds'] / h[0]['slot_rounds']:.3f}, from the host trace)")
    if not a.skip_bench:
        say()
        say("== bench.py --gpus 1 --steps 10 --warmup 3 --dump-outputs DIR, parent (A) and this tree (B), alternating")
        rows = {"A": [], "B": []}
        for rep in range(2):
            for tag, tree in (("A", parent), ("B", HERE)):
                j = run_bench(tree, a.dumps / f"{tag}{rep}", 900)
                rows[tag].append(j)
                say(f"  rep {rep} {tag}  ms_per_step {j['ms_per_step']}  fits/s {j['value']}  fit_ok {j['fit_ok']}")
        names = sorted(p.name for p in (a.dumps / "A0").glob("*.npy"))
        same = True
        for n in names:
            ref = np.load(a.dumps / "A0" / n)
            for tag, rep in (("A", 1), ("B", 0), ("B", 1)):
                got = np.load(a.dumps / f"{tag}{rep}" / n)
                eq = got.shape == ref.shape and np.array_equal(got.view(np.uint64), ref.view(np.uint64))
                same = same and eq
                if not eq:
                    say(f"  DIFFERENT: {n} of {tag}{rep}")
        say(f"  dumped arrays ({', '.join(names)}) bitwise equal across A0, A1, B0, B1: {same}")


if __name__ == "__main__":
    main()
