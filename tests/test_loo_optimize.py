"""The leave-one-out objective inside the device optimiser: GPBatch.optimize(objective="loo")
(gprx_batch_optimize_obj with GPRX_OBJ_LOO: k_lbfgs fed by the six leave-one-out launches, finished
slots masked out of every round) against optim.optimize_batch(objective="loo"), the host restatement
that evaluates every slot in every round, against the independent LBFGS oracle, and against
single-slot runs.  Every comparison is bitwise: both sides consume the same device evaluations."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gprx():
    import gprx as g

    return g


@pytest.fixture(scope="module")
def ctx(gprx):
    c = gprx.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


def compare_opt(dev, host):
    """Minimisers and minima bit for bit; iterations, f/g calls, stop reason and convergence flag equal
    (test_gpu.py's _compare_opt, restated)."""
    assert len(dev) == len(host)
    for s, (r, h) in enumerate(zip(dev, host)):
        assert (r.iterations, r.f_calls, r.g_calls, r.stopped_by, r.converged) == (
            h.iterations, h.f_calls, h.g_calls, h.stopped_by, h.converged), s
        np.testing.assert_array_equal(r.minimizer, h.minimizer)
        assert r.minimum == h.minimum or (math.isnan(r.minimum) and math.isnan(h.minimum)), s


def load(golden_dir, name):
    with np.load(golden_dir / f"{name}.npz") as z:
        return {k: z[k] for k in z.files}


def jittered(th, B, seed, amp=0.05):
    rng = np.random.default_rng(seed)
    return np.stack([th + amp * rng.standard_normal(th.shape[0]) for _ in range(B)])


# ---- 1. device equals host lock-step ------------------------------------------------------------
@pytest.mark.parametrize("name,max_evals", [("cp_n64", 20), ("p1_n50", 40), ("p2_n100", 30)])
def test_device_loo_optimize_matches_host_lockstep(gprx, ctx, golden_dir, name, max_evals):
    from gprx.optim import LBFGS, Options, optimize_batch

    z = load(golden_dir, name)
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = Y.shape[0]
    th0 = jittered(th, B, 7)
    opts = Options(max_evals=max_evals)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    host, hr = optimize_batch(b, th0, LBFGS(), opts, objective="loo")
    dev, dr = b.optimize(th0, LBFGS(), opts, objective="loo")
    compare_opt(dev, host)
    assert dr == hr
    b.close()


# ---- 2. production geometry, ragged, with traces -------------------------------------------------
def test_device_loo_optimize_production_geometry_ragged_traces(gprx, ctx):
    """CP, N = 130 (three tiles, the last partial), B = 33 (k_node8's batch size and small_n = 4; not a
    multiple of the trial's outputs), 12 evaluations, every fifth start far off: the slots finish in
    different rounds of the HOST trace (optimize_batch evaluates every slot in every round and knows no
    mask), and the device's masked rounds ask the same theta and get the same answers, bit for bit."""
    from gprx import data
    from gprx.optim import LBFGS, Options, compare_optimisers, optimize_batch

    B, N = 33, 130
    G = data.make_trial("CP", N, 0, seed=data.trial_seed("CP", 20))["Y"].shape[0]
    trs = [data.make_trial("CP", N, 0, seed=data.trial_seed("CP", 20 + t)) for t in range((B + G - 1) // G)]
    X = np.stack([trs[s // G]["X"] for s in range(B)])
    Y = np.stack([trs[s // G]["Y"][s % G] for s in range(B)])
    th = data.theta0("CP", 128)
    rng = np.random.default_rng(11)
    amp = np.where(np.arange(B) % 5 == 0, 0.6, 0.05)
    T = np.stack([th + amp[s] * rng.standard_normal(th.shape[0]) for s in range(B)])
    b = gprx.GPBatch(B, X.shape[1], N, 0, ctx=ctx)
    b.set_train(X, Y)
    o = Options(max_evals=12)
    htr = []
    host, hr = optimize_batch(b, T, LBFGS(), o, trace=htr, objective="loo")
    htr = np.stack(htr)
    hact = htr[:, :, 0] == 1.0
    last = [int(np.nonzero(hact[:, s])[0].max()) for s in range(B)]
    assert len(set(last)) >= 2, last  # judged from the host run alone: the batch is ragged
    dev, dr = b.optimize(T, LBFGS(), o, trace_rounds=160, objective="loo")
    dtr = b.last_opt_trace
    rep = compare_optimisers(dev, host, dtr, htr)
    assert rep["equal"], rep
    compare_opt(dev, host)
    assert dr == hr and dtr.shape == htr.shape
    np.testing.assert_array_equal(dtr[:, :, 0] == 1.0, hact)
    same_bits(dtr[hact], htr[hact])
    b.close()


# ---- 3. independent oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("name,limit", [("cp_n64", 20), ("p2_n100", 30), ("nonpd_p1", 80)])
def test_device_loo_optimize_matches_the_independent_oracle(gprx, ctx, golden_dir, name, limit):
    """k_lbfgs on the leave-one-out rows against oracle/lbfgs_oracle.py driven per slot by a batch of
    one (run(grad=False), then loo_grad(): the same kernels, the same bits).  nonpd_p1 at its failing
    start: slot 0 answers +Inf with a NaN gradient and takes the NaN-gradient stop, while its neighbour
    at log sigma_n = -2 runs on."""
    from gprx.optim import LBFGS, Options
    from oracle import lbfgs_oracle as LO

    z = load(golden_dir, name)
    X, Y, th = z["X"], z["Y"], z["theta"]
    if name == "nonpd_p1":
        good = th.copy()
        good[0] = -2.0
        B, th0 = 2, np.stack([th, good])
    else:
        B = min(Y.shape[0], 3)
        th0 = jittered(th, B, 11)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y[:B])
    dev, _ = b.optimize(th0, LBFGS(), Options(max_evals=limit), refit=False, objective="loo")
    b.close()
    for s in range(B):
        one = gprx.GPBatch(1, X.shape[0], X.shape[1], 0, ctx=ctx)
        one.set_train(X, Y[s:s + 1])

        def fg(h):
            if not np.all(np.isfinite(h)):
                return math.inf, np.full(h.shape[0], np.nan)
            if one.run(h[None], grad=False)["status"][0] != 0:
                return math.inf, np.full(h.shape[0], np.nan)
            lg = one.loo_grad()
            if lg["status"][0] != 0:
                return math.inf, np.full(h.shape[0], np.nan)
            return -float(lg["logp"][0]), -np.asarray(lg["grad"][0], dtype=np.float64)

        ref = LO.optimize(fg, th0[s], f_calls_limit=limit)
        one.close()
        np.testing.assert_array_equal(dev[s].minimizer, ref["minimizer"])
        assert dev[s].minimum == ref["minimum"] or (math.isnan(dev[s].minimum) and math.isnan(ref["minimum"]))
        assert (dev[s].iterations, dev[s].f_calls, dev[s].g_calls, dev[s].stopped_by, dev[s].converged) == (
            ref["iterations"], ref["f_calls"], ref["g_calls"], ref["stopped_by"], ref["converged"]), s
    if name == "nonpd_p1":
        assert dev[0].stopped_by == "nan_gradient" and not dev[0].converged
        assert dev[1].stopped_by != "nan_gradient" and dev[1].f_calls > dev[0].f_calls and math.isfinite(dev[1].minimum)


# ---- 4. ragged batch equals single-slot runs -----------------------------------------------------
def test_device_loo_optimize_ragged_batch_equals_single_slot_runs(gprx, ctx, golden_dir):
    from gprx.optim import LBFGS, Options

    z = load(golden_dir, "p2_n100")
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = Y.shape[0]
    th0 = jittered(th, B, 11, 0.2)
    opts = Options(iterations=60)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    dev, _ = b.optimize(th0, LBFGS(), opts, refit=False, objective="loo")
    assert len({r.f_calls for r in dev}) > 1  # ragged: the slots stop at different rounds
    one = gprx.GPBatch(1, X.shape[0], X.shape[1], 0, ctx=ctx)
    for s in range(B):
        one.set_train(X, Y[s:s + 1])
        (r1,), _ = one.optimize(th0[s:s + 1], LBFGS(), opts, refit=False, objective="loo")
        compare_opt([r1], [dev[s]])
    one.close()
    b.close()


# ---- 5. refit ------------------------------------------------------------------------------------
def test_device_loo_optimize_refit_leaves_the_batch_at_the_minimisers(gprx, ctx, golden_dir):
    from gprx.optim import LBFGS, Options

    z = load(golden_dir, "p2_n100")
    X, Y, th, Xs = z["X"], z["Y"], z["theta"], z["Xs"]
    B = Y.shape[0]
    th0 = jittered(th, B, 7)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], Xs.shape[1], ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    res, _ = b.optimize(th0, LBFGS(), Options(max_evals=15), objective="loo")
    thmin = np.stack([r.minimizer for r in res])
    assert np.all(np.isfinite(thmin))
    same_bits(-b.loo()["logp"], np.array([r.minimum for r in res]))
    got = dict(lg=b.loo_grad(), pred=b.predict(), alpha=b.alpha())
    r = b.run(thmin, grad=True, predict=True)
    assert np.all(r["status"] == 0)
    ref = dict(lg=b.loo_grad(), pred=b.predict(), alpha=b.alpha())
    for k in ("logp", "grad", "status"):
        same_bits(got["lg"][k], ref["lg"][k])
    same_bits(got["pred"][0], ref["pred"][0])
    same_bits(got["pred"][1], ref["pred"][1])
    same_bits(got["pred"][0], r["mu"])
    same_bits(got["alpha"], ref["alpha"])
    # without the refit the batch holds no factorisation
    b.optimize(th0, LBFGS(), Options(max_evals=15), refit=False, objective="loo")
    with pytest.raises(gprx.GPRXError) as e:
        b.loo()
    assert e.value.status == 5  # GPRX_NOT_READY
    b.close()


# ---- 6. nothing existing moved -------------------------------------------------------------------
def _raw_optimize(gprx, b, th0, opts, objective, trace_rounds, fill=None):
    """The C entry points themselves: gprx_batch_optimize (objective None) or gprx_batch_optimize_obj.
    Returns (rc, outputs, trace); fill: the sentinel the outputs start from."""
    from gprx import _lib as L
    from gprx.batch import opt_options
    from gprx.optim import LBFGS

    B, n = b.B, b.d + 2
    o = opt_options(LBFGS(), opts, True)
    th = np.full((B, n), np.nan if fill is None else fill)
    fmin = np.full(B, np.nan if fill is None else fill)
    its, fc, gc, stp = (np.full(B, -7, dtype=np.int32) for _ in range(4))
    rounds = C.c_int(-7)
    tr = np.full((trace_rounds, B, 2 * n + 2), -3.0)
    if trace_rounds:
        L.check(L.lib.gprx_batch_set_opt_trace(b.h, L.dptr(tr), trace_rounds, tr.size), b.ctx.h)
    try:
        outs = (L.dptr(th), L.dptr(fmin), L.iptr(its), L.iptr(fc), L.iptr(gc), L.iptr(stp), C.byref(rounds))
        if objective is None:
            rc = L.lib.gprx_batch_optimize(b.h, L.dptr(th0), C.byref(o), *outs)
        else:
            rc = L.lib.gprx_batch_optimize_obj(b.h, int(objective), L.dptr(th0), C.byref(o), *outs)
    finally:
        L.lib.gprx_batch_set_opt_trace(b.h, None, 0, 0)
    return rc, dict(theta=th, minimum=fmin, iterations=its, f_calls=fc, g_calls=gc, stopped=stp,
                    rounds=np.array([rounds.value])), tr


def test_obj_mll_is_gprx_batch_optimize_and_unknown_objectives_write_nothing(gprx, ctx, golden_dir):
    from gprx import _lib as L
    from gprx.optim import Options

    z = load(golden_dir, "p2_n100")
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = Y.shape[0]
    th0 = jittered(th, B, 7)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    opts = Options(max_evals=30)
    rc_a, a, tr_a = _raw_optimize(gprx, b, th0, opts, None, 64)
    rc_b, m, tr_b = _raw_optimize(gprx, b, th0, opts, L.OBJ_MLL, 64)
    assert rc_a == rc_b == L.OK and 0 < a["rounds"][0] <= 64
    for k in a:
        if a[k].dtype == np.float64:
            same_bits(a[k], m[k])
        else:
            np.testing.assert_array_equal(a[k], m[k])
    same_bits(tr_a, tr_b)
    assert np.all(tr_a[:a["rounds"][0], :, 0] != -3.0)  # the trace was written
    # an objective the library does not know: GPRX_INVALID_ARGUMENT, sentinels untouched
    rc, out, tr = _raw_optimize(gprx, b, th0, opts, 7, 4, fill=-5.0)
    assert rc == L.INVALID_ARGUMENT
    assert np.all(out["theta"] == -5.0) and np.all(out["minimum"] == -5.0) and out["rounds"][0] == -7
    for k in ("iterations", "f_calls", "g_calls", "stopped"):
        assert np.all(out[k] == -7), k
    assert np.all(tr == -3.0)
    b.close()


@pytest.mark.parametrize("refit", [False, True])
def test_the_mask_is_gone_after_a_ragged_loo_optimize(gprx, ctx, golden_dir, refit):
    """After a ragged leave-one-out optimisation (slots finished, and were masked, in different rounds)
    the public loo() and loo_grad() answer for every slot again: at another theta they equal a fresh
    batch's results bit for bit (a slot still masked would keep its stale rows)."""
    from gprx.optim import LBFGS, Options

    z = load(golden_dir, "p2_n100")
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = Y.shape[0]
    th0 = jittered(th, B, 11, 0.2)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    dev, _ = b.optimize(th0, LBFGS(), Options(iterations=60), refit=refit, objective="loo")
    assert len({r.f_calls for r in dev}) > 1
    th1 = jittered(th, B, 5, 0.1)
    assert np.all(b.run(th1, grad=False)["status"] == 0)
    got_l, got_g = b.loo(), b.loo_grad()
    fresh = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    fresh.set_train(X, Y)
    assert np.all(fresh.run(th1, grad=False)["status"] == 0)
    ref_l, ref_g = fresh.loo(), fresh.loo_grad()
    for k in ("mu", "var", "logp_i", "logp", "status"):
        same_bits(got_l[k], ref_l[k])
    for k in ("logp", "grad", "status"):
        same_bits(got_g[k], ref_g[k])
    fresh.close()
    b.close()


# ---- 7. time limit -------------------------------------------------------------------------------
def test_device_loo_optimize_time_limit_zero(gprx, ctx, golden_dir):
    from gprx.optim import LBFGS, Options

    z = load(golden_dir, "p2_n100")
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = Y.shape[0]
    th0 = jittered(th, B, 7)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    o = Options(time_limit=0.0)
    first, r1 = b.optimize(th0, LBFGS(), o, objective="loo")
    for s, r in enumerate(first):
        assert (r.stopped_by, r.iterations, r.converged) == ("time_limit", 1, False), (s, r)
    again, r2 = b.optimize(th0, LBFGS(), o, objective="loo")
    compare_opt(again, first)
    assert r1 == r2
    b.close()


# ---- 8. search -----------------------------------------------------------------------------------
def test_search_group_loo_on_the_device_equals_the_host_loop(gprx, ctx, monkeypatch):
    """run_search_group(objective="loo") through RankBatch.optimize's device call against the same group
    with RankBatch.optimize pointed at optimize_batch (what it called before): theta, minimum, status,
    f_calls and everything else the optimiser returns, bit for bit."""
    from gprx import search, shard
    from gprx.optim import optimize_batch

    exp, N, ids = "P2_MAX", 16, range(3)
    seen = {"device": [], "host": []}
    device_optimize = shard.RankBatch.optimize

    def recording(self, theta0, method=None, options=None, objective="mll"):
        out = device_optimize(self, theta0, method, options, objective=objective)
        seen["device"].append(out)
        return out

    def host_loop(self, theta0, method=None, options=None, objective="mll"):
        th0 = self._rows(theta0)
        res, rounds = optimize_batch(self.batch, th0, method, options, objective=objective)
        thmin = np.stack([r.minimizer for r in res])
        ok = np.all(np.isfinite(thmin), axis=1)
        r = self.batch.run(np.where(ok[:, None], thmin, th0), grad=False, predict=self.M > 0, variance=False)
        out = {"theta": thmin, "minimum": np.array([x.minimum for x in res]), "mll": r["mll"],
               "status": np.where(ok, r["status"], 2).astype(np.int32),
               "f_calls": np.array([x.f_calls for x in res], dtype=np.int32),
               "iterations": np.array([x.iterations for x in res], dtype=np.int32)}
        if r.get("mu") is not None:
            out["mu"] = r["mu"]
        out = {k: self._shape(v) for k, v in out.items()}
        out["rounds"] = rounds
        seen["host"].append(out)
        return out

    monkeypatch.setattr(shard.RankBatch, "optimize", recording)
    dev = search.run_search_group(exp, N, ids, ctx, 8, 5, 10, objective="loo")
    monkeypatch.setattr(shard.RankBatch, "optimize", host_loop)
    host = search.run_search_group(exp, N, ids, ctx, 8, 5, 10, objective="loo")
    assert len(seen["device"]) == len(seen["host"]) >= 1
    for d, h in zip(seen["device"], seen["host"]):
        assert set(d) == set(h)
        for k in d:
            if k == "rounds":
                assert d[k] == h[k]
            elif np.asarray(d[k]).dtype == np.float64:
                same_bits(d[k], h[k])
            else:
                np.testing.assert_array_equal(d[k], h[k])
    assert set(dev) == set(host)
    for k in sorted(set(dev) - {"t_opt", "t_eval"}):  # the wall times aside
        d, h = np.asarray(dev[k]), np.asarray(host[k])
        if d.dtype == np.float64:
            same_bits(d, h)
        else:
            np.testing.assert_array_equal(d, h)


# ---- the C host ------------------------------------------------------------------------------------
def test_c_host_loo_optimize_equals_the_python_mirror(gprx, ctx, tmp_path):
    """gprx_c_host's leave-one-out optimise (gprx_batch_optimize_obj from plain C) prints what the same
    call gives through GPBatch.optimize, bit for bit."""
    import pathlib
    import subprocess

    from gprx import data, dataset
    from gprx.optim import LBFGS, Options

    host = pathlib.Path(__file__).resolve().parents[1] / "gpr.jl_amd" / "lib" / "gprx_c_host"
    tr = data.make_trial("P2", 130, 4, seed=17)
    th = data.theta0("P2", 128)
    dataset.write_cstates(tmp_path / "t.cst", tr["X"], tr["Y"])
    th.astype("<f8").tofile(tmp_path / "theta.f64")
    np.ascontiguousarray(tr["Xs"].T).astype("<f8").tofile(tmp_path / "xs.f64")
    r = subprocess.run([str(host), str(tmp_path / "t.cst"), str(tmp_path / "theta.f64"), str(tmp_path / "xs.f64"), "4"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in r.stdout.splitlines() if ln.strip()}
    G = tr["Y"].shape[0]
    b = gprx.GPBatch(G, tr["d"], 130, 0, ctx=ctx)
    b.set_train(tr["X"], tr["Y"])
    res, _ = b.optimize(np.tile(th, (G, 1)), LBFGS(), Options(max_evals=15), objective="loo")
    same_bits(out["loo_min"], np.array([x.minimum for x in res]))
    np.testing.assert_array_equal(out["loo_evals"], [x.f_calls for x in res])
    same_bits(-b.loo()["logp"], out["loo_min"])
    b.close()
