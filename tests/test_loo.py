"""gprx_batch_loo on the device against the high-precision truth of tests/golden/loo_*.npz
(tests/golden/make_golden_loo.py), in both distance modes, and its bitwise properties.

Bound, elementwise, for mu, var, logp_i and logp:  |device - truth| <= k max(E_q, eps A_q)  with the
fixture's k = 8, E_q (geometric mean over five fp64 CPU variants of their largest error, per theta and
mode) and A_q (the absolute sum of q's last reduction).  A fixture's slots are its (theta, target)
pairs, repeated up to the batch size; each (fixture, batch size, mode) runs on the device once and
the tests share the record.  The bound test prints `case mode quantity err E ratio`.
"""
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
EPS = 2.0 ** -52
QUANTITIES = ("mu", "var", "logp_i", "logp")
CASES = ("a_p2_1", "a_p2_5", "a_p2_64", "a_p2_65", "b_cp_130", "b_p1_130", "b_fb_130", "e_d1", "c_cp_320", "d_cp_500",
         "f_cp_520")  # g_nonpd_p1: test_failed_slot_reads_nan_and_leaves_its_neighbour
_FX, _DEV = {}, {}


def fixture(name):
    if name not in _FX:
        with np.load(GOLDEN / f"loo_{name}.npz") as z:
            fx = {k: z[k] for k in z.files}
        if "X" not in fx:  # inputs of the hp fixture of the same name
            with np.load(GOLDEN / f"hp_{name}.npz") as z:
                fx.update(X=z["X"], Y=z["Y"], thetas=z["thetas"])
        fx["thetas"] = fx["thetas"][fx["theta_index"]]
        _FX[name] = fx
    return _FX[name]


def _runs():
    out = []
    for n in CASES:
        with np.load(GOLDEN / f"loo_{n}.npz") as z:
            out += [(n, int(B)) for B in z["B"]]
    return out


RUNS = _runs()
RUN_IDS = [f"{n}-B{B}" if B else n for n, B in RUNS]


@pytest.fixture(scope="module")
def gprx():
    import gprx as g

    return g


@pytest.fixture(scope="module")
def ctx(gprx):
    c = gprx.Context(0)
    yield c
    c.close()


def slots_of(fx, B):
    pairs = [(t, g) for t in range(fx["thetas"].shape[0]) for g in range(fx["Y"].shape[0])]
    return [pairs[s % len(pairs)] for s in range(B or len(pairs))]


def make_batch(gprx, c, fx, slots, M_max=0):
    b = gprx.GPBatch(len(slots), fx["X"].shape[0], fx["X"].shape[1], M_max, ctx=c)
    b.set_train(fx["X"], np.stack([fx["Y"][g] for _, g in slots]))
    return b, np.stack([fx["thetas"][t] for t, _ in slots])


def evaluate(gprx, c, fx, B, mode):
    slots = slots_of(fx, B)
    c.set_dist_mode(mode)
    b = None
    try:
        b, th = make_batch(gprx, c, fx, slots)
        r = b.run(th, grad=False)
        rec = b.loo()
        again = b.loo()
        rec.update(run_status=r["status"].copy(), alpha=b.alpha(), again=again)
    finally:
        if b is not None:
            b.close()
        c.set_dist_mode(1)
    return rec


def device(gprx, ctx, name, B, mode):
    if (name, B, mode) not in _DEV:
        _DEV[name, B, mode] = evaluate(gprx, ctx, fixture(name), B, mode)
    return _DEV[name, B, mode]


def truth_and_floor(fx, q, t, g, mode):
    """mu's floor is eps |mu|, and the terms of its last subtraction only where E_mu = 0 (a_p2_1)."""
    if q == "var":
        return fx["var"][t], np.abs(fx["var"][t])
    if q == "logp":
        return fx["logp"][t, g], fx["A_logp"][t, g]
    if q == "mu" and not fx["E"][mode, t, 0] > 0:
        return fx["mu"][t, g], fx["A_mu"][t, g]
    return fx[q][t, g], np.abs(fx[q][t, g])


def worst_ratio(fx, dev_rows, q, qi, pairs, mode):
    """(largest |device - truth| / max(E_q, eps A_q), largest error, E_q) over the slots `pairs`."""
    worst = (-1.0, 0.0, 0.0)
    for row, (t, g) in zip(dev_rows, pairs):
        tr, A = truth_and_floor(fx, q, t, g, mode)
        err = np.abs(row - tr)
        E = float(fx["E"][mode, t, qi])
        den = np.maximum(E, EPS * A)
        ratio = float(np.max(np.divide(err, den, out=np.where(err > 0, np.inf, 0.0), where=den > 0)))
        worst = max(worst, (ratio, float(np.max(err)), E))
    return worst


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_device_within_variant_spread_of_truth(gprx, ctx, name, B, mode):
    fx = fixture(name)
    dev = device(gprx, ctx, name, B, mode)
    k = float(fx["k"])
    assert np.all(dev["run_status"] == 0) and np.all(dev["status"] == 0), dev["status"]
    misses = []
    for qi, q in enumerate(QUANTITIES):
        worst = worst_ratio(fx, dev[q], q, qi, slots_of(fx, B), mode)
        print(f"{name}{'-B%d' % B if B else ''} mode {mode} {q} err {worst[1]:.3e} E {worst[2]:.3e} ratio {worst[0]:.3f}")
        if not worst[0] <= k:
            misses.append(f"{q}: ratio {worst[0]:.3f} > {k}")
    assert not misses, misses


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_repeated_slots_and_calls_are_bit_identical(gprx, ctx, name, B, mode):
    fx = fixture(name)
    dev = device(gprx, ctx, name, B, mode)
    first = {}
    for s, pair in enumerate(slots_of(fx, B)):
        s0 = first.setdefault(pair, s)
        for q in QUANTITIES:
            np.testing.assert_array_equal(dev[q][s], dev[q][s0], err_msg=f"{q} slots {s0}, {s}")
    for q in QUANTITIES + ("status",):
        np.testing.assert_array_equal(dev[q], dev["again"][q], err_msg=f"{q}: second call")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_consistent_with_alpha(gprx, ctx, name, B, mode):
    """y - mu = alpha var, to 4 eps (|y| + |mu|)."""
    fx = fixture(name)
    dev = device(gprx, ctx, name, B, mode)
    for s, (t, g) in enumerate(slots_of(fx, B)):
        y = fx["Y"][g]
        assert np.all(np.abs((y - dev["mu"][s]) - dev["alpha"][s] * dev["var"][s]) <= 4 * EPS * (np.abs(y) + np.abs(dev["mu"][s])))


def test_slot_result_does_not_depend_on_the_batch(gprx, ctx):
    """The same geometry (small_n, leaf tiles pinned) at B = 3 and inside B = 32: slot results equal."""
    from gprx import _lib as L

    fx = fixture("c_cp_320")
    c = gprx.Context(0)
    try:
        c.set_option(L.OPT_LEAF_TILES, 1)
        c.set_option(L.OPT_SMALL_N, 4)
        got = {}
        for B in (3, 32):
            slots = slots_of(fx, B)
            b, th = make_batch(gprx, c, fx, slots)
            assert np.all(b.run(th, grad=False)["status"] == 0)
            got[B] = b.loo()
            b.close()
        for q in QUANTITIES:
            np.testing.assert_array_equal(got[3][q], got[32][q][:3], err_msg=q)
            np.testing.assert_array_equal(got[3][q][0], got[32][q][12], err_msg=q)  # the pairs repeat every 12 slots
    finally:
        c.close()


@pytest.mark.parametrize("name,B", [("d_cp_500", 32), ("f_cp_520", 0)])
def test_unchanged_by_graphs_and_interleaved_predictions(gprx, ctx, name, B):
    from gprx import _lib as L

    fx = fixture(name)
    dev = device(gprx, ctx, name, B, 1)
    c = gprx.Context(0)
    try:
        c.set_option(L.OPT_GRAPHS, 1)
        slots = slots_of(fx, B)
        b, th = make_batch(gprx, c, fx, slots, M_max=5)
        assert np.all(b.run(th, grad=False)["status"] == 0)
        a = b.loo()
        b.set_test(fx["X"][:, :5])
        b.predict()
        b.predict_cov()
        after = b.loo()
        b.close()
        for q in QUANTITIES:
            np.testing.assert_array_equal(a[q], dev[q], err_msg=f"{q}: graphs")
            np.testing.assert_array_equal(after[q], dev[q], err_msg=f"{q}: after predict / predict_cov")
    finally:
        c.close()


def test_not_ready_before_a_run(gprx, ctx):
    from gprx import _lib as L

    fx = fixture("a_p2_5")
    b, _ = make_batch(gprx, ctx, fx, slots_of(fx, 0))
    with pytest.raises(L.GPRXError) as e:
        b.loo()
    assert e.value.status == L.NOT_READY
    b.close()


def test_failed_slot_reads_nan_and_leaves_its_neighbour(gprx, ctx):
    """The failing slot of tests/test_gpu.py (nonpd_p1.npz): NaN rows and status 1 for it.  Its good
    neighbour (the same inputs at log sigma_n = -2, fixture g_nonpd_p1) lies within k max(E_q, eps A_q)
    of the truth and is bit-identical to a run in which both slots are good."""
    fx = fixture("g_nonpd_p1")
    z = np.load(GOLDEN / "nonpd_p1.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    good = fx["thetas"][0]
    np.testing.assert_array_equal(X, fx["X"])
    np.testing.assert_array_equal(Y, fx["Y"])
    assert good[0] == -2.0 and np.array_equal(good[1:], th[1:])
    b = gprx.GPBatch(2, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y[:2])
    r = b.run(np.stack([th, good]))
    assert r["status"][0] == 1 and r["status"][1] == 0
    lo = b.loo()
    assert list(lo["status"]) == [1, 0]
    for q in ("mu", "var", "logp_i"):
        assert np.all(np.isnan(lo[q][0])) and np.all(np.isfinite(lo[q][1]))
    assert np.isnan(lo["logp"][0]) and np.isfinite(lo["logp"][1])
    k, mode = float(fx["k"]), ctx.dist_mode
    for qi, q in enumerate(QUANTITIES):
        ratio, err, E = worst_ratio(fx, [lo[q][1]], q, qi, [(0, 1)], mode)
        print(f"g_nonpd_p1 neighbour mode {mode} {q} err {err:.3e} E {E:.3e} ratio {ratio:.3f}")
        assert ratio <= k, (q, ratio)
    b.run(np.stack([good, good]))
    both = b.loo()
    for q in QUANTITIES:
        np.testing.assert_array_equal(lo[q][1], both[q][1], err_msg=q)
    b.close()


def test_after_optimize_the_values_belong_to_the_minimiser(gprx, ctx):
    from gprx.optim import Options

    fx = fixture("a_p2_65")
    slots = slots_of(fx, 0)[:3]
    b, th = make_batch(gprx, ctx, fx, slots)
    res, _ = b.optimize(th, options=Options(iterations=3), refit=True)
    got = b.loo()
    assert np.all(got["status"] == 0)
    b.run(np.stack([r.minimizer for r in res]), grad=False)
    fresh = b.loo()
    for q in QUANTITIES:
        np.testing.assert_array_equal(got[q], fresh[q], err_msg=q)
    b.close()


def test_gpe_surface(gprx, ctx):
    """predict_LOO adds the prior mean at the training inputs back; logp_LOO is the batch's logp."""
    fx = fixture("a_p2_65")
    X, y, th = fx["X"], fx["Y"][0], fx["thetas"][0]
    mean = gprx.MeanFunction(lambda x: 0.25 + 0.5 * x[0])
    gp = gprx.GP(X, y, mean, gprx.SEArd(th[1:-1], th[-1]), th[0], ctx=ctx)
    mu, var = gprx.predict_LOO(gp)
    lo = gp._batch.loo()
    m = mean.mean(X)
    np.testing.assert_array_equal(mu, lo["mu"][0] + m)
    np.testing.assert_array_equal(var, lo["var"][0])
    assert gprx.logp_LOO(gp) == float(lo["logp"][0]) == gp.logp_LOO()
    # against the batch with the mean taken off by hand
    b = gprx.GPBatch(1, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, (y - m)[None, :])
    b.run(th[None, :], grad=False)
    np.testing.assert_array_equal(b.loo()["mu"][0], lo["mu"][0])
    b.close()


PARENT_KEYS = {"kstep_mse", "projectionerror", "failed", "mll", "theta", "status", "f_calls", "rounds", "t_opt", "t_eval",
               "slots", "batches", "params"}


def test_search_group_records_loo_logp(gprx, ctx):
    """run_search_group(loo=True): loo_logp (n_local, G), finite, equal to GPBatch.loo() on an
    independently built batch at the returned theta; with loo=False the keys are the parent's."""
    from gprx import search

    exp, N, ids = "P2_MAX", 16, range(3)
    r = search.run_search_group(exp, N, ids, ctx, 8, 5, 10, loo=True)
    off = search.run_search_group(exp, N, ids, ctx, 8, 5, 10)
    assert set(off) == PARENT_KEYS and set(r) == PARENT_KEYS | {"loo_logp"}
    for key in ("theta", "mll", "kstep_mse", "status", "f_calls"):
        np.testing.assert_array_equal(r[key], off[key], err_msg=key)
    trials = search.local_trials(exp, N, ids, 8)
    n, G = len(trials), trials[0]["Y"].shape[0]
    assert r["loo_logp"].shape == (n, G) and np.all(r["status"] == 0) and np.all(np.isfinite(r["loo_logp"]))
    b = gprx.GPBatch(n * G, trials[0]["X"].shape[0], N, 0, ctx=ctx)
    b.set_train(np.repeat(np.stack([t["X"] for t in trials]), G, axis=0), np.concatenate([t["Y"] for t in trials]))
    assert np.all(b.run(r["theta"].reshape(n * G, -1), grad=False)["status"] == 0)
    np.testing.assert_array_equal(b.loo()["logp"].reshape(n, G), r["loo_logp"])
    b.close()


def test_chunked_group_records_the_same_loo_logp(gprx, ctx):
    """Three device batches one after another (tests/test_sweep.py's forced budget): loo_logp is taken
    in every batch and equals the single batch's."""
    from gprx import shard, sweep

    mech, N, variant, n_tr, fit = "P2", 128, "min", 9, 4
    trials = sweep.local_trials(mech, N, variant, range(n_tr), 8, ctx)
    G, d = np.atleast_2d(trials[0]["Y"]).shape[0], trials[0]["X"].shape[0]
    one, two = shard.batch_bytes(1, d, N, 0), shard.batch_bytes(2, d, N, 0)
    budget = (2 * one - two) + fit * G * (two - one)
    kw = dict(testsamples=8, simsteps=5, max_evals=12, trials=trials, loo=True)
    single = sweep.run_group(mech, N, variant, range(n_tr), ctx, **kw)
    chunked = sweep.run_group(mech, N, variant, range(n_tr), ctx, budget=budget, **kw)
    assert chunked["batches"] >= 2 and single["batches"] == 1
    assert single["loo_logp"].shape == (n_tr, G) and np.any(np.isfinite(single["loo_logp"]))
    np.testing.assert_array_equal(chunked["loo_logp"], single["loo_logp"])
    np.testing.assert_array_equal(np.isfinite(single["loo_logp"]), single["status"] == 0)
