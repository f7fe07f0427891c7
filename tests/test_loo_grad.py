"""gprx_batch_loo_grad on the device against the high-precision truth of tests/golden/loograd_*.npz
(tests/golden/make_golden_loo_grad.py), in both distance modes, and its bitwise properties.

Bound, for the gradient of logp_LOO with respect to theta = [log sn, log ell_1..d, log sf]:
    |device - truth| <= k      max(E,         eps A[p])   on the vector, and
    |device - truth| <= k_comp max(E_grad[p], eps A[p])   per component,
with the fixture's k = 8, k_comp, E / E_grad (geometric mean over five fp64 CPU variants of their largest
error, per theta and mode) and A[p] = sum_kl |dK_kl W'_kl|.  A fixture's slots are its (theta, target)
pairs, repeated up to the batch size; each (fixture, batch size, mode) runs on the device once and the
tests share the record.  The bound test prints `case mode quantity err E ratio`.
"""
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
EPS = 2.0 ** -52
CASES = ("a_p2_1", "a_p2_5", "a_p2_64", "a_p2_65", "b_cp_130", "b_p1_130", "b_fb_130", "e_d1", "c_cp_320", "d_cp_500",
         "f_cp_520")  # g_nonpd_p1: test_failed_slot_reads_nan_and_leaves_its_neighbour
_FX, _DEV = {}, {}


def fixture(name):
    if name not in _FX:
        with np.load(GOLDEN / f"loograd_{name}.npz") as z:
            fx = {k: z[k] for k in z.files}
        src = GOLDEN / (f"loo_{name}.npz" if name in ("f_cp_520", "g_nonpd_p1") else f"hp_{name}.npz")
        with np.load(src) as z:  # the inputs, by name
            fx.update(X=z["X"], Y=np.atleast_2d(z["Y"]), thetas=z["thetas"][fx["theta_index"]])
        _FX[name] = fx
    return _FX[name]


def _runs():
    out = []
    for n in CASES:
        with np.load(GOLDEN / f"loograd_{n}.npz") as z:
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
        rec = b.loo_grad()
        rec.update(run_status=r["status"].copy(), loo_logp=b.loo()["logp"], again=b.loo_grad())
    finally:
        if b is not None:
            b.close()
        c.set_dist_mode(1)
    return rec


def device(gprx, ctx, name, B, mode):
    if (name, B, mode) not in _DEV:
        _DEV[name, B, mode] = evaluate(gprx, ctx, fixture(name), B, mode)
    return _DEV[name, B, mode]


def _ratio(err, den):
    return float(np.max(np.divide(err, den, out=np.where(err > 0, np.inf, 0.0), where=den > 0)))


def worst_ratios(fx, rows, pairs, mode):
    """((ratio, err, E) on the vector, (ratio, err, E_grad[p]) per component), the largest over the slots."""
    wv, wc = (-1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)
    for row, (t, g) in zip(rows, pairs):
        tr, A = fx["grad"][t, g], fx["A_grad"][t, g]
        if mode == 0:  # expanded distances: a component whose truth is exactly 0 takes that form's operands
            A = np.where(tr == 0.0, fx["A_grad_exp"][t, g], A)
        err = np.abs(row - tr)
        E, Eg = float(fx["E"][mode, t]), fx["E_grad"][mode, t]
        wv = max(wv, (_ratio(err, np.maximum(E, EPS * A)), float(np.max(err)), E))
        den = np.maximum(Eg, EPS * A)
        p = int(np.argmax(np.divide(err, den, out=np.where(err > 0, np.inf, 0.0), where=den > 0)))
        wc = max(wc, (_ratio(err, den), float(err[p]), float(Eg[p])))
    return wv, wc


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_device_within_variant_spread_of_truth(gprx, ctx, name, B, mode):
    fx = fixture(name)
    dev = device(gprx, ctx, name, B, mode)
    k, kc = float(fx["k"]), float(fx["k_comp"])
    assert np.all(dev["run_status"] == 0) and np.all(dev["status"] == 0), dev["status"]
    wv, wc = worst_ratios(fx, dev["grad"], slots_of(fx, B), mode)
    tag = f"{name}{'-B%d' % B if B else ''} mode {mode}"
    print(f"{tag} grad err {wv[1]:.3e} E {wv[2]:.3e} ratio {wv[0]:.3f}")
    print(f"{tag} grad_component err {wc[1]:.3e} E {wc[2]:.3e} ratio {wc[0]:.3f}")
    assert wv[0] <= k, f"vector: ratio {wv[0]:.3f} > {k}"
    assert wc[0] <= kc, f"component: ratio {wc[0]:.3f} > {kc}"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_logp_is_loo_s_and_repeats_are_bit_identical(gprx, ctx, name, B, mode):
    fx = fixture(name)
    dev = device(gprx, ctx, name, B, mode)
    np.testing.assert_array_equal(dev["logp"], dev["loo_logp"], err_msg="logp against gprx_batch_loo")
    first = {}
    for s, pair in enumerate(slots_of(fx, B)):
        s0 = first.setdefault(pair, s)
        for q in ("logp", "grad"):
            np.testing.assert_array_equal(dev[q][s], dev[q][s0], err_msg=f"{q} slots {s0}, {s}")
    for q in ("logp", "grad", "status"):
        np.testing.assert_array_equal(dev[q], dev["again"][q], err_msg=f"{q}: second call")


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
            b, th = make_batch(gprx, c, fx, slots_of(fx, B))
            assert np.all(b.run(th, grad=False)["status"] == 0)
            got[B] = b.loo_grad()
            b.close()
        for q in ("logp", "grad"):
            np.testing.assert_array_equal(got[3][q], got[32][q][:3], err_msg=q)
            np.testing.assert_array_equal(got[3][q][0], got[32][q][12], err_msg=q)  # the pairs repeat every 12 slots
    finally:
        c.close()


@pytest.mark.parametrize("name,B", [("d_cp_500", 32), ("f_cp_520", 0)])
def test_unchanged_by_graphs_and_leaves_the_other_calls_alone(gprx, ctx, name, B):
    """With OPT_GRAPHS on the result keeps its bits; loo, predict, predict_cov and alpha return after
    loo_grad what they returned before it (Lw is nobody's input), and loo_grad after them its own bits."""
    from gprx import _lib as L

    fx = fixture(name)
    dev = device(gprx, ctx, name, B, 1)
    c = gprx.Context(0)
    try:
        c.set_option(L.OPT_GRAPHS, 1)
        b, th = make_batch(gprx, c, fx, slots_of(fx, B), M_max=5)
        assert np.all(b.run(th, grad=False)["status"] == 0)
        b.set_test(fx["X"][:, :5])

        def others():
            lo = b.loo()
            mu, var = b.predict()
            cmu, cov = b.predict_cov()
            return dict(alpha=b.alpha(), mu=mu, var=var, cmu=cmu, cov=cov, **{f"loo_{q}": lo[q] for q in ("mu", "var", "logp_i", "logp")})

        before = others()
        lg = b.loo_grad()
        after = others()
        again = b.loo_grad()
        b.close()
        for q in before:
            np.testing.assert_array_equal(after[q], before[q], err_msg=f"{q}: after loo_grad")
        for q in ("logp", "grad"):
            np.testing.assert_array_equal(lg[q], dev[q], err_msg=f"{q}: graphs")
            np.testing.assert_array_equal(again[q], dev[q], err_msg=f"{q}: after loo / predict / predict_cov / alpha")
    finally:
        c.close()


def test_constant_dimension_gets_zero_and_the_others_keep_their_bits(gprx, ctx):
    """CP's CStates hold constant coordinates: their gradient is exactly 0, and every other component
    equals the run with OPT_ACTIVE_DIMS = 0 (every dimension summed)."""
    from gprx import _lib as L

    fx = fixture("b_cp_130")
    const = np.all(fx["X"] == fx["X"][:, :1], axis=1)
    assert 0 < const.sum() < len(const)
    slots = slots_of(fx, 0)[:4]
    got = {}
    for on in (1, 0):
        c = gprx.Context(0)
        try:
            c.set_option(L.OPT_ACTIVE_DIMS, on)
            b, th = make_batch(gprx, c, fx, slots)
            assert np.all(b.run(th, grad=False)["status"] == 0)
            got[on] = b.loo_grad()
            b.close()
        finally:
            c.close()
    g = got[1]["grad"]
    assert np.all(g[:, 1:-1][:, const] == 0.0) and not np.any(np.signbit(g[:, 1:-1][:, const]))
    keep = np.r_[True, ~const, True]
    np.testing.assert_array_equal(g[:, keep], got[0]["grad"][:, keep])
    np.testing.assert_array_equal(got[1]["logp"], got[0]["logp"])


def test_not_ready_before_a_run(gprx, ctx):
    from gprx import _lib as L

    fx = fixture("a_p2_5")
    b, _ = make_batch(gprx, ctx, fx, slots_of(fx, 0))
    with pytest.raises(L.GPRXError) as e:
        b.loo_grad()
    assert e.value.status == L.NOT_READY
    b.close()


def test_failed_slot_reads_nan_and_leaves_its_neighbour(gprx, ctx):
    """The failing slot of tests/test_gpu.py (nonpd_p1.npz): NaN and status 1 for it.  Its good neighbour
    (the same inputs at log sigma_n = -2, fixture g_nonpd_p1) lies within the bound and is bit-identical
    to a run in which both slots are good."""
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
    lg = b.loo_grad()
    assert list(lg["status"]) == [1, 0]
    assert np.isnan(lg["logp"][0]) and np.all(np.isnan(lg["grad"][0]))
    assert np.isfinite(lg["logp"][1]) and np.all(np.isfinite(lg["grad"][1]))
    k, kc, mode = float(fx["k"]), float(fx["k_comp"]), ctx.dist_mode
    wv, wc = worst_ratios(fx, [lg["grad"][1]], [(0, 1)], mode)
    print(f"g_nonpd_p1 neighbour mode {mode} grad err {wv[1]:.3e} E {wv[2]:.3e} ratio {wv[0]:.3f}")
    print(f"g_nonpd_p1 neighbour mode {mode} grad_component err {wc[1]:.3e} E {wc[2]:.3e} ratio {wc[0]:.3f}")
    assert wv[0] <= k and wc[0] <= kc, (wv, wc)
    b.run(np.stack([good, good]))
    both = b.loo_grad()
    for q in ("logp", "grad"):
        np.testing.assert_array_equal(lg[q][1], both[q][1], err_msg=q)
    b.close()


def test_after_optimize_the_gradient_belongs_to_the_minimiser(gprx, ctx):
    from gprx.optim import Options

    fx = fixture("a_p2_65")
    slots = slots_of(fx, 0)[:3]
    b, th = make_batch(gprx, ctx, fx, slots)
    res, _ = b.optimize(th, options=Options(iterations=3), refit=True)
    got = b.loo_grad()
    assert np.all(got["status"] == 0)
    b.run(np.stack([r.minimizer for r in res]), grad=False)
    fresh = b.loo_grad()
    for q in ("logp", "grad"):
        np.testing.assert_array_equal(got[q], fresh[q], err_msg=q)
    b.close()


def _p2_batch(gprx, ctx, N=16, n_trials=3):
    from gprx import search

    trials = search.local_trials("P2_MAX", N, range(n_trials), 8)
    G = trials[0]["Y"].shape[0]
    b = gprx.GPBatch(n_trials * G, trials[0]["X"].shape[0], N, 0, ctx=ctx)
    b.set_train(np.repeat(np.stack([t["X"] for t in trials]), G, axis=0), np.concatenate([t["Y"] for t in trials]))
    return b, np.concatenate([t["theta"] for t in trials]), trials


def test_loo_objective_descends_and_repeats_on_p2(gprx, ctx):
    """optimize_batch(objective="loo") on P2 (N = 16, 3 trials): the run cut after i iterations ends at the
    i-th accepted point of the full run, so the minima of i = 0, 1, 2, ... are the accepted values of
    -logp: each lower than the one before.  The result equals a second run bit for bit, and its minimum
    is -logp_LOO at its minimiser."""
    from gprx.optim import Options, optimize_batch

    b, th0, _ = _p2_batch(gprx, ctx)
    prev, steps = None, 0
    for it in range(4):
        res, _ = optimize_batch(b, th0, options=Options(iterations=it), objective="loo")
        if prev is not None:
            for r, p in zip(res, prev):
                if r.iterations == it and r.stopped_by != "linesearch":  # the slot accepted an i-th step
                    assert r.minimum < p.minimum, (it, r.minimum, p.minimum)
                    steps += 1
        prev = res
    assert steps >= len(prev)  # every slot took at least one step on average
    again, _ = optimize_batch(b, th0, options=Options(iterations=3), objective="loo")
    for r, a in zip(prev, again):
        np.testing.assert_array_equal(r.minimizer, a.minimizer)
        assert r.minimum == a.minimum or (np.isnan(r.minimum) and np.isnan(a.minimum))
    assert np.all(b.run(np.stack([r.minimizer for r in prev]), grad=False)["status"] == 0)
    np.testing.assert_array_equal(-b.loo()["logp"], np.array([r.minimum for r in prev]))
    b.close()


PARENT_KEYS = {"kstep_mse", "projectionerror", "failed", "mll", "theta", "status", "f_calls", "rounds", "t_opt", "t_eval",
               "slots", "batches", "params"}


def test_search_group_with_the_loo_objective(gprx, ctx):
    """run_search_group(objective="loo") returns the parent's keys; at the returned theta GPBatch.loo()
    gives a logp at least as large as at the start theta."""
    from gprx import search

    exp, N, ids = "P2_MAX", 16, range(3)
    r = search.run_search_group(exp, N, ids, ctx, 8, 5, 10, objective="loo")
    assert set(r) == PARENT_KEYS
    b, th0, trials = _p2_batch(gprx, ctx, N, len(ids))
    n, G = len(trials), trials[0]["Y"].shape[0]
    assert r["theta"].shape == (n, G, th0.shape[1]) and np.all(r["status"] == 0)
    assert np.all(b.run(th0, grad=False)["status"] == 0)
    start = b.loo()["logp"]
    assert np.all(b.run(r["theta"].reshape(n * G, -1), grad=False)["status"] == 0)
    end = b.loo()["logp"]
    assert np.all(end >= start), (start, end)
    assert np.any(end > start)
    b.close()


def test_gpe_surface(gprx, ctx):
    """dlogpdtheta_LOO(gp) is the batch's gradient row, in the order of get_params."""
    fx = fixture("a_p2_65")
    X, y, th = fx["X"], fx["Y"][0], fx["thetas"][0]
    mean = gprx.MeanFunction(lambda x: 0.25 + 0.5 * x[0])
    gp = gprx.GP(X, y, mean, gprx.SEArd(th[1:-1], th[-1]), th[0], ctx=ctx)
    g = gprx.dlogpdtheta_LOO(gp)
    lg = gp._batch.loo_grad()
    assert g.shape == gp.get_params().shape
    np.testing.assert_array_equal(g, lg["grad"][0])
    np.testing.assert_array_equal(g, gp.dlogpdtheta_LOO())
    assert gprx.logp_LOO(gp) == float(lg["logp"][0])
    # against the batch with the mean taken off by hand
    b = gprx.GPBatch(1, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, (y - mean.mean(X))[None, :])
    b.run(th[None, :], grad=False)
    np.testing.assert_array_equal(b.loo_grad()["grad"][0], g)
    b.close()
