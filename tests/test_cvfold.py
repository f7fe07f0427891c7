"""gprx_batch_set_folds / gprx_batch_cvfold on the device against the high-precision truth of
tests/golden/cvfold_*.npz (tests/golden/make_golden_cvfold.py), in both distance modes, its two
limiting cases against loo() and run()'s mll, its bitwise properties, statuses and arguments.

Bound, elementwise, for mu, var, logp_fold and logp:  |device - truth| <= k max(E_q, eps A_q)  with the
fixture's k = 8, E_q (geometric mean over five fp64 CPU variants of their largest error, per layout,
theta and mode) and A_q (the absolute sum of q's last reduction).  A case's slots are its (theta,
target) pairs p = t G + g; a per-slot layout's row p belongs to pair p.  Each (case, mode) runs on the
device once, every layout on that one factorisation, and the tests share the record.  The bound test
prints `case layout mode quantity err E ratio`.
"""
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
EPS = 2.0 ** -52
QUANTITIES = ("mu", "var", "logp_fold", "logp")
CASES = ("a_p2_1", "a_p2_5", "a_p2_64", "a_p2_65", "b_cp_130", "b_p1_130", "b_fb_130", "e_d1", "c_cp_320", "f_cp_520")
STORED = ("f_cp_520", "g_nonpd_p1")  # inputs in loo_<case>.npz; g_nonpd_p1: the failed slot's neighbour
_FX, _DEV = {}, {}


def fixture(name):
    if name not in _FX:
        with np.load(GOLDEN / f"cvfold_{name}.npz") as z:
            fx = {k: z[k] for k in z.files}
        with np.load(GOLDEN / (f"loo_{name}.npz" if name in STORED else f"hp_{name}.npz")) as z:
            fx.update(X=z["X"], Y=z["Y"], thetas=np.atleast_2d(z["thetas"]))
        _FX[name] = fx
    return _FX[name]


@pytest.fixture(scope="module")
def gprx():
    import gprx as g

    return g


@pytest.fixture(scope="module")
def ctx(gprx):
    c = gprx.Context(0)
    yield c
    c.close()


def pairs_of(fx, B=0):
    pairs = [(t, g) for t in range(fx["thetas"].shape[0]) for g in range(fx["Y"].shape[0])]
    return [pairs[s % len(pairs)] for s in range(B or len(pairs))]


def make_batch(gprx, c, fx, pairs, M_max=0):
    b = gprx.GPBatch(len(pairs), fx["X"].shape[0], fx["X"].shape[1], M_max, ctx=c)
    b.set_train(fx["X"], np.stack([fx["Y"][g] for _, g in pairs]))
    return b, np.stack([fx["thetas"][t] for t, _ in pairs])


def layout_rows(fx, ln, pairs):
    """fold_of for a batch: (N,) for a shared layout, else pair p's row for every slot."""
    fo = fx[f"{ln}.fold_of"].astype(np.int32)
    if fo.shape[0] == 1:
        return fo[0]
    G = fx["Y"].shape[0]
    return np.stack([fo[t * G + g] for t, g in pairs])


def device(gprx, c, name, mode):
    if (name, mode) not in _DEV:
        fx = fixture(name)
        pairs = pairs_of(fx)
        c.set_dist_mode(mode)
        b = None
        try:
            b, th = make_batch(gprx, c, fx, pairs)
            r = b.run(th, grad=False)
            rec = dict(run=r, loo=b.loo(), layouts={})
            for ln in fx["layouts"]:
                b.set_folds(layout_rows(fx, ln, pairs))
                first = b.cvfold()
                rec["layouts"][ln] = (first, b.cvfold())
        finally:
            if b is not None:
                b.close()
            c.set_dist_mode(1)
        _DEV[name, mode] = rec
    return _DEV[name, mode]


def floor_of(fx, ln, q, j, g):
    return {"mu": fx[f"{ln}.A_mu"][j, g], "var": np.abs(fx[f"{ln}.var"][j, g]), "logp_fold": fx[f"{ln}.A_logp_fold"][j, g],
            "logp": fx[f"{ln}.A_logp"][j, g]}[q]


def worst_ratio(fx, ln, rows, q, qi, pairs, mode):
    """(largest |device - truth| / max(E_q, eps A_q), largest error, E_q) over the slots whose rung is kept."""
    kept = {int(t): j for j, t in enumerate(fx[f"{ln}.theta_index"])}
    worst = (-1.0, 0.0, 0.0)
    for row, (t, g) in zip(rows, pairs):
        if t not in kept:
            continue
        j = kept[t]
        err = np.abs(row - fx[f"{ln}.{q}"][j, g])
        E = float(fx[f"{ln}.E"][mode, j, qi])
        den = np.maximum(E, EPS * floor_of(fx, ln, q, j, g))
        ratio = float(np.max(np.divide(err, den, out=np.where(err > 0, np.inf, 0.0), where=den > 0)))
        worst = max(worst, (ratio, float(np.max(err)), E))
    return worst


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_device_within_variant_spread_of_truth(gprx, ctx, name, mode):
    fx = fixture(name)
    dev = device(gprx, ctx, name, mode)
    k, pairs = float(fx["k"]), pairs_of(fx)
    assert np.all(dev["run"]["status"] == 0)
    misses = []
    for ln in fx["layouts"]:
        cv = dev["layouts"][ln][0]
        assert np.all(cv["status"] == 0), (ln, cv["status"])
        F = fx[f"{ln}.logp_fold"].shape[-1]
        assert cv["logp_fold"].shape == (len(pairs), F)
        for qi, q in enumerate(QUANTITIES):
            ratio, err, E = worst_ratio(fx, ln, cv[q], q, qi, pairs, mode)
            print(f"{name} {ln} mode {mode} {q} err {err:.3e} E {E:.3e} ratio {ratio:.3f}")
            if not ratio <= k:
                misses.append(f"{ln} {q}: ratio {ratio:.3f} > {k}")
    assert not misses, misses


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_repeated_calls_and_equal_slots_are_bit_identical(gprx, ctx, name, mode):
    fx = fixture(name)
    dev = device(gprx, ctx, name, mode)
    G = fx["Y"].shape[0]
    for ln in fx["layouts"]:
        first, again = dev["layouts"][ln]
        for q in QUANTITIES + ("status",):
            np.testing.assert_array_equal(first[q], again[q], err_msg=f"{ln} {q}: second call")
        if fx[f"{ln}.fold_of"].shape[0] == 1:  # var depends on theta and the layout alone: equal across a rung's targets
            for s in range(len(first["var"])):
                np.testing.assert_array_equal(first["var"][s], first["var"][s - s % G], err_msg=f"{ln} var slot {s}")


def test_empty_fold_contributes_zero(gprx, ctx):
    fx = fixture("b_cp_130")
    cv = device(gprx, ctx, "b_cp_130", 1)["layouts"]["empty_mid"][0]
    ref = device(gprx, ctx, "b_cp_130", 1)["layouts"]["c21"][0]
    assert np.all(cv["logp_fold"][:, 3] == 0.0)
    np.testing.assert_array_equal(np.delete(cv["logp_fold"], 3, axis=1), ref["logp_fold"])
    for q in ("mu", "var", "logp"):
        np.testing.assert_array_equal(cv[q], ref[q], err_msg=q)
    assert fx["empty_mid.logp_fold"].shape[-1] == 8


@pytest.mark.parametrize("name", ["a_p2_5", "a_p2_65", "b_cp_130", "c_cp_320"])
def test_singleton_folds_give_loo(gprx, ctx, name):
    """N folds of one point against loo() of the same batch, within the LOO fixture's bound."""
    fx = fixture(name)
    with np.load(GOLDEN / f"loo_{name}.npz") as z:
        lf = {k: z[k] for k in z.files}
    pairs = pairs_of(fx)
    b, th = make_batch(gprx, ctx, fx, pairs)
    assert np.all(b.run(th, grad=False)["status"] == 0)
    lo = b.loo()
    b.set_folds(np.arange(b.N))
    cv = b.cvfold()
    b.close()
    k, mode = float(lf["k"]), ctx.dist_mode
    kept = {int(t): j for j, t in enumerate(lf["theta_index"])}
    for s, (t, g) in enumerate(pairs):
        if t not in kept:
            continue
        j = kept[t]
        for qi, (q, lq) in enumerate((("mu", "mu"), ("var", "var"), ("logp_fold", "logp_i"), ("logp", "logp"))):
            A = {"mu": np.abs(lf["mu"][j, g]) if lf["E"][mode, j, 0] > 0 else lf["A_mu"][j, g], "var": np.abs(lf["var"][j]),
                 "logp_i": np.abs(lf["logp_i"][j, g]), "logp": lf["A_logp"][j, g]}[lq]
            lim = k * np.maximum(lf["E"][mode, j, qi], EPS * A)
            err = np.abs(cv[q][s] - lo[lq][s])
            assert np.all(err <= lim), (name, s, q, float(np.max(err / lim)))


@pytest.mark.parametrize("name", ["a_p2_64", "a_p2_65"])
def test_one_and_the_rest(gprx, ctx, name):
    """Folds of 1 and N - 1 points (held to the truth with the other layouts): the single point also
    reads what it reads among N singleton folds, bit for bit, and the two folds' logp add up."""
    fx = fixture(name)
    pairs = pairs_of(fx)
    b, th = make_batch(gprx, ctx, fx, pairs)
    assert np.all(b.run(th, grad=False)["status"] == 0)
    b.set_folds(np.arange(b.N))
    single = b.cvfold()
    b.set_folds(np.minimum(np.arange(b.N), 1))
    cv = b.cvfold()
    b.close()
    assert np.all(cv["status"] == 0) and np.all(np.isfinite(cv["mu"])) and np.all(cv["var"] > 0)
    for q in ("mu", "var"):
        np.testing.assert_array_equal(cv[q][:, 0], single[q][:, 0], err_msg=q)
    np.testing.assert_array_equal(cv["logp_fold"][:, 0], single["logp_fold"][:, 0])
    assert np.all(np.abs(cv["logp"] - cv["logp_fold"].sum(axis=1)) <= 2 * EPS * np.abs(cv["logp_fold"]).sum(axis=1))


@pytest.mark.parametrize("name", ["a_p2_1", "a_p2_65", "b_cp_130", "b_fb_130"])
def test_one_fold_gives_the_marginal_likelihood(gprx, ctx, name):
    """One fold of every point: logp against run()'s mll of the same batch, within the hp fixture's bound."""
    fx = fixture(name)
    with np.load(GOLDEN / f"hp_{name}.npz") as z:
        hp = {k: z[k] for k in ("E", "A_mll", "k", "quantities")}
    assert hp["quantities"][0] == "mll"
    dev = device(gprx, ctx, name, 1)
    ln = "all" if "all" in dev["layouts"] else "one"
    cv, mll = dev["layouts"][ln][0], dev["run"]["mll"]
    for s, (t, g) in enumerate(pairs_of(fx)):
        lim = float(hp["k"]) * max(hp["E"][1, t, 0], EPS * hp["A_mll"][t, g])
        assert abs(cv["logp"][s] - mll[s]) <= lim, (name, s, abs(cv["logp"][s] - mll[s]) / lim)
        assert cv["logp_fold"][s, 0] == cv["logp"][s]


def test_slot_result_does_not_depend_on_the_batch(gprx, ctx):
    """B = 3 against B = 32 (geometry pinned), repeated slots, and a shared layout against a per-slot
    copy of it: the same bits."""
    from gprx import _lib as L

    fx = fixture("c_cp_320")
    fo = fx["c20.fold_of"][0].astype(np.int32)
    c = gprx.Context(0)
    try:
        c.set_option(L.OPT_LEAF_TILES, 1)
        c.set_option(L.OPT_SMALL_N, 4)
        got = {}
        for B in (3, 32):
            b, th = make_batch(gprx, c, fx, pairs_of(fx, B))
            assert np.all(b.run(th, grad=False)["status"] == 0)
            b.set_folds(fo)
            got[B] = b.cvfold()
            if B == 32:
                b.set_folds(np.tile(fo, (B, 1)))
                per_slot = b.cvfold()
            b.close()
        for q in QUANTITIES:
            np.testing.assert_array_equal(got[3][q], got[32][q][:3], err_msg=q)
            np.testing.assert_array_equal(got[32][q][0], got[32][q][12], err_msg=q)  # the pairs repeat every 12 slots
            np.testing.assert_array_equal(got[32][q], per_slot[q], err_msg=f"{q}: per-slot copy")
    finally:
        c.close()


def test_interleaved_calls_keep_every_result(gprx, ctx):
    """cvfold() after predict() / loo() / loo_grad() returns its bits; predict, alpha, loo and loo_grad
    after cvfold() return theirs from before it."""
    fx = fixture("b_cp_130")
    pairs = pairs_of(fx)[:4]
    b, th = make_batch(gprx, ctx, fx, pairs, M_max=5)
    assert np.all(b.run(th, grad=False)["status"] == 0)
    b.set_test(fx["X"][:, :5])
    before = dict(pred=b.predict(), alpha=b.alpha(), loo=b.loo(), grad=b.loo_grad())
    b.set_folds(fx["mod7.fold_of"][0].astype(np.int32))
    cv = b.cvfold()
    after = dict(pred=b.predict(), alpha=b.alpha(), loo=b.loo(), grad=b.loo_grad())
    cv2 = b.cvfold()
    b.close()
    for q in QUANTITIES:
        np.testing.assert_array_equal(cv[q], cv2[q], err_msg=q)
        np.testing.assert_array_equal(cv[q], device(gprx, ctx, "b_cp_130", 1)["layouts"]["mod7"][0][q][:4], err_msg=q)
    np.testing.assert_array_equal(before["alpha"], after["alpha"])
    for i in range(2):
        np.testing.assert_array_equal(before["pred"][i], after["pred"][i])
    for key in ("loo", "grad"):
        for q in before[key]:
            np.testing.assert_array_equal(before[key][q], after[key][q], err_msg=f"{key} {q}")


def test_failed_slot_reads_nan_and_leaves_its_neighbour(gprx, ctx):
    """nonpd_p1.npz's failing slot: NaN everywhere and status 1; its good neighbour (fixture g_nonpd_p1)
    lies within the bound and is bit-identical to a run in which both slots are good."""
    fx = fixture("g_nonpd_p1")
    z = np.load(GOLDEN / "nonpd_p1.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    good = fx["thetas"][0]
    np.testing.assert_array_equal(X, fx["X"])
    b = gprx.GPBatch(2, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y[:2])
    r = b.run(np.stack([th, good]))
    assert list(r["status"]) == [1, 0]
    b.set_folds(fx["mod4.fold_of"][0].astype(np.int32))
    cv = b.cvfold()
    assert list(cv["status"]) == [1, 0]
    for q in ("mu", "var", "logp_fold"):
        assert np.all(np.isnan(cv[q][0])) and np.all(np.isfinite(cv[q][1])), q
    assert np.isnan(cv["logp"][0]) and np.isfinite(cv["logp"][1])
    k, mode = float(fx["k"]), ctx.dist_mode
    for qi, q in enumerate(QUANTITIES):
        ratio, err, E = worst_ratio(fx, "mod4", [cv[q][1]], q, qi, [(0, 1)], mode)
        print(f"g_nonpd_p1 mod4 mode {mode} {q} err {err:.3e} E {E:.3e} ratio {ratio:.3f}")
        assert ratio <= k, (q, ratio)
    b.run(np.stack([good, good]))
    both = b.cvfold()
    for q in QUANTITIES:
        np.testing.assert_array_equal(cv[q][1], both[q][1], err_msg=q)
    b.close()


def test_not_ready_and_invalid_arguments(gprx, ctx):
    from gprx import _lib as L

    fx = fixture("a_p2_5")
    pairs = pairs_of(fx)
    b, th = make_batch(gprx, ctx, fx, pairs)
    b.set_folds(np.arange(5))  # folds need no factorisation
    with pytest.raises(L.GPRXError) as e:
        b.cvfold()
    assert e.value.status == L.NOT_READY  # before run
    b.close()
    b, th = make_batch(gprx, ctx, fx, pairs)
    b.run(th, grad=False)
    with pytest.raises(L.GPRXError) as e:
        b.cvfold()
    assert e.value.status == L.NOT_READY  # before set_folds
    for bad, nf in ((np.array([0, 1, 2, 3, 5]), 5), (np.array([0, -1, 0, 0, 0]), 2), (np.zeros(5, int), 0)):
        with pytest.raises(L.GPRXError) as e:
            b.set_folds(bad, nfolds=nf)
        assert e.value.status == L.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        b.set_folds(np.zeros(4, int))
    b.set_folds(np.zeros(5, int))
    assert np.all(b.cvfold()["status"] == 0)
    b.close()
    # a fold of GPRX_CVFOLD_MAX + 1 points, on a batch that is created but never run
    N = L.CVFOLD_MAX + 1
    big = gprx.GPBatch(1, 1, N, 0, ctx=ctx)
    with pytest.raises(L.GPRXError) as e:
        big.set_folds(np.zeros(N, int))
    assert e.value.status == L.INVALID_ARGUMENT
    big.set_folds(np.r_[np.zeros(L.CVFOLD_MAX, int), 1])  # CVFOLD_MAX itself is allowed
    with pytest.raises(L.GPRXError) as e:
        big.cvfold()
    assert e.value.status == L.NOT_READY
    big.close()


def test_folds_belong_to_the_batch_and_its_n(gprx, ctx):
    """N is fixed when a batch is created, so training data of another N means another batch: it starts
    without folds.  set_train with the same N keeps them."""
    from gprx import _lib as L

    fx = fixture("a_p2_5")
    pairs = pairs_of(fx)
    b, th = make_batch(gprx, ctx, fx, pairs)
    b.set_folds(np.arange(5) % 2)
    b.set_train(fx["X"], np.stack([fx["Y"][g] for _, g in pairs]))
    b.run(th, grad=False)
    assert np.all(b.cvfold()["status"] == 0)
    b.close()
    b4 = gprx.GPBatch(len(pairs), fx["X"].shape[0], 4, 0, ctx=ctx)
    b4.set_train(fx["X"][:, :4], np.stack([fx["Y"][g][:4] for _, g in pairs]))
    b4.run(th, grad=False)
    with pytest.raises(L.GPRXError) as e:
        b4.cvfold()
    assert e.value.status == L.NOT_READY
    b4.close()


def test_gpe_surface(gprx, ctx):
    """predict_CVfold adds the prior mean at the training inputs back; logp_CVfold is the batch's logp;
    overlapping and non-covering folds are refused."""
    fx = fixture("a_p2_65")
    X, y, th = fx["X"], fx["Y"][0], fx["thetas"][0]
    mean = gprx.MeanFunction(lambda x: 0.25 + 0.5 * x[0])
    gp = gprx.GP(X, y, mean, gprx.SEArd(th[1:-1], th[-1]), th[0], ctx=ctx)
    folds = [np.flatnonzero(np.arange(65) % 3 == f) for f in range(3)]
    mu, var = gprx.predict_CVfold(gp, folds)
    cv = device(gprx, ctx, "a_p2_65", 1)["layouts"]["mod3"][0]
    lp = gprx.logp_CVfold(gp, folds)
    assert lp == gp.logp_CVfold(folds)
    b = gprx.GPBatch(1, X.shape[0], 65, 0, ctx=ctx)
    b.set_train(X, (y - mean.mean(X))[None, :])
    b.run(th[None, :], grad=False)
    b.set_folds(np.arange(65) % 3)
    ref = b.cvfold()
    b.close()
    np.testing.assert_array_equal(mu, ref["mu"][0] + mean.mean(X))
    np.testing.assert_array_equal(var, ref["var"][0])
    np.testing.assert_array_equal(var, cv["var"][0])  # the variance does not depend on the targets
    assert lp == float(ref["logp"][0])
    for bad in ([folds[0], folds[1]], [folds[0], folds[1], folds[2], folds[0][:1]]):
        with pytest.raises(ValueError):
            gprx.logp_CVfold(gp, bad)


def test_groups_record_cv_logp(gprx, ctx):
    """run_search_group(cv_folds=K): cv_logp (n_local, G), equal to GPBatch.cvfold() on an independently
    built batch at the returned theta; with cv_folds=None the keys and values are the parent's."""
    from gprx import search

    exp, N, ids, K = "P2_MAX", 16, range(3), 4
    r = search.run_search_group(exp, N, ids, ctx, 8, 5, 10, cv_folds=K)
    off = search.run_search_group(exp, N, ids, ctx, 8, 5, 10)
    assert set(off) == {"kstep_mse", "projectionerror", "failed", "mll", "theta", "status", "f_calls", "rounds", "t_opt",
                        "t_eval", "slots", "batches", "params"} and set(r) == set(off) | {"cv_logp"}
    for key in ("theta", "mll", "kstep_mse", "status", "f_calls"):
        np.testing.assert_array_equal(r[key], off[key], err_msg=key)
    trials = search.local_trials(exp, N, ids, 8)
    n, G = len(trials), trials[0]["Y"].shape[0]
    assert r["cv_logp"].shape == (n, G) and np.all(r["status"] == 0) and np.all(np.isfinite(r["cv_logp"]))
    b = gprx.GPBatch(n * G, trials[0]["X"].shape[0], N, 0, ctx=ctx)
    b.set_train(np.repeat(np.stack([t["X"] for t in trials]), G, axis=0), np.concatenate([t["Y"] for t in trials]))
    assert np.all(b.run(r["theta"].reshape(n * G, -1), grad=False)["status"] == 0)
    b.set_folds(np.arange(N) % K)
    np.testing.assert_array_equal(b.cvfold()["logp"].reshape(n, G), r["cv_logp"])
    b.close()
