"""Constant input dimensions are left out of the Gram and the gradient (GPRX_OPT_ACTIVE_DIMS,
DESIGN.md section 3): the results must not notice.

"Equal" here means that mll, grad, alpha, mu, var, status and info of one build agree bit for bit
between option 1 (the default) and option 0 (every dimension kept); +0 and -0 count as equal, NaN
equals NaN.  The count of active dimensions the library found is read through
Context.kernel_stats("active_dims")["launches"].

Shapes: N = 130 is three tiles with a ragged last one (several gradient units, padded points);
N = 320 at B = 32 takes the whole-node kernel and the 64 x 64 GEMM units.  The synthetic cases plant
constant columns among random ones: none, the two sides of the 16-dimension boundary of the
gradient's MFMA halves (da = 16, 17 at d = 33), a single active dimension, and none at all.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 130
QUANTITIES = ("mll", "grad", "alpha", "mu", "var", "status", "info")


@pytest.fixture(scope="module")
def gprx():
    import gprx as g

    return g


def evaluate(gprx, option, X, Y, Xs, theta, mode=1, retrain=None):
    """One fresh context and batch: set_train, set_test, run(grad, predict), alpha.  retrain = (X, Y)
    trains the same batch a second time before the run."""
    from gprx import _lib as L

    c = gprx.Context(0)
    b = None
    try:
        c.set_option(L.OPT_ACTIVE_DIMS, option)
        c.set_dist_mode(mode)
        B, Nn = Y.shape
        b = gprx.GPBatch(B, X.shape[-2], Nn, Xs.shape[-1], ctx=c)
        b.set_train(X, Y)
        if retrain is not None:
            b.set_train(*retrain)
        b.set_test(Xs)
        r = b.run(theta, grad=True, predict=True)
        rec = dict(mll=r["mll"].copy(), grad=r["grad"].copy(), mu=np.array(r["mu"]), var=np.array(r["var"]),
                   status=r["status"].copy(), info=r["info"].copy(), da=int(c.kernel_stats("active_dims")["launches"]))
        rec["alpha"] = b.alpha() if np.all(r["status"] == 0) else np.zeros((B, Nn))
    finally:
        if b is not None:
            b.close()
        c.close()
    return rec


def assert_equal(a, b):
    for q in QUANTITIES:
        np.testing.assert_array_equal(a[q], b[q], err_msg=q)


def both(gprx, X, Y, Xs, theta, mode=1):
    on, off = (evaluate(gprx, o, X, Y, Xs, theta, mode) for o in (1, 0))
    assert off["da"] == X.shape[-2]
    assert_equal(on, off)
    return on, off


# ---- generated data -------------------------------------------------------------------------
def generated(mech, Nn, B, M, key_n):
    """B slots over consecutive trials of a mechanism: slot s is output s mod G of trial s div G."""
    from gprx import data

    X, Y, Xs = [], [], []
    t = 0
    while len(Y) < B:
        tr = data.make_trial(mech, Nn, M, seed=data.trial_seed(mech, t))
        for g in range(tr["Y"].shape[0]):
            X.append(tr["X"]), Y.append(tr["Y"][g]), Xs.append(tr["Xs"])
        t += 1
    return np.stack(X[:B]), np.stack(Y[:B]), np.stack(Xs[:B]), data.theta0(mech, key_n)


@pytest.mark.parametrize("mech,Nn,B,M,key_n,da", [("P2", 130, 6, 17, 128, 14), ("CP", 130, 12, 17, 128, 9),
                                                 ("P2", 320, 32, 17, 256, 14)],
                         ids=["P2-N130-B6", "CP-N130-B12", "P2-N320-B32"])
def test_generated_data(gprx, mech, Nn, B, M, key_n, da):
    X, Y, Xs, th = generated(mech, Nn, B, M, key_n)
    on, _ = both(gprx, X, Y, Xs, th)
    assert np.all(on["status"] == 0), on["status"]
    assert on["da"] == da


# ---- synthetic d and da edges ---------------------------------------------------------------
def synthetic(d, const, B=2, M=9, seed=0, value=None):
    """Random columns with planted constants: const = {dimension: value} (the same in every slot and
    in the test points) or a list of such dicts, one per slot."""
    rng = np.random.default_rng(1000 * d + seed)
    X = rng.standard_normal((B, d, N))
    Xs = rng.standard_normal((B, d, M))
    per_slot = const if isinstance(const, list) else [const] * B
    for s, cs in enumerate(per_slot):
        for p, v in cs.items():
            X[s, p, :] = v
            Xs[s, p, :] = v
    Y = rng.standard_normal((B, N))
    theta = np.concatenate([[-1.5], np.full(d, 0.5 * np.log(d)), [0.2]]) + 0.1 * rng.standard_normal((B, d + 2))
    return X, Y, Xs, theta


EDGES = {
    "none-constant": (7, {}, 7),
    "d33-da16": (33, {p: float(p % 3) - 1.0 for p in range(0, 33, 2)}, 16),           # 17 planted
    "d33-da17": (33, {p: float(p % 3) - 1.0 for p in range(1, 33, 2)}, 17),           # 16 planted
    "da1": (6, {p: 0.5 * p for p in (0, 1, 2, 4, 5)}, 1),
}


@pytest.mark.parametrize("case", list(EDGES))
def test_synthetic_edges(gprx, case):
    d, const, da = EDGES[case]
    on, _ = both(gprx, *synthetic(d, const))
    assert np.all(on["status"] == 0), on["status"]
    assert on["da"] == da
    for p in const:
        assert np.all(on["grad"][:, 1 + p] == 0.0)


def test_every_column_constant(gprx):
    """Nothing varies: dimension 0 is kept so that the kernels have one.  All points coincide, so the
    factorisation may well fail; whatever option 0 reports, option 1 reports too."""
    on, _ = both(gprx, *synthetic(5, {p: 1.0 + p for p in range(5)}))
    assert on["da"] == 1


def test_mixed_batch_drops_only_the_shared_constant(gprx):
    on, _ = both(gprx, *synthetic(8, [{0: 2.0, 5: -1.0}, {5: 3.0, 6: 0.25}]))
    assert on["da"] == 7
    assert np.all(on["status"] == 0)
    assert np.all(on["grad"][:, 1 + 5] == 0.0)


def test_signed_zero_and_nan_are_not_constant(gprx):
    """A column of mixed +0 / -0 differs in bits and stays; so does a column that is NaN throughout
    (its distances are NaN, not 0)."""
    X, Y, Xs, th = synthetic(6, {1: 0.0, 3: 1.0})
    X[:, 1, ::2] = -0.0
    on, _ = both(gprx, X, Y, Xs, th)
    assert on["da"] == 5
    X[:, 3, :] = np.nan
    on, _ = both(gprx, X, Y, Xs, th)
    assert on["da"] == 6


def test_non_dyadic_constant(gprx):
    """A constant that is no dyadic rational (0.3).  Its component of the gradient is exactly 0 with
    the dimension dropped, and every other output is as with it kept.  With it kept the component
    must meet tests/test_hp_parity.py's bound for a constant coordinate in direct mode: the truth is
    0, every term of its sum is 0 (A = 0) and the fp64 CPU variants form (0.3 - 0.3)^2 = 0 (E = 0), so
    the bound k max(E, eps A) is 0."""
    on, off = both(gprx, *synthetic(6, {2: 0.3}))
    assert on["da"] == 5
    assert np.all(on["status"] == 0)
    print("d mll / d log ell_2, option 1:", on["grad"][:, 3], "option 0:", off["grad"][:, 3])
    assert np.all(on["grad"][:, 3] == 0.0)
    assert np.all(np.abs(off["grad"][:, 3]) <= 0.0)


def test_overflowing_scale_of_a_dropped_dimension(gprx):
    """log ell = -400 on a constant dimension: il2 = Inf and the scaled difference is Inf - Inf (or
    0 Inf - 0 Inf) = NaN, not 0.  Dropping the dimension must not hide that: K is NaN and the slot
    fails, with or without it.  The other slot, with ordinary hyper-parameters, is untouched."""
    X, Y, Xs, th = synthetic(6, {1: 0.0, 4: 2.5})
    for p in (1, 4):
        t = th.copy()
        t[0, 1 + p] = -400.0
        on, _ = both(gprx, X, Y, Xs, t)
        assert on["da"] == 4
        assert on["status"][0] == 1 and on["status"][1] == 0, on["status"]
        assert np.all(np.isnan(on["grad"][0])) and np.all(on["grad"][1, [2, 5]] == 0.0)


def test_deviating_test_point(gprx):
    """A test point that leaves the training constant in a dropped dimension: the prediction must
    use every dimension (k_pred_cross does, always)."""
    X, Y, Xs, th = synthetic(6, {1: 0.75, 4: 0.0})
    Xs[:, 1, 3] = 0.5
    Xs[0, 4, 0] = -2.0
    on, _ = both(gprx, X, Y, Xs, th)
    assert on["da"] == 4
    Xs_c = Xs.copy()
    Xs_c[:, 1, :] = 0.75
    Xs_c[:, 4, :] = 0.0
    same = evaluate(gprx, 1, X, Y, Xs_c, th)
    assert not np.array_equal(same["mu"], on["mu"])  # the deviation is seen


def test_repeated_set_train(gprx):
    """Two trainings of one batch with different constant sets: each evaluation is a fresh batch's."""
    A = synthetic(9, {0: 1.0, 3: 0.0, 7: -2.0}, seed=1)
    Bq = synthetic(9, {3: 0.5, 4: 0.0}, seed=2)
    for first, second in ((A, Bq), (Bq, A)):
        X, Y, Xs, th = second
        fresh = evaluate(gprx, 1, X, Y, Xs, th)
        again = evaluate(gprx, 1, first[0], first[1], Xs, th, retrain=(X, Y))
        assert fresh["da"] == again["da"] == (7 if second is Bq else 6)
        assert_equal(again, fresh)
        assert_equal(again, evaluate(gprx, 0, X, Y, Xs, th))


def test_expanded_mode_keeps_every_dimension(gprx):
    on, _ = both(gprx, *synthetic(6, {1: 0.3, 4: 0.0}), mode=0)
    assert on["da"] == 6
    assert np.all(on["status"] == 0)


def test_mode_change_after_training(gprx):
    """The distance mode is a setting of the evaluation, the active set one of the training set: a
    batch trained in direct mode and evaluated in expanded mode keeps every dimension."""
    X, Y, Xs, th = synthetic(6, {1: 0.3, 4: 0.0})
    c = gprx.Context(0)
    b = None
    try:
        b = gprx.GPBatch(Y.shape[0], 6, N, Xs.shape[-1], ctx=c)
        b.set_train(X, Y)
        assert c.kernel_stats("active_dims")["launches"] == 4
        b.set_test(Xs)
        for mode, da in ((0, 6), (1, 4)):
            c.set_dist_mode(mode)
            r = b.run(th, grad=True, predict=True)
            assert c.kernel_stats("active_dims")["launches"] == da
            want = evaluate(gprx, 0, X, Y, Xs, th, mode)
            for q in ("mll", "grad", "mu", "var", "status"):
                np.testing.assert_array_equal(r[q], want[q], err_msg=f"mode {mode} {q}")
    finally:
        if b is not None:
            b.close()
        c.close()
