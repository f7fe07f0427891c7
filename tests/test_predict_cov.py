"""Joint predictive covariance and posterior samples on the device (gprx_batch_predict_cov,
gprx_batch_sample and the GPE surface over them) against references built from oracle pieces.

Reference, per slot and distance mode: U from O.lml, K* and K** from O.dist_stack / O.weighted_r /
O.kernel_params, V = solve_triangular(U, K*, trans="T"), Sigma = K** - V^T V.

Tolerances:
  Sigma  |d| <= max(1e-9 sf^2, 10 x the reference's spread between the two distance modes), every
         entry (the project's variance rule)
  factor max|L L^T - (Sigma_dev + j I)| <= 3 (M + 1) eps (max_i Sigma_ii + j): one gamma_{M+1} for the
         factorisation's backward error (|L||L^T| <= max diag), one for this test's own product, one
         of slack for the square roots and the 1 / (1 - gamma)
  sample |samples - (mu + L z)| <= (M + 2) eps (|mu| + |L||z|) elementwise
L is recovered with Z = I.  samples = mu + L e_s would round L by eps |mu|, far above the factor
bound where Sigma ~ 1e-6 sf^2, so the recovery runs on the same batch with zero targets: mu is then
exactly 0 and Sigma, which does not depend on y, is bitwise the one of the real targets (asserted).
The jitter is 0 or 10^k tau with tau = (N + M) eps sf^2; the device derives sf^2 with its own exp,
so "exactly" is checked to 8 eps relative against numpy's.
Each (case, mode) runs on the device once; the tests assert on the shared record.
"""
import functools
import math

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

from oracle import gp_oracle as O  # noqa: E402

EPS = 2.0 ** -52
DEFAULT_MODE = 1
CP_SHAPES = [(1, 1), (65, 7), (130, 65), (200, 130), (320, 64)]
CASES = [f"cp_{n}_{m}" for n, m in CP_SHAPES] + ["fb", "d3", "d3wide", "p2", "p2dup"]
LADDER_WELL = ["p2", "fb"]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """X (B, d, N), Y (B, N), Xs (B, d, M), theta (B, d + 2) of a case."""
    from gprx import data

    if case.startswith("cp_"):
        N, M = (int(v) for v in case.split("_")[1:])
        B = 3
        trs = [data.make_trial("CP", N, M, seed=200 + s) for s in range(B)]
        rng = np.random.default_rng(N)
        th = np.stack([data.theta0("CP", 512) + 0.1 * rng.standard_normal(28) for _ in range(B)])
        return (np.stack([t["X"] for t in trs]), np.stack([t["Y"][s % 4] for s, t in enumerate(trs)]),
                np.stack([t["Xs"] for t in trs]), th)
    if case in ("d3", "d3wide"):  # the random inputs of test_input_dimension_extremes, d = 3; "wide":
        # M beyond one workgroup's 256 threads (the factorisation's strided row loops)
        d, (N, M, B) = 3, ((130, 70, 2) if case == "d3" else (70, 300, 1))
        rng = np.random.default_rng(100 + d)
        X = rng.standard_normal((B, d, N))
        Xs = rng.standard_normal((B, d, M))
        Y = np.stack([np.sin(X[s].sum(axis=0)) + 0.05 * rng.standard_normal(N) for s in range(B)])
        th = np.stack([np.concatenate([[-2.0], np.log(np.full(d, 1.5 * np.sqrt(d)) * (1 + 0.1 * rng.random(d))), [0.1]])
                       for _ in range(B)])
        return X, Y, Xs, th
    B = 2
    if case == "fb":
        tr, th = data.make_trial("FB", 65, 7, seed=7), data.theta0("FB", 64)
    else:
        tr, th = data.make_trial("P2", 130, 40, seed=7), data.theta0("P2", 128)
    Xs = tr["Xs"].copy()
    if case == "p2dup":
        Xs[:, 1] = Xs[:, 0]  # Sigma exactly singular
    return np.tile(tr["X"], (B, 1, 1)), tr["Y"][:B].copy(), np.tile(Xs, (B, 1, 1)), np.tile(th, (B, 1))


def ref_cov(X, y, theta, Xs, mode):
    d = X.shape[0]
    U = O.lml(X, y, theta, mode)[2]["U"]
    il2, sf2, _, _ = O.kernel_params(theta, d)
    Ks = sf2 * np.exp(-O.weighted_r(O.dist_stack(X, Xs, mode), il2) * 0.5)
    Kss = sf2 * np.exp(-O.weighted_r(O.dist_stack(Xs, Xs, mode), il2) * 0.5)
    V = sla.solve_triangular(U, Ks, trans="T", lower=False)
    return Kss - V.T @ V


@functools.lru_cache(maxsize=None)
def reference(case, mode):
    """Per slot: Sigma in `mode`, its spread to the other mode, sf2."""
    X, Y, Xs, th = inputs(case)
    out = []
    for s in range(X.shape[0]):
        a, b = ref_cov(X[s], Y[s], th[s], Xs[s], mode), ref_cov(X[s], Y[s], th[s], Xs[s], 1 - mode)
        out.append(dict(cov=a, other=b, spread=float(np.max(np.abs(a - b))), sf2=math.exp(2 * th[s][-1])))
    return out


def cov_tol(ref):
    return max(1e-9 * ref["sf2"], 10 * ref["spread"])


@pytest.fixture(scope="module")
def gprx():
    import gprx as g

    return g


@pytest.fixture(scope="module")
def ctx(gprx):
    c = gprx.Context(0)
    yield c
    c.close()


_DEV = {}


def device(gprx, ctx, case, mode):
    """One device pass of a case in a mode: predict, predict_cov twice, samples with a shared and a
    per-slot Z, then L from Z = I on the same batch with zero targets."""
    if (case, mode) in _DEV:
        return _DEV[case, mode]
    X, Y, Xs, th = inputs(case)
    B, d, N = X.shape
    M = Xs.shape[2]
    ctx.set_dist_mode(mode)
    try:
        b = gprx.GPBatch(B, d, N, M, ctx=ctx)
        b.set_train(X, Y)
        b.set_test(Xs)
        r = b.run(th, grad=False, predict=True)
        assert np.all(r["status"] == 0)
        mu, cov = b.predict_cov()
        mu2, cov2 = b.predict_cov()
        rng = np.random.default_rng(5)
        Zs, Zb = rng.standard_normal((3, M)), rng.standard_normal((B, 3, M))
        smp_s, jit_s = b.sample(Zs)
        smp_b, jit_b = b.sample(Zb)
        b.set_train(X, np.zeros_like(Y))
        assert np.all(b.run(th, grad=False)["status"] == 0)
        mu0, cov0 = b.predict_cov()
        Lt, jit = b.sample(np.eye(M))
        b.close()
    finally:
        ctx.set_dist_mode(DEFAULT_MODE)
    np.testing.assert_array_equal(cov0, cov)
    assert not np.any(mu0)
    np.testing.assert_array_equal(jit, jit_s)
    np.testing.assert_array_equal(jit, jit_b)
    rec = dict(mu=mu, cov=cov, mu2=mu2, cov2=cov2, mu_p=np.array(r["mu"]), var_p=np.array(r["var"]), Zs=Zs, Zb=Zb,
               smp_s=smp_s, smp_b=smp_b, L=np.swapaxes(Lt, 1, 2).copy(), jit=jit)
    _DEV[case, mode] = rec
    return rec


def tau_of(case, s):
    X, _, Xs, th = inputs(case)
    return (X.shape[2] + Xs.shape[2]) * EPS * math.exp(2 * th[s][-1])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", [c for c in CASES if c != "p2dup"])
def test_cov_against_reference(gprx, ctx, case, mode):
    """Sigma meets the reference in both context modes, at every edge of the tiling and where Sigma
    is of order sf^2 (fb, d3).  Largest error seen on the MI355X, in units of sf^2: DESIGN.md."""
    dev, ref = device(gprx, ctx, case, mode), reference(case, mode)
    for s, f in enumerate(ref):
        err = float(np.max(np.abs(dev["cov"][s] - f["cov"])))
        print(f"{case} mode {mode} slot {s}: max|dSigma| = {err / f['sf2']:.3e} sf2, bound {cov_tol(f) / f['sf2']:.3e} sf2, "
              f"max|Sigma| = {np.max(np.abs(f['cov'])) / f['sf2']:.3e} sf2")
        assert np.all(np.abs(dev["cov"][s] - f["cov"]) <= cov_tol(f))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_cov_properties(gprx, ctx, case, mode):
    """Bitwise symmetry, the clamped diagonal against the oracle's variance, mu bitwise the
    per-point prediction's, and two calls bitwise equal."""
    X, Y, Xs, th = inputs(case)
    dev = device(gprx, ctx, case, mode)
    for s in range(X.shape[0]):
        c = dev["cov"][s]
        np.testing.assert_array_equal(c, c.T)
        f = O.fit(X[s], Y[s], th[s], Xs[s], mode)
        f2 = O.fit(X[s], Y[s], th[s], Xs[s], 1 - mode)
        tol = max(1e-9 * math.exp(2 * th[s][-1]), 10 * float(np.max(np.abs(f["var"] - f2["var"]))))
        assert np.max(np.abs(np.maximum(np.diag(c), 0.0) - f["var"])) <= tol
    np.testing.assert_array_equal(dev["mu"], dev["mu_p"])
    np.testing.assert_array_equal(dev["mu"], dev["mu2"])
    np.testing.assert_array_equal(dev["cov"], dev["cov2"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_factor_and_samples(gprx, ctx, case, mode):
    """L (from Z = I) is lower triangular and factors Sigma_device + j I within the backward-error
    bound; j is 0 or one of 10^k tau; samples with a shared and a per-slot Z are mu + L z."""
    dev = device(gprx, ctx, case, mode)
    B, M = dev["mu"].shape
    for s in range(B):
        L, j, S = dev["L"][s], float(dev["jit"][s]), dev["cov"][s]
        assert np.all(np.isfinite(L)) and not np.any(np.triu(L, 1))
        tau = tau_of(case, s)
        assert j == 0.0 or any(abs(j / tau - 10.0 ** k) <= 8 * EPS * 10.0 ** k for k in range(1, 9)), (j, tau)
        res = float(np.max(np.abs(L @ L.T - (S + j * np.eye(M)))))
        bound = 3 * (M + 1) * EPS * (float(np.max(np.diag(S))) + j)
        print(f"{case} mode {mode} slot {s}: jitter {j:.3e} ({j / tau:.3g} tau), residual {res:.3e}, bound {bound:.3e}")
        assert res <= bound
        for Z, smp in ((dev["Zs"], dev["smp_s"][s]), (dev["Zb"][s], dev["smp_b"][s])):
            want = dev["mu"][s][None, :] + Z @ L.T
            lim = (M + 2) * EPS * (np.abs(dev["mu"][s])[None, :] + np.abs(Z) @ np.abs(L).T)
            assert np.all(np.abs(smp - want) <= lim)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", LADDER_WELL)
def test_ladder_stays_at_zero_when_well_conditioned(gprx, ctx, case, mode):
    """lambda_min(Sigma_ref) >= 1e3 tau on the reference, so the device takes no jitter and its
    factor is the reference's: |L - cholesky(Sigma_ref)| <= max(1e-9 sf, 10 x the spread of the
    reference factor between the modes)."""
    dev, ref = device(gprx, ctx, case, mode), reference(case, mode)
    for s, f in enumerate(ref):
        assert np.linalg.eigvalsh(f["cov"])[0] >= 1e3 * tau_of(case, s)
        assert dev["jit"][s] == 0.0
        La, Lb = np.linalg.cholesky(f["cov"]), np.linalg.cholesky(f["other"])
        tol = max(1e-9 * math.sqrt(f["sf2"]), 10 * float(np.max(np.abs(La - Lb))))
        assert np.max(np.abs(dev["L"][s] - La)) <= tol


@pytest.mark.parametrize("mode", [0, 1])
def test_ladder_duplicated_test_column(gprx, ctx, mode):
    """Test column 1 = column 0: Sigma is exactly singular, the factorisation needs a jitter (which
    rung is not asserted; the factor bound with it is test_factor_and_samples') and the samples
    are finite."""
    dev = device(gprx, ctx, "p2dup", mode)
    assert np.all(dev["jit"] > 0.0)
    assert np.all(np.isfinite(dev["smp_s"])) and np.all(np.isfinite(dev["smp_b"]))


def test_fewer_test_points_than_capacity(gprx, ctx):
    """M_max = 130: after a call at M = 130, set_test with 5 other points; the 5 x 5 result meets
    the reference (nothing from the stale columns or the padded points) and factors."""
    X, Y, Xs, th = inputs("cp_200_130")
    B, d, N = X.shape
    b = gprx.GPBatch(B, d, N, 130, ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    assert np.all(b.run(th, grad=False)["status"] == 0)
    b.predict_cov()
    b.sample(np.eye(130))
    Xs5 = np.ascontiguousarray(Xs[:, :, 60:65])
    b.set_test(Xs5)
    mu, cov = b.predict_cov()
    Lt, jit = b.sample(np.eye(5))
    assert cov.shape == (B, 5, 5)
    for s in range(B):
        a = ref_cov(X[s], Y[s], th[s], Xs5[s], ctx.dist_mode)
        o = ref_cov(X[s], Y[s], th[s], Xs5[s], 1 - ctx.dist_mode)
        sf2 = math.exp(2 * th[s][-1])
        assert np.all(np.abs(cov[s] - a) <= max(1e-9 * sf2, 10 * float(np.max(np.abs(a - o)))))
        np.testing.assert_array_equal(cov[s], cov[s].T)
        L = (Lt[s] - mu[s][None, :]).T  # 5 x 5: recovered to eps |mu|, enough for the triangle and finiteness
        assert np.all(np.isfinite(Lt[s])) and np.all(np.abs(np.triu(L, 1)) <= 2 * EPS * np.max(np.abs(mu[s])))
    b.close()


def test_failed_slot_is_nan_and_isolated(gprx, ctx, golden_dir):
    """Slot 0 at the non-positive-definite theta of nonpd_p1: NaN mu, cov, samples and jitter; slot
    1 is right, and the sample call itself does not fail."""
    z = np.load(golden_dir / "nonpd_p1.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    good = th.copy()
    good[0] = -2.0
    Xs = np.ascontiguousarray(X[:, 3:10] * 1.01)
    b = gprx.GPBatch(2, X.shape[0], X.shape[1], 7, ctx=ctx)
    b.set_train(X, Y[:2])
    b.set_test(Xs)
    r = b.run(np.stack([th, good]), grad=False)
    assert r["status"][0] == 1 and r["status"][1] == 0
    mu, cov = b.predict_cov()
    smp, jit = b.sample(np.eye(7))
    assert np.all(np.isnan(mu[0])) and np.all(np.isnan(cov[0])) and np.all(np.isnan(smp[0])) and np.isnan(jit[0])
    a = ref_cov(X, Y[1], good, Xs, ctx.dist_mode)
    o = ref_cov(X, Y[1], good, Xs, 1 - ctx.dist_mode)
    assert np.all(np.abs(cov[1] - a) <= max(1e-9 * math.exp(2 * good[-1]), 10 * float(np.max(np.abs(a - o)))))
    assert np.all(np.isfinite(smp[1])) and np.isfinite(jit[1])
    b.close()


def test_after_optimize_uses_the_minimisers(gprx, ctx, golden_dir):
    """GPBatch.optimize(..., refit=True) on p1_n50 leaves the batch factorised at the minimisers:
    Sigma is the reference's there."""
    from gprx.optim import LBFGS, Options

    z = np.load(golden_dir / "p1_n50.npz")
    X, Y, th, Xs = z["X"], z["Y"], z["theta"], z["Xs"]
    B = Y.shape[0]
    rng = np.random.default_rng(7)
    th0 = np.stack([th + 0.05 * rng.standard_normal(th.shape[0]) for _ in range(B)])
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], Xs.shape[1], ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    res, _ = b.optimize(th0, LBFGS(), Options(max_evals=40), refit=True)
    _, cov = b.predict_cov()
    for s in range(B):
        t = res[s].minimizer
        a = ref_cov(X, Y[s], t, Xs, ctx.dist_mode)
        o = ref_cov(X, Y[s], t, Xs, 1 - ctx.dist_mode)
        assert np.all(np.abs(cov[s] - a) <= max(1e-9 * math.exp(2 * t[-1]), 10 * float(np.max(np.abs(a - o)))))
    b.close()


def test_runs_on_the_device_and_is_profiled(gprx):
    """One predict_cov and one sample leave launches of the new kernels in kernel_stats."""
    X, Y, Xs, th = inputs("cp_65_7")
    c = gprx.Context(0)
    try:
        c.set_profiling(True)
        b = gprx.GPBatch(X.shape[0], X.shape[1], X.shape[2], 7, ctx=c)
        b.set_train(X, Y)
        b.set_test(Xs)
        b.run(th, grad=False)
        c.reset_stats()
        b.predict_cov()
        b.sample(np.eye(7))
        for k in ("pred_whiten", "pred_cov", "cov_chol", "cov_sample"):
            st = c.kernel_stats(k)
            assert st["launches"] >= 1 and st["flops"] > 0 and st["bytes"] > 0, (k, st)
        b.close()
    finally:
        c.close()


def test_not_ready_and_invalid_arguments(gprx, ctx):
    """GPRX_NOT_READY before a factorisation and without test points; GPRX_INVALID_ARGUMENT for a
    NULL cov / Z / samples, S < 1 and, for sample, M > 1024 (predict_cov still answers there)."""
    from gprx import _lib as L

    rng = np.random.default_rng(3)
    N, d, M = 64, 2, 1025
    X, y = rng.standard_normal((d, N)), rng.standard_normal((1, N))
    th = np.array([[-2.0, 0.3, 0.3, 0.0]])
    b = gprx.GPBatch(1, d, N, 4, ctx=ctx)
    b.set_train(X, y)
    b.set_test(rng.standard_normal((d, 4)))
    with pytest.raises(gprx.GPRXError) as e:
        b.predict_cov()
    assert e.value.status == L.NOT_READY
    assert np.all(b.run(th, grad=False)["status"] == 0)
    b.set_test(np.zeros((d, 0)))  # factorised, but no test points
    buf = np.zeros(16)
    assert L.lib.gprx_batch_predict_cov(b.h, None, L.dptr(buf)) == L.NOT_READY
    assert L.lib.gprx_batch_sample(b.h, L.dptr(buf), 1, 0, L.dptr(buf), None, None) == L.NOT_READY
    b.set_test(rng.standard_normal((d, 4)))
    out, Z = np.zeros(16), np.zeros(4)
    assert L.lib.gprx_batch_predict_cov(b.h, None, None) == L.INVALID_ARGUMENT
    assert L.lib.gprx_batch_sample(b.h, None, 1, 0, L.dptr(out), None, None) == L.INVALID_ARGUMENT
    assert L.lib.gprx_batch_sample(b.h, L.dptr(Z), 1, 0, None, None, None) == L.INVALID_ARGUMENT
    assert L.lib.gprx_batch_sample(b.h, L.dptr(Z), 0, 0, L.dptr(out), None, None) == L.INVALID_ARGUMENT
    assert L.lib.gprx_batch_sample(b.h, L.dptr(Z), 1, 0, L.dptr(out), None, None) == L.OK  # jitter, status NULL
    b.set_test(rng.standard_normal((d, M)))
    with pytest.raises(gprx.GPRXError) as e:
        b.sample(np.zeros((1, M)))
    assert e.value.status == L.INVALID_ARGUMENT
    _, cov = b.predict_cov()
    assert cov.shape == (1, M, M) and np.all(np.isfinite(cov))
    b.close()


def test_more_samples_than_one_pass(gprx, ctx):
    """S beyond the Mpad vectors the device buffers hold goes in passes: every sample is mu + L z
    with the L of Z = I."""
    X, Y, Xs, th = inputs("cp_65_7")
    B, M, S = X.shape[0], 7, 150
    b = gprx.GPBatch(B, X.shape[1], X.shape[2], M, ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    b.run(th, grad=False)
    Z = np.random.default_rng(9).standard_normal((B, S, M))
    smp, _ = b.sample(Z)
    mu, _ = b.predict_cov()
    b.set_train(X, np.zeros_like(Y))
    b.run(th, grad=False)
    Lt, _ = b.sample(np.eye(M))
    for s in range(B):
        L = Lt[s].T
        lim = (M + 2) * EPS * (np.abs(mu[s])[None, :] + np.abs(Z[s]) @ np.abs(L).T)
        assert np.all(np.abs(smp[s] - (mu[s][None, :] + Z[s] @ L.T)) <= lim)
    b.close()


def test_gpe_full_cov_and_rand(gprx, ctx, golden_dir):
    """GPE.predict_f / predict_y(full_cov=True) and rand: the batch results plus the prior mean and
    the noise on the diagonal; rand is (M, n), reproducible from its rng, and the batch's samples
    from the same normals plus the prior mean."""
    z = np.load(golden_dir / "p2_n100.npz")
    X, y, th, Xs = z["X"], z["Y"][2], z["theta"], z["Xs"]
    M = Xs.shape[1]
    gp = gprx.GP(X, y, gprx.MeanFunction(lambda x: 0.1 * x[8]), gprx.SEArd(th[1:-1], th[-1]), ctx=ctx)
    ms = 0.1 * Xs[8]
    mu0 = 0.1 * X[8]
    a = ref_cov(X, y - mu0, th, Xs, ctx.dist_mode)
    o = ref_cov(X, y - mu0, th, Xs, 1 - ctx.dist_mode)
    tol = max(1e-9 * math.exp(2 * th[-1]), 10 * float(np.max(np.abs(a - o))))
    mu_f, cov_f = gprx.predict_f(gp, Xs, full_cov=True)
    mu_v, var_v = gprx.predict_f(gp, Xs)
    np.testing.assert_array_equal(mu_f, mu_v)
    assert np.all(np.abs(cov_f - a) <= tol)
    mu_y, cov_y = gprx.predict_y(gp, Xs, full_cov=True)
    np.testing.assert_array_equal(mu_y, mu_f + ms)
    want = cov_f.copy()
    want[np.diag_indices(M)] += math.exp(2 * th[0])
    np.testing.assert_array_equal(cov_y, want)
    r1 = gprx.rand(gp, Xs, 4, rng=np.random.default_rng(1))
    r2 = gp.rand(Xs, 4, rng=np.random.default_rng(1))
    assert r1.shape == (M, 4)
    np.testing.assert_array_equal(r1, r2)
    Zr = np.random.default_rng(1).standard_normal((4, M))
    smp, _ = gp._batch.sample(Zr)  # the batch's f-space draws from the same normals
    np.testing.assert_array_equal(r1, (smp[0] + ms[None, :]).T)
