"""Parity of the gfx950 path (through the C ABI) with the oracle restatement.

Tolerances (fp64; DESIGN.md 'Parity'), each the larger of a fixed bound and 10x the spread
between the oracle's two legitimate distance formulations (expanded a^2+b^2-2ab vs direct
(a-b)^2) on the same inputs -- the problem's own sensitivity to rounding, as SURVEY.md 8(d)
prescribes for calibrating the tolerance -- and, for the LML, 10x the oracle's mll_sens =
4 eps ||W o K||_F, the LML change a rounding-level (4-ulp) perturbation of K makes: any other
summation order of the Gram or of the blocked factorisation perturbs K that much, and on the
cond(K) ~ 1e8 cartpole inputs that alone moves the LML by ~1e-9 relative.  On well-conditioned inputs the spread is ~1e-14 and the
fixed bounds apply; on the ill-conditioned cartpole cases (cond(K) ~ 1e8) the two CPU
formulations already differ by up to 7.5e-10 in the LML.
  mll   |d| <= max(1e-9 * max(1, |mll|),        10 spread, 10 mll_sens)
  grad  |d| <= max(1e-7 * max(1, max|grad|),    10 spread)
  mu    |d| <= max(1e-9 * max|y|,               10 spread)
  var   |d| <= max(1e-9 * sf^2,                 10 spread)
The LML bound is 1e-10 relative, flat, on the well-conditioned P2 and FB inputs (SURVEY.md 8(d);
measured: <= 1.8e-11 on the golden P2/FB cases in both modes, ~1e-14 at the full P2 N=2048 and FB
N=4096 sizes).  The adaptive bound above is kept only for the cartpole and pendulum inputs, whose
cond(K) puts the oracle's own two formulations up to 7.5e-10 apart.
Status / pivot index / CState indexing: exact.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import gp_oracle as O  # noqa: E402

TOL_MLL, TOL_GRAD, TOL_MU, TOL_VAR = 1e-9, 1e-7, 1e-9, 1e-9
TOL_MLL_STRICT = 1e-10  # P2 / FB (well-conditioned): flat, no adaptive term
STRICT = ("p2", "fb")
DEFAULT_MODE = 1  # GPRX_DIST_DIRECT, the library default


def tolerances(f, f2, y, theta, strict=False):
    """Per-quantity bounds for a result compared against oracle fit f (f2: the same fit in the
    other distance mode).  strict: the flat 1e-10 LML bound of the well-conditioned mechanisms."""
    def spread(k):
        return float(np.max(np.abs(np.asarray(f[k]) - np.asarray(f2[k])))) if k in f and k in f2 else 0.0

    sf2 = math.exp(2 * theta[-1])
    mll_adaptive = max(TOL_MLL * max(1.0, abs(f["mll"])), 10 * spread("mll"), 10 * float(f.get("mll_sens", 0.0)))
    return dict(
        mll=TOL_MLL_STRICT * max(1.0, abs(f["mll"])) if strict else mll_adaptive,
        grad=max(TOL_GRAD * max(1.0, float(np.max(np.abs(f["grad"])))), 10 * spread("grad")),
        mu=max(TOL_MU * float(np.max(np.abs(y))), 10 * spread("mu")),
        var=max(TOL_VAR * sf2, 10 * spread("var")),
    )


def check_slot(r, s, X, y, theta, Xs, mode, strict=False):
    f = O.fit(X, y, theta, Xs, mode)
    t = tolerances(f, O.fit(X, y, theta, Xs, 1 - mode), y, theta, strict)
    assert r["status"][s] == 0
    assert abs(r["mll"][s] - f["mll"]) <= t["mll"]
    if r["grad"] is not None:
        assert np.max(np.abs(r["grad"][s] - f["grad"])) <= t["grad"]
    if r["mu"] is not None:
        assert np.max(np.abs(r["mu"][s] - f["mu"])) <= t["mu"]
        assert np.max(np.abs(r["var"][s] - f["var"])) <= t["var"]


@pytest.fixture(scope="module")
def gprx():
    import gprx as g

    return g


@pytest.fixture(scope="module")
def ctx(gprx):
    c = gprx.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["p1_n50", "cp_n64", "p2_n100", "p2_n256", "fb_n64"])
@pytest.mark.parametrize("mode", [0, 1])
def test_golden_batch(gprx, ctx, golden_dir, name, mode):
    z = np.load(golden_dir / f"{name}.npz")
    ctx.set_dist_mode(mode)
    tag = "exp" if mode == 0 else "dir"
    X, Y, Xs, th = z["X"], z["Y"], z["Xs"], z["theta"]
    G, N = Y.shape
    b = gprx.GPBatch(G, X.shape[0], N, Xs.shape[1], ctx=ctx)
    b.set_train(X, Y)  # shared X: the G outputs of one trial
    b.set_test(Xs)
    r = b.run(np.tile(th, (G, 1)), grad=True, predict=True)
    assert np.all(r["status"] == 0)
    other = "dir" if tag == "exp" else "exp"
    for g in range(G):
        f = {k: z[f"{k}_{tag}"][g] for k in ("mll", "grad", "mu", "var")}
        f2 = {k: z[f"{k}_{other}"][g] for k in ("mll", "grad", "mu", "var")}
        t = tolerances(f, f2, Y[g], th, name.startswith(STRICT))
        assert abs(r["mll"][g] - f["mll"]) <= t["mll"]
        assert np.max(np.abs(r["grad"][g] - f["grad"])) <= t["grad"]
        assert np.max(np.abs(r["mu"][g] - f["mu"])) <= t["mu"]
        assert np.max(np.abs(r["var"][g] - f["var"])) <= t["var"]
    ctx.set_dist_mode(DEFAULT_MODE)


@pytest.mark.parametrize("N", [1, 2, 5, 33, 63, 64, 65, 127, 130, 200, 320])
def test_ragged_sizes_per_slot_inputs(gprx, ctx, N):
    from gprx import data

    B, M = 3, 7
    trs = [data.make_trial("CP", N, M, seed=200 + s) for s in range(B)]
    X = np.stack([t["X"] for t in trs])
    Y = np.stack([t["Y"][s % 4] for s, t in enumerate(trs)])
    Xs = np.stack([t["Xs"] for t in trs])
    rng = np.random.default_rng(N)
    th = np.stack([data.theta0("CP", 512) + 0.1 * rng.standard_normal(28) for _ in range(B)])
    b = gprx.GPBatch(B, 26, N, M, ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    r = b.run(th, grad=True, predict=True)
    for s in range(B):
        check_slot(r, s, X[s], Y[s], th[s], Xs[s], ctx.dist_mode)


@pytest.mark.parametrize("d", [1, 3, 17, 64])
def test_input_dimension_extremes(gprx, ctx, d):
    """d from 1 to DMAX = 64 (the Gram's 1/ell staging, the gradient epilogue's 16-dimension MFMA
    chunks and their zero padding), ragged N, against the oracle; d = 65 is rejected."""
    rng = np.random.default_rng(100 + d)
    N, M, B = 130, 9, 2
    X = rng.standard_normal((B, d, N))
    Xs = rng.standard_normal((B, d, M))
    Y = np.stack([np.sin(X[s].sum(axis=0)) + 0.05 * rng.standard_normal(N) for s in range(B)])
    th = np.stack([np.concatenate([[-2.0], np.log(np.full(d, 1.5 * np.sqrt(d)) * (1 + 0.1 * rng.random(d))), [0.1]])
                   for _ in range(B)])
    b = gprx.GPBatch(B, d, N, M, ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    r = b.run(th, grad=True, predict=True)
    for s in range(B):
        check_slot(r, s, X[s], Y[s], th[s], Xs[s], ctx.dist_mode)
    b.close()
    with pytest.raises(gprx.GPRXError):
        gprx.GPBatch(1, 65, 64, 0, ctx=ctx)


def test_full_size_p2_against_oracle_and_determinism(gprx, ctx):
    """BASELINE size N=2048, d=26, M=100: one slot against the oracle, and 8 slots bit-identical
    to each other and across repeated runs (size-independent properties)."""
    from gprx import data

    tr = data.make_trial("P2", 2048, 100, seed=data.trial_seed("P2", 0))
    th = data.theta0("P2", 2048)
    B = 8
    b = gprx.GPBatch(B, 26, 2048, 100, ctx=ctx)
    b.set_train(tr["X"], np.tile(tr["Y"][0], (B, 1)))
    b.set_test(tr["Xs"])
    r1 = b.run(np.tile(th, (B, 1)), grad=True, predict=True)
    r2 = b.run(np.tile(th, (B, 1)), grad=True, predict=True)
    check_slot(r1, 0, tr["X"], tr["Y"][0], th, tr["Xs"], ctx.dist_mode, strict=True)
    for k in ("mll", "grad", "mu", "var"):
        np.testing.assert_array_equal(r1[k], r2[k])
        for s in range(1, B):
            np.testing.assert_array_equal(r1[k][s], r1[k][0])
    # predictive variance at training inputs is small; mean reproduces the noisy targets closely
    b.set_test(tr["X"][:, :64])
    mu, var = b.predict()
    assert np.all(var[0] >= 0) and np.all(var[0] < math.exp(2 * th[-1]))


def test_not_positive_definite_status_and_pivot(gprx, ctx, golden_dir):
    z = np.load(golden_dir / "nonpd_p1.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = 2
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y[:B])
    good = th.copy()
    good[0] = -2.0
    r = b.run(np.stack([th, good]), grad=True)
    assert r["status"][0] == 1 and 21 <= r["info"][0] <= X.shape[1]
    assert r["status"][1] == 0
    check_slot(r, 1, X, Y[1], good, None, ctx.dist_mode)


def test_overflowing_hyperparameters(gprx, ctx, golden_dir):
    """exp overflow in the kernel parameters (Julia's exp gives Inf, as numpy's): sf2 = Inf,
    il2 = Inf or a noise of Inf make K non-finite and the slot fails with status 1, as the oracle's
    cholesky (dpotrf, then its finite-diagonal check); the pivot index follows LAPACK dpotf2's rule
    (first pivot <= 0 or NaN: an Inf first pivot passes, the NaN after it fails), which for these
    cases is the first NaN pivot, not the oracle's first non-finite diagonal.  A vanishing sf2
    (exp(-800) = 0 + noise) stays a valid fit."""
    z = np.load(golden_dir / "p1_n50.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    b = gprx.GPBatch(1, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y[:1])
    for i, v in [(-1, 400.0), (1, -400.0), (0, 400.0)]:
        t = th.copy()
        t[i] = v
        r = b.run(t[None], grad=True)
        with pytest.raises(O.NotPosDef):
            O.lml(X, Y[0], t)
        assert r["status"][0] == 1 and 1 <= r["info"][0] <= 2
    t = th.copy()
    t[-1] = -400.0
    r = b.run(t[None], grad=True)
    f = O.fit(X, Y[0], t)
    assert r["status"][0] == 0 and abs(r["mll"][0] - f["mll"]) <= TOL_MLL * abs(f["mll"])
    b.close()


def test_nonfinite_theta_is_invalid_argument(gprx, ctx, golden_dir):
    z = np.load(golden_dir / "p1_n50.npz")
    b = gprx.GPBatch(2, 13, 50, 0, ctx=ctx)
    b.set_train(z["X"], z["Y"][:2])
    th = np.tile(z["theta"], (2, 1))
    th[1, 3] = np.nan
    r = b.run(th, grad=True)
    assert r["status"][0] == 0 and r["status"][1] == 2


def test_gpe_mirror_api(gprx, ctx, golden_dir):
    z = np.load(golden_dir / "p2_n100.npz")
    X, y, th, Xs = z["X"], z["Y"][2], z["theta"], z["Xs"]
    mean = gprx.MeanFunction(lambda x: 0.1 * x[8])  # θ-independent prior mean (MeanDynamics role)
    gp = gprx.GP(X, y, mean, gprx.SEArd(th[1:-1], th[-1]), ctx=ctx)
    mu0 = np.array([0.1 * X[8, t] for t in range(X.shape[1])])
    f = O.fit(X, y - mu0, th, Xs, ctx.dist_mode)
    assert abs(gp.mll - f["mll"]) <= TOL_MLL_STRICT * abs(f["mll"])
    gp.update_mll_and_dmll()
    assert np.max(np.abs(gp.dmll - f["grad"])) <= TOL_GRAD * np.max(np.abs(f["grad"]))
    mu_y, var_y = gprx.predict_y(gp, Xs)
    ms = np.array([0.1 * Xs[8, m] for m in range(Xs.shape[1])])
    np.testing.assert_allclose(mu_y, f["mu"] + ms, rtol=0, atol=TOL_MU * np.max(np.abs(y)))
    np.testing.assert_allclose(var_y, f["var"] + math.exp(2 * th[0]), rtol=0, atol=TOL_VAR * math.exp(2 * th[-1]))
    # single-column prediction, the predictdynamics.jl:13 call shape
    m1, v1 = gp.predict_y(Xs[:, 3])
    assert m1.shape == (1,) and abs(m1[0] - mu_y[3]) <= 1e-12 * max(1, abs(mu_y[3]))


def test_optimize_with_budget_improves_mll(gprx, ctx, golden_dir):
    from gprx.optim import LBFGS, Options, optimize

    z = np.load(golden_dir / "cp_n64.npz")
    th = z["theta"]
    gp = gprx.GP(z["X"], z["Y"][0], gprx.MeanZero(), gprx.SEArd(th[1:-1], th[-1]), ctx=ctx)
    m0 = gp.mll
    res = optimize(gp, LBFGS(), Options(max_evals=30))
    assert gp.mll >= m0 and (res.converged or res.f_calls >= 30)
    np.testing.assert_allclose(gp.get_params(), res.minimizer)


def test_device_pointer_inputs(gprx, ctx, golden_dir):
    import torch

    z = np.load(golden_dir / "p2_n256.npz")
    X, Y, th, Xs = z["X"], z["Y"], z["theta"], z["Xs"]
    G, N = Y.shape
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()  # ABI layout: N x d row-major
    Yd = torch.from_numpy(Y).cuda()
    Xsd = torch.from_numpy(np.ascontiguousarray(Xs.T)).cuda()
    torch.cuda.synchronize()
    b = gprx.GPBatch(G, X.shape[0], N, Xs.shape[1], ctx=ctx)
    b.set_train_device(Xd.data_ptr(), 0, Yd.data_ptr(), N)
    b.set_test_device(Xsd.data_ptr(), Xs.shape[1], 0)
    r = b.run(np.tile(th, (G, 1)), grad=True, predict=True)
    tag = "exp" if ctx.dist_mode == 0 else "dir"
    np.testing.assert_allclose(r["mll"], z[f"mll_{tag}"], rtol=TOL_MLL_STRICT)
    np.testing.assert_allclose(r["mu"], z[f"mu_{tag}"], rtol=0, atol=TOL_MU * np.max(np.abs(Y)))


def test_gpu_evaluator_for_sharding(gprx, ctx, golden_dir):
    from gprx import shard

    z = np.load(golden_dir / "fb_n64.npz")
    ev = shard.gpu_evaluator(ctx=ctx)
    G = z["Y"].shape[0]
    trial = dict(X=z["X"], Y=z["Y"], theta=np.tile(z["theta"], (G, 1)), Xs=z["Xs"])
    r = ev([trial, trial])  # two local trials -> one batch of 2 G slots
    tag = "exp" if ctx.dist_mode == 0 else "dir"
    assert r["mll"].shape == (2, G) and r["mu"].shape == (2, G, z["Xs"].shape[1])
    for t in range(2):
        np.testing.assert_allclose(r["mll"][t], z[f"mll_{tag}"], rtol=TOL_MLL_STRICT)
    np.testing.assert_array_equal(r["mll"][0], r["mll"][1])


def test_optimize_batch_matches_single_gp_runs(gprx, ctx, golden_dir):
    """Lock-step batched LBFGS (one device call per round for all slots) gives every slot the
    same trajectory as optimising its GP alone through the GPE mirror (CPnoise.jl:37-43 loop)."""
    from gprx.optim import LBFGS, Options, optimize, optimize_batch

    z = np.load(golden_dir / "cp_n64.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = Y.shape[0]
    opts = Options(max_evals=20)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    res, rounds = optimize_batch(b, np.tile(th, (B, 1)), LBFGS(), opts)
    assert rounds < sum(r.f_calls for r in res)
    for s in range(B):
        gp = gprx.GP(X, Y[s], gprx.MeanZero(), gprx.SEArd(th[1:-1], th[-1]), ctx=ctx)
        ref = optimize(gp, LBFGS(), opts)
        np.testing.assert_array_equal(res[s].minimizer, ref.minimizer)
        assert res[s].minimum == ref.minimum


def test_graph_replay_matches_direct_launches(gprx, golden_dir):
    """The hipGraph replay (default) and direct stream launches give bit-identical results,
    including after the test set (and so the captured geometry) changes."""
    z = np.load(golden_dir / "p2_n256.npz")
    X, Y, th, Xs = z["X"], z["Y"], z["theta"], z["Xs"]
    out = []
    for graphs in (1, 0):
        c = gprx.Context(0)
        c.set_option(gprx.OPT_GRAPHS, graphs)
        b = gprx.GPBatch(Y.shape[0], X.shape[0], X.shape[1], Xs.shape[1], ctx=c)
        b.set_train(X, Y)
        b.set_test(Xs)
        r1 = b.run(np.tile(th, (Y.shape[0], 1)), grad=True, predict=True)
        b.set_test(Xs[:, :7])
        r2 = b.run(np.tile(th, (Y.shape[0], 1)), grad=True, predict=True)
        out.append((r1, r2))
        b.close()
        c.close()
    for k in ("mll", "grad", "mu", "var"):
        np.testing.assert_array_equal(out[0][0][k], out[1][0][k])
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k])
    np.testing.assert_array_equal(out[0][1]["mu"], out[0][0]["mu"][:, :7])


@pytest.mark.parametrize("leaf,small_n", [(1, 0), (2, 0), (4, 0), (8, 0), (1, 1), (4, 64)])
def test_factorisation_paths_match_golden(gprx, golden_dir, leaf, small_n):
    """Every recursion leaf (fused k_leaf for 2..8 tiles, the standalone 64x64 diagonal kernel at
    leaf 1) and both GEMM unit shapes (64 x 32 pair units below small_n tiles, 64 x 64 above)
    give the golden results at N=256 (4 tiles), the oracle's at N=130 (ragged) and N=512 (an
    8-tile leaf at leaf 8), and report the same failing pivot on a non-PD slot."""
    c = gprx.Context(0)
    c.set_option(gprx.OPT_LEAF_TILES, leaf)
    c.set_option(gprx.OPT_SMALL_N, small_n)
    try:
        z = np.load(golden_dir / "p2_n256.npz")
        X, Y, th, Xs = z["X"], z["Y"], z["theta"], z["Xs"]
        G, N = Y.shape
        b = gprx.GPBatch(G, X.shape[0], N, Xs.shape[1], ctx=c)
        b.set_train(X, Y)
        b.set_test(Xs)
        r = b.run(np.tile(th, (G, 1)), grad=True, predict=True)
        assert np.all(r["status"] == 0)
        t = "exp" if c.dist_mode == 0 else "dir"
        for g in range(G):
            assert abs(r["mll"][g] - z[f"mll_{t}"][g]) <= TOL_MLL_STRICT * max(1.0, abs(z[f"mll_{t}"][g]))
            gs = max(1.0, np.max(np.abs(z[f"grad_{t}"][g])))
            assert np.max(np.abs(r["grad"][g] - z[f"grad_{t}"][g])) <= TOL_GRAD * gs
            assert np.max(np.abs(r["mu"][g] - z[f"mu_{t}"][g])) <= TOL_MU * np.max(np.abs(Y[g]))
            assert np.max(np.abs(r["var"][g] - z[f"var_{t}"][g])) <= TOL_VAR * math.exp(2 * th[-1])
        b.close()
        Xr, yr = X[:, :130], Y[0, :130]
        b = gprx.GPBatch(1, X.shape[0], 130, 9, ctx=c)
        b.set_train(Xr, yr[None])
        b.set_test(Xs[:, :9])
        r = b.run(th[None], grad=True, predict=True)
        check_slot(r, 0, Xr, yr, th, Xs[:, :9], c.dist_mode)
        b.close()
        # N = 512: 8 tiles, one fused leaf of 28 off-diagonal tiles at leaf 8 (two rounds of the
        # leaf's z-partial buffer)
        from gprx import data

        tr = data.make_trial("P2", 512, 9, seed=data.trial_seed("P2", 3))
        th5 = data.theta0("P2", 512)
        b = gprx.GPBatch(1, tr["X"].shape[0], 512, 9, ctx=c)
        b.set_train(tr["X"], tr["Y"][:1])
        b.set_test(tr["Xs"])
        r = b.run(th5[None], grad=True, predict=True)
        check_slot(r, 0, tr["X"], tr["Y"][0], th5, tr["Xs"], c.dist_mode)
        b.close()
        zn = np.load(golden_dir / "nonpd_p1.npz")
        b = gprx.GPBatch(1, zn["X"].shape[0], zn["X"].shape[1], 0, ctx=c)
        b.set_train(zn["X"], zn["Y"][:1])
        r = b.run(zn["theta"][None], grad=True)
        assert r["status"][0] == 1 and r["info"][0] == int(zn["info"])
        b.close()
    finally:
        c.close()


def test_retired_option_id_is_unknown(gprx, ctx):
    """Id 4 selected a launch form that no longer exists (the 4-wave node); it is not reused."""
    with pytest.raises(gprx.GPRXError, match="unknown option") as e:
        ctx.set_option(4, 4)
    assert e.value.status == 2  # GPRX_INVALID_ARGUMENT


def test_fused_node_failure_isolated(gprx, ctx):
    """The fused 8-tile node (k_node8: top leaf + TRSM + SYRK+TT + bottom leaf + LINV21 in one launch)
    at B = 32, N = 512: a slot whose point p has NaN coordinates fails at pivot p + 1 (dpotf2's
    first pivot that is not > 0), once in the top leaf (p = 100) and once in the bottom leaf
    (p = 300); every other slot is bit-identical to a run without those slots' NaNs."""
    from gprx import data

    B, N = 32, 512
    trs = [data.make_trial("P2", N, 1, seed=data.trial_seed("P2", t)) for t in range(B // 6 + 1)]
    X = np.stack([trs[s // 6]["X"] for s in range(B)])
    Y = np.stack([trs[s // 6]["Y"][s % 6] for s in range(B)])
    th = np.tile(data.theta0("P2", N), (B, 1))
    b = gprx.GPBatch(B, X.shape[1], N, 0, ctx=ctx)
    b.set_train(X, Y)
    ref = b.run(th, grad=True)
    assert np.all(ref["status"] == 0)
    Xn = X.copy()
    Xn[5][:, 100] = np.nan
    Xn[9][:, 300] = np.nan
    b.set_train(Xn, Y)
    r = b.run(th, grad=True)
    assert r["status"][5] == 1 and r["info"][5] == 101
    assert r["status"][9] == 1 and r["info"][9] == 301
    keep = [s for s in range(B) if s not in (5, 9)]
    assert np.all(r["status"][keep] == 0)
    np.testing.assert_array_equal(r["mll"][keep], ref["mll"][keep])
    np.testing.assert_array_equal(r["grad"][keep], ref["grad"][keep])
    b.close()


@pytest.fixture(scope="module")
def node8_golden(golden_dir):
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_golden_node8", golden_dir / "make_golden_node8.py")
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    with np.load(golden_dir / "node8_parent.npz") as f:
        return make, {k: f[k] for k in f.files}


@pytest.mark.parametrize("N,B,mech", [(512, 64, "CP"), (1024, 40, "P2"), (500, 36, "P2"), (2048, 32, "P2")])
def test_node8_matches_recorded_results(gprx, ctx, node8_golden, N, B, mech):
    """The whole-8-tile-node kernel (k_node8) and everything around it against results recorded on
    an MI355X from commit 58cbc88 (tests/golden/node8_parent.npz, by tests/golden/make_golden_node8.py,
    whose make_case builds the inputs here too): LML, gradient, mean, variance, status and failing
    pivot of every slot bit for bit, including a failing slot (NaN point: pivot 101 in the top leaf,
    301 in the bottom leaf) and the nodes an ancestor's SYRK updated (N = 1024, 2048: nodes read
    from S); N = 500 pads the last tile.  Two runs of the batch agree bit for bit, and the first good
    slot agrees with the oracle.  The inputs' digest is checked first: a host whose generator rounds
    differently has other inputs, not another kernel."""
    make, rec = node8_golden
    assert (N, B, mech) in make.CASES
    X, Y, Xs, T = make.make_case(N, B, mech)
    assert make.digest(X, Y, Xs, T) == str(rec[make.key(N, B, mech, "sha256")]), "inputs differ from the recorded ones"
    r1, r2 = make.run_case(gprx, ctx, X, Y, Xs, T)
    assert r1["status"][3] == 1 and r1["info"][3] == 101
    assert r1["status"][B - 2] == 1 and r1["info"][B - 2] == 301
    assert np.sum(r1["status"] == 0) == B - 2
    for k in make.OUTPUTS:
        assert make.same_bits(r1[k], r2[k]), f"{k}: two runs differ"
        assert make.same_bits(r1[k], rec[make.key(N, B, mech, k)]), f"{k}: differs from the recorded result"
    ok = np.nonzero(r1["status"] == 0)[0]
    check_slot(r1, int(ok[0]), X[ok[0]], Y[ok[0]], T[ok[0]], Xs[ok[0]], ctx.dist_mode, strict=mech != "CP")


def test_production_path_b32_full_size(gprx, ctx):
    """The bench's configuration: B >= 32 slots (fused 256x256 leaves, folded 64x64 GEMM units,
    folded lauum jobs) at N=2048, d=26, M=100; three slots against the oracle, all slots finite
    and bit-identical across repeated runs."""
    from gprx import data

    B = 32
    trs = [data.make_trial("P2", 2048, 100, seed=data.trial_seed("P2", t)) for t in range(B // 6 + 1)]
    X = np.stack([trs[s // 6]["X"] for s in range(B)])
    Y = np.stack([trs[s // 6]["Y"][s % 6] for s in range(B)])
    Xs = np.stack([trs[s // 6]["Xs"] for s in range(B)])
    rng = np.random.default_rng(5)
    th0 = data.theta0("P2", 2048)
    T = np.stack([th0 + 0.05 * rng.standard_normal(th0.shape[0]) for _ in range(B)])
    b = gprx.GPBatch(B, 26, 2048, 100, ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    r1 = b.run(T, grad=True, predict=True)
    r2 = b.run(T, grad=True, predict=True)
    assert np.all(r1["status"] == 0)
    for k in ("mll", "grad", "mu", "var"):
        assert np.all(np.isfinite(r1[k]))
        np.testing.assert_array_equal(r1[k], r2[k])
    for s in (0, 13, 31):
        check_slot(r1, s, X[s], Y[s], T[s], Xs[s], ctx.dist_mode, strict=True)
    b.close()


@pytest.mark.parametrize("N", [512, 1024, 960, 500, 1000])
def test_production_path_n8_plan(gprx, ctx, N):
    """B >= 32 at N = 512 (the root is an 8-tile node: k_node8, its SYRK + TT on the fixed plan of
    gemm_unit, node tiles read from K), N = 1024 (two 8-tile children: the bottom one reads the
    updated tiles from S), N = 960 (15 tiles: 7/8-tile nodes, the plan only where h = 4), and the
    padded sizes N = 500 and 1000 (the last tile part padding, inside k_node8); slots against the
    oracle and bit-identical across runs."""
    from gprx import data

    B = 32
    trs = [data.make_trial("P2", N, 100, seed=data.trial_seed("P2", 7 + t)) for t in range(B // 6 + 1)]
    X = np.stack([trs[s // 6]["X"] for s in range(B)])
    Y = np.stack([trs[s // 6]["Y"][s % 6] for s in range(B)])
    Xs = np.stack([trs[s // 6]["Xs"] for s in range(B)])
    rng = np.random.default_rng(N)
    th0 = data.theta0("P2", 2048)
    T = np.stack([th0 + 0.05 * rng.standard_normal(th0.shape[0]) for _ in range(B)])
    b = gprx.GPBatch(B, 26, N, 100, ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    r1 = b.run(T, grad=True, predict=True)
    r2 = b.run(T, grad=True, predict=True)
    assert np.all(r1["status"] == 0)
    for k in ("mll", "grad", "mu", "var"):
        np.testing.assert_array_equal(r1[k], r2[k])
    for s in (0, 19, 31):
        check_slot(r1, s, X[s], Y[s], T[s], Xs[s], ctx.dist_mode, strict=True)
    b.close()


def test_mean_only_prediction_matches_full(gprx, ctx, golden_dir):
    """var == NULL skips the variance GEMM; the means are bit-identical to the full prediction
    (GPE predict_y_mean: the predictdynamics.jl:13 rollout call)."""
    z = np.load(golden_dir / "p2_n256.npz")
    X, Y, th, Xs = z["X"], z["Y"], z["theta"], z["Xs"]
    G = Y.shape[0]
    b = gprx.GPBatch(G, X.shape[0], X.shape[1], Xs.shape[1], ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    full = b.run(np.tile(th, (G, 1)), grad=False, predict=True)
    mean_only = b.run(np.tile(th, (G, 1)), grad=False, predict=True, variance=False)
    assert mean_only["var"] is None
    np.testing.assert_array_equal(full["mu"], mean_only["mu"])
    mu2, var2 = b.predict(variance=False)
    assert var2 is None
    np.testing.assert_array_equal(mu2, full["mu"])
    mu3, var3 = b.predict()
    np.testing.assert_array_equal(var3, full["var"])
    b.close()
    gp = gprx.GP(X, Y[1], gprx.MeanZero(), gprx.SEArd(th[1:-1], th[-1]), ctx=ctx)
    m_full, _ = gp.predict_y(Xs)
    np.testing.assert_array_equal(gp.predict_y_mean(Xs), m_full)


def test_fb_full_size_n4096_d52(gprx, ctx):
    """BASELINE config FB "with mDynamics variational-integrator mean": N=4096, d=52, the 12
    per-output GPs of one trial with the MeanDynamics prior mean subtracted (mu(X): one
    variational-integrator step per training state, gprx.mdynamics.mean_max -- getμ(vωindices) of
    experiment_fb_md_max, FBnoise.jl), M=100 test states.  Two slots against the oracle (mll to the
    flat 1e-10 relative bound, gradient, mean, variance), every slot finite and bit-identical across
    repeated runs."""
    from gprx import data, mdynamics

    tr = data.make_trial("FB", 4096, 100, seed=data.trial_seed("FB", 0))
    th = data.theta0("FB", 512)  # the largest FB key of config.json
    G = tr["Y"].shape[0]
    mu0 = mdynamics.mean_max("FB", tr["X"])  # (12, 4096), theta-independent
    assert np.all(np.isfinite(mu0))
    Y = tr["Y"] - mu0
    b = gprx.GPBatch(G, 52, 4096, 100, ctx=ctx)
    b.set_train(tr["X"], Y)
    b.set_test(tr["Xs"])
    T = np.tile(th, (G, 1))
    r1 = b.run(T, grad=True, predict=True)
    r2 = b.run(T, grad=True, predict=True)
    assert np.all(r1["status"] == 0)
    for k in ("mll", "grad", "mu", "var"):
        assert np.all(np.isfinite(r1[k]))
        np.testing.assert_array_equal(r1[k], r2[k])
    for s in (0, 7):
        f = O.fit(tr["X"], Y[s], th, tr["Xs"], ctx.dist_mode)
        assert abs(r1["mll"][s] - f["mll"]) <= TOL_MLL_STRICT * abs(f["mll"])
        assert np.max(np.abs(r1["grad"][s] - f["grad"])) <= TOL_GRAD * max(1.0, np.max(np.abs(f["grad"])))
        assert np.max(np.abs(r1["mu"][s] - f["mu"])) <= TOL_MU * np.max(np.abs(Y[s]))
        assert np.max(np.abs(r1["var"][s] - f["var"])) <= TOL_VAR * math.exp(2 * th[-1])
    b.close()


def test_cp_all_26_outputs_n512(gprx, ctx):
    """BASELINE config CP: N=512, d=26, all 26 CState coordinates as output GPs of one trial (one
    batch sharing X); three outputs against the oracle in both distance tolerances."""
    from gprx import data

    tr = data.make_trial("CP", 512, 64, seed=data.trial_seed("CP", 3))
    Y = tr["Xcurr"]  # 26 x N: every coordinate of the next state
    th = data.theta0("CP", 512)
    b = gprx.GPBatch(26, 26, 512, 64, ctx=ctx)
    b.set_train(tr["X"], Y)
    b.set_test(tr["Xs"])
    r = b.run(np.tile(th, (26, 1)), grad=True, predict=True)
    assert np.all(r["status"] == 0)  # one K for all outputs; constant coordinates just give y = 0
    for s in (0, 8, 21, 22):  # a constant coordinate, cart v_y, pole omega_x, pole v_y
        check_slot(r, s, tr["X"], Y[s], th, tr["Xs"], ctx.dist_mode)
    b.close()


def test_cp_production_path_across_resident_rounds(gprx, ctx):
    """BASELINE config CP on the path its throughput figures run through: 19 trials x all 26 CState
    outputs = 494 slots (B >= 32: k_node8, one 8-wave workgroup per slot and CU, so the 256 CUs take
    the slots in two resident rounds), CP inputs and the CP theta of config.json, each trial
    jittered.  Slots from both rounds against the oracle at the adaptive CP bounds (cond(K) ~ 1e8),
    and the whole batch bit-identical across two runs (CPnoise.jl:37-43)."""
    from gprx import data

    n_tr, G, N, M = 19, 26, 512, 64
    trs = [data.make_trial("CP", N, M, seed=data.trial_seed("CP", 50 + t)) for t in range(n_tr)]
    B = n_tr * G
    X = np.stack([trs[s // G]["X"] for s in range(B)])
    Y = np.stack([trs[s // G]["Xcurr"][s % G] for s in range(B)])
    Xs = np.stack([trs[s // G]["Xs"] for s in range(B)])
    th0 = data.theta0("CP", 512)
    rng = np.random.default_rng(19)
    T = np.repeat(np.stack([th0 + 0.05 * rng.standard_normal(th0.shape[0]) for _ in range(n_tr)]), G, axis=0)
    b = gprx.GPBatch(B, 26, N, M, ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    r1 = b.run(T, grad=True, predict=True)
    r2 = b.run(T, grad=True, predict=True)
    assert np.all(r1["status"] == 0)
    for k in ("mll", "grad", "mu", "var"):
        assert np.all(np.isfinite(r1[k]))
        np.testing.assert_array_equal(r1[k], r2[k])
    # first and last slots of each resident round of 256, and outputs of every kind: a constant
    # coordinate (y = 0), positions, velocities, angular velocities
    for s in (0, 8, 130, 255, 256, 300, 411, 493):
        check_slot(r1, s, X[s], Y[s], T[s], Xs[s], ctx.dist_mode)
    b.close()


def test_pinned_and_pageable_outputs_identical(gprx, ctx, golden_dir):
    """The predictive mean / variance reach a page-locked caller buffer by one pitched DMA copy
    (GPBatch allocates its outputs pinned) and a pageable one through the batch's staging buffer:
    the same values either way, from gprx_batch_run and gprx_batch_predict."""
    from gprx import _lib as L
    from gprx.batch import host_empty

    z = np.load(golden_dir / "p2_n256.npz")
    X, Y, th, Xs = z["X"], z["Y"], z["theta"], z["Xs"]
    G, M = Y.shape[0], Xs.shape[1]
    b = gprx.GPBatch(G, X.shape[0], X.shape[1], M, ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    T = np.ascontiguousarray(np.tile(th, (G, 1)))
    pin_mu, pin_var = host_empty((G, M)), host_empty((G, M))
    mu, var = np.empty((G, M)), np.empty((G, M))
    mll = np.empty(G)
    st, info = np.empty(G, dtype=np.int32), np.empty(G, dtype=np.int32)
    for m_, v_ in ((mu, var), (pin_mu, pin_var)):
        assert L.lib.gprx_batch_run(b.h, L.dptr(T), L.WANT_PREDICT, L.dptr(mll), None, L.dptr(m_), L.dptr(v_), L.iptr(st),
                                    L.iptr(info)) == L.OK
    np.testing.assert_array_equal(mu, pin_mu)
    np.testing.assert_array_equal(var, pin_var)
    r = b.run(T, grad=False, predict=True)
    np.testing.assert_array_equal(r["mu"], mu)
    np.testing.assert_array_equal(r["var"], var)
    pm, pv = b.predict()
    np.testing.assert_array_equal(pm, mu)
    np.testing.assert_array_equal(pv, var)
    assert L.lib.gprx_batch_predict(b.h, L.dptr(mu), L.dptr(var)) == L.OK
    np.testing.assert_array_equal(mu, pm)
    b.close()


def test_batch_bytes_match_the_allocation(gprx, ctx):
    """gprx_batch_bytes (the chunk planner's size) against the device memory a batch actually takes
    (hipMemGetInfo before and after gprx_batch_create): equal up to the allocator's rounding."""
    import ctypes as C

    from gprx import _lib as L, shard

    def free():
        f, t = C.c_uint64(), C.c_uint64()
        L.check(L.lib.gprx_ctx_mem_info(ctx.h, C.byref(f), C.byref(t)))
        assert 0 < f.value <= t.value
        return f.value

    for B, d, N, M in ((8, 26, 2048, 100), (3, 52, 4096, 0)):
        want = shard.batch_bytes(B, d, N, M)
        f0 = free()
        b = gprx.GPBatch(B, d, N, M, ctx=ctx)
        used = f0 - free()
        b.close()
        assert abs(used - want) <= 0.01 * want + (64 << 20), (B, d, N, M, used, want)


def _capacity(b):
    import ctypes as C

    from gprx import _lib as L

    m = C.c_int()
    L.check(L.lib.gprx_batch_dims(b.h, None, None, None, C.byref(m)))
    return m.value


def test_regrown_test_buffers_give_a_fresh_batch_s_results(gprx, ctx, golden_dir):
    """gprx_batch_set_test past the capacity frees and re-allocates the test buffers, and the next
    gprx_batch_predict_cov re-allocates its workspace for the new capacity: a batch created for 0
    test points (capacity 64) that predicts at 5 and then at 70 points (capacity 128) answers bit
    for bit as a batch created for 70, in the mean, the variance and the joint covariance."""
    z = np.load(golden_dir / "p2_n256.npz")
    X, Y, th, Xs = z["X"], z["Y"], z["theta"], z["Xs"]
    G = Y.shape[0]
    T = np.tile(th, (G, 1))
    assert Xs.shape[1] >= 5
    Xs70 = np.tile(Xs, (1, -(-70 // Xs.shape[1])))[:, :70]

    fresh = gprx.GPBatch(G, X.shape[0], X.shape[1], 70, ctx=ctx)
    fresh.set_train(X, Y)
    fresh.set_test(Xs70)
    assert np.all(fresh.run(T, grad=False)["status"] == 0)
    mu_f, var_f = fresh.predict()
    muc_f, cov_f = fresh.predict_cov()
    fresh.close()
    np.testing.assert_array_equal(muc_f, mu_f)

    b = gprx.GPBatch(G, X.shape[0], X.shape[1], 0, ctx=ctx)
    assert _capacity(b) == 64
    b.set_train(X, Y)
    assert np.all(b.run(T, grad=False)["status"] == 0)
    b.set_test(Xs70[:, :5])
    mu5, var5 = b.predict()
    muc5, _ = b.predict_cov()  # a workspace for capacity 64 exists before the regrow
    assert _capacity(b) == 64
    b.set_test(Xs70)
    assert _capacity(b) == 128
    mu70, var70 = b.predict()
    muc70, cov70 = b.predict_cov()
    b.close()
    np.testing.assert_array_equal(mu5, mu_f[:, :5])
    np.testing.assert_array_equal(var5, var_f[:, :5])
    np.testing.assert_array_equal(muc5, mu5)
    np.testing.assert_array_equal(mu70, mu_f)
    np.testing.assert_array_equal(var70, var_f)
    np.testing.assert_array_equal(muc70, mu70)
    np.testing.assert_array_equal(cov70, cov_f)


def test_regrow_and_covariance_workspace_match_their_byte_counts(gprx, ctx):
    """Device memory in use (hipMemGetInfo, as test_batch_bytes_match_the_allocation reads it, and
    to its tolerance of 1 % + 64 MiB for the allocator's rounding) follows the library's own
    accounting through a batch's life: growing the test capacity from 64 to 2048 points takes the
    difference of gprx_batch_bytes, the first gprx_batch_predict_cov takes gprx_batch_cov_bytes
    (1.3 GB here: a buffer missing from or doubled in either would show), and closing the batch
    gives everything back."""
    import ctypes as C

    from gprx import _lib as L, data, shard

    def free():
        f, t = C.c_uint64(), C.c_uint64()
        L.check(L.lib.gprx_ctx_mem_info(ctx.h, C.byref(f), C.byref(t)))
        assert 0 < f.value <= t.value
        return f.value

    def close_to(used, want):
        print("device bytes used", used, "accounted", want)
        return abs(used - want) <= 0.01 * want + (64 << 20)

    B, d, N = 8, 26, 2048
    tr = data.make_trial("P2", N, 64, seed=data.trial_seed("P2", 0))
    th = data.theta0("P2", N)
    cov_want = C.c_uint64()
    L.check(L.lib.gprx_batch_cov_bytes(B, N, N, C.byref(cov_want)))
    assert cov_want.value > 1.3e9
    f0 = free()
    b = gprx.GPBatch(B, d, N, 64, ctx=ctx)
    b.set_train(tr["X"], np.tile(tr["Y"][0], (B, 1)))
    f1 = free()
    b.set_test(tr["X"])  # N test points: the training inputs
    f2 = free()
    assert close_to(f1 - f2, shard.batch_bytes(B, d, N, N) - shard.batch_bytes(B, d, N, 64))
    assert np.all(b.run(np.tile(th, (B, 1)), grad=False)["status"] == 0)
    b.predict_cov()
    f3 = free()
    assert close_to(f2 - f3, cov_want.value)
    b.close()
    assert close_to(f0 - free(), 0)


def test_opt_trace_capacity_checked(gprx, ctx, golden_dir):
    """gprx_batch_set_opt_trace refuses a buffer smaller than max_rounds * B * (2(d+2)+2) doubles
    (the write size was implied) and registers one that is large enough."""
    from gprx import _lib as L

    z = np.load(golden_dir / "p1_n50.npz")
    b = gprx.GPBatch(2, z["X"].shape[0], z["X"].shape[1], 0, ctx=ctx)
    n = z["X"].shape[0] + 2
    need = 3 * 2 * (2 * n + 2)
    buf = np.zeros(need)
    assert L.lib.gprx_batch_set_opt_trace(b.h, L.dptr(buf), 3, need - 1) == L.INVALID_ARGUMENT
    assert L.lib.gprx_batch_set_opt_trace(b.h, L.dptr(buf), 3, need) == L.OK
    assert L.lib.gprx_batch_set_opt_trace(b.h, None, 0, 0) == L.OK
    b.close()


def test_batch_create_refuses_sizes_past_the_buffer_range(gprx, ctx):
    """Npad * max(Npad, Mpad) * 8 >= 2^31 - 16 is refused before any allocation (the kernels'
    32-bit buffer offsets would read zeros past it), for the training size and the test points."""
    with pytest.raises(gprx.GPRXError) as e:
        gprx.GPBatch(1, 4, 16321, 0, ctx=ctx)
    assert e.value.status == 2
    with pytest.raises(gprx.GPRXError) as e:
        gprx.GPBatch(1, 4, 2048, 131009, ctx=ctx)
    assert e.value.status == 2
    b = gprx.GPBatch(1, 4, 2048, 64, ctx=ctx)
    with pytest.raises(gprx.GPRXError) as e:  # growing the test capacity past the range
        b.set_test(np.zeros((4, 131009)))
    assert e.value.status == 2
    b.close()


def test_out_of_memory_batch_is_an_error_not_a_hang(gprx, ctx, golden_dir):
    """A batch larger than HBM fails with GPRX_OUT_OF_MEMORY (its partial allocations released
    under the context's own lock) and the context stays usable."""
    with pytest.raises(gprx.GPRXError) as e:
        gprx.GPBatch(4000, 26, 4096, 0, ctx=ctx)  # 4000 x 4 x 134 MB of matrices
    assert e.value.status == 4
    z = np.load(golden_dir / "p1_n50.npz")
    b = gprx.GPBatch(1, z["X"].shape[0], z["X"].shape[1], 0, ctx=ctx)
    b.set_train(z["X"], z["Y"][:1])
    assert b.run(z["theta"][None])["status"][0] == 0
    b.close()


def test_threads_share_a_context(gprx, ctx, golden_dir):
    """Threading contract (include/gprx.h): calls on one context from several host threads
    serialise on its mutex (ctypes releases the GIL) and give the serial results bit for bit."""
    import threading

    names = ["p1_n50", "cp_n64", "p2_n100", "fb_n64"]
    zs = [np.load(golden_dir / f"{n}.npz") for n in names]
    batches = []
    for z in zs:
        b = gprx.GPBatch(z["Y"].shape[0], z["X"].shape[0], z["X"].shape[1], z["Xs"].shape[1], ctx=ctx)
        b.set_train(z["X"], z["Y"])
        b.set_test(z["Xs"])
        batches.append(b)
    serial = [b.run(np.tile(z["theta"], (z["Y"].shape[0], 1)), grad=True, predict=True) for b, z in zip(batches, zs)]
    got = [None] * len(zs)

    def work(i):
        for _ in range(5):
            got[i] = batches[i].run(np.tile(zs[i]["theta"], (zs[i]["Y"].shape[0], 1)), grad=True, predict=True)

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(zs))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    for i in range(len(zs)):
        for k in ("mll", "grad", "mu", "var"):
            np.testing.assert_array_equal(got[i][k], serial[i][k])
    for b in batches:
        b.close()


def test_threads_with_own_contexts(gprx, golden_dir):
    """The reference's pattern (Threads.@threads over trials, core.jl:28) with one context per
    thread on the same device: each context's stream runs concurrently with the others and every
    thread reproduces the serial results bit for bit."""
    import threading

    z = np.load(golden_dir / "p2_n100.npz")
    G = z["Y"].shape[0]
    th = np.tile(z["theta"], (G, 1))
    ref_ctx = gprx.Context(0)
    b0 = gprx.GPBatch(G, z["X"].shape[0], z["X"].shape[1], z["Xs"].shape[1], ctx=ref_ctx)
    b0.set_train(z["X"], z["Y"])
    b0.set_test(z["Xs"])
    ref = b0.run(th, grad=True, predict=True)
    b0.close()
    ref_ctx.close()
    got = [None] * 4

    def work(i):
        c = gprx.Context(0)
        b = gprx.GPBatch(G, z["X"].shape[0], z["X"].shape[1], z["Xs"].shape[1], ctx=c)
        b.set_train(z["X"], z["Y"])
        b.set_test(z["Xs"])
        for _ in range(5):
            got[i] = b.run(th, grad=True, predict=True)
        b.close()
        c.close()

    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=60)
    for i in range(4):
        for k in ("mll", "grad", "mu", "var"):
            np.testing.assert_array_equal(got[i][k], ref[k])


def _compare_opt(dev, host):
    """Device LBFGS (k_lbfgs) against the host restatement (gprx.optim.optimize_batch) driven
    through the same batch: both derive the kernel parameters on the device (derive_params) and
    sum dot products in the same sequential order, so every decision (evaluation counts,
    iterations, stop reason) and every iterate is bit-identical."""
    for s, (r, h) in enumerate(zip(dev, host)):
        assert (r.iterations, r.f_calls, r.g_calls, r.stopped_by, r.converged) == (
            h.iterations, h.f_calls, h.g_calls, h.stopped_by, h.converged), s
        np.testing.assert_array_equal(r.minimizer, h.minimizer)
        assert r.minimum == h.minimum or (math.isnan(r.minimum) and math.isnan(h.minimum)), s


@pytest.mark.parametrize("name,max_evals", [("cp_n64", 20), ("p1_n50", 40), ("p2_n100", 30)])
def test_device_optimize_matches_host_lockstep(gprx, ctx, golden_dir, name, max_evals):
    from gprx.optim import LBFGS, Options, optimize_batch

    z = np.load(golden_dir / f"{name}.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = Y.shape[0]
    rng = np.random.default_rng(7)
    th0 = np.stack([th + 0.05 * rng.standard_normal(th.shape[0]) for _ in range(B)])
    opts = Options(max_evals=max_evals)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    host, hr = optimize_batch(b, th0, LBFGS(), opts)
    dev, dr = b.optimize(th0, LBFGS(), opts)
    _compare_opt(dev, host)
    assert dr == hr


def test_device_optimize_bench_shape_bit_identical(gprx, ctx):
    """The bench's optimiser leg (bench.py, P2noise.jl:41's optimize!): B = 48 slots at N=2048,
    d=26, a 30-evaluation budget, starts jittered by different amounts so the slots finish at
    different rounds (masked evaluation rounds at the end).  Device and host minimisers, minima,
    counts and stop reasons are bit-identical, and so are the two legs' evaluation traces round by
    round (the same theta asked, the same answer given: gprx_batch_set_opt_trace against
    optimize_batch's trace)."""
    from gprx import data
    from gprx.optim import LBFGS, Options, compare_optimisers, optimize_batch

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
    htr = []
    host, hr = optimize_batch(b, T, LBFGS(), o, trace=htr)
    dev, dr = b.optimize(T, LBFGS(), o, refit=True, trace_rounds=160)
    dtr = b.last_opt_trace
    htr = np.stack(htr)
    rep = compare_optimisers(dev, host, dtr, htr)
    assert rep["equal"], rep
    _compare_opt(dev, host)
    assert dr == hr and dtr.shape == htr.shape
    act = dtr[:, :, 0] == 1.0
    np.testing.assert_array_equal(act, htr[:, :, 0] == 1.0)
    np.testing.assert_array_equal(dtr[act].view(np.uint64), htr[act].view(np.uint64))
    last = [int(np.nonzero(act[:, s])[0].max()) for s in range(B)]
    assert len(set(last)) > 1, last  # the slots finished at different rounds
    b.close()


def test_device_optimize_ragged_batch_equals_single_slot_runs(gprx, ctx, golden_dir):
    """Slots that stop at different rounds (Optim's own stops, no budget): finished slots are
    masked out of the later rounds' evaluations, and every slot's result is bit-identical to
    optimising that GP alone."""
    from gprx.optim import LBFGS, Options

    z = np.load(golden_dir / "p2_n100.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = Y.shape[0]
    rng = np.random.default_rng(11)
    th0 = np.stack([th + 0.2 * rng.standard_normal(th.shape[0]) for _ in range(B)])
    opts = Options(iterations=60)
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    dev, rounds = b.optimize(th0, LBFGS(), opts, refit=False)
    assert len({r.f_calls for r in dev}) > 1  # ragged: the slots stop at different rounds
    one = gprx.GPBatch(1, X.shape[0], X.shape[1], 0, ctx=ctx)
    for s in range(B):
        one.set_train(X, Y[s:s + 1])
        (r1,), _ = one.optimize(th0[s:s + 1], LBFGS(), opts, refit=False)
        assert (r1.iterations, r1.f_calls, r1.g_calls, r1.stopped_by) == (
            dev[s].iterations, dev[s].f_calls, dev[s].g_calls, dev[s].stopped_by), s
        np.testing.assert_array_equal(r1.minimizer, dev[s].minimizer)
        assert r1.minimum == dev[s].minimum
    one.close()
    b.close()


def test_device_optimize_to_convergence_and_refit(gprx, ctx, golden_dir):
    """optimize! to Optim's own stop (no budget) on every slot, then update_target!: the batch is
    left factorised at the minimisers, so predict() answers for them."""
    from gprx.optim import LBFGS, Options, optimize_batch

    z = np.load(golden_dir / "p1_n50.npz")
    X, Y, th, Xs = z["X"], z["Y"], z["theta"], z["Xs"]
    B = Y.shape[0]
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], Xs.shape[1], ctx=ctx)
    b.set_train(X, Y)
    b.set_test(Xs)
    th0 = np.tile(th, (B, 1))
    dev, rounds = b.optimize(th0)
    assert rounds > 0
    mu_dev, var_dev = b.predict()
    host, _ = optimize_batch(b, th0, LBFGS(), Options())
    thmin = np.stack([r.minimizer for r in dev])
    for s in range(B):
        assert dev[s].stopped_by in ("g_tol", "x_tol", "f_tol", "linesearch")
        assert dev[s].minimum <= host[s].minimum + 1e-6 * max(1.0, abs(host[s].minimum))
    r = b.run(thmin, grad=True, predict=True)
    np.testing.assert_allclose(-r["mll"], [d.minimum for d in dev], rtol=1e-12)
    np.testing.assert_array_equal(r["mu"], mu_dev)
    np.testing.assert_array_equal(r["var"], var_dev)
    for s in range(B):  # the LML at the minimiser against the oracle (the gradient there is ~0 and
        # its ill-conditioned rounding is no parity signal)
        f = O.fit(X, Y[s], thmin[s], None, ctx.dist_mode)
        t = tolerances(f, O.fit(X, Y[s], thmin[s], None, 1 - ctx.dist_mode), Y[s], thmin[s])
        assert abs(r["mll"][s] - f["mll"]) <= t["mll"]


def test_device_optimize_failed_start_and_time_limit(gprx, ctx, golden_dir):
    """A slot whose start is not positive definite answers +Inf with a NaN gradient: both
    optimisers take one iteration of halvings and stop on Optim's NaN-gradient break while the
    healthy slot runs on; a zero time limit stops every slot after its first iteration."""
    from gprx.optim import LBFGS, Options, optimize_batch

    z = np.load(golden_dir / "nonpd_p1.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    good = th.copy()
    good[0] = -2.0
    th0 = np.stack([th, good])
    b = gprx.GPBatch(2, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y[:2])
    opts = Options(max_evals=80)
    host, _ = optimize_batch(b, th0, LBFGS(), opts)
    dev, _ = b.optimize(th0, LBFGS(), opts, refit=False)
    _compare_opt(dev, host)
    assert dev[0].stopped_by == "nan_gradient" and dev[0].minimum == math.inf
    assert dev[1].stopped_by == "max_evals"
    dev, _ = b.optimize(np.stack([good, good]), LBFGS(), Options(time_limit=0.0), refit=False)
    assert all(r.stopped_by == "time_limit" and r.iterations == 1 for r in dev)


def test_device_optimize_refit_failure_is_reported(gprx, ctx, golden_dir):
    """optimize! with the closing refit (update_target!) on a slot whose search ended at a
    non-finite minimiser (the NaN-gradient stop of a non-PD start): the call reports the refit's
    failure (first failing slot) with the search results attached, and the batch is left
    unfactorised, so predict() answers NOT_READY instead of values for the wrong theta."""
    from gprx.optim import LBFGS, Options

    z = np.load(golden_dir / "nonpd_p1.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    good = th.copy()
    good[0] = -2.0
    b = gprx.GPBatch(2, X.shape[0], X.shape[1], 4, ctx=ctx)
    b.set_train(X, Y[:2])
    b.set_test(X[:, :4])
    b.run(np.stack([good, good]))  # factorised before the call
    with pytest.raises(gprx.GPRXError) as e:
        b.optimize(np.stack([th, good]), LBFGS(), Options(max_evals=80), refit=True)
    assert e.value.status in (1, 2)
    res, _ = e.value.results
    assert res[0].stopped_by == "nan_gradient" and res[1].stopped_by in ("max_evals", "g_tol", "f_tol", "x_tol")
    with pytest.raises(gprx.GPRXError) as e2:
        b.predict()
    assert e2.value.status == 5  # GPRX_NOT_READY
    # a healthy batch refits and predicts as before
    res2, _ = b.optimize(np.stack([good, good]), LBFGS(), Options(max_evals=10), refit=True)
    mu, var = b.predict()
    r = b.run(np.stack([x.minimizer for x in res2]), grad=False, predict=True)
    np.testing.assert_array_equal(mu, r["mu"])
    b.close()


def test_device_optimize_rejects_invalid_options(gprx, ctx, golden_dir):
    """Invalid options are rejected before the search: ValueError from the Python side; through the
    raw C ABI GPRX_INVALID_ARGUMENT with every output left unwritten (distinguishable from a refit
    failure, which fills the outputs); the batch is still usable afterwards."""
    import ctypes as C

    from gprx import _lib as L
    from gprx.optim import LBFGS, Options

    z = np.load(golden_dir / "p1_n50.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    b = gprx.GPBatch(2, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y[:2])
    th0 = np.stack([th, th])
    for bad in (dict(method=LBFGS(m=65)), dict(method=LBFGS(m=0)), dict(options=Options(iterations=-1)),
                dict(method=LBFGS(alphaguess=math.inf))):
        with pytest.raises(ValueError):
            b.optimize(th0, **bad)
    o = gprx.batch.opt_options()
    o.m = 100
    stp = np.full(2, -7, dtype=np.int32)
    th_out = np.full((2, th.shape[0]), 123.0)
    rc = L.lib.gprx_batch_optimize(b.h, L.dptr(th0), C.byref(o), L.dptr(th_out), None, None, None, None, L.iptr(stp),
                                   None)
    assert rc == L.INVALID_ARGUMENT
    assert np.all(stp == -7) and np.all(th_out == 123.0)
    res, _ = b.optimize(th0, LBFGS(), Options(max_evals=5))
    assert all(r.f_calls >= 1 for r in res)
    b.close()


def test_alpha_of_a_failed_slot_is_nan(gprx, ctx, golden_dir):
    """gprx_batch_alpha: alpha is defined only for the slots whose last evaluation succeeded; a
    failed slot (not positive definite) reads NaN, the others the oracle's alpha."""
    z = np.load(golden_dir / "nonpd_p1.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    good = th.copy()
    good[0] = -2.0
    b = gprx.GPBatch(2, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y[:2])
    r = b.run(np.stack([th, good]))
    assert r["status"][0] == 1 and r["status"][1] == 0
    a = b.alpha()
    assert np.all(np.isnan(a[0]))
    # the good slot's alpha is unaffected by its failed neighbour (bit-identical to a run where both
    # slots are good) and agrees with the oracle to 10x what a 4-ulp relative perturbation of K moves
    # it by (these nearly duplicated points make cond(K) ~ 3e8: any other summation order of the Gram
    # or of a blocked factorisation moves alpha by ~6e-7 here)
    b.run(np.stack([good, good]))
    np.testing.assert_array_equal(a[1], b.alpha()[1])
    f = O.fit(X, Y[1], good, None, ctx.dist_mode)
    K = O.gram(X, good, ctx.dist_mode)[0]
    E = np.random.default_rng(0).uniform(-1.0, 1.0, K.shape)
    sens = np.max(np.abs(np.linalg.solve(K * (1.0 + 2.0 * np.finfo(float).eps * (E + E.T)), Y[1]) - f["alpha"]))
    tol = max(1e-9 * np.max(np.abs(f["alpha"])), 10 * sens)
    np.testing.assert_allclose(a[1], f["alpha"], rtol=0, atol=tol)
    b.close()


def test_alpha_export_matches_oracle(gprx, ctx, golden_dir):
    """gprx_batch_alpha (gp.alpha for hosts that keep GaussianProcesses' fields current) equals
    the oracle's alpha = K^-1 y; before any factorisation it answers NOT_READY."""
    z = np.load(golden_dir / "p2_n100.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    G = Y.shape[0]
    b = gprx.GPBatch(G, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    with pytest.raises(gprx.GPRXError) as e:
        b.alpha()
    assert e.value.status == 5
    b.run(np.tile(th, (G, 1)))
    a = b.alpha()
    for g in range(G):
        f = O.fit(X, Y[g], th, None, ctx.dist_mode)
        np.testing.assert_allclose(a[g], f["alpha"], rtol=0, atol=1e-9 * np.max(np.abs(f["alpha"])))
    b.close()


@pytest.mark.parametrize("name,limit", [("cp_n64", 20), ("p1_n50", 40), ("p2_n100", 30), ("nonpd_p1", 80)])
def test_device_optimize_matches_the_independent_oracle(gprx, ctx, golden_dir, name, limit):
    """k_lbfgs (device, lock-step over the batch) against oracle/lbfgs_oracle.py -- the independent
    restatement of Optim 1.4.1 LBFGS + LineSearches 7.1.1 BackTracking(order=2) -- driven by the
    same device evaluations (each slot evaluated alone through a batch of one: same kernels, same
    bits).  Every iterate decision must agree: minimiser and minimum bit for bit, iterations, f/g
    calls (NLSolversBase counting), stop reason.  Optim itself is not runnable here (unpinned)."""
    from gprx.optim import LBFGS, Options
    from oracle import lbfgs_oracle as LO

    z = np.load(golden_dir / f"{name}.npz")
    X, Y, th = z["X"], z["Y"], z["theta"]
    B = min(Y.shape[0], 3)
    rng = np.random.default_rng(11)
    th0 = np.stack([th + (0.05 * rng.standard_normal(th.shape[0]) if name != "nonpd_p1" else 0.0) for _ in range(B)])
    b = gprx.GPBatch(B, X.shape[0], X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y[:B])
    dev, _ = b.optimize(th0, LBFGS(), Options(max_evals=limit), refit=False)
    for s in range(B):
        one = gprx.GPBatch(1, X.shape[0], X.shape[1], 0, ctx=ctx)
        one.set_train(X, Y[s:s + 1])

        def fg(h):
            if not np.all(np.isfinite(h)):
                return math.inf, np.full(h.shape[0], np.nan)
            r = one.run(h[None], grad=True)
            if r["status"][0] != 0:
                return math.inf, np.full(h.shape[0], np.nan)
            return -float(r["mll"][0]), -np.asarray(r["grad"][0], dtype=np.float64)

        ref = LO.optimize(fg, th0[s], f_calls_limit=limit)
        one.close()
        np.testing.assert_array_equal(dev[s].minimizer, ref["minimizer"])
        assert dev[s].minimum == ref["minimum"] or (math.isnan(dev[s].minimum) and math.isnan(ref["minimum"]))
        assert (dev[s].iterations, dev[s].f_calls, dev[s].g_calls, dev[s].stopped_by, dev[s].converged) == (
            ref["iterations"], ref["f_calls"], ref["g_calls"], ref["stopped_by"], ref["converged"]), s
    b.close()


def test_reproducible_beside_another_gpu_process(gprx, ctx):
    """Evaluations stay bit-identical while another process loads the same GPU (fp64 GEMMs from
    torch).  Before the k_gram store fix, memory back-pressure let a MUBUF store read its data
    registers after the next exp had overwritten them: one slot in every few evaluations got K
    elements ~6.76e15 and a non-PD pivot ("Store-data hazard"; scratch/concurrency.py
    measured 20% of B=240 evaluations).  Alternating thetas, so a stale or racy value cannot hide
    behind a repeat of the same inputs."""
    import subprocess
    import sys
    import time

    from gprx import data

    B, N = 96, 2048
    trs = [data.make_trial("P2", N, 0, seed=data.trial_seed("P2", 40 + t)) for t in range(B // 6)]
    X = np.stack([trs[s // 6]["X"] for s in range(B)])
    Y = np.stack([trs[s // 6]["Y"][s % 6] for s in range(B)])
    th0 = data.theta0("P2", 2048)
    rng = np.random.default_rng(3)
    Ta = np.stack([th0 + 0.05 * rng.standard_normal(th0.shape[0]) for _ in range(B)])
    Tb = Ta + 0.02 * rng.standard_normal(Ta.shape)
    b = gprx.GPBatch(B, 26, N, 0, ctx=ctx)
    b.set_train(X, Y)
    ref = {k: b.run(t, grad=True) for k, t in (("a", Ta), ("b", Tb))}
    load = ("import time, torch\n"
            "a = torch.randn(4096, 4096, dtype=torch.float64, device='cuda')\n"
            "t0 = time.time()\n"
            "while time.time() - t0 < 25:\n"
            "    a = torch.tanh(a @ a * 1e-3); torch.cuda.synchronize()\n")
    p = subprocess.Popen([sys.executable, "-c", load])
    try:
        time.sleep(6)  # torch import + first kernels on the card
        assert p.poll() is None, "load process ended early"
        n, t0 = 0, time.time()
        while time.time() - t0 < 12:
            k = "ab"[n % 2]
            r = b.run(Ta if k == "a" else Tb, grad=True)
            n += 1
            assert np.all(r["status"] == 0), (n, np.nonzero(r["status"])[0], r["info"][r["status"] != 0])
            np.testing.assert_array_equal(r["mll"], ref[k]["mll"])
            np.testing.assert_array_equal(r["grad"], ref[k]["grad"])
        assert n >= 40
    finally:
        p.wait(timeout=60)
        b.close()


@pytest.mark.parametrize("N", [256, 1024])
def test_first_launches_from_concurrent_contexts_in_a_fresh_process(golden_dir, N):
    """Kernel attributes (dynamic LDS above 64 KB: k_leaf9 / k_node8 151 KB, LINV21's k_gemm 67.6 KB,
    k_lauum_grad, k_lbfgs) are set once per device when a context is created (gprx_ctx_create,
    std::call_once), not by a process-wide flag at the first launch: four threads of a fresh process
    each create a context and at once run a B = 32 batch and its optimiser; every thread gets the
    serial results.  N = 256: the fused 4-tile leaf; N = 1024: two k_node8 nodes and the root's
    LINV21 k_gemm, the launches whose LDS exceeds the 64 KB default."""
    import subprocess
    import sys

    script = r'''
import sys, threading, numpy as np
sys.path.insert(0, sys.argv[1])
import gprx
from gprx import data
from gprx.optim import LBFGS, Options
B, N = 32, int(sys.argv[2])
trs = [data.make_trial("P2", N, 0, seed=data.trial_seed("P2", t)) for t in range(B // 6 + 1)]
X = np.stack([trs[s // 6]["X"] for s in range(B)])
Y = np.stack([trs[s // 6]["Y"][s % 6] for s in range(B)])
T = np.tile(data.theta0("P2", min(N, 2048)), (B, 1))
go = threading.Barrier(4)
out = [None] * 4
def work(i):
    go.wait()
    c = gprx.Context(0)
    b = gprx.GPBatch(B, 26, N, 0, ctx=c)
    b.set_train(X, Y)
    r = b.run(T, grad=True)
    res, _ = b.optimize(T, LBFGS(), Options(max_evals=6))
    out[i] = (r["mll"].copy(), r["grad"].copy(), np.stack([q.minimizer for q in res]))
    b.close(); c.close()
ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
[t.start() for t in ts]; [t.join(120) for t in ts]
assert all(o is not None for o in out), "a thread failed"
for o in out[1:]:
    for a, b in zip(out[0], o):
        np.testing.assert_array_equal(a, b)
assert np.all(np.isfinite(out[0][0]))
print("ok")
'''
    import pathlib

    pkg = str(pathlib.Path(__file__).resolve().parents[1] / "gpr.jl_amd")
    r = subprocess.run([sys.executable, "-c", script, pkg, str(N)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
