"""MeanDynamics GPs rolled out in one device launch (gprx_rollout_max_md / gprx_rollout_min_md:
k_rollout_max's MeanDynamics form and k_rollout_min_md) against the oracle loop -- the oracle GP's
alpha on y - mu(X), oracle/vi_oracle.vi_step as the physics mean, oracle/projection_oracle's
projectv! -- and against the stepwise host loop (gprx.mdynamics.rollout_max / rollout_min) on the
same batch; rollout groups, steps = 0, a failing physics step, the sweep's md_rollout="device" and
GPEs that carry MeanDynamics.

Tolerances: the project's rollout form |out - ref| <= max(1e-9 max(1, |ref|), 10 |ref - alt|), alt
the same reference in the other distance mode (tests/test_projection.py); the projection error
rtol 1e-6, atol 1e-12.  The oracle rollouts are computed once per (mechanism, form, N, steps) in
both distance modes and shared by the two modes' cases (the oracle VI step is the cost: about 0.1 s
(P1) to 1.3 s (FB) per state)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import gp_oracle as O  # noqa: E402
from oracle import projection_oracle as PO  # noqa: E402
from oracle import vi_oracle as VO  # noqa: E402

MECHS = ("P1", "P2", "CP", "FB")
T, STEPS = 3, 8
# The generator trial of the oracle comparisons: data.trial_seed(mech, 5), except the four-bar's
# maximal form.  There trial 5's third start makes the ORACLE's projectv! run out of its 100
# iterations at step 3 (13, 32, 100, ... per step; the device's and the stepwise path's do the same),
# after which the projection error follows the last bits of the input (the two distance modes of the
# oracle differ by 3e-2 in it).  The oracle's own statuses have to be clean before it is a
# reference, so that case takes trial 7 (4 to 7 iterations per step on every start).
MAX_TRIAL = {"P1": 5, "P2": 5, "CP": 5, "FB": 7}
_CACHE: dict = {}


@pytest.fixture(scope="module")
def ctx():
    import gprx

    c = gprx.Context(0)
    mode = c.dist_mode
    yield c
    c.set_dist_mode(mode)
    c.close()


def _tol(ref, alt):
    return np.maximum(1e-9 * np.maximum(1.0, np.abs(ref)), 10 * np.abs(ref - alt))


def _trial(ctx, mech, form, N, M=T, trial=5):
    """One trial of the sweep's generator with MeanDynamics targets: X (d, N), Y = Y_raw - mu(X) with
    mu from the device (mdynamics.mean_max / mean_min), theta (the N = 64 configuration), the M
    start states and the stepwise path's test points Xs."""
    from gprx import data, mdynamics

    key = ("trial", mech, form, N, M, trial)
    if key not in _CACHE:
        seed = data.trial_seed(mech, trial)
        if form == "max":
            tr = data.make_trial(mech, N, M, seed=seed)
            th = data.theta0(mech, 64)
            mu = mdynamics.mean_max(mech, tr["X"], ctx=ctx)
            start, Xs = tr["Xs"].T.copy(), tr["Xs"]
        else:
            usesin = form == "min_sin"
            tr = data.make_trial_min(mech, N, M, seed=seed, usesin=usesin)
            th = data.theta0_min(mech, 64, usesin)
            mu = mdynamics.mean_min(mech, tr["X"], usesin, ctx=ctx)
            start, Xs = tr["start"].copy(), data.min_features(mech, tr["start"], usesin)
        assert np.all(np.isfinite(mu))
        _CACHE[key] = dict(X=tr["X"], Y=tr["Y"] - mu, Y_raw=tr["Y"], th=th, start=start, Xs=Xs, d=tr["X"].shape[0],
                           G=tr["Y"].shape[0])
    return _CACHE[key]


def _gp_mean_fn(tr, md):
    """x (d,) -> the G oracle GP means k*^T alpha in distance mode md."""
    alphas = [O.lml(tr["X"], tr["Y"][g], tr["th"], md)[2]["alpha"] for g in range(tr["G"])]
    il2, sf2, _, _ = O.kernel_params(tr["th"], tr["d"])

    def f(x):
        Ks = sf2 * np.exp(-O.weighted_r(O.dist_stack(tr["X"], x[:, None], md), il2) * 0.5)[:, 0]
        return np.array([Ks @ a for a in alphas])

    return f


def _phys(mech, cstate):
    """The oracle's physics step; its own status must be clean before anything is compared."""
    s, sol = VO.vi_step(mech, cstate)
    assert sol.success and np.all(np.isfinite(s)), (mech, sol.status)
    return s


def _oracle_max(mech, tr, steps, md):
    """tests/test_sweep.py's maximal-coordinate oracle loop (projection_oracle.predictdynamics written
    out, so that projectv!'s iteration count is seen): (final CStates (T, d), projection error (T,)).
    A projection that runs out of its 100 iterations is an oracle failure like a failed physics step:
    what the iterate is after them depends on the last bits of its input."""
    from gprx import data
    from gprx.projection import REGULARIZER

    key = ("omax", mech, tr["X"].shape[1], steps, md)
    if key not in _CACHE:
        gp = _gp_mean_fn(tr, md)
        vwi = data.VW_INDICES[mech]
        idx = np.asarray(vwi) - 1
        m = PO.mechanism(mech)
        nb = m["nb"]
        fin, perr = [], []
        for s in tr["start"]:
            st = PO.State(s, nb, PO.DT)
            obs = np.asarray(s, dtype=np.float64).copy()
            e = 0.0
            for _ in range(steps):
                vu, wu = PO.getvw(gp(obs) + _phys(mech, obs)[idx], vwi, nb)
                v, w, it = PO.projectv(m, st, vu, wu, regularizer=REGULARIZER[mech])
                assert it < 100, (mech, "the oracle's projection did not converge")
                e += float(np.linalg.norm(np.concatenate([np.concatenate([v[b] - vu[b] for b in range(nb)]),
                                                          np.concatenate([w[b] - wu[b] for b in range(nb)])])))
                st.update()
                obs = st.cstate()
            st.update()
            fin.append(st.cstate())
            perr.append(e / steps)
        _CACHE[key] = (np.stack(fin), np.array(perr))
    return _CACHE[key]


def _oracle_min(mech, tr, usesin, steps, md):
    """tests/test_sweep.py's minimal-coordinate oracle loop: the final coordinates q_cur (T, nc)."""
    from gprx import data, mdynamics

    key = ("omin", mech, usesin, tr["X"].shape[1], steps, md)
    if key not in _CACHE:
        gp = _gp_mean_fn(tr, md)
        out = []
        for s in tr["start"]:
            q_old, qd_old = s[0::2].copy(), s[1::2].copy()
            q_cur = q_old + 0.01 * qd_old
            for _ in range(steps):
                obs = np.empty(2 * len(q_old))
                obs[0::2], obs[1::2] = q_old, qd_old
                feat = data.min_features(mech, obs[None, :], usesin)[:, 0]
                o = _phys(mech, mdynamics.xtransform(mech, feat[:, None], usesin)[0])
                mo = (np.array([o[10], o[23] - o[10]]) if mech == "P2" else o[np.asarray(mdynamics.MIN_IDX[mech]) - 1])
                rates = gp(feat) + mo
                q_old, qd_old = q_cur, rates
                q_cur = q_cur + 0.01 * rates
            out.append(q_cur)
        _CACHE[key] = np.stack(out)
    return _CACHE[key]


def _fit(ctx, tr):
    import gprx

    b = gprx.GPBatch(tr["G"], tr["d"], tr["X"].shape[1], 0, ctx=ctx)
    b.set_train(tr["X"], tr["Y"])
    assert np.all(b.run(np.tile(tr["th"], (tr["G"], 1)))["status"] == 0)
    return b


def _cstates(mech, q):
    from gprx.rollout import final_cstate

    return np.stack([final_cstate(mech, r) for r in q])


# ------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("mech,N,steps", [(m, n, STEPS) for m in MECHS for n in (48, 300)] + [("P1", 48, 20)])
def test_max_rollout_matches_oracle(ctx, mech, N, steps, mode):
    from gprx import data
    from gprx.projection import predictdynamics_md

    ctx.set_dist_mode(mode)
    tr = _trial(ctx, mech, "max", N, trial=MAX_TRIAL[mech])
    b = _fit(ctx, tr)
    out, pe, st, vst = predictdynamics_md(mech, [[(b, g) for g in range(tr["G"])]], tr["start"], steps,
                                          data.VW_INDICES[mech], ctx=ctx)
    b.close()
    assert np.all(st == 0) and not np.any(vst & 2), (st, vst)  # vi status 1 (the four-bar: |ds| stalls above eps) is no failure
    ref, pref = _oracle_max(mech, tr, steps, mode)
    alt, _ = _oracle_max(mech, tr, steps, 1 - mode)
    tol = _tol(ref, alt)
    print(mech, N, steps, mode, "max |out - ref| / tol", float(np.max(np.abs(out - ref) / tol)), "spread",
          float(np.max(np.abs(ref - alt))))
    assert np.all(np.isfinite(out))
    assert np.all(np.abs(out - ref) <= tol), float(np.max(np.abs(out - ref) / tol))
    np.testing.assert_allclose(pe, pref, rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("usesin", (False, True))
@pytest.mark.parametrize("mech,N", [(m, n) for m in MECHS for n in (48, 300)])
def test_min_rollout_matches_oracle(ctx, mech, N, usesin, mode):
    from gprx.rollout import rollout_min_md

    ctx.set_dist_mode(mode)
    tr = _trial(ctx, mech, "min_sin" if usesin else "min", N)
    b = _fit(ctx, tr)
    fin, st, vst = rollout_min_md(mech, [[(b, g) for g in range(tr["G"])]], tr["start"], STEPS, usesin, ctx=ctx)
    b.close()
    assert np.all(st == 0) and not np.any(vst & 2), (st, vst)  # vi status 1 (the four-bar: |ds| stalls above eps) is no failure
    out = _cstates(mech, fin[:, 0::2])
    ref = _cstates(mech, _oracle_min(mech, tr, usesin, STEPS, mode))
    alt = _cstates(mech, _oracle_min(mech, tr, usesin, STEPS, 1 - mode))
    tol = _tol(ref, alt)
    print(mech, N, usesin, mode, "max |out - ref| / tol", float(np.max(np.abs(out - ref) / tol)), "spread",
          float(np.max(np.abs(ref - alt))))
    assert np.all(np.isfinite(out))
    assert np.all(np.abs(out - ref) <= tol), float(np.max(np.abs(out - ref) / tol))


# ----------------------------------------------------------- one rank batch: two trials, two groups
def _rank_batch(ctx, mech, form, N, mode, M=T):
    """Trials 5 and 6 in one shard.RankBatch, factorised at theta in distance mode `mode`."""
    from gprx import shard

    ctx.set_dist_mode(mode)
    trs = [_trial(ctx, mech, form, N, M, k) for k in (5, 6)]
    rb = shard.RankBatch([dict(X=t["X"], Y=t["Y"], Xs=t["Xs"]) for t in trs], ctx=ctx)
    r = rb.evaluate(np.stack([np.tile(t["th"], (t["G"], 1)) for t in trs]), grad=False, predict=False)
    assert np.all(r["status"] == 0)
    return rb, trs, np.stack([t["start"] for t in trs])


@pytest.mark.parametrize("mech", MECHS)
def test_fused_max_matches_stepwise(ctx, mech):
    from gprx import mdynamics

    mode = 1
    res = {}
    for md in (mode, 1 - mode):
        rb, _, starts = _rank_batch(ctx, mech, "max", 48, md)
        res[md] = mdynamics.rollout_max(mech, rb, [0, 1], starts, STEPS, ctx=ctx)
        if md == mode:
            dev = mdynamics.rollout_max_device(mech, rb, [0, 1], starts, STEPS, ctx=ctx)
        rb.close()
    (ref, pref, sref), (alt, palt, _) = res[mode], res[1 - mode]
    assert np.all(sref == 0) and np.all(dev[2] == 0)
    assert dev[0].shape == ref.shape and dev[1].shape == pref.shape and dev[2].shape == sref.shape
    # the final states and the projection error under the same form (both paths run the same projection
    # code; where it runs out of iterations, as for one FB start here, its result follows the last
    # bits of the GP means, and the two distance modes differ as much)
    tol, ptol = _tol(ref, alt), _tol(pref, palt)
    print(mech, "fused vs stepwise, max |d| / tol", float(np.max(np.abs(dev[0] - ref) / tol)), "perr",
          float(np.max(np.abs(dev[1] - pref) / ptol)))
    assert np.all(np.abs(dev[0] - ref) <= tol), float(np.max(np.abs(dev[0] - ref) / tol))
    assert np.all(np.abs(dev[1] - pref) <= ptol), float(np.max(np.abs(dev[1] - pref) / ptol))


@pytest.mark.parametrize("usesin", (False, True))
@pytest.mark.parametrize("mech", MECHS)
def test_fused_min_matches_stepwise(ctx, mech, usesin):
    from gprx import mdynamics

    mode = 1
    form = "min_sin" if usesin else "min"
    res = {}
    for md in (mode, 1 - mode):
        rb, _, starts = _rank_batch(ctx, mech, form, 48, md)
        res[md] = mdynamics.rollout_min(mech, rb, [0, 1], starts, STEPS, usesin, ctx=ctx)
        if md == mode:
            dev = mdynamics.rollout_min_device(mech, rb, [0, 1], starts, STEPS, usesin, ctx=ctx)
        rb.close()
    ref, alt = res[mode], res[1 - mode]
    assert dev.shape == ref.shape and np.all(np.isfinite(ref))
    tol = _tol(ref, alt)
    print(mech, usesin, "fused vs stepwise, max |d| / tol", float(np.max(np.abs(dev - ref) / tol)))
    assert np.all(np.abs(dev - ref) <= tol), float(np.max(np.abs(dev - ref) / tol))


@pytest.mark.parametrize("mode", (0, 1))
def test_groups_are_independent_and_bit_identical(ctx, mode):
    """Two rollout groups in one launch, the trajectories interleaved over them: every trajectory is
    bit-identical to the same trajectory launched alone with its group only."""
    from gprx import data
    from gprx.projection import predictdynamics_md
    from gprx.rollout import rollout_min_md

    mech = "P2"
    tg = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
    rb, trs, starts = _rank_batch(ctx, mech, "max", 48, mode)
    groups = [[(rb.batch, rb.slot(i, g)) for g in range(rb.G)] for i in range(2)]
    start = np.stack([starts[tg[k], k // 2] for k in range(6)])
    out, pe, st, vst = predictdynamics_md(mech, groups, start, STEPS, data.VW_INDICES[mech], traj_group=tg, ctx=ctx)
    assert np.all(st == 0)
    assert not np.array_equal(out[0], out[1])
    for k in range(6):
        o1, p1, s1, v1 = predictdynamics_md(mech, [groups[tg[k]]], start[k:k + 1], STEPS, data.VW_INDICES[mech], ctx=ctx)
        np.testing.assert_array_equal(o1[0], out[k])
        assert p1[0] == pe[k] and s1[0] == st[k] and v1[0] == vst[k]
    rb.close()
    rb, trs, starts = _rank_batch(ctx, mech, "min_sin", 48, mode)
    groups = [[(rb.batch, rb.slot(i, g)) for g in range(rb.G)] for i in range(2)]
    start = np.stack([starts[tg[k], k // 2] for k in range(6)])
    fin, st, vst = rollout_min_md(mech, groups, start, STEPS, True, traj_group=tg, ctx=ctx)
    assert np.all(st == 0)
    for k in range(6):
        f1, s1, v1 = rollout_min_md(mech, [groups[tg[k]]], start[k:k + 1], STEPS, True, ctx=ctx)
        np.testing.assert_array_equal(f1[0], fin[k])
        assert s1[0] == st[k] and v1[0] == vst[k]
    rb.close()


def test_zero_steps(ctx):
    """steps = 0: the maximal form is the closing updatestate! only (x + v dt, q wbar(w) dt / 2, the
    velocities kept: a dozen roundings per entry of magnitude <= a few, hence 1e-14), the minimal
    form q + dt qdot with qdot unchanged, bit for bit; status 0 in both."""
    from gprx import data, mdynamics
    from gprx.projection import NBODIES, predictdynamics_md
    from gprx.rollout import rollout_min_md

    for mech in ("P2", "FB"):
        rb, trs, starts = _rank_batch(ctx, mech, "max", 48, 1)
        g0 = [[(rb.batch, rb.slot(0, g)) for g in range(rb.G)]]
        out, pe, st, vst = predictdynamics_md(mech, g0, starts[0], 0, data.VW_INDICES[mech], ctx=ctx)
        nb = NBODIES[mech]
        S = starts[:1]
        want = mdynamics._update(S, S.reshape(1, T, nb, 13)[..., 7:13], nb)[0]
        np.testing.assert_allclose(out, want, rtol=0, atol=1e-14)
        assert np.all(pe == 0.0) and np.all(st == 0) and np.all(vst == 0)
        rb.close()
        rb, trs, starts = _rank_batch(ctx, mech, "min", 48, 1)
        g0 = [[(rb.batch, rb.slot(0, g)) for g in range(rb.G)]]
        fin, st, vst = rollout_min_md(mech, g0, starts[0], 0, False, ctx=ctx)
        np.testing.assert_array_equal(fin[:, 0::2], starts[0][:, 0::2] + 0.01 * starts[0][:, 1::2])
        np.testing.assert_array_equal(fin[:, 1::2], starts[0][:, 1::2])
        assert np.all(st == 0) and np.all(vst == 0)
        rb.close()


def test_failed_physics_step_stops_only_its_trajectory(ctx):
    """A start with |w| = 250 > 2 / dt on body 1: the physics step's sqrt(4 / dt^2 - w.w) is not finite
    (the reference throws a DomainError).  That trajectory ends with status 2, a NaN row and
    vi_status & 2; the launch's other trajectories are bit-identical to a launch without it."""
    from gprx import data
    from gprx.projection import predictdynamics_md
    from gprx.rollout import rollout_min_md

    mech = "P2"
    rb, trs, starts = _rank_batch(ctx, mech, "max", 48, 1)
    g0 = [[(rb.batch, rb.slot(0, g)) for g in range(rb.G)]]
    good = starts[0]
    bad = good[1].copy()
    bad[10] = 250.0  # w_x of body 1
    mixed = np.stack([good[0], bad, good[1], good[2]])
    out, pe, st, vst = predictdynamics_md(mech, g0, mixed, STEPS, data.VW_INDICES[mech], ctx=ctx)
    ref, pref, sref, vref = predictdynamics_md(mech, g0, good, STEPS, data.VW_INDICES[mech], ctx=ctx)
    assert st[1] == 2 and (vst[1] & 2) and np.all(np.isnan(out[1])) and np.isnan(pe[1])
    np.testing.assert_array_equal(out[[0, 2, 3]], ref)
    np.testing.assert_array_equal(pe[[0, 2, 3]], pref)
    assert np.all(st[[0, 2, 3]] == 0) and np.all(sref == 0)
    rb.close()
    rb, trs, starts = _rank_batch(ctx, mech, "min", 48, 1)
    g0 = [[(rb.batch, rb.slot(0, g)) for g in range(rb.G)]]
    good = starts[0]
    bad = good[1].copy()
    bad[1] = 250.0  # the rate of theta1: w_x of body 1
    mixed = np.stack([good[0], bad, good[1], good[2]])
    fin, st, vst = rollout_min_md(mech, g0, mixed, STEPS, False, ctx=ctx)
    ref, sref, vref = rollout_min_md(mech, g0, good, STEPS, False, ctx=ctx)
    assert st[1] == 2 and (vst[1] & 2) and np.all(np.isnan(fin[1]))
    np.testing.assert_array_equal(fin[[0, 2, 3]], ref)
    assert np.all(st[[0, 2, 3]] == 0) and np.all(sref == 0)
    rb.close()


# ------------------------------------------------------------------------------ the sweep and GPEs
def test_sweep_device_rollout_matches_stepwise(ctx):
    """sweep.run_group(md_rollout="device") against "stepwise" for the three md variants of P2:
    kstep_mse within the rollout tolerance form (alt: the stepwise group in the other distance
    mode), projectionerror rtol 1e-6 / atol 1e-12, the same trials failed."""
    from gprx import sweep

    mech, mode = "P2", 1
    kw = dict(testsamples=4, simsteps=3, max_evals=10)
    for var in ("md_max", "md_min", "md_min_sin"):
        ctx.set_dist_mode(mode)
        step = sweep.run_group(mech, 16, var, range(2), ctx, md_rollout="stepwise", **kw)
        dev = sweep.run_group(mech, 16, var, range(2), ctx, md_rollout="device", **kw)
        ctx.set_dist_mode(1 - mode)
        alt = sweep.run_group(mech, 16, var, range(2), ctx, md_rollout="stepwise", **kw)
        ctx.set_dist_mode(mode)
        np.testing.assert_array_equal(dev["failed"], step["failed"])
        assert not np.any(step["failed"])
        tol = _tol(step["kstep_mse"], alt["kstep_mse"])
        print(var, "kstep_mse", dev["kstep_mse"], step["kstep_mse"], "tol", tol)
        assert np.all(np.abs(dev["kstep_mse"] - step["kstep_mse"]) <= tol)
        np.testing.assert_allclose(dev["projectionerror"], step["projectionerror"], rtol=1e-6, atol=1e-12)


def test_gpe_with_meandynamics_rolls_out(ctx):
    """GPEs built with MeanDynamics roll out through the new wrappers, bit-identical to the
    (batch, slot) form on y - mu(X); MeanZero GPEs are refused there and MeanDynamics GPEs by the
    MeanZero entry points."""
    import gprx
    from gprx import data
    from gprx.projection import predictdynamics, predictdynamics_md
    from gprx.rollout import rollout_min, rollout_min_md

    ctx.set_dist_mode(1)
    mech = "P1"

    def gpes(tr, variant, mean=None):
        th = tr["th"]
        return [gprx.GPE(tr["X"], tr["Y_raw"][g], mean or gprx.MeanDynamics(mech, g + 1, variant, ctx=ctx),
                         gprx.SEArd(th[1:-1], th[-1]), logNoise=th[0], ctx=ctx) for g in range(tr["G"])]

    tr = _trial(ctx, mech, "min", 48)
    gp = gpes(tr, "min")
    b = _fit(ctx, tr)
    fin, st, vst = rollout_min_md(mech, [gp], tr["start"], STEPS, False, ctx=ctx)
    ref, sref, vref = rollout_min_md(mech, [[(b, 0)]], tr["start"], STEPS, False, ctx=ctx)
    np.testing.assert_array_equal(fin, ref)
    assert np.all(st == 0) and np.all(sref == 0)
    with pytest.raises(NotImplementedError):
        rollout_min(mech, [gp], tr["start"], STEPS, ctx=ctx)
    with pytest.raises(NotImplementedError):
        rollout_min_md(mech, [gpes(tr, "min", gprx.MeanZero())], tr["start"], STEPS, False, ctx=ctx)
    with pytest.raises(ValueError):  # the mean's variant must be the rollout's
        rollout_min_md(mech, [gp], tr["start"], STEPS, True, ctx=ctx)
    b.close()
    tr = _trial(ctx, mech, "max", 48)
    gp = gpes(tr, "max")
    b = _fit(ctx, tr)
    idx = data.VW_INDICES[mech]
    out = predictdynamics_md(mech, [gp], tr["start"], STEPS, idx, ctx=ctx)
    ref = predictdynamics_md(mech, [[(b, g) for g in range(tr["G"])]], tr["start"], STEPS, idx, ctx=ctx)
    for a, r in zip(out, ref):
        np.testing.assert_array_equal(a, r)
    assert np.all(out[2] == 0)
    with pytest.raises(NotImplementedError):
        predictdynamics(mech, [gp], tr["start"], STEPS, idx, ctx=ctx)
    b.close()
