"""The recorded, resumable rollouts (gprx_rollout_max_rec, gprx_rollout_max_md_rec,
gprx_rollout_min_rec, gprx_rollout_min_md_rec) on the device.

What is held, bit for bit (np.array_equal), against the one-launch entry points, whose kernels are
the parent's (tests/test_rollout_recorded.py):
  * launch splitting carries everything: for steps_per_launch in {1, 4, 6, 0} every final output
    equals the one-launch call's, and the records are the same for all four (4 does not divide the 6
    steps: an uneven last launch);
  * the records are the trajectory: with F the one-launch final state at steps = k, F's pose is the
    pose of record k + 2 and F's rates are the rates of record k + 1 (1-based storage indices; the
    closing updatestate! copies the discrete pose into the pose and re-reads the same solution; in
    minimal coordinates the next step's q_old is this step's q_cur), and record 1 is the start;
  * a sparse, repeated rec picks rows of the full record; a rec that ends early changes no output;
  * a trajectory whose physics mean fails keeps its start, has NaN afterwards and status 2, and
    leaves the call's other trajectories as they are without it.
Against the oracle (maximal form, one mechanism per mean): the states projection_oracle's
predictdynamics hands its predict callback, at tests/test_projection.py's bound.

Shapes: the cases of tests/golden/make_golden_rollouts.py (its inputs, T = 3 in two groups) that
cross the kernels' strides -- N = 48 and 300 (past the maximal kernel's 256 threads), 48 and 1100
(past the minimal kernel's 4 x 256) -- over 6 steps, every mechanism, both distance modes.
"""
import importlib.util

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MECHS = ("P1", "P2", "CP", "FB")
SIZES = {"max": (48, 300), "min": (48, 1100), "min_sin": (48, 1100)}
CASES = [(mech, form, N) for form in SIZES for mech in MECHS for N in SIZES[form]]
STEPS = 6
SPLITS = (1, 4, 6, 0)
SPARSE, EARLY = [1, 1, 4, 7], [2, 3]
_CACHE: dict = {}


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def make(golden_dir):
    return _load(golden_dir / "make_golden_rollouts.py", "make_golden_rollouts")


@pytest.fixture(scope="module")
def inputs(golden_dir):
    with np.load(golden_dir / "rollouts_parent.npz") as f:
        return {k: f[k] for k in f.files if ".n" not in k}


@pytest.fixture(scope="module")
def ctx():
    import gprx

    c = gprx.Context(0)
    mode = c.dist_mode
    yield c
    c.set_dist_mode(mode)
    c.close()


def _entries(mech, form, groups, start, kw):
    """{mean: (one(steps) -> outputs, rec(steps, rec, spl) -> (traj, *outputs))} of a coordinate form."""
    from gprx import data
    from gprx.projection import predictdynamics, predictdynamics_md, predictdynamics_md_rec, predictdynamics_rec
    from gprx.rollout import rollout_min, rollout_min_md, rollout_min_md_rec, rollout_min_rec

    if form == "max":
        vwi = data.VW_INDICES[mech]
        return {"mz": (lambda s: predictdynamics(mech, groups, start, s, vwi, **kw),
                       lambda s, r, n: predictdynamics_rec(mech, groups, start, s, vwi, r, steps_per_launch=n, **kw)),
                "md": (lambda s: predictdynamics_md(mech, groups, start, s, vwi, **kw),
                       lambda s, r, n: predictdynamics_md_rec(mech, groups, start, s, vwi, r, steps_per_launch=n, **kw))}
    us = form == "min_sin"
    return {"mz": (lambda s: (rollout_min(mech, groups, start, s, us, **kw),),
                   lambda s, r, n: rollout_min_rec(mech, groups, start, s, r, us, steps_per_launch=n, **kw)),
            "md": (lambda s: rollout_min_md(mech, groups, start, s, us, **kw),
                   lambda s, r, n: rollout_min_md_rec(mech, groups, start, s, r, us, steps_per_launch=n, **kw))}


def _case(ctx, make, inputs, mech, form, N, mode):
    """Every call of a case, made once: per mean {"one": [outputs at steps = 0 .. STEPS], "rec":
    {spl: (traj, *outputs)}, "sparse", "early"}, and the start."""
    key = (mech, form, N, mode)
    if key not in _CACHE:
        import gprx

        ctx.set_dist_mode(mode)
        X = inputs[f"{form}.{mech}.X"][:, :N] / make.SCALE
        Y = inputs[f"{form}.{mech}.Y"][:, :N] / make.SCALE
        theta, start = inputs[f"{form}.{mech}.theta"], inputs[f"{form}.{mech}.start"]
        G = Y.shape[0]
        b = gprx.GPBatch(2 * G, X.shape[0], N, 0, ctx=ctx)
        b.set_train(X, np.concatenate([Y, Y]))
        assert np.all(b.run(np.repeat(theta, G, axis=0), grad=False)["status"] == 0)
        groups = [[(b, k * G + j) for j in range(G)] for k in range(2)]
        res = {"start": start}
        for mean, (one, rec) in _entries(mech, form, groups, start, dict(traj_group=make.TRAJ_GROUP, ctx=ctx)).items():
            # (steps = 0 is not asked of the MeanZero maximal form, whose final state is unset there)
            res[mean] = {"one": [one(s) if (s or mean == "md" or form != "max") else None for s in range(STEPS + 1)],
                         "rec": {n: rec(STEPS, None, n) for n in SPLITS},
                         "sparse": rec(STEPS, SPARSE, 4), "early": rec(STEPS, EARLY, 4),
                         "none": rec(STEPS, np.empty(0, dtype=np.int32), 4)}
        b.close()
        _CACHE[key] = res
    return _CACHE[key]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _pose_rates(form, a):
    """(pose, rates) of rows (..., w): x, q and v, omega per body; q and qdot per coordinate."""
    if form == "max":
        c = a.reshape(a.shape[:-1] + (-1, 13))
        return c[..., :7], c[..., 7:]
    return a[..., 0::2], a[..., 1::2]


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("mech,form,N", CASES)
def test_launch_splitting_carries_everything(ctx, make, inputs, mech, form, N, mode):
    c = _case(ctx, make, inputs, mech, form, N, mode)
    for mean in ("mz", "md"):
        one = c[mean]["one"][STEPS]
        full = c[mean]["rec"][SPLITS[0]][0]
        assert full.shape == (3, STEPS + 1, c["start"].shape[1]) and np.all(np.isfinite(full))
        for n in SPLITS:
            traj, *outs = c[mean]["rec"][n]
            assert len(outs) == len(one)
            for k, (a, w) in enumerate(zip(outs, one)):
                assert _same(a, w), (mean, n, k, a, w)
            assert _same(traj, full), (mean, n)
        for name in ("sparse", "early", "none"):  # what is recorded changes no output
            for k, (a, w) in enumerate(zip(c[mean][name][1:], one)):
                assert _same(a, w), (mean, name, k)
        if form == "max":
            assert np.all(one[2] == 0)  # nothing stopped: the records are a trajectory


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("mech,form,N", CASES)
def test_records_are_the_one_launch_states(ctx, make, inputs, mech, form, N, mode):
    c = _case(ctx, make, inputs, mech, form, N, mode)
    for mean in ("mz", "md"):
        full = c[mean]["rec"][0][0]
        assert _same(full[:, 0], c["start"]), mean  # record 1
        pose, rates = _pose_rates(form, full)
        # the MeanZero maximal kernel leaves the solution unset at steps = 0 (its comment): k from 1
        for k in range(1 if (form == "max" and mean == "mz") else 0, STEPS):
            fp, fr = _pose_rates(form, c[mean]["one"][k][0])
            assert np.array_equal(fp, pose[:, k + 1]), (mean, k, "pose of record k + 2")    # 0-based row k + 1
            assert np.array_equal(fr, rates[:, k]), (mean, k, "rates of record k + 1")


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("mech,form,N", CASES)
def test_sparse_records_are_rows_of_the_full_record(ctx, make, inputs, mech, form, N, mode):
    c = _case(ctx, make, inputs, mech, form, N, mode)
    for mean in ("mz", "md"):
        full = c[mean]["rec"][0][0]
        assert _same(c[mean]["sparse"][0], full[:, np.array(SPARSE) - 1]), mean
        assert _same(c[mean]["early"][0], full[:, np.array(EARLY) - 1]), mean
        assert c[mean]["none"][0].shape == (3, 0, full.shape[2])


def test_per_trajectory_rec(ctx, make, inputs):
    """rec (T, R): each trajectory its own indices."""
    from gprx import data
    from gprx.projection import predictdynamics_rec

    c = _case(ctx, make, inputs, "P2", "max", 48, 1)
    import gprx

    ctx.set_dist_mode(1)
    X, Y = inputs["max.P2.X"][:, :48] / make.SCALE, inputs["max.P2.Y"][:, :48] / make.SCALE
    G = Y.shape[0]
    b = gprx.GPBatch(2 * G, X.shape[0], 48, 0, ctx=ctx)
    b.set_train(X, np.concatenate([Y, Y]))
    assert np.all(b.run(np.repeat(inputs["max.P2.theta"], G, axis=0), grad=False)["status"] == 0)
    groups = [[(b, k * G + j) for j in range(G)] for k in range(2)]
    rec = np.array([[1, 2, 3], [5, 6, 7], [2, 2, 7]])
    traj, out, pe, st = predictdynamics_rec("P2", groups, c["start"], STEPS, data.VW_INDICES["P2"], rec, steps_per_launch=2,
                                            traj_group=make.TRAJ_GROUP, ctx=ctx)
    b.close()
    full = c["mz"]["rec"][0][0]
    for t in range(3):
        assert _same(traj[t], full[t, rec[t] - 1]), t
    assert _same(out, c["mz"]["one"][STEPS][0])


# ------------------------------------------------------------------------------ a trajectory that stops
def test_failed_physics_mean_stops_only_its_trajectory(ctx):
    """tests/test_md_rollout.py's failing input: |w| = 250 > 2 / dt on body 1 of the double pendulum, the
    physics step's sqrt(4 / dt^2 - w.w) is not finite (status 2, the documented route).  The step that
    fails is the first: record 1 (the start as given) is kept, every later one is NaN."""
    import gprx
    from gprx import data, mdynamics
    from gprx.projection import predictdynamics_md, predictdynamics_md_rec
    from gprx.rollout import rollout_min_md, rollout_min_md_rec

    mech, N, steps = "P2", 48, 5
    for form, bad_at in (("max", 10), ("min", 1)):
        seed = data.trial_seed(mech, 5)
        if form == "max":
            tr = data.make_trial(mech, N, 3, seed=seed)
            th, start = data.theta0(mech, 64), tr["Xs"].T.copy()
            mu = mdynamics.mean_max(mech, tr["X"], ctx=ctx)
        else:
            tr = data.make_trial_min(mech, N, 3, seed=seed, usesin=False)
            th, start = data.theta0_min(mech, 64, False), tr["start"].copy()
            mu = mdynamics.mean_min(mech, tr["X"], False, ctx=ctx)
        G = tr["Y"].shape[0]
        b = gprx.GPBatch(G, tr["X"].shape[0], N, 0, ctx=ctx)
        b.set_train(tr["X"], tr["Y"] - mu)
        assert np.all(b.run(np.tile(th, (G, 1)), grad=False)["status"] == 0)
        g0 = [[(b, g) for g in range(G)]]
        mixed = start.copy()
        mixed[1, bad_at] = 250.0
        if form == "max":
            vwi = data.VW_INDICES[mech]
            one = predictdynamics_md(mech, g0, mixed, steps, vwi, ctx=ctx)
            got = {n: predictdynamics_md_rec(mech, g0, mixed, steps, vwi, steps_per_launch=n, ctx=ctx) for n in (1, 2, 0)}
            clean = predictdynamics_md_rec(mech, g0, start, steps, vwi, steps_per_launch=2, ctx=ctx)
        else:
            one = rollout_min_md(mech, g0, mixed, steps, False, ctx=ctx)
            got = {n: rollout_min_md_rec(mech, g0, mixed, steps, None, False, steps_per_launch=n, ctx=ctx) for n in (1, 2, 0)}
            clean = rollout_min_md_rec(mech, g0, start, steps, None, False, steps_per_launch=2, ctx=ctx)
        b.close()
        st_at = 3 if form == "max" else 2  # status among (traj, *outputs)
        for n, (traj, *outs) in got.items():
            for a, w in zip(outs, one):
                assert _same(a, w), (form, n)
            assert outs[st_at - 1][1] == 2 and np.all(np.isnan(outs[0][1]))
            assert np.array_equal(traj[1, 0], mixed[1]) and np.all(np.isnan(traj[1, 1:])), (form, n)
            for t in (0, 2):  # the others: as without it
                assert np.array_equal(traj[t], clean[0][t]) and np.all(np.isfinite(traj[t])), (form, n, t)
                for a, w in zip(outs, clean[1:]):
                    assert np.array_equal(a[t], w[t]), (form, n, t)
                assert outs[st_at - 1][t] == 0


# ------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("mech,md", [("P2", False), ("CP", True)])
def test_records_match_the_oracle(ctx, mech, md, mode):
    """Records 1 .. steps + 1 are the states projection_oracle.predictdynamics hands its predict callback
    when run with steps + 1 steps, at tests/test_projection.py::test_device_max_rollout_matches_oracle's
    bound: 1e-9 max(1, |ref|), or 10 x the spread between the oracles of the two distance modes."""
    import gprx
    from gprx import data, mdynamics
    from gprx.projection import REGULARIZER, predictdynamics_md_rec, predictdynamics_rec
    from oracle import gp_oracle as O
    from oracle import projection_oracle as PO
    from oracle import vi_oracle as VO

    N, T, steps = 48, 3, STEPS
    ctx.set_dist_mode(mode)
    tr = data.make_trial(mech, N, T, seed=data.trial_seed(mech, 5))
    th, idx = data.theta0(mech, 64), data.VW_INDICES[mech]
    Y = tr["Y"] - mdynamics.mean_max(mech, tr["X"], ctx=ctx) if md else tr["Y"]
    G = Y.shape[0]
    b = gprx.GPBatch(G, tr["d"], N, 0, ctx=ctx)
    b.set_train(tr["X"], Y)
    assert np.all(b.run(np.tile(th, (G, 1)))["status"] == 0)
    f = predictdynamics_md_rec if md else predictdynamics_rec
    traj, out, pe, st = f(mech, [[(b, g) for g in range(G)]], tr["Xs"].T, steps, idx, steps_per_launch=4, ctx=ctx)[:4]
    b.close()
    assert np.all(st == 0)

    def oracle_run(dm):
        key = ("oracle", mech, md, dm)
        if key not in _CACHE:
            alphas = [O.lml(tr["X"], Y[g], th, dm)[2]["alpha"] for g in range(G)]
            il2, sf2, _, _ = O.kernel_params(th, tr["d"])
            rows = []
            for t in range(T):
                seen = []

                def predict(obs):
                    seen.append(np.array(obs, dtype=np.float64))
                    Ks = sf2 * np.exp(-O.weighted_r(O.dist_stack(tr["X"], obs[:, None], dm), il2) * 0.5)[:, 0]
                    mu = np.array([Ks @ a for a in alphas])
                    if md:
                        s, sol = VO.vi_step(mech, obs)
                        assert sol.success and np.all(np.isfinite(s))
                        mu = mu + s[np.asarray(idx) - 1]
                    return mu

                PO.predictdynamics(mech, predict, tr["Xs"][:, t], steps + 1, idx, regularizer=REGULARIZER[mech])
                assert len(seen) == steps + 1
                rows.append(np.stack(seen))
            _CACHE[key] = np.stack(rows)
        return _CACHE[key]

    ref, alt = oracle_run(mode), oracle_run(1 - mode)
    tol = np.maximum(1e-9 * np.maximum(1.0, np.abs(ref)), 10 * np.abs(ref - alt))
    print(mech, md, mode, "max |traj - ref| / tol", float(np.max(np.abs(traj - ref) / tol)), "spread",
          float(np.max(np.abs(ref - alt))))
    assert np.all(np.isfinite(traj))
    assert np.all(np.abs(traj - ref) <= tol), float(np.max(np.abs(traj - ref) / tol))
