"""The device's two physics solves (k_project / project<NW>, k_vi_step / vi_newton, the shared
lu_solve) against the high-precision truth of tests/golden/hp_phys_<mech>.npz (oracle/hp_physics.py),
and the parts of gprx_projectv's / gprx_vi_step's contract that ran in no test: newton_iter and
eps, dt other than 0.01, T = 0 / 1 / 4097, the singular KKT matrix (status 1, also in
gprx_rollout_max), a non-finite system in projectv, and the 4-wave projection inside
k_rollout_max bit for bit against the 1-wave k_project.

Bound (elementwise on the twists v, w): |device - truth| <= k max(E, eps A), E, A and k from the
fixtures, i.e. from the fp64 CPU variants alone (make_golden_hp_physics.py).  Nothing here is fitted to the
device.  Every test prints `mech case quantity err_device E ratio` (ratio = err / max(E, eps A);
within the bound iff <= k).  Iteration counts: within 1 of the dgetf2-order variant's, except on
the four-bar, whose regularised iteration stalls differently on either side (printed only), as in
test_projection.py.
Each mechanism and entry point runs once per dt for the truth (the `dev` record); the other tests
launch a handful of single-wave solves each.
"""
import numpy as np
import pytest

from oracle import hp_physics as HP

pytestmark = pytest.mark.gpu
MECHS = HP.MECHS
DGETF2 = HP.VARIANTS.index("dgetf2")
NONFINITE_STATUS = 0  # what k_project answers for a non-finite system (include/gprx.h, gprx_projectv)


@pytest.fixture(scope="module")
def fxs(golden_dir):
    out = {}
    for mech in MECHS:
        with np.load(golden_dir / f"hp_phys_{mech}.npz") as z:
            out[mech] = {k: z[k] for k in z.files}
    return out


@pytest.fixture(scope="module")
def ctx():
    import gprx

    c = gprx.Context(0)
    yield c
    c.close()


def by_dt(fx):
    return [(float(dt), np.nonzero(fx["dt"] == dt)[0]) for dt in np.unique(fx["dt"])]


@pytest.fixture(scope="module")
def dev(fxs, ctx):
    """{mech: {"pj" | "vi": (twists (ncase, 6 nb), iterations, status, full output rows)}}: every
    fixture case at its dt, one launch per dt."""
    import gprx.projection as GP

    rec = {}
    for mech, fx in fxs.items():
        n, nb = len(fx["dt"]), HP.nbodies(mech)
        pj = [np.empty((n, 6 * nb)), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), None]
        vi = [np.empty((n, 6 * nb)), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty((n, 13 * nb))]
        for dt, ix in by_dt(fx):
            o, it, st = GP.projectv(mech, fx["cstates"][ix], fx["vw_pred"][ix], dt=dt, ctx=ctx)
            pj[0][ix], pj[1][ix], pj[2][ix] = o, it, st
            o, it, st = GP.vi_step(mech, fx["vi_states"][ix], dt=dt, ctx=ctx)
            vi[0][ix], vi[1][ix], vi[2][ix], vi[3][ix] = twists(o, nb), it, st, o
        rec[mech] = dict(pj=tuple(pj), vi=tuple(vi))
    return rec


def twists(out, nb):
    o = np.asarray(out).reshape(-1, nb, 13)
    return o[:, :, 7:13].reshape(o.shape[0], 6 * nb)


def held(mech, fx, what, got, truth, E, A, label=None):
    """Prints the table rows and returns the cases beyond k max(E, eps A)."""
    k, bad = float(fx["k"]), []
    for c in range(len(E)):
        err = np.abs(got[c] - truth[c])
        r = HP.ratio(err, E[c], A[c])
        print(f"{mech} {c}:{fx['kinds'][c]}@{fx['dt'][c]:g} {label or what} err {np.max(err):.3e} E {E[c]:.3e} ratio {r:.2f}")
        if not np.all(err <= HP.H.bound(E[c], A[c], k)):
            bad.append((c, float(np.max(err)), r))
    return bad


# ---- the truth --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mech", MECHS)
def test_projectv_against_the_truth(fxs, dev, mech):
    fx = fxs[mech]
    out, it, st, _ = dev[mech]["pj"]
    assert np.all(st == 0)
    print(f"{mech} projectv iterations: device {it.tolist()}, dgetf2 variant {fx['pj_its'][:, DGETF2].tolist()}")
    bad = held(mech, fx, "projectv", out, fx["pj_truth"], fx["pj_E"], fx["pj_A"])
    assert not bad, bad
    if mech != "FB":
        assert np.max(np.abs(it - fx["pj_its"][:, DGETF2])) <= 1


@pytest.mark.parametrize("mech", MECHS)
def test_vi_step_against_the_truth(fxs, dev, mech):
    fx = fxs[mech]
    out, it, st, rows = dev[mech]["vi"]
    assert np.all(st == 0) and np.all(np.isfinite(rows))
    print(f"{mech} vi_step iterations: device {it.tolist()}, dgetf2 variant {fx['vi_its'][:, DGETF2].tolist()}")
    bad = held(mech, fx, "vi_step", out, fx["vi_truth"], fx["vi_E"], fx["vi_A"])
    assert not bad, bad
    if mech != "FB":
        assert np.max(np.abs(it - fx["vi_its"][:, DGETF2])) <= 1


# ---- newton_iter and eps ----------------------------------------------------------------------------
def _pose2(mech, states, dt):
    """The discrete pose columns of the solution CState as the host restatement forms them."""
    nb = HP.nbodies(mech)
    c = np.asarray(states).reshape(-1, nb, 13)
    return c[..., 0:3] + c[..., 7:10] * dt, HP.VI.step_q(c[..., 3:7], c[..., 10:13], dt)


@pytest.mark.parametrize("mech", MECHS)
def test_newton_iter_zero(fxs, ctx, mech):
    import gprx.projection as GP

    fx, nb = fxs[mech], HP.nbodies(mech)
    for dt, ix in by_dt(fx):
        o, it, st = GP.projectv(mech, fx["cstates"][ix], fx["vw_pred"][ix], newton_iter=0, dt=dt, ctx=ctx)
        np.testing.assert_array_equal(o, fx["vw_pred"][ix])
        assert not it.any() and not st.any()
        o, it, st = GP.vi_step(mech, fx["vi_states"][ix], newton_iter=0, dt=dt, ctx=ctx)
        assert np.all(st == 1) and not it.any()
        np.testing.assert_array_equal(twists(o, nb), twists(fx["vi_states"][ix], nb))
        x2, q2 = _pose2(mech, fx["vi_states"][ix], dt)
        np.testing.assert_array_equal(o.reshape(-1, nb, 13)[..., 0:3], x2)
        np.testing.assert_array_equal(o.reshape(-1, nb, 13)[..., 3:7], q2)


@pytest.mark.parametrize("mech", MECHS)
def test_newton_iter_one_and_two(fxs, ctx, mech):
    """The capped solves return the iteration's own iterate: held to the high-precision iterate by
    the bound the CPU variants' iterates give (pj_it_* / vi_it_* of the fixtures)."""
    import gprx.projection as GP

    fx, nb = fxs[mech], HP.nbodies(mech)
    bad = []
    for i, cap in enumerate(fx["iterates"]):
        cap = int(cap)
        pj, vi = np.empty_like(fx["pj_truth"]), np.empty_like(fx["vi_truth"])
        for dt, ix in by_dt(fx):
            o, it, st = GP.projectv(mech, fx["cstates"][ix], fx["vw_pred"][ix], newton_iter=cap, dt=dt, ctx=ctx)
            assert np.all(it == cap) and not st.any()
            pj[ix] = o
            o, it, st = GP.vi_step(mech, fx["vi_states"][ix], newton_iter=cap, dt=dt, ctx=ctx)
            assert np.all(it == cap) and np.all(st <= 1)
            vi[ix] = twists(o, nb)
        bad += held(mech, fx, "projectv", pj, fx["pj_it_truth"][i], fx["pj_it_E"][i], fx["pj_it_A"][i], f"projectv[iter={cap}]")
        bad += held(mech, fx, "vi_step", vi, fx["vi_it_truth"][i], fx["vi_it_E"][i], fx["vi_it_A"][i], f"vi_step[iter={cap}]")
    assert not bad, bad


@pytest.mark.parametrize("mech", MECHS)
def test_eps_zero_runs_every_iteration(fxs, ctx, mech):
    import gprx.projection as GP

    fx, nb = fxs[mech], HP.nbodies(mech)
    pj, vi = np.empty_like(fx["pj_truth"]), np.empty_like(fx["vi_truth"])
    for dt, ix in by_dt(fx):
        o, it, st = GP.projectv(mech, fx["cstates"][ix], fx["vw_pred"][ix], newton_iter=12, eps=0.0, dt=dt, ctx=ctx)
        assert np.all(it == 12) and not st.any()
        pj[ix] = o
        o, it, st = GP.vi_step(mech, fx["vi_states"][ix], newton_iter=12, eps=0.0, dt=dt, ctx=ctx)
        assert np.all(it == 12) and np.all(st == 1)
        vi[ix] = twists(o, nb)
    bad = held(mech, fx, "projectv", pj, fx["pj_truth"], fx["pj_E"], fx["pj_A"], "projectv[eps=0]")
    bad += held(mech, fx, "vi_step", vi, fx["vi_truth"], fx["vi_E"], fx["vi_A"], "vi_step[eps=0]")
    assert not bad, bad


@pytest.mark.parametrize("mech", MECHS)
def test_eps_huge_stops_after_one_iteration(fxs, ctx, mech):
    import gprx.projection as GP

    fx = fxs[mech]
    for dt, ix in by_dt(fx):
        _, it, st = GP.projectv(mech, fx["cstates"][ix], fx["vw_pred"][ix], eps=1e300, dt=dt, ctx=ctx)
        assert np.all(it == 1) and not st.any()
        _, it, st = GP.vi_step(mech, fx["vi_states"][ix], eps=1e300, dt=dt, ctx=ctx)
        assert np.all(it == 1) and not st.any()


# ---- sizes ------------------------------------------------------------------------------------------
def test_T_zero_writes_nothing(ctx):
    import gprx._lib as L
    from gprx.rollout import MECH

    out, it, st = np.full(26, 7.0), np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int32)
    cs = np.zeros(26)
    L.check(L.lib.gprx_projectv(ctx.h, MECH["P2"], 0.01, 0, L.dptr(cs), L.dptr(cs), 0.0, 100, 1e-10, L.dptr(out), L.iptr(it),
                                L.iptr(st)), ctx.h)
    L.check(L.lib.gprx_vi_step(ctx.h, MECH["P2"], 0.01, 0, L.dptr(cs), 0.0, 100, 1e-10, L.dptr(out), L.iptr(it), L.iptr(st)), ctx.h)
    L.check(L.lib.gprx_projectv(ctx.h, MECH["P2"], 0.01, 0, None, None, 0.0, 100, 1e-10, None, None, None), ctx.h)
    assert np.all(out == 7.0) and np.all(it == 7) and np.all(st == 7)


@pytest.mark.parametrize("mech", MECHS)
def test_T_one_and_4097_repeat_the_record(fxs, dev, ctx, mech):
    """A launch of one state, and 4097 states (the dt = 0.01 cases tiled): every row is bit-identical
    to the same case in the record's launch."""
    import gprx.projection as GP

    fx = fxs[mech]
    ix = np.nonzero(fx["dt"] == 0.01)[0]
    o, it, st = GP.projectv(mech, fx["cstates"][ix[:1]], fx["vw_pred"][ix[:1]], ctx=ctx)
    np.testing.assert_array_equal(o[0], dev[mech]["pj"][0][ix[0]])
    assert it[0] == dev[mech]["pj"][1][ix[0]] and st[0] == 0
    o, it, st = GP.vi_step(mech, fx["vi_states"][ix[:1]], ctx=ctx)
    np.testing.assert_array_equal(o[0], dev[mech]["vi"][3][ix[0]])
    assert it[0] == dev[mech]["vi"][1][ix[0]] and st[0] == 0
    rep = ix[np.arange(4097) % len(ix)]
    o, it, st = GP.projectv(mech, fx["cstates"][rep], fx["vw_pred"][rep], ctx=ctx)
    np.testing.assert_array_equal(o, dev[mech]["pj"][0][rep])
    np.testing.assert_array_equal(it, dev[mech]["pj"][1][rep])
    assert not st.any()
    o, it, st = GP.vi_step(mech, fx["vi_states"][rep], ctx=ctx)
    np.testing.assert_array_equal(o, dev[mech]["vi"][3][rep])
    np.testing.assert_array_equal(it, dev[mech]["vi"][1][rep])
    assert not st.any()


# ---- the singular KKT matrix (status 1) -------------------------------------------------------------
def _gen3(fx):
    """The first three dt = 0.01 generator cases: states and predicted twists."""
    return fx["cstates"][:3].copy(), fx["vw_pred"][:3].copy()


def _zero_last_quaternion(cs, nb):
    """An all-zero quaternion on the last body: q3 = 0, so the rotational rows of G that hold only
    that body's columns are exactly zero -- with regulariser 0 an exact zero pivot."""
    c = cs.copy().reshape(nb, 13)
    c[nb - 1, 3:7] = 0.0
    return c.reshape(-1)


@pytest.mark.parametrize("mech", MECHS)
def test_singular_state_is_isolated_in_projectv(fxs, ctx, mech):
    import gprx.projection as GP

    nb = HP.nbodies(mech)
    cs, su = _gen3(fxs[mech])
    good, git, gst = GP.projectv(mech, cs, su, ctx=ctx)
    bad = cs.copy()
    bad[1] = _zero_last_quaternion(cs[1], nb)
    out, it, st = GP.projectv(mech, bad, su, ctx=ctx)
    np.testing.assert_array_equal(out[[0, 2]], good[[0, 2]])
    np.testing.assert_array_equal(it[[0, 2]], git[[0, 2]])
    np.testing.assert_array_equal(st[[0, 2]], gst[[0, 2]])
    print(f"{mech} zero quaternion: status {st[1]}, iterations {it[1]}, row {out[1]}")
    if mech != "FB":  # the four-bar's regulariser 1e-10 keeps the pivot away from zero: the launch ends, no more is claimed
        assert st[1] == 1 and np.isnan(out[1]).all()


def _zero_mean_gps(mech, ctx, n=8):
    """G GPs on CState inputs with zero targets: alpha = 0, so every predicted mean is exactly 0."""
    import gprx
    import gprx.data as D

    tr = D.make_trial(mech, n, 0, seed=D.trial_seed(mech, 3))
    G = tr["Y"].shape[0]
    b = gprx.GPBatch(G, tr["d"], n, 0, ctx=ctx)
    b.set_train(tr["X"], np.zeros((G, n)))
    assert np.all(b.run(np.tile(D.theta0(mech, 64), (G, 1)))["status"] == 0)
    return b, G, D.VW_INDICES[mech]


def test_singular_projection_stops_its_rollout_alone(fxs, ctx):
    import gprx.projection as GP

    b, G, idx = _zero_mean_gps("P2", ctx)
    cs, _ = _gen3(fxs["P2"])
    good, gpe, gst = GP.predictdynamics("P2", [[(b, g) for g in range(G)]], cs, 3, idx, ctx=ctx)
    assert not gst.any() and np.all(np.isfinite(good))
    bad = cs.copy()
    bad[1] = _zero_last_quaternion(cs[1], 2)
    out, pe, st = GP.predictdynamics("P2", [[(b, g) for g in range(G)]], bad, 3, idx, ctx=ctx)
    assert st[1] == 1 and np.isnan(out[1]).all() and np.isnan(pe[1])
    np.testing.assert_array_equal(out[[0, 2]], good[[0, 2]])
    np.testing.assert_array_equal(pe[[0, 2]], gpe[[0, 2]])
    assert not st[[0, 2]].any()
    b.close()


# ---- a non-finite system in projectv -----------------------------------------------------------------
@pytest.mark.parametrize("mech", ("P2", "FB"))
def test_nonfinite_state_is_isolated_in_projectv(fxs, ctx, mech):
    """|w| = 250 > 2/dt on one body: sqrt(4/dt^2 - w.w) is NaN (the reference's sqrt throws a
    DomainError).  project<NW> has no finiteness test: the NaN system runs every iteration and the
    row comes back NaN with status NONFINITE_STATUS -- the contract include/gprx.h states."""
    import gprx.projection as GP

    nb = HP.nbodies(mech)
    cs, su = _gen3(fxs[mech])
    good, git, gst = GP.projectv(mech, cs, su, newton_iter=20, ctx=ctx)
    bad = cs.copy().reshape(3, nb, 13)
    bad[1, nb - 1, 10:13] = [250.0, 0.0, 0.0]
    out, it, st = GP.projectv(mech, bad.reshape(3, -1), su, newton_iter=20, ctx=ctx)
    print(f"{mech} |w| = 250: status {st[1]}, iterations {it[1]}, row {out[1]}")
    np.testing.assert_array_equal(out[[0, 2]], good[[0, 2]])
    np.testing.assert_array_equal(it[[0, 2]], git[[0, 2]])
    np.testing.assert_array_equal(st[[0, 2]], gst[[0, 2]])
    assert np.isnan(out[1]).all() and 0 <= it[1] <= 20
    assert st[1] == NONFINITE_STATUS and it[1] == 20  # the documented contract: every iteration runs


# ---- the 1-wave and the 4-wave projection -------------------------------------------------------------
@pytest.mark.parametrize("mech", MECHS)
def test_rollout_projection_equals_projectv_bit_for_bit(fxs, ctx, mech):
    """gprx_rollout_max with zero-mean GPs and steps = 1 projects the zero twist on 4 waves
    (project<4>) and hands it through updatestate! into the v, w slots of the final CState; k_project
    runs project<1> on the same start and prediction.  "Each element sees the same operations in the
    same order for any NW" (gprx_projection.hip): the two are bit-identical."""
    import gprx.projection as GP

    fx, nb = fxs[mech], HP.nbodies(mech)
    ix = np.nonzero((fx["dt"] == 0.01) & (fx["kinds"] != "rest") & (fx["kinds"] != "spin"))[0]
    cs = fx["cstates"][ix]
    b, G, idx = _zero_mean_gps(mech, ctx)
    out, pe, st = GP.predictdynamics(mech, [[(b, g) for g in range(G)]], cs, 1, idx, ctx=ctx)
    ref, it, rst = GP.projectv(mech, cs, np.zeros((len(ix), 6 * nb)), ctx=ctx)
    print(f"{mech} projection of the zero twist: iterations {it.tolist()}, status {rst.tolist()} / rollout {st.tolist()}")
    assert np.all(it >= 2) and not rst.any() and not st.any()
    np.testing.assert_array_equal(twists(out, nb), ref)
    b.close()
