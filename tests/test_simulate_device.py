"""gprx_simulate (k_simulate through gprx.projection.simulate): many variational-integrator steps per
launch with per-trajectory bodies and friction.  One step against the 70-digit fixtures of
tests/test_hp_sim.py at their bound; S steps against S chained calls of one step and against other
launch lengths, bit for bit; nominal parameters against the existing stepwise path; the recording
rules; failure isolation.  T <= 8 trajectories and <= 400 steps throughout."""
import numpy as np
import pytest

import hp_sim as HS
from gprx import data, mdynamics, projection, vi
from oracle import hp_oracle as H

pytestmark = pytest.mark.gpu
MECHS = ("P1", "P2", "CP", "FB")
S_STEPS = 37
T = 6


@pytest.fixture(scope="module")
def ctx():
    import gprx

    c = gprx.Context(0)
    yield c
    c.close()


def _case(mech):
    """T noise-free generator states with their own perturbed bodies and friction."""
    nb = projection.NBODIES[mech]
    rng = np.random.default_rng(30 + MECHS.index(mech))
    S = data.make_trial(mech, 2, T, seed=5, noise=False)["Xs"].T.copy()
    ms, Js, cs = [], [], []
    for _ in range(T):
        m, J = vi.body_params(mech, 1 + 0.1 * rng.uniform(-1, 1, nb), 1 + 0.1 * rng.uniform(-1, 1, nb))
        ms.append(m)
        Js.append(J)
        cs.append(vi.friction_damp(mech, rng.uniform(0, 1, nb) * np.asarray(HS.FRICTION_MAX[mech])))
    return S, np.stack(ms), np.stack(Js), np.stack(cs)


@pytest.fixture(scope="module")
def full(ctx):
    """Per mechanism: the case and its whole recorded trajectory (every index 1 .. S_STEPS + 1), computed
    once and left unchanged."""
    out = {}
    for mech in MECHS:
        S, m, J, c = _case(mech)
        rec, st = projection.simulate(mech, S, S_STEPS, np.arange(1, S_STEPS + 2), m, J, c, ctx=ctx)
        rec.setflags(write=False)
        out[mech] = (S, m, J, c, rec, st)
    return out


@pytest.mark.parametrize("mech", MECHS)
def test_one_step_against_the_high_precision_truth(ctx, mech):
    """steps = 1 on the fixtures of tests/test_hp_sim.py, at the bound fixed there from the CPU."""
    fx = HS.load(mech)
    nb = projection.NBODIES[mech]
    out, st = projection.simulate(mech, fx["cstates"], 1, [1, 2], fx["mass"], fx["inertia"], fx["damp"], dt=float(fx["dt"]), ctx=ctx)
    np.testing.assert_array_equal(out[:, 0], fx["cstates"])  # index 1 is the start
    assert np.all(st == 0)
    k = HS.k_of(mech)
    for ci in range(len(fx["cases"])):
        err = float(np.max(np.abs(out[ci, 1].reshape(nb, 13)[:, 7:13].reshape(-1) - fx["truth"][ci])))
        bound = float(H.bound(fx["E"][ci], fx["A"][ci], k))
        print(f"{mech} {fx['cases'][ci]}: device error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (mech, ci, err, bound)


@pytest.mark.parametrize("mech", MECHS)
def test_many_steps_are_chained_single_steps_bit_for_bit(ctx, mech, full):
    S, m, J, c, rec, st = full[mech]
    np.testing.assert_array_equal(rec[:, 0], S)
    cur, flags = S, np.zeros(T, dtype=np.int32)
    for k in range(S_STEPS):  # the host carries the state
        nxt, s1 = projection.simulate(mech, cur, 1, [2], m, J, c, ctx=ctx)
        cur = nxt[:, 0]
        flags |= s1
        np.testing.assert_array_equal(cur, rec[:, k + 1])
    np.testing.assert_array_equal(flags, st)
    assert np.all(np.isfinite(rec))
    for spl in (1, 7, 1024):  # the launches' length does not show
        r2, s2 = projection.simulate(mech, S, S_STEPS, np.arange(1, S_STEPS + 2), m, J, c, steps_per_launch=spl, ctx=ctx)
        np.testing.assert_array_equal(r2, rec)
        np.testing.assert_array_equal(s2, st)
    # the step is the host restatement's (same equations, both solved to 1e-10)
    h, _, hs = vi.vi_step(mech, S, m=m, J=J, damp=c)
    ok = hs == 0
    np.testing.assert_allclose(rec[ok, 1], h[ok], rtol=0, atol=1e-9)


@pytest.mark.parametrize("mech", MECHS)
def test_nominal_parameters_are_the_stepwise_path(ctx, mech):
    """NULL parameters, 21 steps, against the gprx_vi_step chain (mdynamics.simulate(steps=20): steps + 1
    physics steps) at tests/test_vi_device.py::test_device_baseline_simulation's tolerance."""
    S = data.make_trial(mech, 2, 8, seed=5)["Xs"].T
    fin, bad = mdynamics.simulate(mech, S, 20, ctx=ctx)
    out, st = projection.simulate(mech, S, 21, [22], ctx=ctx)
    np.testing.assert_array_equal(st, bad)
    ok = bad == 0
    np.testing.assert_allclose(out[ok, 0], fin[ok], rtol=0, atol=1e-8)
    print(f"{mech}: bit-identical to the stepwise path: {np.array_equal(out[:, 0], fin)}")
    # and with the nominal values handed over explicitly
    m, J = vi.body_params(mech)
    out2, st2 = projection.simulate(mech, S, 21, [22], m, J, vi.friction_damp(mech), ctx=ctx)
    np.testing.assert_array_equal(out2, out)
    np.testing.assert_array_equal(st2, st)


@pytest.mark.parametrize("mech", ("P2", "FB"))
def test_recording(ctx, mech, full):
    S, m, J, c, rec, st = full[mech]
    last = S_STEPS + 1
    for idx in ([1, 5, 5, last], [last], [3, 3, 3, 4], [1]):
        out, s = projection.simulate(mech, S, S_STEPS, idx, m, J, c, ctx=ctx)
        np.testing.assert_array_equal(out, rec[:, np.asarray(idx) - 1])
    # per-trajectory lists: one trajectory ends early, the others do not notice
    lists = np.tile(np.array([2, 9, 20, last], dtype=np.int32), (T, 1))
    lists[2] = [1, 2, 2, 3]
    out, s = projection.simulate(mech, S, S_STEPS, lists, m, J, c, ctx=ctx)
    for t in range(T):
        np.testing.assert_array_equal(out[t], rec[t, lists[t] - 1])
    np.testing.assert_array_equal(np.delete(s, 2), np.delete(st, 2))


def test_invalid_arguments(ctx):
    import gprx._lib as L

    S = data.make_trial("P2", 2, 2, seed=5)["Xs"].T
    for bad in ([0, 1], [3, 2], [1, 7]):  # below 1, decreasing, beyond steps + 1
        with pytest.raises(L.GPRXError) as e:
            projection.simulate("P2", S, 5, bad, ctx=ctx)
        assert e.value.status == L.INVALID_ARGUMENT
    with pytest.raises(L.GPRXError):
        projection.simulate("P2", S, -1, [1], ctx=ctx)
    out, st = projection.simulate("P2", S, 0, [1, 1], ctx=ctx)  # no step: the start, twice
    np.testing.assert_array_equal(out, np.stack([S, S], axis=1))
    assert L.lib.gprx_simulate(ctx.h, 2, 0.01, 5, 0, None, None, None, None, 0.0, 100, 1e-10, 1, None, 0, None, None) == L.OK


@pytest.mark.parametrize("mech", ("P2", "FB"))
def test_failed_trajectory_is_isolated(ctx, mech, full):
    """|w| beyond 2/dt at the start (a non-finite input: ConstrainedDynamics' sqrt throws): status 2, the
    start recorded, NaN afterwards; the launch's other trajectories are bit-identical to a launch
    without it (tests/test_vi_device.py::test_failed_state_is_isolated_on_the_device's pattern)."""
    S, m, J, c, rec, st = full[mech]
    bad = S.copy()
    bad[1, 10:13] = 1e3 / vi.DT
    out, s = projection.simulate(mech, bad, S_STEPS, np.arange(1, S_STEPS + 2), m, J, c, ctx=ctx)
    assert s[1] == 2 and np.isnan(out[1, 1:]).all()
    np.testing.assert_array_equal(out[1, 0], bad[1])
    keep = [0] + list(range(2, T))
    np.testing.assert_array_equal(out[keep], rec[keep])
    np.testing.assert_array_equal(s[keep], st[keep])


@pytest.mark.parametrize("mech", ("P1", "P2", "CP"))
def test_a_stagnated_solve_ends_at_the_rounding_floor(ctx, mech):
    """dt = 1e-4, eps = 1e-10: newton!'s test cannot hold (the multipliers' rounding floor is ~1e-8); the step
    ends by the stagnation rule at the twist the host reaches with the same rule and, after all
    100 iterations, without it (steps below eps = 1e-10 apart: compared at 10 eps)."""
    S = data.make_trial(mech, 2, T, seed=9, noise=False)["Xs"].T
    out, st = projection.simulate(mech, S, 1, [2], dt=1e-4, ctx=ctx)
    full, it, hs = vi.vi_step(mech, S, dt=1e-4)
    cut, it2, hs2 = vi.vi_step(mech, S, dt=1e-4, stall_stop=True)
    assert np.any(it == 100) and np.all(it2 <= 12)
    assert np.all(st != 2)  # 0 or 1: which side of eps the last |ds| falls on is the rounding's to decide
    np.testing.assert_allclose(out[:, 0], cut, rtol=0, atol=1e-9)
    np.testing.assert_allclose(out[:, 0], full, rtol=0, atol=1e-9)
