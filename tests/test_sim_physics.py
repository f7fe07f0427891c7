"""The external force and the per-trajectory bodies of the variational-integrator step
(gprx/vi.py vi_step(m=, J=, damp=), what gprx_simulate's step is compared with), pinned physically on
the pendulum P1 -- ConstrainedDynamics' source is absent, so the sign and the factor 2 of the torque
term, and where the mass and the inertia enter, are held to the rigid pendulum's own equation
    (J_xx + m l^2 / 4) w' = -m g (l / 2) sin(theta) - c w."""
import numpy as np
import pytest

from gprx import data, vi

L = 1.0
# (dm, dJ, c): nominal, a heavier body, a smaller inertia, friction
PARAMS = ((1.0, 1.0, 0.0), (1.1, 1.0, 0.0), (1.0, 0.9, 0.0), (1.0, 1.0, 1.0))


def _wdot(th, om, m, Jxx, c):
    return -(m * vi.GRAV * L / 2 * np.sin(th) + c * om) / (Jxx + m * L * L / 4)


@pytest.mark.parametrize("dm,dJ,c", PARAMS)
def test_one_step_is_the_damped_pendulum(dm, dJ, c):
    """w2 - w1 = dt w'(theta, w1) + O(dt^2) with a stable constant: the tolerance form of
    tests/test_vi.py::test_pendulum_continuous_time_limit.  A torque entering once instead of twice,
    or with the other sign, or a mass or inertia not reaching the rows, is an O(dt) error, whose ratio
    to dt^2 doubles from one dt to the next."""
    rng = np.random.default_rng(0)
    th, om = rng.uniform(-3, 3, 100), rng.uniform(-2, 2, 100)
    X = data._cstates("P1", dict(th=th, om=om))
    m, J = vi.body_params("P1", dm, dJ)
    ratios = []
    for dt in (0.01, 0.005, 0.0025):
        s, _, st = vi.vi_step("P1", X.T, dt=dt, m=m, J=J, damp=vi.friction_damp("P1", c))
        assert np.all(st == 0)
        ratios.append(np.max(np.abs(s[:, 10] - (om + dt * _wdot(th, om, m[0], J[0, 0, 0], c)))) / dt ** 2)
    print(f"dm {dm} dJ {dJ} c {c}: |error| / dt^2 = {ratios}")
    assert max(ratios) < 50 and max(ratios) / min(ratios) < 1.1


def test_half_or_reversed_torque_would_fail_the_one_step_test():
    """What the test above rejects: the same comparison against the pendulum with c / 2 or -c."""
    rng = np.random.default_rng(0)
    th, om = rng.uniform(-3, 3, 100), rng.uniform(-2, 2, 100)
    X = data._cstates("P1", dict(th=th, om=om))
    m, J = vi.body_params("P1")
    for wrong in (0.5, -1.0):
        ratios = []
        for dt in (0.01, 0.005, 0.0025):
            s, _, _ = vi.vi_step("P1", X.T, dt=dt, damp=vi.friction_damp("P1", 1.0))
            ratios.append(np.max(np.abs(s[:, 10] - (om + dt * _wdot(th, om, m[0], J[0, 0, 0], wrong)))) / dt ** 2)
        assert max(ratios) > 50 and max(ratios) / min(ratios) > 1.5


def _energy(S, m, J):
    c = S.reshape(S.shape[0], 1, 13)
    v, w = c[:, 0, 7:10], c[:, 0, 10:13]
    return 0.5 * m[0] * np.sum(v * v, axis=1) + 0.5 * np.einsum("ti,ij,tj->t", w, J[0], w) + m[0] * vi.GRAV * c[:, 0, 2]


def test_friction_dissipates_c_w_squared():
    """2000 steps at dt = 1e-4 with c = 1: the energy falls by c sum(w1^2) dt to 1% (the integrator's
    own error is O(dt x rates <~ 10 / s) ~ 1e-3; a wrong factor or sign is off by >= 50%).
    Measured on this restatement: relative deviations 1.1e-04 .. 5.0e-03 over the 8 starts, an absolute
    ~1e-3 J whatever the work (0.16 .. 1.36 J): the O(dt)-level ripple of the energy read from (v1, w1).
    eps = 1e-7: at dt = 1e-4 the multipliers' rounding floor, (m / dt) (1e-16 / dt) ~ 1e-8, keeps |ds|
    above newton!'s 1e-10 and every step would run all its iterations."""
    rng = np.random.default_rng(2)
    dt, c = 1e-4, 1.0
    S = np.concatenate([_start(th, om) for th, om in zip(rng.uniform(-2, 2, 8), rng.uniform(1, 3, 8) * rng.choice((-1, 1), 8))])
    m, J = vi.body_params("P1", 1.05, 0.95)
    damp = vi.friction_damp("P1", c)
    E0, work = _energy(S, m, J), np.zeros(8)
    for _ in range(2000):
        work += c * S[:, 10] ** 2 * dt
        S, _, st = vi.vi_step("P1", S, dt=dt, eps=1e-7, m=m, J=J, damp=damp)
        assert np.all(st == 0)
    dE = _energy(S, m, J) - E0
    rel = np.abs(dE + work) / work
    print(f"dE {dE}, -work {-work}, relative deviation {rel.min():.1e} .. {rel.max():.1e}")
    assert np.all(work > 0.05) and np.all(rel < 0.01)


def _start(th, om):
    from gprx import simdata

    return simdata.initial_cstate("P1", dict(th=th, om=om))


def test_energy_stays_bounded_with_perturbed_bodies():
    """tests/test_vi.py::test_energy_stays_bounded's bound (1000 steps of 10 ms, no friction) with dm = 1.1,
    dJ = 0.9: the discrete energy of the perturbed pendulum oscillates but does not drift."""
    tr = data.make_trial("P1", 8, 0, seed=3, noise=False)
    S = tr["X"].T
    m, J = vi.body_params("P1", 1.1, 0.9)
    E0 = _energy(S, m, J)
    Es = []
    for _ in range(1000):
        S, _, st = vi.vi_step("P1", S, m=m, J=J, damp=vi.friction_damp("P1", 0.0))
        assert np.all(st == 0)
        Es.append(_energy(S, m, J))
    Es = np.array(Es)
    scale = 1.0 + np.abs(E0)
    assert np.max(np.abs(Es - E0) / scale) < 0.1
    drift = np.abs(Es[-200:].mean(axis=0) - Es[:200].mean(axis=0)) / scale
    assert np.max(drift) < 0.03


def test_defaults_are_the_nominal_step_bit_for_bit():
    """m, J, damp left out, given as the nominal values, or per trajectory: the same bits."""
    for mech in ("P1", "P2", "CP", "FB"):
        S = data.make_trial(mech, 5, 0, seed=1)["X"].T
        ref = vi.vi_step(mech, S)
        m, J = vi.body_params(mech)
        np.testing.assert_array_equal(m, vi.MECHANISMS[mech]["m"])
        np.testing.assert_array_equal(J, np.stack(vi.MECHANISMS[mech]["J"]))
        for kw in (dict(m=m, J=J), dict(m=np.tile(m, (5, 1)), J=np.tile(J, (5, 1, 1, 1)), damp=np.zeros((5, len(m), 6)))):
            out = vi.vi_step(mech, S, **kw)
            for a, b in zip(out, ref):
                np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mech", ("P1", "P2", "CP"))
def test_stagnation_stop_ends_a_solve_at_the_rounding_floor(mech):
    """At dt = 1e-4 the multipliers' rounding floor (m/dt)(1e-16/dt) ~ 1e-8 lies above eps = 1e-10: newton!'s
    test cannot hold and the solve runs all its iterations; stall_stop (gprx_simulate's rule) ends it once
    the residual and the twist's step are below eps and |ds| no longer falls, at the same twist -- two
    solutions of one system whose steps are below eps = 1e-10, compared at 10 eps.  At dt = 0.01, where
    newton!'s test holds, the rule changes nothing."""
    S = data.make_trial(mech, 2, 6, seed=9, noise=False)["Xs"].T
    full, it, st = vi.vi_step(mech, S, dt=1e-4)
    cut, it2, st2 = vi.vi_step(mech, S, dt=1e-4, stall_stop=True)
    assert np.any(it == 100) and np.all(it2 <= 12)
    np.testing.assert_array_equal(st2[st == 1], 1)
    np.testing.assert_allclose(cut, full, rtol=0, atol=1e-9)
    for a, b in zip(vi.vi_step(mech, S), vi.vi_step(mech, S, stall_stop=True)):
        np.testing.assert_array_equal(a, b)
