"""gprx.energy, examples/energy.jl restated: the energy and explicit Euler by hand, and on the device
the GP rollout's recorded (θ, ω) series against the one-launch rollout on the same GPs."""
import math

import numpy as np
import pytest


def test_energy_by_hand():
    from gprx import energy as E

    # I = m l^2 / 12 + m (l / 2)^2 = 1 / 3;  E = m g l / 2 (1 - cos θ) + I ω^2 / 2
    assert E.I_S == pytest.approx(1 / 3, rel=1e-15)
    assert float(E.energy(0.0, 0.0)) == 0.0
    assert float(E.energy(math.pi / 2, 0.0)) == pytest.approx(9.81 * 0.5, rel=1e-15)
    assert float(E.energy(0.0, 3.0)) == pytest.approx(1.5, rel=1e-15)
    assert float(E.energy(0.3, 0.5)) == pytest.approx(4.905 * (1 - math.cos(0.3)) + 0.25 / 6, rel=1e-15)
    e = E.relative_error(np.array([math.pi / 2, 0.0]), np.array([0.0, 0.0]), math.pi / 2)
    assert e.tolist() == [0.0, 100.0]


def test_explicit_euler_two_steps_by_hand():
    """From (π/2, 0) with Δt = 0.01: both increments use the old state.  Step 1: Δθ = 0, Δω = -1.5 g
    sin(π/2) Δt = -0.14715.  Step 2: Δθ = -0.14715 Δt, Δω = -1.5 g sin(π/2) Δt again (θ has not moved)."""
    from gprx import energy as E

    th, om = E.explicit_euler(2, 0.01, math.pi / 2, 0.0)
    d = -1.5 * 9.81 * 0.01
    assert th.tolist() == [math.pi / 2, math.pi / 2 + d * 0.01]
    assert om.tolist() == [d, d + d]
    th, om = E.explicit_euler(2, 0.1, 0.0, 1.0)  # from the bottom with ω = 1: no torque in step 1
    assert th.tolist() == [0.1, 0.2] and om[0] == 1.0
    assert om[1] == 1.0 + -1.5 * math.sin(0.1) * 9.81 / 1.0 * 0.1


@pytest.mark.gpu
def test_gp_variational_integration_records_the_rollout():
    """steps = 50 from rest at π/2, 20 samples of a swing simulated at Δt = 1e-3 (2000 steps): finite
    (θ, ω) of length 50, and the last recorded ω is, bit for bit, the final state's ω of the one-launch
    predictdynamics over 50 steps on the same GPs.  The drift itself is not bounded: nobody has
    measured it."""
    import gprx
    from gprx import energy as E
    from gprx.projection import predictdynamics

    ctx = gprx.Context(0)
    theta, steps = math.pi / 2, 50
    b = E.pendulum_gps(theta, 20, 1, 1e-3, ctx)
    th, om = E.gp_variational_integration(steps, theta, 20, 1, 1e-3, ctx, batch=b)
    assert th.shape == (steps,) and om.shape == (steps,)
    assert np.all(np.isfinite(th)) and np.all(np.isfinite(om))
    fin, _, st = predictdynamics("P1", [[(b, g) for g in range(3)]], E.rest_cstate(theta), steps, E.VW_INDICES, ctx=ctx)
    assert st[0] == 0 and om[-1] == fin[0, 10]
    th2, om2 = E.gp_variational_integration(steps, theta, 20, 1, 1e-3, ctx, batch=b, steps_per_launch=7)
    assert np.array_equal(th, th2) and np.array_equal(om, om2)
    print("relative energy error % after 50 steps: GP", float(E.relative_error(th, om, theta)[-1]), "Euler",
          float(E.relative_error(*E.explicit_euler(steps, 0.01, theta, 0.0), theta)[-1]))
    b.close()
    # fitted inside the call: the issue's signature
    th3, om3 = E.gp_variational_integration(steps, theta, 20, 1, 1e-3, ctx)
    assert th3.shape == (steps,) and np.all(np.isfinite(th3)) and np.all(np.isfinite(om3))
    ctx.close()
