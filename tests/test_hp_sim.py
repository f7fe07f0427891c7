"""The variational-integrator step with per-trajectory bodies and friction (gprx/vi.py vi_step(m=, J=,
damp=), the host restatement gprx_simulate's step is compared with) against the 70-digit truth of
tests/hp_sim.py, which subclasses oracle/hp_physics._Step: per mechanism one generator state with
nominal bodies and one with dm, dJ at their +-10% extremes and the largest friction draw.  Bound:
hp_oracle.bound(E, A, k), E the geometric mean of the two fp64 CPU evaluations' errors ("lapack": vi_step
as it stands; "rev": the bodies reversed), A the largest operand of the last s - ds, k of
tests/golden/hp_phys_<mech>.npz -- fixed when tests/golden/make_golden_hp_sim.py wrote the fixtures,
from the CPU alone.  tests/test_simulate_device.py holds the device's one-step result to the same
fixtures and bound."""
import numpy as np
import pytest

import hp_sim as S
from oracle import hp_oracle as H

MECHS = ("P1", "P2", "CP", "FB")


@pytest.mark.parametrize("mech", MECHS)
def test_fixtures_are_the_cases_and_hold_the_cpu_evaluations(mech):
    fx = S.load(mech)
    k = S.k_of(mech)
    assert k >= 4
    for ci, (name, cs, m, J, damp) in enumerate(S.cases(mech)):
        assert fx["cases"][ci] == name
        for a, b in ((fx["cstates"][ci], cs), (fx["mass"][ci], m), (fx["inertia"][ci], J), (fx["damp"][ci], damp)):
            np.testing.assert_array_equal(a, b)
        ev = S.evaluations(mech, cs, float(fx["dt"]), m, J, damp)
        bound = H.bound(fx["E"][ci], fx["A"][ci], k)
        for v, (s, it, st) in ev.items():
            err = float(np.max(np.abs(s - fx["truth"][ci])))
            print(f"{mech} {name} {v}: error {err:.3e}, bound {float(bound):.3e}, iterations {it}")
            assert st == 0 and err <= bound, (mech, name, v, err, bound)
    # the extreme case is one: the parameters and the friction do move the solution
    assert np.all(fx["damp"][0] == 0) and np.any(fx["damp"][1] != 0) and np.all(fx["mass"][0] == 1) and np.all(fx["mass"][1] != 1)


@pytest.mark.parametrize("mech,ci", (("P1", 1), ("CP", 1), ("P2", 0)))
def test_truth_is_reproduced(mech, ci):
    """The stored truth is what the high-precision step gives today (the four-bar's takes several
    seconds: make_golden_hp_sim.py regenerates it byte for byte)."""
    fx = S.load(mech)
    name, cs, m, J, damp = S.cases(mech)[ci]
    ev = S.evaluations(mech, cs, float(fx["dt"]), m, J, damp)
    tr = S.truth(mech, cs, float(fx["dt"]), ev["lapack"][0], m, J, damp)
    np.testing.assert_array_equal(tr["s"], fx["truth"][ci])
    assert tr["A"] == fx["A"][ci]


@pytest.mark.parametrize("mech", MECHS)
def test_a_torque_entering_once_is_rejected(mech):
    """The seeded fault: tau instead of 2 tau in the rotational row (hp_sim.half_torque)."""
    fx = S.load(mech)
    name, cs, m, J, damp = S.cases(mech)[1]
    ev = S.evaluations(mech, cs, float(fx["dt"]), m, J, S.half_torque(damp))
    bound = float(H.bound(fx["E"][1], fx["A"][1], S.k_of(mech)))
    err = float(np.max(np.abs(ev["lapack"][0] - fx["truth"][1])))
    print(f"{mech}: faulty error {err:.3e}, bound {bound:.3e}")
    assert err > 1e3 * bound
