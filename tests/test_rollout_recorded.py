"""The four device rollouts against recorded results: every output array of gprx_rollout_min,
gprx_rollout_min_md, gprx_rollout_max and gprx_rollout_max_md, statuses included, is bit for bit
what the library gave before the minimal-coordinate kernels, the host calls and the Python wrappers
were each stated once (tests/golden/rollouts_parent.npz, recorded from that build on an MI355X by
tests/golden/make_golden_rollouts.py, which documents the cases; the inputs are stored with the
results).  The GPs are fitted on the device here, so the evaluation before the rollout is held too.
Without a device: the four wrappers share their argument checks."""
import importlib.util

import numpy as np
import pytest


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def make(golden_dir):
    return _load(golden_dir / "make_golden_rollouts.py", "make_golden_rollouts")


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with np.load(golden_dir / "rollouts_parent.npz") as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def ctx():
    import gprx

    c = gprx.Context(0)
    yield c
    c.close()


def _cases():
    sizes = {"max": (48, 300), "min": (48, 300, 1100), "min_sin": (48, 300, 1100)}
    return [(mech, form, N) for form in sizes for mech in ("P1", "P2", "CP", "FB") for N in sizes[form]]


def test_the_cases_are_the_recorded_ones(make, recorded):
    assert _cases() == make.CASES
    assert (make.T, make.STEPS, make.TRAJ_GROUP.tolist()) == (3, 3, [0, 1, 0])
    outputs = [k for k in recorded if ".n" in k]
    # per case and mode: min 1 + 3 arrays, max 3 + 4
    assert len(outputs) == 2 * sum(7 if form == "max" else 4 for _, form, _ in make.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("mech,form,N", _cases())
def test_bit_identical_to_the_recorded_results(make, recorded, ctx, mech, form, N, mode):
    got = make.run_case(ctx, recorded, mech, form, N, mode)
    assert len(got) == (7 if form == "max" else 4)
    for name, a in got.items():
        want = recorded[make.key(mech, form, N, mode, name)]
        assert a.dtype == want.dtype and a.shape == want.shape, name
        assert np.array_equal(a, want), (name, a, want)


def test_every_wrapper_checks_the_shape_of_traj_group():
    """One group index per trajectory, or ValueError before anything reaches the C call (which reads
    T entries) -- in predictdynamics and rollout_min as in their MeanDynamics forms."""
    from gprx.projection import predictdynamics, predictdynamics_md
    from gprx.rollout import rollout_min, rollout_min_md

    for tg in ([0], [0, 0, 0], [[0, 0]]):
        for f in (predictdynamics, predictdynamics_md):
            with pytest.raises(ValueError, match="traj_group"):
                f("P1", [[]], np.zeros((2, 13)), 1, [9, 10, 11], traj_group=tg)
        for f in (rollout_min, rollout_min_md):
            with pytest.raises(ValueError, match="traj_group"):
                f("P1", [[]], np.zeros((2, 2)), 1, traj_group=tg)
