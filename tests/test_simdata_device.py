"""The dataset generator end to end (gprx.simdata.generate_dataset over gprx_simulate) and the sweep's
opt-in dataset path: with dtsim = 0.01 (scaling 1), nominal bodies and no friction a test pair is
(j, j + simsteps + 1) of one trajectory of the experiments' own mechanism step, so the physics-only
baseline started at sold must arrive at sfuture -- the index arithmetic through every layer."""
import numpy as np
import pytest

from gprx import mdynamics, simdata, sweep

pytestmark = pytest.mark.gpu
CONFIG = dict(dtsim=0.01, trainsamples=2, testsamples=2, simsteps=5, sigma=dict(dm=0.0, dJ=0.0), friction=0.0)


@pytest.fixture(scope="module")
def ctx():
    import gprx

    c = gprx.Context(0)
    yield c
    c.close()


def test_dataset_pairs_are_steps_of_one_trajectory(ctx):
    ds = simdata.generate_dataset("P2", 7, CONFIG, ctx=ctx)  # 2 training + 2 test trajectories of 199 steps
    assert ds["train_old"].shape == ds["train_curr"].shape == (2, 26) and ds["test_old"].shape == ds["test_future"].shape == (2, 26)
    assert ds["train_old_uniform"].shape == (2, 26) and np.all(ds["dm"] == 1) and np.all(ds["friction"] == 0)
    for k in ("train_old", "train_curr", "test_old", "test_future", "train_curr_uniform", "test_future_uniform"):
        assert np.all(np.isfinite(ds[k])), k
    # a training pair is one mechanism step apart, a test pair simsteps + 1 (test_simulate_device's
    # tolerance against the stepwise path: both solve the same steps to 1e-10)
    nxt, bad = mdynamics.simulate("P2", ds["train_old"], 0, ctx=ctx)
    np.testing.assert_allclose(nxt, ds["train_curr"], rtol=0, atol=1e-8)
    fin, bad = mdynamics.simulate("P2", ds["test_old"], CONFIG["simsteps"], ctx=ctx)
    assert not bad.any()
    np.testing.assert_allclose(fin, ds["test_future"], rtol=0, atol=1e-8)
    fin, _ = mdynamics.simulate("P2", ds["test_old_uniform"], CONFIG["simsteps"], ctx=ctx)
    np.testing.assert_allclose(fin, ds["test_future_uniform"], rtol=0, atol=1e-8)
    # the sweep's vi variant on the noise-free trial: the squared position error of states equal to 1e-8
    r = sweep.run_vi_baseline("P2", [0], testsamples=2, simsteps=CONFIG["simsteps"], ctx=ctx, dataset=ds, noise=False)
    assert not r["failed"].any() and r["kstep_mse"][0] <= (1e-8) ** 2
    # reproducible by seed; another seed, other trajectories
    again = simdata.generate_dataset("P2", 7, CONFIG, ctx=ctx)
    np.testing.assert_array_equal(again["test_future"], ds["test_future"])
    assert not np.array_equal(simdata.generate_dataset("P2", 8, CONFIG, ctx=ctx)["test_old"], ds["test_old"])


def test_perturbed_dataset_and_the_sweep_on_it(ctx):
    """A reduced mz_max group on a simulated dataset (perturbed bodies, friction, dtsim = 1e-3) keeps as
    many trials as on the synthetic generator's data, with finite errors."""
    cfg = dict(dtsim=1e-3, trainsamples=16, testsamples=4, simsteps=3, max_trajectories=16, eps=1e-8)
    ds = simdata.generate_dataset("P2", 3, cfg, ctx=ctx)
    assert ds["train_old"].shape == (16, 26) and ds["test_old"].shape == (4, 26)
    assert np.all(ds["dm"] != 1) and np.all(ds["friction"] > 0)
    kw = dict(testsamples=4, simsteps=3, max_evals=5)
    syn = sweep.run_group("P2", 8, "max", range(2), ctx, **kw)
    sim = sweep.run_group("P2", 8, "max", range(2), ctx, dataset=ds, **kw)
    assert int((~sim["failed"]).sum()) == int((~syn["failed"]).sum()) == 2
    assert np.all(np.isfinite(sim["kstep_mse"]))
    # the truth is the dataset's own sfuture: the errors are not the synthetic path's
    assert not np.array_equal(sim["kstep_mse"], syn["kstep_mse"])
