"""gprx_simulate's host surface and the dataset generator's host paths (no GPU): the entry point is
declared, exported and bound with ABI version 3 unchanged; the sampling rules of
examples/parallel/dataframes.jl; the start states of examples/utils/data/simulations.jl lie on the
constraints with tangent velocities; the dataset files round-trip bit-exactly; a noise-free trial
returns the stored rows."""
import inspect
import pathlib
import re

import numpy as np
import pytest

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "gprx.h"
MECHS = ("P1", "P2", "CP", "FB")


def test_entry_point_is_declared_exported_and_bound():
    import gprx._lib as L
    import gprx.simdata  # noqa: F401

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+gprx_simulate\s*\(", text)
    assert "gprx_simulate" in L.SIGNATURES and getattr(L.lib, "gprx_simulate") is not None
    proto = re.search(r"\bgprx_simulate\s*\(([^)]*)\)", text).group(1)
    assert len(proto.split(",")) == 17 == len(L.SIGNATURES["gprx_simulate"][1])
    assert L.lib.gprx_abi_version() == 3  # an entry point added, nothing changed
    assert L.lib.gprx_simulate(None, 2, 0.01, 5, 1, None, None, None, None, 0.0, 100, 1e-10, 1, None, 0, None,
                               None) == L.INVALID_ARGUMENT
    assert "gprx_simulate" in (HEADER.parents[1] / "INTEGRATION.md").read_text()


def test_sweep_takes_a_dataset():
    from gprx import sweep

    assert inspect.signature(sweep.run_group).parameters["dataset"].default is None  # the synthetic path is the default
    assert inspect.signature(sweep.run_vi_baseline).parameters["dataset"].default is None
    with pytest.raises(ValueError):  # minimal-coordinate trials are not built from datasets
        sweep.local_trials("P2", 8, "min", range(1), 4, dataset={})


def test_sample_indices_follow_pushsamples():
    from gprx import simdata as SD

    for scaling, n, lo, hi in ((1, 5, 1, 199), (100, 21, 1, 19900), (100, 1, 1, 17900)):
        j = SD.sample_indices(np.random.default_rng(4), n, lo, hi, scaling)
        assert j.shape == (n,) and j.min() >= lo and j.max() <= hi
        if n > 1:
            gaps = np.diff(np.sort(j))
            assert gaps.min() > 2 * scaling  # (j, j + scaling) pairs of two samples never intersect
        np.testing.assert_array_equal(j, SD.sample_indices(np.random.default_rng(4), n, lo, hi, scaling))
        assert not np.array_equal(j, SD.sample_indices(np.random.default_rng(5), n, lo, hi, scaling)) or n == 0
    with pytest.raises(AssertionError):  # (4 scaling + 1) nsamples < length(samplerange)
        SD.sample_indices(np.random.default_rng(0), 5, 1, 25, 1)
    # _pushuniformsamples!: samplerange[i div(length, nsamples)]; one sample: div(length, 2)
    np.testing.assert_array_equal(SD.uniform_indices(4, 1, 100), [25, 50, 75, 100])
    np.testing.assert_array_equal(SD.uniform_indices(21, 1, 19900), [947 * i for i in range(1, 22)])
    np.testing.assert_array_equal(SD.uniform_indices(1, 1, 17900), [8950])
    with pytest.raises(AssertionError):
        SD.uniform_indices(5, 1, 5)


def test_plan_is_generate_dataframes():
    from gprx import simdata as SD

    P = SD.plan(SD.default_config())  # getconfig(): 2048 training samples, 100 test samples, dtsim 1e-4
    assert (P["scaling"], P["nsteps"], P["ntrain"], P["ntest"], P["train_samples"], P["test_samples"]) == (100, 20000, 100, 100, 21, 1)
    assert P["train_range"] == (1, 19900) and P["train_off"] == 100
    assert P["test_range"] == (1, 20000 - 2100) and P["test_off"] == 2100
    P = SD.plan(dict(SD.default_config(), dtsim=0.01, trainsamples=2, testsamples=2, simsteps=5))
    assert (P["scaling"], P["nsteps"], P["ntrain"], P["ntest"], P["train_samples"], P["test_samples"]) == (1, 200, 2, 2, 1, 1)
    assert P["test_off"] == 6
    with pytest.raises(ValueError):
        SD.plan(dict(SD.default_config(), dtsim=0.003))  # Int(0.01 / dtsim) is inexact


@pytest.mark.parametrize("mech", MECHS)
def test_parameter_and_start_draws(mech):
    from gprx import simdata as SD

    cfg = SD.default_config()
    nb = SD.NBODIES[mech]
    rng = np.random.default_rng(1)
    for _ in range(20):
        p = SD.draw_parameters(mech, cfg, rng)
        assert p["dm"].shape == (nb,) and np.all(np.abs(p["dm"] - 1) <= 0.1) and np.all(np.abs(p["dJ"] - 1) <= 0.1)
        assert p["dJ"].shape == ((1,) if mech == "CP" else (nb,))
        assert np.all(p["friction"] >= 0) and np.all(p["friction"] <= SD.FRICTION_SCALE[mech])
    p0 = SD.draw_parameters(mech, dict(cfg, sigma=dict(dm=0.0, dJ=0.0), friction=0.0), rng)
    assert np.all(p0["dm"] == 1) and np.all(p0["dJ"] == 1) and np.all(p0["friction"] == 0)
    angle = {"P1": "th", "P2": "t1", "CP": "th", "FB": "t1"}[mech]
    for _ in range(50):
        a1, a2 = SD.draw_start(mech, "exp1", rng)[angle], SD.draw_start(mech, "exp2", rng)[angle]
        assert abs(a1) <= np.pi / 2
        if mech != "FB":  # exp2 starts in the upper half (datasets.jl:19, 39, 60)
            assert np.pi / 2 <= abs(a2) <= np.pi


@pytest.mark.parametrize("mech", MECHS)
def test_initial_cstate_lies_on_the_constraints_with_tangent_velocities(mech):
    """g(x, q) <= 1e-15 scale (scale: the largest position coordinate, at least 1) for 50 draws, and
    d/dt g = Gpos (v, w / 2) at rounding level: along q (1, phi) the variation rate is w / 2."""
    from gprx import simdata as SD
    from gprx import vi

    rng = np.random.default_rng(11)
    M = vi.MECHANISMS[mech]
    nb = M["nb"]
    starts = [SD.draw_start(mech, ("exp1", "exp2", "exptest")[i % 3], rng) for i in range(50)]
    if mech in ("P2", "FB"):  # the experiments start these at rest: give the chain rates, too
        for s in starts[25:]:
            s["o1"], s["o2"] = rng.uniform(-2, 2), rng.uniform(-2, 2)
    X = np.concatenate([SD.initial_cstate(mech, s) for s in starts])
    c = X.reshape(-1, nb, 13)
    x, q, v, w = c[..., 0:3], c[..., 3:7], c[..., 7:10], c[..., 10:13]
    scale = max(1.0, float(np.max(np.abs(x))))
    assert np.max(np.abs(vi.constraints(M, x, q))) <= 1e-15 * scale
    rate = np.concatenate([v, w / 2.0], axis=-1).reshape(-1, 6 * nb)
    gdot = np.einsum("tcj,tj->tc", vi.jac_phi(M, x, q), rate)
    vmax = max(1.0, float(np.max(np.abs(rate))))
    assert np.max(np.abs(gdot)) <= 8 * np.finfo(float).eps * vmax
    if mech == "FB":  # simulations.jl:171-189: links 1 and 4 at t1 + t2, links 2 and 3 at t1 - t2
        s = starts[0]
        np.testing.assert_allclose(SD.rot_angle(q[0]), [s["t1"] + s["t2"], s["t1"] - s["t2"], s["t1"] - s["t2"], s["t1"] + s["t2"]],
                                   rtol=0, atol=1e-15)
        assert np.all(c[:25, :, 7:13] == 0)


def _fake_dataset(mech, n=6, seed=3):
    from gprx import data
    from gprx import simdata as SD

    rng = np.random.default_rng(seed)
    st = lambda: data._cstates(mech, data._sample_minimal(mech, n, rng)).T.copy()  # noqa: E731
    ds = {k: st() for pair in SD._PAIRS.values() for k in pair}
    ds.update(dm=np.array([1.05] * SD.NBODIES[mech]), dJ=np.array([0.95] * SD.NBODIES[mech]), friction=np.array([0.3] * SD.NBODIES[mech]),
              mech=mech, seed=seed, config=SD.default_config())
    return ds


def test_dataset_files_round_trip_bit_exactly(tmp_path):
    from gprx import simdata as SD

    ds = _fake_dataset("P2")
    SD.write_dataset(tmp_path / "P2", ds)
    back = SD.read_dataset(tmp_path / "P2")
    assert set(back) == set(ds)
    for k, v in ds.items():
        if isinstance(v, np.ndarray):
            assert back[k].dtype == v.dtype and back[k].tobytes() == v.tobytes(), k
        else:
            assert back[k] == v, k
    assert len(SD.load_datasets(tmp_path, "P2")) == 1
    SD.write_dataset(tmp_path / "CP" / "0", _fake_dataset("CP", seed=1))
    SD.write_dataset(tmp_path / "CP" / "1", _fake_dataset("CP", seed=2))
    assert [d["seed"] for d in SD.load_datasets(tmp_path, "CP")] == [1, 2]


@pytest.mark.parametrize("mech", MECHS)
def test_trial_from_dataset(mech):
    from gprx import data
    from gprx import simdata as SD

    ds = _fake_dataset(mech)
    tr = SD.trial_from_dataset(mech, ds, 4, 3, seed=9, noise=False)
    d = 13 * SD.NBODIES[mech]
    assert tr["X"].shape == (d, 4) and tr["Xs"].shape == (d, 3) and tr["truth"].shape == (3, d) and tr["d"] == d
    rows = lambda A, B: [int(np.nonzero(np.all(B == a, axis=1))[0][0]) for a in A]  # noqa: E731
    itr, ite = rows(tr["X"].T, ds["train_old"]), rows(tr["Xs"].T, ds["test_old"])
    assert len(set(itr)) == 4 and len(set(ite)) == 3  # a shuffle's first rows, stored bit for bit
    np.testing.assert_array_equal(tr["Xcurr"].T, ds["train_curr"][itr])
    np.testing.assert_array_equal(tr["truth"], ds["test_future"][ite])
    np.testing.assert_array_equal(tr["Y"], tr["Xcurr"][np.asarray(data.VW_INDICES[mech]) - 1])
    # the noisy trial: the same rows moved by ~Sigma, the truth untouched, the minimal coordinates read back
    nz = SD.trial_from_dataset(mech, ds, 4, 3, seed=9, noise=True)
    np.testing.assert_array_equal(nz["truth"], tr["truth"])
    dev = np.abs(nz["X"] - tr["X"])
    assert 0 < dev.max() < 0.1
    m = SD.to_minimal(mech, ds["train_old"])
    back = data._cstates(mech, m).T
    for b in range(SD.NBODIES[mech]):  # an angle beyond pi comes back wrapped: -q, the same rotation
        back[:, 13 * b + 3:13 * b + 7] *= np.where(back[:, 13 * b + 3] * ds["train_old"][:, 13 * b + 3] < 0, -1.0, 1.0)[:, None]
    vel = np.concatenate([np.r_[13 * b + 7:13 * b + 10] for b in range(SD.NBODIES[mech])])
    rest = np.setdiff1d(np.arange(back.shape[1]), vel)
    # the angles come back to a few ulps (8 eps of an angle up to 2 pi ~ 1e-14); the linear velocities
    # are their forward difference over h = 1e-4, which divides that by h
    np.testing.assert_allclose(back[:, rest], ds["train_old"][:, rest], rtol=0, atol=1e-14)
    np.testing.assert_allclose(back[:, vel], ds["train_old"][:, vel], rtol=0, atol=1e-14 / data.DT_SIM)


def test_rot_angle_is_the_signed_rotation_angle():
    from gprx import simdata as SD

    th = np.array([-3.0, -1.0, 0.0, 0.5, 3.1])
    q = np.stack([np.cos(th / 2), np.sin(th / 2), 0 * th, 0 * th], axis=1)
    np.testing.assert_allclose(SD.rot_angle(q), th, rtol=0, atol=1e-15)
    np.testing.assert_allclose(SD.rot_angle(-q), th, rtol=0, atol=1e-15)  # q and -q: the same rotation


def test_four_bar_datasets_and_unsupported_sweep_variants_are_refused_at_once():
    from gprx import simdata as SD
    from gprx import sweep

    with pytest.raises(ValueError, match="four-bar"):  # before any draw or device work (no context is touched)
        SD.generate_dataset("FB", 0)
    with pytest.raises(ValueError, match="--variants"):  # before any group runs
        sweep.run(mechs=("P2",), sizes=(8,), variants=("vi", "max", "min"), n_trials=1, ctx=object(), dataset="nowhere")
    # the regulariser follows the constraint block's dt^2 from the experiments' value at dt = 0.01
    assert SD.regularizer("FB", dict(dtsim=0.01)) == 1e-10 and SD.regularizer("P2", dict(dtsim=1e-4)) == 0.0
    assert abs(SD.regularizer("FB", dict(dtsim=1e-4)) - 1e-14) < 1e-28 and SD.regularizer("FB", dict(dtsim=1e-4, regularizer=1e-12)) == 1e-12


def test_p2_noise_falls_on_the_second_link_itself():
    """applynoise! perturbs body 2's own angle and rate (transformations.jl:69-70): their deviations have the
    variance of one draw, not of two."""
    from gprx import data
    from gprx import simdata as SD

    rng = np.random.default_rng(0)
    X = data._cstates("P2", dict(t1=rng.uniform(-1, 1, 4000), t2=rng.uniform(-1, 1, 4000), o1=rng.uniform(-1, 1, 4000),
                                 o2=rng.uniform(-1, 1, 4000))).T
    N = SD.apply_noise("P2", X, np.random.default_rng(1))
    for col in (10, 23):  # w_x of link 1 and of link 2
        assert abs(np.std(N[:, col] - X[:, col]) / data.SIGMA - 1.0) < 0.05
    assert abs(np.std(SD.rot_angle(N[:, 16:20]) - SD.rot_angle(X[:, 16:20])) / data.SIGMA - 1.0) < 0.05
