"""k-fold cross-validation, host side (no GPU): the names in the header, the ctypes table and the
Julia shim; NULL handles; gprx_batch_bytes unchanged; the fixtures tests/golden/cvfold_*.npz against the
five fp64 CPU variants of tests/golden/make_golden_cvfold.py, recomputed here; seeded faults that the
bound must catch; simdata.trial_folds; the fold-list validation; and the key sets of run_group /
run_search_group with cv_folds=None."""
import ctypes as C
import importlib.util
import inspect
import pathlib
import re

import numpy as np
import pytest

from gprx import _lib as L

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
NAMES = {"gprx_batch_set_folds": 4, "gprx_batch_cvfold": 6, "gprx_gp_set_folds": 3, "gprx_gp_cvfold": 5}
_spec = importlib.util.spec_from_file_location("make_golden_cvfold", GOLDEN / "make_golden_cvfold.py")
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)
WANT = {"a_p2_1": ("one",), "a_p2_5": ("singletons", "odd_even"), "a_p2_64": ("all", "one_rest", "mod3"),
        "a_p2_65": ("all", "one_rest", "mod3"), "b_cp_130": ("c21", "mod7", "straddle65", "all", "empty_mid", "per_slot"),
        "b_p1_130": ("c21", "mod7", "straddle65", "all"), "b_fb_130": ("c21", "mod7", "straddle65", "all"),
        "e_d1": ("mod2",), "c_cp_320": ("c20", "t64_128_128"), "f_cp_520": ("all", "mod25"), "g_nonpd_p1": ("mod4",)}
CHECKED = [(c, ln) for c, lays in WANT.items() for ln in lays]  # every layout of every case


def load(name):
    with np.load(GOLDEN / f"cvfold_{name}.npz") as z:
        return {k: z[k] for k in z.files}


def test_names_in_header_ctypes_and_julia():
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "gprx.h").read_text(), flags=re.S)
    jl = (REPO / "gpr.jl_amd" / "julia" / "GPRx.jl").read_text()
    for name, nargs in NAMES.items():
        m = re.search(r"^int " + name + r"\(([^)]*)\);", hdr, flags=re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.SIGNATURES[name][1])
        assert L.SIGNATURES[name][0] is C.c_int
        assert hasattr(L.lib, name)
    assert "#define GPRX_CVFOLD_MAX 1024\n" in (REPO / "include" / "gprx.h").read_text() and L.CVFOLD_MAX == 1024
    assert ":gprx_gp_cvfold" in jl and ":gprx_gp_set_folds" in jl and "predict_CVfold" in jl and "logp_CVfold" in jl
    assert L.lib.gprx_abi_version() == 3


def test_null_handles_are_invalid_arguments():
    out = np.empty(4)
    fo = np.zeros(4, dtype=np.int32)
    st = np.empty(1, dtype=np.int32)
    assert L.lib.gprx_batch_set_folds(None, L.iptr(fo), 0, 1) == L.INVALID_ARGUMENT
    assert L.lib.gprx_batch_cvfold(None, L.dptr(out), L.dptr(out), L.dptr(out), L.dptr(out), L.iptr(st)) == L.INVALID_ARGUMENT
    assert L.lib.gprx_batch_cvfold(None, None, None, None, None, None) == L.INVALID_ARGUMENT
    assert L.lib.gprx_gp_set_folds(None, L.iptr(fo), 1) == L.INVALID_ARGUMENT
    assert L.lib.gprx_gp_cvfold(None, None, None, None, None) == L.INVALID_ARGUMENT


@pytest.mark.parametrize("shape,want", [((1, 26, 65, 0), 799860), ((32, 26, 520, 17), 445888000),
                                        ((240, 26, 2048, 100), 41270444352)])
def test_batch_bytes_are_the_parent_commits(shape, want):
    b = C.c_uint64()
    assert L.lib.gprx_batch_bytes(*shape, C.byref(b)) == 0
    assert b.value == want


def test_every_case_and_layout_of_the_issue_is_stored():
    assert set(WANT) == set(M.CASES)
    for name, lays in WANT.items():
        fx = load(name)
        X, Y, thetas = M.case_inputs(name)
        assert float(fx["k"]) == 8.0 and tuple(fx["quantities"]) == M.QUANTITIES
        assert set(fx["layouts"]) == set(lays), name
        left = M.LEFT_OUT.get(name, ())
        assert len(left) <= 1 and len(left) < len(thetas)  # at most one rung, never the whole case
        for ln in lays:
            assert list(fx[f"{ln}.theta_index"]) == [t for t in range(len(thetas)) if t not in left]
            assert fx[f"{ln}.fold_of"].shape in ((1, X.shape[1]), (len(thetas) * Y.shape[0], X.shape[1]))
    assert M.LEFT_OUT == {"b_p1_130": (2,)}
    # the one exception to "five variants" in E, by the points outside the largest fold
    assert M.refit_left_out(load("a_p2_65")["all.fold_of"]) == ("mu", "var")
    assert M.refit_left_out(load("a_p2_65")["one_rest.fold_of"]) == ("var",)
    assert M.refit_left_out(load("a_p2_65")["mod3.fold_of"]) == ()
    assert M.refit_left_out(load("b_cp_130")["per_slot.fold_of"]) == ()


@pytest.mark.parametrize("name,only", CHECKED, ids=[f"{c}-{ln}" for c, ln in CHECKED])
def test_fixture_variants_within_bound(name, only):
    fx = load(name)
    X, Y, thetas = M.case_inputs(name)
    k = float(fx["k"])
    for ln in fx["layouts"]:
        if ln != only:
            continue
        fo = fx[f"{ln}.fold_of"].astype(np.int64)
        tr = {q: fx[f"{ln}.{q}"] for q in M.QUANTITIES + ("A_mu", "A_logp_fold", "A_logp")}
        for j, t in enumerate(fx[f"{ln}.theta_index"]):
            for mode in (0, 1):
                for vn, res in M.variants(X, Y, thetas[t], mode, fo, int(t)).items():
                    ratio = M.worst_ratio(res, tr, fx[f"{ln}.E"], mode, j)
                    assert ratio <= k, (name, ln, int(t), mode, vn, ratio)


@pytest.mark.parametrize("fault", M.FAULTS)
def test_seeded_faults_are_refused(fault):
    """A fold's points in the wrong order, the variance without sn2, log|Q| / 2 with the wrong sign, a
    dropped last fold: each lies outside k max(E_q, eps A_q) of b_cp_130's contiguous 21-point folds."""
    name, ln = "b_cp_130", "c21"
    fx = load(name)
    X, Y, thetas = M.case_inputs(name)
    fo = fx[f"{ln}.fold_of"].astype(np.int64)
    tr = {q: fx[f"{ln}.{q}"] for q in M.QUANTITIES + ("A_mu", "A_logp_fold", "A_logp")}
    for mode in (0, 1):
        bad = M.faulty(X, Y, thetas[0], mode, fo, 0, fault)
        assert M.worst_ratio(bad, tr, fx[f"{ln}.E"], mode, 0) > float(fx["k"]), (fault, mode)


def test_trial_folds_follow_trial_from_dataset():
    """A tiny synthetic dataset dict whose training rows carry their own index: the rows
    trial_from_dataset keeps are those trial_folds numbers, row // plan(config)["train_samples"]."""
    from gprx import data, simdata

    mech = "P1"
    cfg = dict(dtsim=0.001, trainsamples=30, testsamples=5, simsteps=20, max_trajectories=10)
    per = simdata.plan(cfg)["train_samples"]
    assert per == 3
    ntr, width = 10 * per, max(data.VW_INDICES[mech]) + 3
    rows = np.arange(ntr, dtype=np.float64)[:, None] + np.zeros((ntr, width))
    ds = dict(mech=mech, config=cfg, train_old=rows, train_curr=rows + 0.5, test_old=rows[:5], test_future=rows[:5])
    for seed, N in ((0, 7), (3, ntr)):
        tr = simdata.trial_from_dataset(mech, ds, N, M=2, seed=seed, noise=False)
        kept = tr["X"][0].astype(np.int64)
        fo = simdata.trial_folds(ds, N, seed=seed)
        assert fo.shape == (N,) and fo.dtype == np.int32 and fo.max() < 10
        np.testing.assert_array_equal(fo, kept // per)
    assert sorted(np.bincount(simdata.trial_folds(ds, ntr, seed=3))) == [per] * 10
    # run_group's cv_folds="trajectory": one row per trial, by the trial's own dataset and seed
    from gprx import sweep

    got = sweep.cv_fold_ids(mech, 7, [dict(trial=0, seed=5), dict(trial=1, seed=6)], "trajectory", dataset=[ds, ds])
    for row, seed in zip(got, (5, 6)):
        np.testing.assert_array_equal(row, simdata.trial_folds(ds, 7, seed=seed))
    with pytest.raises(ValueError):
        simdata.trial_folds(ds, ntr + 1)


def test_fold_lists_are_validated():
    from gprx.gp import folds_to_ids

    np.testing.assert_array_equal(folds_to_ids([[0, 2, 4], [1, 3]], 5), [0, 1, 0, 1, 0])
    np.testing.assert_array_equal(folds_to_ids([[1], [], [0, 2]], 3), [2, 0, 2])
    for bad in ([[0, 1], [1, 2]], [[0, 1]], [[0, 0], [1, 2]], [[0, 1, 3], [2]], [[-1, 0], [1, 2]], [], [[0.5, 1.0], [2, 0]]):
        with pytest.raises(ValueError):
            folds_to_ids(bad, 3)


def test_cv_folds_is_off_by_default_and_checked():
    from gprx import search, sweep

    assert inspect.signature(sweep.run_group).parameters["cv_folds"].default is None
    assert inspect.signature(search.run_search_group).parameters["cv_folds"].default is None
    assert sweep.cv_fold_ids("P2", 8, [{}] * 3, None) is None
    rows = sweep.cv_fold_ids("P2", 8, [{}] * 2, 3)
    assert len(rows) == 2 and list(rows[0]) == [0, 1, 2, 0, 1, 2, 0, 1]
    for bad in (0, -2, "loo", 2.5, True):
        with pytest.raises(ValueError):
            sweep.cv_fold_ids("P2", 8, [{}], bad)
    with pytest.raises(ValueError):
        sweep.cv_fold_ids("P2", 8, [{}], "trajectory")  # no dataset
