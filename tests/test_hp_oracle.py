"""CPU checks of the high-precision oracle and its fixtures (oracle/hp_oracle.py,
tests/golden/hp_*.npz): the fp64 references alone stay inside every bound the device is held to,
the truth is reproducible, the float80 backend agrees with mpmath, and subtle seeded faults are
rejected.  No GPU and no built library: gprx/data.py is loaded by file path.
"""
import importlib.util
import pathlib
import sys

import numpy as np
import pytest
import threadpoolctl

from oracle import gp_oracle as O
from oracle import hp_oracle as H

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
# the GP cases a..e of make_golden_hp.py; hp_phys_* are the physics' (test_hp_physics_oracle.py).  A GP case
# named "f" needs this pattern (and test_hp_parity.py's) widened: test_case_table_is_complete fails until then
GP_FIXTURES = "hp_[a-e]_*.npz"
NAMES = sorted(p.stem[3:] for p in GOLDEN.glob(GP_FIXTURES))
FLOAT80_MARGIN = 1e-2  # of E_q; expected 2^-63 / 2^-52 = 5e-4


def fixture(name):
    with np.load(GOLDEN / f"hp_{name}.npz") as z:
        return {k: z[k] for k in z.files}


def truth_of(fx, t):
    return {k: fx[k][t] for k in fx if k in H.QUANTITIES or k.startswith("A_")}


def ratios(res, tr, fx, mode, t):
    """Per quantity: max |result - truth| / max(E_q, eps A_q) over the bound's k (k_grad for the
    gradient's second, per-component bound "grad_comp"): within the bound iff <= 1."""
    out = {}
    for qi, q in enumerate(H.QUANTITIES):
        if q in tr:
            floor = H.EPS * H.floor_of(tr, q, mode)
            out[q] = H.ratio(np.abs(res[q] - tr[q]), fx["E"][mode, t, qi], floor) / float(fx["k"])
            if q == "grad":
                out["grad_comp"] = H.ratio(np.abs(res[q] - tr[q]), fx["E_grad"][mode, t], floor) / float(fx["k_grad"])
    return out


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def test_case_table_is_complete():
    make = _load(GOLDEN / "make_golden_hp.py", "make_golden_hp")
    assert NAMES == sorted(c["name"] for c in make.CASES)
    assert all(p.stat().st_size <= 372 * 1024 for p in GOLDEN.glob(GP_FIXTURES))  # the largest committed file
    for key in ("k", "k_grad"):
        ks = {float(fixture(n)[key]) for n in NAMES}
        assert len(ks) == 1 and ks.pop() >= 4.0


@pytest.mark.parametrize("name", NAMES)
def test_variants_stay_inside_the_bounds(name):
    """gp_oracle.fit (LAPACK) and the explicit-inverse restatement, in both modes, against the
    stored truth: this pins gp_oracle.py to the truth and proves the bounds admit the references."""
    fx = fixture(name)
    stacks = [O.dist_stack(fx["X"], fx["X"], mode) for mode in (0, 1)]
    with threadpoolctl.threadpool_limits(4):  # 64-row tiles and N <= 512: more BLAS threads only cost time
        for t, th in enumerate(fx["thetas"]):
            tr = truth_of(fx, t)
            for mode in (0, 1):
                for vn, res in H.variants(fx["X"], fx["Y"], th, fx["Xs"], mode, D=stacks[mode]).items():
                    r = ratios(res, tr, fx, mode, t)
                    assert all(v <= 1.0 for v in r.values()), (name, t, mode, vn, r)
                    if mode == 1:  # constant coordinates: exactly zero
                        assert not np.any(res["grad"][tr["grad"] == 0.0])


def test_point_order_spread_is_what_E_q_estimates():
    """Why E_q takes the two reversed-order variants.  gp_oracle.lml over 40 random orders of the d = 1
    case's training points, expanded mode, is 40 correct fp64 evaluations of one LML.  Their largest
    error lies beyond k times the E_q of the first three variants (which share K's rounding or the
    factorisation): that bound rejects correct references.  With the five variants the median
    order's error is within a factor k of E_q either way, and every order is inside the bound."""
    fx = fixture("e_d1")
    k, th, qi = float(fx["k"]), fx["thetas"][0], H.QUANTITIES.index("mll")
    rng = np.random.default_rng(0)
    errs = []
    for _ in range(40):
        p = rng.permutation(fx["X"].shape[1])
        errs.append(max(abs(O.lml(fx["X"][:, p], y[p], th, 0)[0] - m) for y, m in zip(fx["Y"], fx["mll"][0])))
    E5 = float(fx["E"][0, 0, qi])
    E3 = H.geomean(fx["verr"][0, :3, 0, qi])
    med, top = float(np.median(errs)), float(np.max(errs))
    print(f"LML error over 40 point orders: median {med:.3e}, largest {top:.3e}; E_q of three variants {E3:.3e}, "
          f"of five {E5:.3e}")
    assert tuple(fx["variant_names"][:3]) == ("lapack", "explicit", "staged")
    assert top > k * E3
    assert E5 / k <= med <= k * E5 and top <= k * max(E5, H.EPS * float(np.max(fx["A_mll"][0])))


def test_fresh_truth_is_bit_identical():
    fx = fixture("a_p2_33")
    tr = H.truth(fx["X"], fx["Y"], fx["thetas"][0], fx["Xs"], "mp")
    for key, v in tr.items():
        np.testing.assert_array_equal(v, fx[key][0], err_msg=key)


def test_float80_backend_against_mpmath():
    """N = 130 on the worst ladder rung: the float80 evaluation differs from the stored mpmath truth
    by at most 1e-2 E_q in every quantity."""
    fx = fixture("b_cp_130")
    assert str(fx["backend"]) == "mp"
    t = int(np.argmax(fx["cond"]))
    ld = H.truth(fx["X"], fx["Y"], fx["thetas"][t], fx["Xs"], "ld", want_cov="cov" in fx)
    for qi, q in enumerate(H.QUANTITIES):
        if q not in fx:
            continue
        E = float(np.min(fx["E"][:, t, qi]))
        d = float(np.max(np.abs(ld[q] - fx[q][t])))
        print(f"float80 vs mpmath {q}: {d:.3e} = {d / E:.2e} E_q")
        assert d <= FLOAT80_MARGIN * E


def _old_tolerances():
    return _load(pathlib.Path(__file__).resolve().parent / "test_gpu.py", "_test_gpu_for_tolerances").tolerances


@pytest.mark.parametrize("name", ["b_p2_130", "b_cp_130"])
def test_seeded_faults_are_rejected(name):
    """Each subtle fault seeded into the explicit-inverse variant breaks the bound of at least one
    quantity.  Printed: which of them the fixed bounds of test_gpu.py's tolerances() accept -- the
    gap these fixtures close."""
    fx = fixture(name)
    th, X, Y, Xs, k = fx["thetas"][0], fx["X"], fx["Y"], fx["Xs"], float(fx["k"])
    tr = truth_of(fx, 0)
    tolerances = _old_tolerances()
    fits = [[O.fit(X, y, th, Xs, mode) for y in Y] for mode in (0, 1)]
    accepted_by_old = []
    for fault in H.FAULTS:
        res = H.variants(X, Y, th, Xs, 1, fault=fault)["explicit"]
        r = ratios(res, tr, fx, 1, 0)
        broken = [q for q, v in r.items() if not v <= 1.0]
        old_ok = True
        for g, y in enumerate(Y):
            tol = tolerances(fits[1][g], fits[0][g], y, th, strict=name == "b_p2_130")
            f = fits[1][g]
            old_ok &= (abs(res["mll"][g] - f["mll"]) <= tol["mll"] and np.max(np.abs(res["grad"][g] - f["grad"])) <= tol["grad"]
                       and np.max(np.abs(res["mu"][g] - f["mu"])) <= tol["mu"]
                       and np.max(np.abs(np.maximum(res["var"], 0.0) - f["var"])) <= tol["var"])
        if old_ok:
            accepted_by_old.append(fault)
        print(f"{name} {fault}: new bound rejects {broken} (largest error {max(r.values()):.3g} of its bound); "
              f"old bounds {'accept' if old_ok else 'reject'}")
        assert broken, (fault, r)
    print(f"{name}: faults the old bounds accept: {accepted_by_old}")
