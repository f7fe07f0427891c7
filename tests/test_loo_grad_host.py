"""Gradient of the leave-one-out log predictive probability, host side (no GPU): the two names in the
header, the ctypes table and the Julia shim; NULL handles; the self-check of the fixtures
tests/golden/loograd_*.npz (tests/golden/make_golden_loo_grad.py: every CPU variant stored lies within
k max(E, eps A) of the truth on the vector and within k_comp max(E_grad[p], eps A[p]) per component, in
both distance modes) and their byte-identical regeneration for one small case; and
optim.optimize_batch's objective switch through a stub batch."""
import ctypes as C
import importlib.util
import pathlib
import re

import numpy as np
import pytest

from gprx import _lib as L
from gprx import optim

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
EPS = 2.0 ** -52
CASES = ("a_p2_1", "a_p2_5", "a_p2_64", "a_p2_65", "b_cp_130", "b_p1_130", "b_fb_130", "e_d1", "c_cp_320", "d_cp_500",
         "f_cp_520", "g_nonpd_p1")
VARIANTS = ("lapack", "lapack_rev", "r513", "staged", "staged_rev")
NAMES = {"gprx_batch_loo_grad": 4, "gprx_gp_loo_grad": 3}


def load(name):
    with np.load(GOLDEN / f"loograd_{name}.npz") as z:
        return {k: z[k] for k in z.files}


def floor_of(fx, t, mode):
    """A per (target, component) of rung t; in expanded mode (0) a component whose truth is exactly 0
    takes the expanded distance form's operands (make_golden_loo_grad.py)."""
    return np.where(fx["grad"][t] == 0.0, fx["A_grad_exp"][t], fx["A_grad"][t]) if mode == 0 else fx["A_grad"][t]


def test_names_in_header_ctypes_and_julia():
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "gprx.h").read_text(), flags=re.S)
    jl = (REPO / "gpr.jl_amd" / "julia" / "GPRx.jl").read_text()
    for name, nargs in NAMES.items():
        m = re.search(r"^int " + name + r"\(([^)]*)\);", hdr, flags=re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.SIGNATURES[name][1])
        assert L.SIGNATURES[name][0] is C.c_int
        assert ":" + name in jl
        assert hasattr(L.lib, name)
    assert "dlogpdθ_LOO" in jl
    assert L.lib.gprx_abi_version() == 3


def test_null_handles_are_invalid_arguments():
    out = np.empty(4)
    st = np.empty(1, dtype=np.int32)
    assert L.lib.gprx_batch_loo_grad(None, L.dptr(out), L.dptr(out), L.iptr(st)) == L.INVALID_ARGUMENT
    assert L.lib.gprx_batch_loo_grad(None, None, None, None) == L.INVALID_ARGUMENT
    assert L.lib.gprx_gp_loo_grad(None, L.dptr(out), L.dptr(out)) == L.INVALID_ARGUMENT


@pytest.mark.parametrize("name", CASES)
def test_fixture_variants_within_bound(name):
    fx = load(name)
    with np.load(GOLDEN / "hp_a_p2_1.npz") as z:
        assert float(fx["k"]) == float(z["k"]) == 8.0
    k, kc = float(fx["k"]), float(fx["k_comp"])
    assert kc >= 4.0 and math_is_pow2(kc) and kc == float(load("a_p2_1")["k_comp"])
    assert tuple(fx["variant_names"]) == VARIANTS
    T, (G, n) = len(fx["theta_index"]), fx["grad"].shape[1:]
    assert T >= 1 and fx["E"].shape == (2, T) and fx["E_grad"].shape == (2, T, n) and fx["logp"].shape == (T, G)
    for mode in (0, 1):
        for t in range(T):
            floor = EPS * floor_of(fx, t, mode)
            lim = k * np.maximum(fx["E"][mode, t], floor)
            limc = kc * np.maximum(fx["E_grad"][mode, t][None, :], floor)
            for vn in VARIANTS:
                err = np.abs(fx[f"d_{vn}"][mode, t])
                assert np.all(err <= lim), (name, mode, t, vn, "vector")
                assert np.all(err <= limc), (name, mode, t, vn, "component")


def math_is_pow2(v):
    m, _ = np.frexp(v)
    return m == 0.5


def test_small_fixture_regenerates_byte_identically(tmp_path):
    spec = importlib.util.spec_from_file_location("make_golden_loo_grad", GOLDEN / "make_golden_loo_grad.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for case, rungs in mod.LEFT_OUT.items():  # at most one rung per case, never a log sigma_n = -2 rung
        assert len(rungs) <= 1 and all(mod.case_inputs(case)[2][t][0] != -2.0 for t in rungs)
        assert sorted(set(range(len(mod.case_inputs(case)[2]))) - set(rungs)) == list(load(case)["theta_index"])
    mod.main(["--only", "a_p2_5", "--out", str(tmp_path), "-j", "1"])
    assert (tmp_path / "loograd_a_p2_5.npz").read_bytes() == (GOLDEN / "loograd_a_p2_5.npz").read_bytes()


class StubBatch:
    """-logp = |theta - target|^2 / 2 per slot; records every call."""

    def __init__(self, target):
        self.target = np.asarray(target, dtype=np.float64)
        self.calls = []
        self.th = None

    def run(self, theta, **kw):
        self.calls.append(("run", dict(kw)))
        self.th = np.array(theta, dtype=np.float64)
        dlt = self.th - self.target
        r = dict(status=np.zeros(len(dlt), dtype=np.int32), mll=-0.5 * np.sum(dlt * dlt, axis=1),
                 grad=-dlt if kw.get("grad") else None)
        return r

    def loo_grad(self):
        self.calls.append(("loo_grad", {}))
        dlt = self.th - self.target
        return dict(logp=-0.5 * np.sum(dlt * dlt, axis=1), grad=-dlt, status=np.zeros(len(dlt), dtype=np.int32))


def test_optimize_batch_loo_minimises_a_quadratic_through_a_stub():
    target = np.array([[1.0, -2.0, 0.5], [0.0, 3.0, -1.0]])
    stub = StubBatch(target)
    res, rounds = optim.optimize_batch(stub, np.zeros((2, 3)), objective="loo")
    assert rounds >= 1
    for s, r in enumerate(res):
        np.testing.assert_allclose(r.minimizer, target[s], atol=1e-7)
        assert r.minimum <= 1e-14
    kinds = [c[0] for c in stub.calls]
    assert kinds == ["run", "loo_grad"] * rounds
    assert all(kw == dict(grad=False, predict=False) for kind, kw in stub.calls if kind == "run")
    with pytest.raises(ValueError):
        optim.optimize_batch(stub, np.zeros((2, 3)), objective="other")


def test_optimize_batch_default_objective_calls_run_as_before():
    target = np.array([[1.0, -2.0, 0.5], [0.0, 3.0, -1.0]])
    a, b = StubBatch(target), StubBatch(target)
    res_a, rounds_a = optim.optimize_batch(a, np.zeros((2, 3)))
    res_b, rounds_b = optim.optimize_batch(b, np.zeros((2, 3)), objective="mll")
    assert rounds_a == rounds_b and a.calls == b.calls
    assert a.calls == [("run", dict(grad=True, predict=False))] * rounds_a  # one evaluation per round, no loo_grad
    for s, (ra, rb) in enumerate(zip(res_a, res_b)):
        assert np.array_equal(ra.minimizer, rb.minimizer) and ra.minimum == rb.minimum
        np.testing.assert_allclose(ra.minimizer, target[s], atol=1e-7)
