"""Leave-one-out entry points, host side (no GPU): the two names in the header, the ctypes table and
the Julia shim; the ABI version; NULL handles; gprx_batch_bytes unchanged; and the self-check of the
fixtures tests/golden/loo_*.npz (tests/golden/make_golden_loo.py): every CPU variant stored in a
fixture lies within k max(E_q, eps A_q) of the truth, elementwise, in both distance modes."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from gprx import _lib as L

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
EPS = 2.0 ** -52
QUANTITIES = ("mu", "var", "logp_i", "logp")
CASES = ("a_p2_1", "a_p2_5", "a_p2_64", "a_p2_65", "b_cp_130", "b_p1_130", "b_fb_130", "e_d1", "c_cp_320", "d_cp_500",
         "f_cp_520", "g_nonpd_p1")
NAMES = {"gprx_batch_loo": 6, "gprx_gp_loo": 4}


def floor_of(fx, q, t, mode):
    """A_q of theta rung t: (G, N) for mu and logp_i, (N) for var, (G) for logp.  mu's is |mu|, and the
    terms of its last subtraction only where E_mu = 0 (make_golden_loo.py: a_p2_1)."""
    mu = np.abs(fx["mu"][t]) if fx["E"][mode, t, 0] > 0 else fx["A_mu"][t]
    return {"mu": mu, "var": np.abs(fx["var"][t]), "logp_i": np.abs(fx["logp_i"][t]), "logp": fx["A_logp"][t]}[q]


def test_names_in_header_ctypes_and_julia():
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "gprx.h").read_text(), flags=re.S)
    jl = (REPO / "gpr.jl_amd" / "julia" / "GPRx.jl").read_text()
    for name, nargs in NAMES.items():
        m = re.search(r"^int " + name + r"\(([^)]*)\);", hdr, flags=re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.SIGNATURES[name][1])
        assert L.SIGNATURES[name][0] is C.c_int
    assert ":gprx_gp_loo" in jl and "predict_LOO" in jl and "logp_LOO" in jl


def test_abi_version_stays_3():
    assert L.lib.gprx_abi_version() == 3


def test_null_handles_are_invalid_arguments():
    out = np.empty(4)
    st = np.empty(1, dtype=np.int32)
    assert L.lib.gprx_batch_loo(None, L.dptr(out), L.dptr(out), L.dptr(out), L.dptr(out), L.iptr(st)) == L.INVALID_ARGUMENT
    assert L.lib.gprx_batch_loo(None, None, None, None, None, None) == L.INVALID_ARGUMENT
    assert L.lib.gprx_gp_loo(None, L.dptr(out), L.dptr(out), L.dptr(out)) == L.INVALID_ARGUMENT


@pytest.mark.parametrize("shape,want", [((1, 26, 65, 0), 799860), ((32, 26, 520, 17), 445888000),
                                        ((240, 26, 2048, 100), 41270444352)])
def test_batch_bytes_are_the_parent_commits(shape, want):
    """The leave-one-out workspace comes from the context scratch: gprx_batch_bytes keeps the values
    recorded at the parent commit."""
    b = C.c_uint64()
    assert L.lib.gprx_batch_bytes(*shape, C.byref(b)) == 0
    assert b.value == want


@pytest.mark.parametrize("name", CASES)
def test_fixture_variants_within_bound(name):
    with np.load(GOLDEN / f"loo_{name}.npz") as z:
        fx = {k: z[k] for k in z.files}
    assert tuple(fx["quantities"]) == QUANTITIES and float(fx["k"]) == 8.0
    k, T = float(fx["k"]), len(fx["theta_index"])
    assert T >= 1 and fx["E"].shape == (2, T, len(QUANTITIES))
    # the alternative floor of mu is in use at N = 1 only
    assert np.all(fx["E"][:, :, 0] > 0) == (name != "a_p2_1")
    for mode in (0, 1):
        for t in range(T):
            for qi, q in enumerate(QUANTITIES):
                lim = k * np.maximum(fx["E"][mode, t, qi], EPS * floor_of(fx, q, t, mode))
                for vn in fx["variant_names"]:
                    err = np.abs(fx[f"d_{vn}_{q}"][mode, t].astype(np.float64))
                    assert np.all(err <= lim), (name, mode, t, q, vn, float(np.max(err / lim)))
