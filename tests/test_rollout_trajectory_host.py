"""The recorded rollouts without a device: the four entry points exist with the header's signatures and
are bound, the ABI version is unchanged, a null context is refused, and the Python wrappers refuse a
bad rec or traj_group before any C call.  (The device tests are tests/test_rollout_trajectory.py.)"""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
NAMES = ("gprx_rollout_min_rec", "gprx_rollout_min_md_rec", "gprx_rollout_max_rec", "gprx_rollout_max_md_rec")
CTYPE = {"int": C.c_int, "double": C.c_double, "gprx_ctx*": C.c_void_p, "const int*": C.POINTER(C.c_int),
         "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "int*": C.POINTER(C.c_int),
         "gprx_batch* const*": C.POINTER(C.c_void_p)}


def _header_args(name):
    """The parameter types of `int name(...)` in include/gprx.h, as ctypes."""
    text = (REPO / "include" / "gprx.h").read_text()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        t = re.sub(r"\s+", " ", p.strip())
        t = re.sub(r"\s*\b\w+$", "", t)  # drop the parameter's name
        out.append(CTYPE[t])
    return out


def _one_launch_args(name):
    return _header_args(name[:-4])


@pytest.mark.parametrize("name", NAMES)
def test_symbols_are_bound_with_the_headers_signatures(name):
    from gprx import _lib as L

    fn = getattr(L.lib, name)
    assert fn.restype is C.c_int
    want = _header_args(name)
    assert list(fn.argtypes) == want, name
    # the one-launch call's arguments plus (R, rec, steps_per_launch, traj)
    assert want == _one_launch_args(name) + [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double)]
    assert list(getattr(L.lib, name[:-4]).argtypes) == _one_launch_args(name)


def test_abi_version_is_still_3():
    from gprx import _lib as L

    assert L.lib.gprx_abi_version() == 3
    assert re.search(r"#define\s+GPRX_ABI_VERSION\s+3\b", (REPO / "include" / "gprx.h").read_text())


@pytest.mark.parametrize("name", NAMES)
def test_null_context_is_an_invalid_argument(name):
    from gprx import _lib as L

    fn = getattr(L.lib, name)
    args = [None if t in (C.c_void_p,) or hasattr(t, "contents") else t(1) for t in fn.argtypes]
    assert fn(*args) == L.INVALID_ARGUMENT


def _wrappers():
    from gprx.projection import predictdynamics_md_rec, predictdynamics_rec
    from gprx.rollout import rollout_min_md_rec, rollout_min_rec

    mx = lambda f: (lambda rec, **kw: f("P1", [[]], np.zeros((2, 13)), 3, [9, 10, 11], rec, **kw))
    mn = lambda f: (lambda rec, **kw: f("P1", [[]], np.zeros((2, 2)), 3, rec, **kw))
    return [mx(predictdynamics_rec), mx(predictdynamics_md_rec), mn(rollout_min_rec), mn(rollout_min_md_rec)]


@pytest.mark.parametrize("k", range(4))
def test_wrappers_refuse_a_bad_rec_before_the_c_call(k):
    """steps = 3, T = 2; groups [[]] hold no GP, so anything that got past the checks would fail
    otherwise (a group needs its GPs)."""
    f = _wrappers()[k]
    for rec, what in (([2, 1], "non-decreasing"), ([[1, 2], [3, 2]], "non-decreasing"), ([0, 1], r"\[1, steps \+ 1\]"),
                      ([1, 5], r"\[1, steps \+ 1\]"), ([[1, 2]], "rec must be"), (np.zeros((2, 2, 2), dtype=int), "rec must be"),
                      ([1.0, 2.0], "integers")):
        with pytest.raises(ValueError, match=what):
            f(rec)
    with pytest.raises(ValueError, match="steps_per_launch"):
        f(None, steps_per_launch=-1)
    for tg in ([0], [0, 0, 0], [[0, 0]]):
        with pytest.raises(ValueError, match="traj_group"):
            f(None, traj_group=tg)
    with pytest.raises(ValueError, match="GP"):  # a good rec reaches the group check
        f([1, 1, 4])


def test_record_indices():
    from gprx.rollout import record_indices

    a = record_indices(None, 2, 3)
    assert a.dtype == np.int32 and a.flags.c_contiguous and a.tolist() == [[1, 2, 3, 4]] * 2
    assert record_indices([1, 1, 4], 2, 3).tolist() == [[1, 1, 4]] * 2
    assert record_indices([[1, 2], [4, 4]], 2, 3).tolist() == [[1, 2], [4, 4]]
    assert record_indices([], 2, 3).shape == (2, 0)
    assert record_indices(None, 1, 0).tolist() == [[1]]
