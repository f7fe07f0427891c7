"""gprx_batch_optimize_obj, host side (no GPU): the symbol's arity and the two objective constants in
the header, the ctypes table and the Julia shim; the objective check of GPBatch.optimize before any
device call; NULL handles and unknown objectives; and the help text of the search's --objective."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from gprx import _lib as L

REPO = pathlib.Path(__file__).resolve().parents[1]
NAME = "gprx_batch_optimize_obj"


def header():
    return (REPO / "include" / "gprx.h").read_text()


def test_symbol_and_constants_in_header_ctypes_and_julia():
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    jl = (REPO / "gpr.jl_amd" / "julia" / "GPRx.jl").read_text()
    m = re.search(r"^int " + NAME + r"\(([^)]*)\);", hdr, flags=re.M)
    assert m, NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 == len(L.SIGNATURES[NAME][1]) and args[1] == "int objective"
    # gprx_batch_optimize's arguments behind the objective
    base = re.search(r"^int gprx_batch_optimize\(([^)]*)\);", hdr, flags=re.M)
    assert [a.strip() for a in base.group(1).split(",")] == args[:1] + args[2:]
    assert L.SIGNATURES[NAME][0] is C.c_int and L.SIGNATURES[NAME][1][1] is C.c_int
    assert L.SIGNATURES[NAME][1][:1] + L.SIGNATURES[NAME][1][2:] == L.SIGNATURES["gprx_batch_optimize"][1]
    assert hasattr(L.lib, NAME)
    # the ccall: the symbol, and one argument type more than gprx_batch_optimize's
    call = re.search(r"ccall\(\(:" + NAME + r", LIB\), Cint,\s*\(([^)]*)\)", jl)
    assert call and len(call.group(1).split(",")) == 11 and call.group(1).split(",")[1].strip() == "Cint"
    consts = dict(re.findall(r"^#define GPRX_OBJ_(MLL|LOO) (\d+)", header(), flags=re.M))
    assert consts == {"MLL": "0", "LOO": "1"}
    assert (L.OBJ_MLL, L.OBJ_LOO) == (int(consts["MLL"]), int(consts["LOO"]))
    assert f"const OBJ_MLL, OBJ_LOO = Cint({consts['MLL']}), Cint({consts['LOO']})" in jl
    assert "objective::Symbol=:mll" in jl
    assert L.lib.gprx_abi_version() == 3 and "#define GPRX_ABI_VERSION 3\n" in header()


def test_null_handle_and_unknown_objective_are_invalid_arguments():
    th = np.zeros(4)
    for obj in (L.OBJ_MLL, L.OBJ_LOO, 7, -1):
        assert L.lib.gprx_batch_optimize_obj(None, obj, L.dptr(th), None, None, None, None, None, None, None,
                                             None) == L.INVALID_ARGUMENT


def test_gpbatch_optimize_rejects_an_unknown_objective_before_any_device_call():
    """No batch handle, no context: the check comes first, so nothing of the library is reached."""
    from gprx.batch import GPBatch

    b = GPBatch.__new__(GPBatch)
    b.h = None  # what close() leaves; __del__ then has nothing to free
    with pytest.raises(ValueError, match="objective"):
        b.optimize(np.zeros((1, 3)), objective="x")


def test_search_help_names_the_device_optimiser_for_loo(capsys):
    from gprx import search

    with pytest.raises(SystemExit) as e:
        search.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--objective" in out and "logp_LOO" in " ".join(out.split())
    assert "host loop" not in " ".join(out.split())
    import inspect

    from gprx import shard, sweep

    for fn in (search.run_search_group, sweep.run_group, shard.RankBatch.optimize):
        doc = " ".join(inspect.getdoc(fn).split())
        assert "on the host loop" not in doc and "optimize_batch's host loop" not in doc, fn.__qualname__
