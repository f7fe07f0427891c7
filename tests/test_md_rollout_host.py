"""The MeanDynamics device rollouts' host surface (no GPU): the header declares gprx_rollout_max_md /
gprx_rollout_min_md and the library exports them, a NULL context is refused before anything else is
looked at, gprx exports MeanDynamics, and sweep.run_group takes md_rollout."""
import inspect
import pathlib
import re

import pytest

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "gprx.h"
NEW = ("gprx_rollout_max_md", "gprx_rollout_min_md")


def test_header_declares_and_library_exports_the_entry_points():
    import gprx._lib as L

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in L.SIGNATURES
        assert getattr(L.lib, name) is not None
    # the prototypes' argument counts (include/gprx.h) against the binding's
    for name, n in zip(NEW, (18, 15)):
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == n == len(L.SIGNATURES[name][1])
    assert L.lib.gprx_abi_version() == 3  # entry points added, nothing changed


def test_null_context_is_invalid_argument():
    import gprx._lib as L

    assert L.lib.gprx_rollout_max_md(None, 2, 0.01, 5, 0.0, 0.0, 1, None, None, 1, None, 1, None, None, None, None, None,
                                     None) == L.INVALID_ARGUMENT
    assert L.lib.gprx_rollout_min_md(None, 2, 0, 0.01, 5, 0.0, 1, None, None, 1, None, None, None, None,
                                     None) == L.INVALID_ARGUMENT


def test_meandynamics_is_exported_and_parameter_free():
    import gprx

    assert "MeanDynamics" in gprx.__all__
    m = gprx.MeanDynamics("P2", 2, "min_sin")
    assert m.num_params() == 0 and (m.mech, m.mu_id, m.variant) == ("P2", 2, "min_sin")
    for bad in (("XX", 1, "max"), ("P1", 1, "mid"), ("P1", 2, "min"), ("P2", 0, "max"), ("P2", 7, "max")):
        with pytest.raises(ValueError):
            gprx.MeanDynamics(*bad)
    assert callable(gprx.rollout_min_md)
    from gprx import mdynamics, projection

    assert callable(projection.predictdynamics_md)
    assert callable(mdynamics.rollout_max_device) and callable(mdynamics.rollout_min_device)


def test_run_group_takes_md_rollout():
    from gprx import sweep

    p = inspect.signature(sweep.run_group).parameters["md_rollout"]
    assert p.default == "stepwise"  # the default path is the stepwise one
    assert sweep.MD_ROLLOUTS == ("stepwise", "device")
    with pytest.raises(ValueError):  # refused before any device work (ctx is not touched)
        sweep.run_group("P1", 8, "md_max", range(1), None, md_rollout="fused")
    with pytest.raises(SystemExit):  # the command line offers the same two values
        sweep.main(["--md-rollout", "fused"])
