"""The device against the 50-digit truth of tests/golden/hp_*.npz (oracle/hp_oracle.py,
tests/golden/make_golden_hp.py), in both distance modes.

Bound, elementwise, for LML, every gradient component, alpha, mu*, sigma^2* (truth clamped at 0) and
the joint Sigma:  |device - truth| <= k max(E_q, eps A_q)  with the fixture's k, E_q (geometric mean
over the fp64 CPU variants of their largest error against the truth, per theta and mode) and A_q (sum
of the absolute terms of q's last reduction).  The gradient is held a second time per component
("grad_comp"): to k_grad max(E_grad[p], eps A_q[p]), E_grad and k_grad being the same figures formed
for each component alone, so that a small component is held to its own scale and not to g[0]'s.  Nothing here is fitted to the device: the device may
sit as far from the truth as independent correct fp64 evaluations sit from each other.  A gradient
component whose truth is exactly zero (a constant coordinate) must be exactly zero in direct mode; in
expanded mode its floor takes the operands a^2 + b^2 of the cancellation.

A fixture's slots are its (theta, target) pairs, repeated up to the batch size; repeated slots must
be bit-identical.  Each (fixture, batch size, mode) runs on the device once and the tests share the
record.  Every bound test prints `case mode quantity err_device E_q ratio` per quantity, ratio =
max err / max(E_q, eps A_q) <= k; DESIGN.md section 2 holds the table of one run.
"""
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
EPS = 2.0 ** -52
QUANTITIES = ("mll", "grad", "alpha", "mu", "var", "cov")
_FX, _DEV = {}, {}


def fixture(name):
    if name not in _FX:
        with np.load(GOLDEN / f"hp_{name}.npz") as z:
            _FX[name] = {k: z[k] for k in z.files}
        assert tuple(_FX[name]["quantities"]) == QUANTITIES
    return _FX[name]


def _runs():
    out = []
    # the GP cases a..e of make_golden_hp.py (a case "f" needs the pattern widened, here and in
    # test_hp_oracle.py); hp_phys_* are test_hp_physics.py's
    for p in sorted(GOLDEN.glob("hp_[a-e]_*.npz")):
        with np.load(p) as z:
            out += [(p.stem[3:], int(B)) for B in z["B"]]
    return out


RUNS = _runs()
RUN_IDS = [f"{n}-B{B}" if B else n for n, B in RUNS]
OPTION_RUNS = [(n, B, "graphs") for n, B in RUNS if n[0] in "cd"]


@pytest.fixture(scope="module")
def gprx():
    import gprx as g

    return g


@pytest.fixture(scope="module")
def ctx(gprx):
    c = gprx.Context(0)
    yield c
    c.close()


def slots_of(fx, B):
    pairs = [(t, g) for t in range(fx["thetas"].shape[0]) for g in range(fx["Y"].shape[0])]
    return [pairs[s % len(pairs)] for s in range(B or len(pairs))]


def evaluate(gprx, c, fx, B, mode):
    """set_train, set_test, run(grad, predict), alpha and, where Sigma is stored, predict_cov."""
    slots = slots_of(fx, B)
    X, Xs = fx["X"], fx["Xs"]
    c.set_dist_mode(mode)
    b = None
    try:
        b = gprx.GPBatch(len(slots), X.shape[0], X.shape[1], Xs.shape[1], ctx=c)
        b.set_train(X, np.stack([fx["Y"][g] for _, g in slots]))
        b.set_test(Xs)
        r = b.run(np.stack([fx["thetas"][t] for t, _ in slots]), grad=True, predict=True)
        rec = dict(status=r["status"].copy(), mll=r["mll"].copy(), grad=r["grad"].copy(), mu=np.array(r["mu"]),
                   var=np.array(r["var"]), alpha=b.alpha())
        if "cov" in fx:
            rec["cov"] = b.predict_cov()[1]
    finally:
        if b is not None:
            b.close()
        c.set_dist_mode(1)
    return rec


def device(gprx, ctx, name, B, mode):
    if (name, B, mode) not in _DEV:
        _DEV[name, B, mode] = evaluate(gprx, ctx, fixture(name), B, mode)
    return _DEV[name, B, mode]


def truth_and_floor(fx, q, t, g, mode):
    """Truth and A_q of slot (theta t, target g); sigma^2* and Sigma do not depend on the target."""
    if q in ("var", "cov"):
        tr, A = fx[q][t], fx["A_" + q][t]
        return (np.maximum(tr, 0.0) if q == "var" else tr), A
    tr, A = fx[q][t, g], fx["A_" + q][t, g]
    if q == "grad" and mode == 0:
        A = np.where(tr == 0.0, fx["A_grad_exp"][t, g], A)
    return tr, A


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_device_within_variant_spread_of_truth(gprx, ctx, name, B, mode):
    fx = fixture(name)
    dev = device(gprx, ctx, name, B, mode)
    k = float(fx["k"])
    assert np.all(dev["status"] == 0), dev["status"]
    misses = []
    for qi, q in enumerate(QUANTITIES):
        if q not in dev:
            continue
        for label, lim in ((q, k),) + ((("grad_comp", float(fx["k_grad"])),) if q == "grad" else ()):
            worst = (-1.0, 0.0, 0.0)
            for s, (t, g) in enumerate(slots_of(fx, B)):
                tr, A = truth_and_floor(fx, q, t, g, mode)
                err = np.abs(dev[q][s] - tr)
                E = fx["E_grad"][mode, t] if label == "grad_comp" else float(fx["E"][mode, t, qi])
                den = np.maximum(E, EPS * A)
                ratio = float(np.max(np.divide(err, den, out=np.where(err > 0, np.inf, 0.0), where=den > 0)))
                worst = max(worst, (ratio, float(np.max(err)), float(np.max(E))))
                if label == "grad" and mode == 1 and np.any(dev[q][s][tr == 0.0] != 0.0):
                    misses.append(f"{q} slot {s}: a constant coordinate's component is not exactly zero")
            print(f"{name}{'-B%d' % B if B else ''} mode {mode} {label} err_device {worst[1]:.3e} E_q {worst[2]:.3e} "
                  f"ratio {worst[0]:.3f}")
            if not worst[0] <= lim:
                misses.append(f"{label}: ratio {worst[0]:.3f} > {lim}")
    assert not misses, misses


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_repeated_slots_are_bit_identical(gprx, ctx, name, B, mode):
    fx = fixture(name)
    dev = device(gprx, ctx, name, B, mode)
    first = {}
    for s, pair in enumerate(slots_of(fx, B)):
        s0 = first.setdefault(pair, s)
        for q in dev:
            np.testing.assert_array_equal(dev[q][s], dev[q][s0], err_msg=f"{q} slots {s0}, {s}")
    if "cov" in dev:  # Sigma and sigma^2* do not depend on the target
        for s, (t, _) in enumerate(slots_of(fx, B)):
            s0 = [u for u, (tu, _) in enumerate(slots_of(fx, B)) if tu == t][0]
            np.testing.assert_array_equal(dev["cov"][s], dev["cov"][s0])
            np.testing.assert_array_equal(dev["var"][s], dev["var"][s0])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,B", [r for r in RUNS if "cov" in fixture(r[0])],
                         ids=[i for r, i in zip(RUNS, RUN_IDS) if "cov" in fixture(r[0])])
def test_cov_diagonal_agrees_with_variance(gprx, ctx, name, B, mode):
    fx = fixture(name)
    dev = device(gprx, ctx, name, B, mode)
    qi = QUANTITIES.index("var")
    for s, (t, _) in enumerate(slots_of(fx, B)):
        lim = float(fx["k"]) * np.maximum(float(fx["E"][mode, t, qi]), EPS * fx["A_var"][t])
        assert np.all(np.abs(np.maximum(np.diag(dev["cov"][s]), 0.0) - dev["var"][s]) <= lim)


@pytest.mark.parametrize("name,B,option", OPTION_RUNS, ids=[f"{n}-{o}" for n, _, o in OPTION_RUNS])
def test_launch_options_are_bit_equal(gprx, ctx, name, B, option):
    """Captured graphs are a launch choice only."""
    from gprx import _lib as L

    dev = device(gprx, ctx, name, B, 1)
    c = gprx.Context(0)
    try:
        c.set_option(L.OPT_GRAPHS, 1)
        got = evaluate(gprx, c, fixture(name), B, 1)
    finally:
        c.close()
    for q in dev:
        np.testing.assert_array_equal(got[q], dev[q], err_msg=q)
