"""Regenerates tests/golden/hp_sim_<mech>.npz (P1, P2, CP, FB): the two cases per mechanism of
tests/hp_sim.py (a generator state with nominal bodies; another with dm, dJ at their +-10% extremes
and the largest friction draw), the 70-digit truth of the parametrised variational-integrator step,
and E, A of the fp64 CPU evaluations ("lapack": gprx/vi.py vi_step as it stands, "rev": the bodies
reversed).  k is read from hp_phys_<mech>.npz by the tests.  Byte-identical on every run; about half
a minute (the four-bar's 48-unknown solves in mpmath).

    python tests/golden/make_golden_hp_sim.py [-j PROCS]
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import importlib.util
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path[:0] = [str(REPO), str(REPO / "tests")]

import hp_sim as S  # noqa: E402
from oracle import hp_physics as HP  # noqa: E402


def _save_npz():
    spec = importlib.util.spec_from_file_location("make_golden_hp", HERE / "make_golden_hp.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.save_npz


def solve(job):
    mech, ci = job
    name, cs, m, J, damp = S.cases(mech)[ci]
    ev = S.evaluations(mech, cs, S.DT, m, J, damp)
    assert all(r[2] == 0 and np.all(np.isfinite(r[0])) for r in ev.values()), (mech, name, ev)
    tr = S.truth(mech, cs, S.DT, ev["lapack"][0], m, J, damp)
    E, errs = S.error_scale(ev, tr["s"])
    return mech, ci, dict(cs=cs, m=m, J=J, damp=damp, truth=tr["s"], A=tr["A"], E=E, verr=errs,
                          its=np.array([ev[v][1] for v in ("lapack", "rev")]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    jobs = [(mech, ci) for mech in ("FB", "P2", "CP", "P1") for ci in range(len(S.CASES))]
    recs = {}
    with cf.ProcessPoolExecutor(a.j) as ex:
        for mech, ci, rec in ex.map(solve, jobs):
            recs.setdefault(mech, {})[ci] = rec
            print(f"{mech} {S.CASES[ci]}: E {rec['E']:.2e} A {rec['A']:.3g} errors {rec['verr'].tolist()} its {rec['its'].tolist()}",
                  flush=True)
    save = _save_npz()
    for mech in HP.MECHS:
        r = recs[mech]
        n = len(S.CASES)
        fx = dict(mech=np.array(mech), cases=np.array(S.CASES), dt=np.array(S.DT), variant_names=np.array(("lapack", "rev")))
        for key, name in (("cs", "cstates"), ("m", "mass"), ("J", "inertia"), ("damp", "damp"), ("truth", "truth"), ("A", "A"),
                          ("E", "E"), ("verr", "verr"), ("its", "its")):
            fx[name] = np.stack([np.asarray(r[c][key]) for c in range(n)])
        save(HERE / f"hp_sim_{mech}.npz", fx)


if __name__ == "__main__":
    main()
