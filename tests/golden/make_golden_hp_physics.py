"""Regenerates tests/golden/hp_phys_<mech>.npz (P1, P2, CP, FB): the inputs of projectv! and of the
variational-integrator step, their high-precision truths (oracle/hp_physics.py), the fp64 CPU
variants' errors and iteration counts, E, A and k.  Byte-identical on every run; about 45 seconds
with the default 8 processes (the four-bar's 48-unknown solves in mpmath are nearly all of it).

    python tests/golden/make_golden_hp_physics.py [-j PROCS]

Cases per mechanism (SPECS; a case is one mechanism state with one predicted twist):
  gen   x3  generator states (gprx/data.py), predicted twist = the state's own + 0.1 N(0, 1): the
            family test_projection.py draws
  far   x2  the same with 1.0 N(0, 1): more Newton iterations, larger multipliers
  rest  x2  all velocities zero (x3 = x, q3 = q at the start)
  qneg  x1  the last body's quaternion negated: the same pose, qk of the other sign
  spin  x1  one angle turning at |w| = 0.9 * 2/dt, where sqrt(4/dt^2 - w.w) loses digits; velocities
            and predicted twist follow the discrete map's chords (see draw)
  P2 and FB: the first gen and the first far case again at dt = 0.02 and dt = 0.005
Everything else runs at dt = 0.01.  The step's input is the same state carrying the predicted twist
as its velocities (an inconsistent start, so Newton has work to do); rest and spin states are
stepped as they are.  From most spin states the step's first Newton iterate goes beyond |w| = 2/dt
(status 2 in every variant), which is no reference: the spin case tries up to 40 seeds where the
others try 10 (P1 takes its first, CP its 2nd, P2 its 13th, FB its 17th).
A case is stored only if every variant of both solves converges within 30 iterations ("qr" is run
to eps = 0 for 100 iterations by design and its count is stored as such); the seed of a case is
raised until that holds, which the run prints.  The four-bar's regularised iteration stalls on some
states (tests/test_md_rollout.py records one): such a state is no reference.
Besides the converged truths each file holds the truths of the iterates after 1 and 2 Newton
steps from the documented start (newton_iter = 1, 2 on the device), with their own E and A.
k is the largest ratio of a variant's error to max(E, eps A) over every mechanism, case, solve and
iterate, rounded up to a power of two and at least 4; it is stored in each file.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import importlib.util
import math
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO))

from oracle import hp_physics as HP  # noqa: E402

MAX_ITS = 30
ITERATES = (1, 2)
_BASE = [("gen", 0.1, 0.01)] * 3 + [("far", 1.0, 0.01)] * 2 + [("rest", 0.1, 0.01)] * 2 + [("qneg", 0.1, 0.01), ("spin", 0.1, 0.01)]
_DTS = [("gen", 0.1, 0.02), ("far", 1.0, 0.02), ("gen", 0.1, 0.005), ("far", 1.0, 0.005)]
SPECS = {"P1": _BASE, "P2": _BASE + _DTS, "CP": _BASE, "FB": _BASE + _DTS}


def _save_npz():
    spec = importlib.util.spec_from_file_location("make_golden_hp", HERE / "make_golden_hp.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.save_npz


SPIN = 0.9        # |w| of the spin case over 2/dt
SPIN_SEEDS = 40   # seeds tried for the spin case, 10 for every other


def _spin(D, mech, m, dt, frac):
    """One angle turning at |w| = frac * 2/dt, every other rate zero.  The linear velocities are the
    chords of the discrete map (a wbar step turns by 2 asin(w dt / 2)), so that pose 2 lies on the
    constraints; the generator's tangent velocities would leave it 0.9 l away from them.  Returns
    the CState (nb, 13) and the twist that continues the turn (6 nb)."""
    nb = HP.nbodies(mech)
    angle, rate = {"P1": ("th", "om"), "P2": ("t1", "o1"), "CP": ("th", "om"), "FB": ("t1", "o1")}[mech]
    w = frac * 2.0 / dt * float(np.sign(m[rate][0]))
    turn = 2.0 * math.asin(w * dt / 2.0)
    still = {k: (v if k in ("th", "t1", "t2", "x") else np.zeros(1)) for k, v in m.items()}
    pos = [D._cstates(mech, {**still, angle: still[angle] + j * turn})[:, 0].reshape(nb, 13)[:, 0:3] for j in range(3)]
    cs = D._cstates(mech, {**still, rate: np.array([w])})[:, 0].reshape(nb, 13)
    cs[:, 7:10] = (pos[1] - pos[0]) / dt
    return cs, np.concatenate([(pos[2] - pos[1]) / dt, cs[:, 10:13]], axis=1).reshape(-1)


def draw(mech, ci, seed):
    """The state and the predicted twist of case ci of `mech` at `seed`, and the step's state."""
    kind, pert, dt = SPECS[mech][ci]
    D = HP._load_gprx("data")
    nb = HP.nbodies(mech)
    rng = np.random.default_rng(seed)
    m = D._sample_minimal(mech, 1, rng)
    if kind == "spin":
        cs, base = _spin(D, mech, m, dt, SPIN)
    else:
        cs = D._cstates(mech, m)[:, 0].reshape(nb, 13)
    if kind == "rest":
        cs[:, 7:] = 0.0
    if kind == "qneg":
        cs[nb - 1, 3:7] = -cs[nb - 1, 3:7]
    cs = cs.reshape(-1)
    su = (base if kind == "spin" else HP._twist_of(cs, nb)) + pert * rng.standard_normal(6 * nb)
    vs = cs.reshape(nb, 13).copy()
    if kind not in ("rest", "spin"):
        vs[:, 7:13] = su.reshape(nb, 6)
    return cs, su, vs.reshape(-1), dt


def _converged(var):
    """Every variant but "qr" (run to eps = 0 by design) stops within MAX_ITS iterations with status 0
    (the step reports one; projectv stops only by convergence) and a finite twist."""
    lu = [var[v] for v in HP.VARIANTS if v != "qr"]
    return (max(r[1] for r in lu) <= MAX_ITS and all(len(r) < 3 or r[2] == 0 for r in lu)
            and all(np.all(np.isfinite(r[0])) for r in var.values()))


def candidates(mech, ci):
    """The seeds of a case in the order they are tried."""
    seed0 = 1000 * (1 + HP.MECHS.index(mech)) + 10 * ci
    seeds = list(range(seed0, seed0 + 10))
    if SPECS[mech][ci][0] == "spin":
        seeds += list(range(100 * seed0, 100 * seed0 + SPIN_SEEDS - 10))
    return seeds


def solve(job):
    mech, ci = job
    kind = SPECS[mech][ci][0]
    for seed in candidates(mech, ci):
        cs, su, vs, dt = draw(mech, ci, seed)
        its = {}
        try:
            with HP.quiet():
                vv = HP.variants_vi(mech, vs, dt, qr_eps=0.0)  # the step first: it is what fails on a spin state
                its["step"] = [vv[v][1:] for v in HP.VARIANTS]
                ok = _converged(vv)
                if ok:
                    vp = HP.variants_projectv(mech, cs, su, dt, qr_eps=0.0)
                    its["projectv"] = [vp[v][1] for v in HP.VARIANTS]
                    ok = _converged(vp)
        except (ValueError, HP.Singular, np.linalg.LinAlgError) as e:  # an iterate beyond |w| = 2/dt, a singular matrix
            ok, its["raised"] = False, type(e).__name__
        if ok:
            break
        print(f"{mech} case {ci} ({kind}): seed {seed} dropped, {its}", flush=True)
    else:
        raise RuntimeError(f"{mech} case {ci}: no seed converges")
    rec = dict(seed=seed, cs=cs, su=su, vs=vs, dt=dt)
    for name, var, tr in (("pj", vp, HP.truth_projectv(mech, cs, su, dt, vp["lapack"][0])),
                          ("vi", vv, HP.truth_vi(mech, vs, dt, vv["lapack"][0]))):
        E, errs = HP.error_scale(var, tr["s"])
        rec[name] = dict(truth=tr["s"], A=tr["A"], E=E, verr=errs, its=np.array([var[v][1] for v in HP.VARIANTS]))
    for k in ITERATES:
        for name, tr, var in (("pj", HP.iterate_projectv(mech, cs, su, dt, k), HP.variants_projectv(mech, cs, su, dt, iters=k)),
                              ("vi", HP.iterate_vi(mech, vs, dt, k), HP.variants_vi(mech, vs, dt, iters=k))):
            E, errs = HP.error_scale(var, tr["s"])
            rec[f"{name}_it{k}"] = dict(truth=tr["s"], A=tr["A"], E=E, verr=errs)
    return mech, ci, rec


def assemble(mech, recs):
    """The fixture arrays of a mechanism and its largest variant ratio."""
    n = len(recs)
    fx = dict(mech=np.array(mech), kinds=np.array([s[0] for s in SPECS[mech]]), variant_names=np.array(HP.VARIANTS),
              seeds=np.array([recs[c]["seed"] for c in range(n)]),
              dt=np.array([recs[c]["dt"] for c in range(n)]),
              cstates=np.stack([recs[c]["cs"] for c in range(n)]), vw_pred=np.stack([recs[c]["su"] for c in range(n)]),
              vi_states=np.stack([recs[c]["vs"] for c in range(n)]), iterates=np.array(ITERATES))
    worst = 0.0
    for name in ("pj", "vi"):
        for key in ("truth", "A", "E", "verr", "its"):
            fx[f"{name}_{key}"] = np.stack([np.asarray(recs[c][name][key]) for c in range(n)])
        for key in ("truth", "A", "E", "verr"):
            fx[f"{name}_it_{key}"] = np.stack([np.stack([np.asarray(recs[c][f"{name}_it{k}"][key]) for c in range(n)])
                                               for k in ITERATES])
        for E, A, verr in ((fx[f"{name}_E"], fx[f"{name}_A"], fx[f"{name}_verr"]),
                           *((fx[f"{name}_it_E"][i], fx[f"{name}_it_A"][i], fx[f"{name}_it_verr"][i]) for i in range(len(ITERATES)))):
            for c in range(n):
                worst = max(worst, max(HP.ratio(e, E[c], A[c]) for e in verr[c]))
    return fx, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    jobs = [(mech, ci) for mech in ("FB", "P2", "CP", "P1") for ci in range(len(SPECS[mech]))]
    recs = {}
    with cf.ProcessPoolExecutor(a.j) as ex:
        for mech, ci, rec in ex.map(solve, jobs):
            recs.setdefault(mech, {})[ci] = rec
            print(f"{mech} case {ci} ({SPECS[mech][ci][0]}, dt {rec['dt']}): seed {rec['seed']}, projectv E {rec['pj']['E']:.2e} "
                  f"its {rec['pj']['its'].tolist()}, step E {rec['vi']['E']:.2e} its {rec['vi']['its'].tolist()}", flush=True)
    out, worst = {}, 0.0
    for mech in HP.MECHS:
        out[mech], w = assemble(mech, recs[mech])
        print(f"{mech}: largest variant ratio {w:.2f}")
        worst = max(worst, w)
    k = max(4.0, 2.0 ** math.ceil(math.log2(worst)))
    print(f"largest ratio {worst:.3f} -> k = {k}")
    save = _save_npz()
    for mech, fx in out.items():
        fx["k"] = np.array(k)
        save(HERE / f"hp_phys_{mech}.npz", fx)


if __name__ == "__main__":
    main()
