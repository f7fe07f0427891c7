"""The reference's datasets, simulated on the device: a numpy restatement of
examples/utils/data/datasets.jl (the per-dataset parameter draws and the per-experiment start draws),
examples/utils/data/simulations.jl (setPosition! / setVelocity! of the start, the bodies, control!)
and examples/parallel/dataframes.jl (generate_dataframes: which storage indices become samples),
with every trajectory of a dataset run by one gprx_simulate call (gprx.projection.simulate).

Per mechanism the reference builds Ndfs = 100 datasets; each draws its own body masses (dm), inertias
(dJ) and viscous joint friction, and simulates 100 training trajectories (50 of exp1, 50 of exp2) and
100 test trajectories (exptest) of 2 / dtsim variational-integrator steps at dtsim = 1e-4.  Training
samples are storage pairs (j, j + scaling), test samples (j, j + scaling (simsteps + 1)), scaling =
0.01 / dtsim, so a pair is one (or simsteps + 1) steps of the experiments' mechanism dt = 0.01 apart.

What is not the reference's: the random stream (numpy.random.default_rng(seed); Julia's cannot be
matched, and the reference's threads make its own order of draws nondeterministic), and the physics'
parity with ConstrainedDynamics 0.7.4, which is unpinned (gprx/vi.py; the storage convention --
index 1 is the start, saveToStorage! before each step -- and the force terms are recalled, not read).

Four-bar datasets are refused (generate_dataset raises at once unless config["fourbar"] is set, for
experiments).  Two causes were found on the host restatement (dataset simulation).
The impulses' fixed regulariser 1e-10 (gprx/vi.py REGULARIZER, the experiments' value at dt = 0.01) weighs
1e4 times more against the constraint block G (M/dt)^-1 Gpos^T ~ dt^2 at dtsim = 1e-4, and the loop
constraints slip (a start 0.1 rad from the stretched configuration fails at its third step; on the device
every trajectory had failed by step 15 000); the generator therefore passes 1e-10 (dtsim / 0.01)^2.  And the
folded configuration (links 1 and 2 parallel), which a swinging four-bar crosses, is a kinematic
singularity at which the loop's branches meet: past it the solve no longer converges with any regulariser
tried.  With the scaled one 145 of 200 trajectories reach the end of a pass (209.6 s), but what they do past
the fold is not verified.

At dtsim = 1e-4 newton!'s eps = 1e-10 is below the multipliers' rounding floor; gprx_simulate ends such a
stagnated solve instead of running all newton_iter iterations.

Config keys (getconfig, datasets.jl:110-114, in ASCII): dtsim, trainsamples, testsamples, simsteps,
sigma = {dm, dJ}; and, beyond the reference, friction (a factor on the friction draws; 0: none),
max_trajectories (100), eps and newton_iter (newton!'s 1e-10 and 100), regularizer (None: scaled as above), fourbar (False).
"""
from __future__ import annotations

import json
import math
import pathlib

import numpy as np

from . import data, dataset, vi

NBODIES = data.NBODIES
FRICTION_SCALE = {"P1": [1.0], "P2": [2.0, 0.5], "CP": [1.0, 0.5], "FB": [2.0, 0.5, 2.0, 0.5]}  # datasets.jl:15,35,57,78
MAX_RUNS = 10  # _run_experiment!'s maxruns (dataframes.jl:41)
# the bodies whose (angle, rate) applynoise! perturbs (transformations.jl:48-140); CP also the cart's y, v_y
_NOISY_BODIES = {"P1": (0,), "P2": (0, 1), "CP": (1,), "FB": (0, 2)}


def default_config() -> dict:
    """getconfig() (datasets.jl:110-114)."""
    return dict(dtsim=1e-4, Ndfs=100, trainsamples=2048, testsamples=100, simsteps=20, sigma=dict(dm=0.1, dJ=0.1),
                friction=1.0, max_trajectories=100, eps=1e-10, newton_iter=100, regularizer=None, fourbar=False)


def _int(x: float) -> int:
    """Julia's Int(x): exact or an error."""
    if x != int(x):
        raise ValueError(f"Int({x!r}) is inexact")
    return int(x)


# ---- datasets.jl: the draws ---------------------------------------------------------------------
def draw_parameters(mech: str, config: dict, rng) -> dict:
    """dm, dJ, friction of one dataset, drawn in the reference's order (datasets.jl:15-17, 35-37,
    55-57, 76-78).  dm, friction: (nb,); dJ: (nb,) (CP: one value, the pole's)."""
    nb = NBODIES[mech]
    sm, sj = float(config["sigma"]["dm"]), float(config["sigma"]["dJ"])
    fs = float(config.get("friction", 1.0)) * np.asarray(FRICTION_SCALE[mech])
    pert = lambda s, n: 1 + s * 2 * (rng.random(n) - 0.5)  # noqa: E731
    if mech in ("P1", "P2"):
        fr = rng.random(nb) * fs
        dJ = pert(sj, nb)
        dm = pert(sm, nb)
    elif mech == "CP":
        dJ = pert(sj, 1)
        dm = pert(sm, nb)
        fr = rng.random(nb) * fs
    elif mech == "FB":
        dJ = pert(sj, nb)
        dm = pert(sm, nb)
        fr = rng.random(nb) * fs
    else:
        raise ValueError(f"unknown mechanism {mech}")
    return dict(dm=dm, dJ=dJ, friction=fr)


def draw_start(mech: str, exp: str, rng) -> dict:
    """The start of one exp1 / exp2 / exptest trajectory in minimal coordinates, as data._cstates takes
    them (datasets.jl:18-20, 38-40, 59-61, 79-81).  exp2 starts in the upper half: an angle in
    [-pi, -pi/2] u [pi/2, pi]."""
    if exp not in ("exp1", "exp2", "exptest"):
        raise ValueError(exp)
    u = rng.random
    upper = lambda: (u() / 2 + 0.5) * rng.choice((-1, 1))  # noqa: E731
    pi = math.pi
    if mech == "P1":
        th = {"exp1": lambda: (u() - 0.5) * pi, "exp2": lambda: upper() * pi, "exptest": lambda: (u() - 0.5) * 2 * pi}[exp]()
        return dict(th=th, om=2 * (u() - 0.5))
    if mech == "P2":
        if exp == "exp1":
            t = (u(2) - 0.5) * np.array([pi, 2 * pi])
        elif exp == "exp2":
            t = np.array([upper(), 2 * (u() - 0.5)]) * pi
        else:
            t = (u(2) - 0.5) * 2 * pi
        return dict(t1=t[0], t2=t[1], o1=0.0, o2=0.0)
    if mech == "CP":
        x = u() - 0.5
        th = {"exp1": lambda: (u() - 0.5) * pi, "exp2": lambda: upper() * pi, "exptest": lambda: 2 * pi * (u() - 0.5)}[exp]()
        return dict(x=x, th=th, v=2 * (u() - 0.5), om=2 * (u() - 0.5))
    if mech == "FB":
        t = (u(2) - 0.5) * pi
        return dict(t1=t[0], t2=t[1], o1=0.0, o2=0.0)
    raise ValueError(f"unknown mechanism {mech}")


# ---- simulations.jl: the start state ----------------------------------------------------------------
def initial_cstate(mech: str, m: dict) -> np.ndarray:
    """setPosition! / setVelocity! of the experiments (simulations.jl:25-27, 75-78, 129-132, 171-189) for
    n starts in minimal coordinates (draw_start's keys; scalars or (n,) arrays): the CStates (n, 13 nb).
    Positions and RotX quaternions from the kinematic chains of data._cstates; the linear velocities are
    the exact derivatives v = w x r along the chain, not the noise model's forward difference.  P2's
    second link has the absolute angle t1 + t2 and rate o1 + o2.  The four-bar's (t1, t2) are the
    reference's thetastart: links 1 and 4 at the absolute angle t1 + t2, links 2 and 3 at t1 - t2, at
    rest."""
    m = {k: np.atleast_1d(np.asarray(v, dtype=np.float64)) for k, v in m.items()}
    if mech == "FB":
        z = np.zeros_like(m["t1"])
        return data._cstates(mech, dict(t1=m["t1"] + m["t2"], t2=m["t1"] - m["t2"], o1=z, o2=z)).T.copy()
    X = data._cstates(mech, m).T.copy()  # (n, 13 nb): x, q, w as wanted; v by the forward difference
    if mech == "P1":
        th, om, l = m["th"], m["om"], 1.0
        X[:, 8], X[:, 9] = l / 2 * np.cos(th) * om, l / 2 * np.sin(th) * om
    elif mech == "P2":
        t1, o1, l1, l2 = m["t1"], m["o1"], 1.0, 1.0
        t12, o12 = m["t1"] + m["t2"], m["o1"] + m["o2"]
        X[:, 8], X[:, 9] = l1 / 2 * np.cos(t1) * o1, l1 / 2 * np.sin(t1) * o1
        X[:, 21] = l1 * np.cos(t1) * o1 + l2 / 2 * np.cos(t12) * o12
        X[:, 22] = l1 * np.sin(t1) * o1 + l2 / 2 * np.sin(t12) * o12
    elif mech == "CP":
        th, om, l = m["th"], m["om"], 0.5
        X[:, 21], X[:, 22] = m["v"] + l / 2 * np.cos(th) * om, l / 2 * np.sin(th) * om
    else:
        raise ValueError(f"unknown mechanism {mech}")
    return X


# ---- dataframes.jl: which storage indices become samples --------------------------------------------
def sample_indices(rng, nsamples: int, lo: int, hi: int, scaling: int) -> np.ndarray:
    """_pushsamples! (dataframes.jl:58-75): nsamples draws uniform in samplerange = lo:hi, a draw within
    +-2 scaling of a kept index rejected, so that no two samples' (j, j + scaling) pairs intersect."""
    n = hi - lo + 1
    assert (4 * scaling + 1) * nsamples < n, "samplerange too short for the samples"
    kept: list[int] = []
    for _ in range(nsamples):
        while True:
            j = int(rng.integers(lo, hi + 1))
            if not any(abs(j - k) <= 2 * scaling for k in kept):
                break
        kept.append(j)
    return np.array(kept, dtype=np.int64)


def uniform_indices(nsamples: int, lo: int, hi: int) -> np.ndarray:
    """_pushuniformsamples! (dataframes.jl:80-93): samplerange[i div(length, nsamples)], i = 1..nsamples;
    one sample: div(length, 2) itself."""
    n = hi - lo + 1
    assert n > nsamples
    if nsamples > 1:
        return np.array([lo + i * (n // nsamples) - 1 for i in range(1, nsamples + 1)], dtype=np.int64)
    return np.array([n // 2], dtype=np.int64)


def plan(config: dict) -> dict:
    """generate_dataframes' counts and ranges (dataframes.jl:9-14, 31-35)."""
    maxt = int(config.get("max_trajectories", 100))
    dtsim = float(config["dtsim"])
    scaling = _int(0.01 / dtsim)
    nsteps = 2 * _int(1 / dtsim)
    ntrain = min(int(config["trainsamples"]), maxt) // 2 * 2  # two loops of div(Ntrajectories, 2)
    ntest = min(int(config["testsamples"]), maxt)
    off_test = scaling * (int(config["simsteps"]) + 1)
    return dict(scaling=scaling, nsteps=nsteps, ntrain=ntrain, ntest=ntest,
                train_samples=int(math.ceil(config["trainsamples"] / maxt)),
                test_samples=int(math.ceil(config["testsamples"] / ntest)) if ntest else 0,
                train_range=(1, nsteps - scaling), train_off=scaling, test_range=(1, nsteps - off_test), test_off=off_test)


def regularizer(mech: str, config: dict) -> float:
    """The impulses' regularisation of a dataset's simulations: config["regularizer"], or the
    experiments' value at dt = 0.01 scaled with dtsim^2 as the constraint block it stands against."""
    r = config.get("regularizer")
    return float(r) if r is not None else vi.REGULARIZER[mech] * (float(config["dtsim"]) / 0.01) ** 2


def _simulate(mech, start, steps, rec, par, config, ctx):
    from .projection import simulate

    m, J = vi.body_params(mech, par["dm"], par["dJ"])
    return simulate(mech, start, steps, rec, m, J, vi.friction_damp(mech, par["friction"]), regularizer=regularizer(mech, config),
                    newton_iter=int(config.get("newton_iter", 100)), eps=float(config.get("eps", 1e-10)),
                    dt=float(config["dtsim"]), ctx=ctx)


def generate_dataset(mech: str, seed: int, config: dict | None = None, ctx=None) -> dict:
    """One dataset of generate<mech>dataset (datasets.jl) through generate_dataframes(...;
    generate_uniform = true) (P1, P2, CP; the four-bar is refused, see the module's docstring): parameters, starts and sample indices drawn beforehand, every
    trajectory in one gprx_simulate call that records only the sampled storage indices.  A trajectory
    whose simulation fails (a step with status 2, where the reference throws) is drawn and run again,
    at most MAX_RUNS times in all, as _run_experiment! does; then RuntimeError.
    Returns train_old / train_curr (rows: CStates), test_old / test_future, their *_uniform variants,
    and dm, dJ, friction, mech, seed, config."""
    config = {**default_config(), **(config or {})}
    if mech == "FB" and not config.get("fourbar"):
        raise ValueError("four-bar datasets are not supported: past the folded configuration its simulation does not "
                         "converge and the trajectories fail (gprx.simdata's docstring); config['fourbar'] = True tries anyway")
    rng = np.random.default_rng(seed)
    P = plan(config)
    par = draw_parameters(mech, config, rng)
    kinds = ["exp1"] * (P["ntrain"] // 2) + ["exp2"] * (P["ntrain"] // 2) + ["exptest"] * P["ntest"]
    T = len(kinds)
    if T == 0:
        raise ValueError("the config asks for no trajectory")
    starts = [draw_start(mech, k, rng) for k in kinds]
    # per trajectory the wanted storage indices [random old, random paired, uniform old, uniform paired]
    want = []
    for k in kinds:
        ns, (lo, hi), off = ((P["train_samples"], P["train_range"], P["train_off"]) if k != "exptest" else
                             (P["test_samples"], P["test_range"], P["test_off"]))
        j, ju = sample_indices(rng, ns, lo, hi, P["scaling"]), uniform_indices(ns, lo, hi)
        want.append(np.concatenate([j, j + off, ju, ju + off]))
    R = max(len(w) for w in want)
    rec = np.empty((T, R), dtype=np.int32)
    order = []
    for t, w in enumerate(want):  # sorted for the device, padded with the last index
        o = np.argsort(w, kind="stable")
        order.append(o)
        rec[t, :len(w)] = w[o]
        rec[t, len(w):] = w[o][-1]
    steps = P["nsteps"] - 1  # the storage holds nsteps states
    out = np.empty((T, R, 13 * NBODIES[mech]))
    todo = np.arange(T)
    for _ in range(MAX_RUNS):
        S = np.concatenate([initial_cstate(mech, starts[t]) for t in todo])
        o, st = _simulate(mech, S, steps, rec[todo], par, config, ctx)
        out[todo] = o
        if len(todo) >= 8 and np.all(st == 2):  # nothing to hope for from another pass
            raise RuntimeError(f"every one of the {len(todo)} trajectories of a pass failed")
        todo = todo[st == 2]
        if len(todo) == 0:
            break
        for t in todo:
            starts[t] = draw_start(mech, kinds[t], rng)
    else:
        raise RuntimeError(f"Experiment failed to execute {MAX_RUNS} times")
    rows = {k: [] for k in ("train_old", "train_curr", "train_old_uniform", "train_curr_uniform", "test_old", "test_future",
                            "test_old_uniform", "test_future_uniform")}
    for t, k in enumerate(kinds):
        n = len(want[t]) // 4
        got = np.empty((4 * n, out.shape[2]))
        got[order[t]] = out[t, :4 * n]
        a, b = ("train_old", "train_curr") if k != "exptest" else ("test_old", "test_future")
        rows[a].append(got[0:n])
        rows[b].append(got[n:2 * n])
        rows[a + "_uniform"].append(got[2 * n:3 * n])
        rows[b + "_uniform"].append(got[3 * n:4 * n])
    d = 13 * NBODIES[mech]
    ds = {k: (np.concatenate(v) if v else np.empty((0, d))) for k, v in rows.items()}
    ds.update(dm=par["dm"], dJ=par["dJ"], friction=par["friction"], mech=mech, seed=int(seed), config=config)
    return ds


# ---- files ------------------------------------------------------------------------------------------
_PAIRS = {"trainset": ("train_old", "train_curr"), "testset": ("test_old", "test_future"),
          "trainset_uniform": ("train_old_uniform", "train_curr_uniform"),
          "testset_uniform": ("test_old_uniform", "test_future_uniform")}  # savedatasets' names (datasets.jl:128)


def write_dataset(path, ds: dict) -> None:
    """The dataset as GPRXCST1 files (gprx.dataset: X = the old states, Y = the paired states, G = d)
    <path>/<trainset|testset|trainset_uniform|testset_uniform>.cst and <path>/params.json."""
    p = pathlib.Path(path)
    p.mkdir(parents=True, exist_ok=True)
    for name, (a, b) in _PAIRS.items():
        dataset.write_cstates(p / f"{name}.cst", ds[a].T, ds[b].T)
    with open(p / "params.json", "w") as f:
        json.dump(dict(mech=ds["mech"], seed=ds["seed"], config=ds["config"], dm=[float(v) for v in ds["dm"]],
                       dJ=[float(v) for v in ds["dJ"]], friction=[float(v) for v in ds["friction"]]), f)


def read_dataset(path) -> dict:
    p = pathlib.Path(path)
    with open(p / "params.json") as f:
        par = json.load(f)
    ds = dict(mech=par["mech"], seed=par["seed"], config=par["config"], dm=np.array(par["dm"]), dJ=np.array(par["dJ"]),
              friction=np.array(par["friction"]))
    for name, (a, b) in _PAIRS.items():
        r = dataset.read_cstates(p / f"{name}.cst", mmap=False)
        ds[a], ds[b] = r["X"].T.copy(), r["Y"].T.copy()
    return ds


def load_datasets(path, mech: str) -> list:
    """The datasets of one mechanism under <path>: <path>/<mech>/<k>/ for k = 0, 1, ... (trial t uses
    dataset t mod their number, as the reference's trial id picks df[id]), or the single <path>/<mech>/."""
    p = pathlib.Path(path) / mech
    subs = sorted((q for q in p.iterdir() if q.is_dir() and q.name.isdigit()), key=lambda q: int(q.name)) if p.is_dir() else []
    if subs:
        return [read_dataset(q) for q in subs]
    return [read_dataset(p)]


# ---- a trial of the experiments from a dataset -------------------------------------------------------
def rot_angle(q) -> np.ndarray:
    """Rotations.rotation_angle(q) sign(q.x) sign(q.w) (transformations.jl:53): the signed angle about x
    of q (..., 4) = (w, x, y, z), 2 atan2(q.x sign(q.w), |q.w|)."""
    q = np.asarray(q, dtype=np.float64)
    return 2.0 * np.arctan2(q[..., 1] * np.where(q[..., 0] < 0, -1.0, 1.0), np.abs(q[..., 0]))


def to_minimal(mech: str, X) -> dict:
    """CStates (n, 13 nb) -> the minimal coordinates data._cstates takes, read as applynoise! reads them
    (transformations.jl:48-140): angles from the quaternions, rates from w_x; P2's second pair relative
    to the first link; the four-bar's from bodies 1 and 3."""
    X = np.asarray(X, dtype=np.float64)
    ang = lambda b: rot_angle(X[:, 13 * b + 3:13 * b + 7])  # noqa: E731
    wx = lambda b: X[:, 13 * b + 10]  # noqa: E731
    if mech == "P1":
        return dict(th=ang(0), om=wx(0))
    if mech == "P2":
        return dict(t1=ang(0), t2=ang(1) - ang(0), o1=wx(0), o2=wx(1) - wx(0))
    if mech == "CP":
        return dict(x=X[:, 1], v=X[:, 8], th=ang(1), om=wx(1))
    if mech == "FB":
        return dict(t1=ang(0), t2=ang(2), o1=wx(0), o2=wx(2))
    raise ValueError(f"unknown mechanism {mech}")


def apply_noise(mech: str, X, rng) -> np.ndarray:
    """applynoise! (transformations.jl:40-140) on CStates (n, 13 nb): minimal coordinates, N(0, Sigma)
    noise on each perturbed quantity (data.SIGMA, noise.jl:42), and the CState rebuilt from them with the
    linear velocities by the dtsim forward difference (data._cstates).  The noise falls where the reference
    puts it: on each noisy body's own (absolute) angle and rate, so P2's relative pair (t2, o2) carries the
    difference of two draws (transformations.jl:67-73).  A noisy body keeps its quaternion's sign (the
    reference multiplies the stored quaternion by the noise rotation)."""
    X = np.asarray(X, dtype=np.float64)
    m = to_minimal(mech, X)
    n = {k: data.SIGMA * rng.standard_normal(v.shape[0]) for k, v in m.items()}
    if mech == "P2":  # n["t2"], n["o2"] are body 2's absolute noise
        n["t2"], n["o2"] = n["t2"] - n["t1"], n["o2"] - n["o1"]
    m = {k: v + n[k] for k, v in m.items()}
    out = data._cstates(mech, m).T.copy()
    for b in _NOISY_BODIES[mech]:
        neg = X[:, 13 * b + 3] < 0
        out[neg, 13 * b + 3:13 * b + 7] *= -1.0
    return out


def trial_from_dataset(mech: str, ds: dict, N: int, M: int = 100, seed: int = 0, noise: bool = True) -> dict:
    """One trial of the maximal-coordinate experiments from a dataset (e.g. P2noise.jl:12-27): the
    rows shuffled and the first N training / M test rows kept, applynoise! on both frames (noise=False:
    the stored rows, as hyperparameter.jl uses them).  Returns make_trial's dict -- X (d, N), Xcurr
    (d, N), Y (G, N), Xs (d, M), idx, d -- plus truth (M, d): the noise-free sfuture rows
    (xtest_future_true, :17)."""
    rng = np.random.default_rng(seed)
    ntr, nte = ds["train_old"].shape[0], ds["test_old"].shape[0]
    if N > ntr or M > nte:
        raise ValueError(f"the dataset holds {ntr} training and {nte} test rows; asked for {N} and {M}")
    itr, ite = rng.permutation(ntr)[:N], rng.permutation(nte)[:M]
    old, cur = ds["train_old"][itr], ds["train_curr"][itr]
    told, truth = ds["test_old"][ite], ds["test_future"][ite].copy()
    if noise:  # the truth is the stored sfuture (the reference copies it before applynoise!)
        old, cur = apply_noise(mech, old, rng), apply_noise(mech, cur, rng)
        told = apply_noise(mech, told, rng)
    idx = data.VW_INDICES[mech]
    X, Xcurr = old.T.copy(), cur.T.copy()
    Y = np.stack([Xcurr[i - 1, :] for i in idx], axis=0)
    return dict(X=X, Xcurr=Xcurr, Y=Y, Xs=told.T.copy() if M > 0 else None, idx=idx, d=X.shape[0], truth=truth)


def trial_folds(ds: dict, N: int, seed: int = 0) -> np.ndarray:
    """The trajectory index (N,) of each training row that trial_from_dataset(mech, ds, N, seed=seed)
    keeps: its permutation of the training rows, and row // plan(config)["train_samples"], since
    generate_dataset appends the rows trajectory by trajectory.  The folds of leave-one-trajectory-out
    cross-validation (GPBatch.set_folds; ids that no kept row carries are empty folds)."""
    rng = np.random.default_rng(seed)
    ntr = ds["train_old"].shape[0]
    if N > ntr:
        raise ValueError(f"the dataset holds {ntr} training rows; asked for {N}")
    itr = rng.permutation(ntr)[:N]
    return (itr // plan(ds["config"])["train_samples"]).astype(np.int32)
