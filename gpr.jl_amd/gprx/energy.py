"""examples/energy.jl on the MI355X: the energy drift of a pendulum rolled out by three GPs and
projectv! (the "GP variational integrator") against explicit Euler.

The reference fits three MeanZero GPs (outputs v_y, v_z, w_x of the pendulum's CState, vωindices
[9, 10, 11]) on nsamples pairs (state, state 0.01 s later) drawn from one simulated swing, rolls
them out for 600 000 steps of 0.01 s from rest at θ, keeps the mechanism's CState after every step
(energy.jl:75-83) and plots |E / E_true - 1| against explicit Euler's (:104-117).  Here the swing
is one gprx.projection.simulate trajectory of which only the sampled storage indices are recorded,
the fits run in the device optimiser, and the rollout is the recorded maximal-coordinate rollout
(gprx.projection.predictdynamics_rec): every step on the device, in bounded launches, the CState
after every step kept.

Differences from the reference, all unpinnable there: the samples come from numpy's generator (the
reference's rand() is unseeded), and optimize! stops at the sweep's evaluation budget instead of a
10 s wall limit.
"""
from __future__ import annotations

import argparse
import json
import math
import time

import numpy as np

G_ACC = 9.81
M = 1.0
LEN = 1.0
I_S = 1 / 12 * M * LEN ** 2 + M * (0.5 * LEN) ** 2  # about the joint (energy.jl:17)
VW_INDICES = [9, 10, 11]                            # energy.jl:54
MAX_EVALS = 30                                      # the sweep's evaluation budget (gprx.sweep.run)
DT = 0.01


def energy(theta, omega):
    """Epot + Ekin of the pendulum (energy.jl:19-23); arrays or scalars."""
    theta, omega = np.asarray(theta, dtype=np.float64), np.asarray(omega, dtype=np.float64)
    ekin = 0.5 * I_S * omega ** 2
    epot = M * G_ACC * 0.5 * LEN * (1 - np.cos(theta))
    return epot + ekin


def explicit_euler(steps: int, dt: float, theta: float, omega: float):
    """explicitEuler (energy.jl:25-37): both increments from the old state; (θs, ωs) after each step."""
    ths, oms = np.zeros(steps), np.zeros(steps)
    for i in range(steps):
        dth = omega * dt
        dom = -1.5 * math.sin(theta) * G_ACC / LEN * dt
        theta += dth
        omega += dom
        ths[i], oms[i] = theta, omega
    return ths, oms


def relative_error(theta, omega, theta0: float):
    """|E / E_true - 1| * 100 with E_true the potential energy at rest at theta0 (energy.jl:104, 108)."""
    return np.abs(energy(theta, omega) / float(energy(theta0, 0.0)) - 1) * 100


def rest_cstate(theta: float) -> np.ndarray:
    """The pendulum at rest at θ (energy.jl:72), (1, 13)."""
    from . import simdata

    return simdata.initial_cstate("P1", dict(th=float(theta), om=0.0))


def training_pairs(theta: float, nsamples: int, seed: int, dtsim: float = 1e-4, ctx=None):
    """energy.jl:40-55: one swing of 200 * offset storage entries at Δt = dtsim from rest at θ
    (offset = 0.01 / dtsim), nsamples indices i uniform in 1 .. length - offset, and the pairs
    (state i, state i + offset).  Only those indices are recorded.  Returns (X (13, n), Y (3, n))."""
    from .projection import simulate

    offset = int(round(DT / dtsim))
    length = 200 * offset
    rng = np.random.default_rng(seed)
    i = rng.integers(1, length - offset + 1, size=int(nsamples))
    rec = np.unique(np.concatenate([i, i + offset]))
    out, st = simulate("P1", rest_cstate(theta), length, rec, dt=float(dtsim), ctx=ctx)
    if st[0] & 2 or not np.all(np.isfinite(out)):
        raise RuntimeError("the training swing's simulation failed")
    old = out[0, np.searchsorted(rec, i)]
    cur = out[0, np.searchsorted(rec, i + offset)]
    return np.ascontiguousarray(old.T), np.ascontiguousarray(cur[:, np.array(VW_INDICES) - 1].T)


def pendulum_gps(theta: float, nsamples: int, seed: int, dtsim: float = 1e-4, ctx=None):
    """The three GPs of energy.jl:62-70 as one device batch, optimised from θ₀ = P1_MAX16 and left
    factorised at the minimisers (optimize!'s update_target!).  Close it when done."""
    from . import data
    from .batch import GPBatch
    from .optim import LBFGS, Options

    X, Y = training_pairs(theta, nsamples, seed, dtsim, ctx)
    b = GPBatch(len(VW_INDICES), 13, X.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    b.optimize(np.tile(data.theta0("P1", 16), (len(VW_INDICES), 1)), LBFGS(), Options(max_evals=MAX_EVALS))
    return b


def gp_variational_integration(steps: int, theta: float, nsamples: int, seed: int, dtsim: float = 1e-4, ctx=None,
                               batch=None, steps_per_launch: int = 0):
    """gpVariationalIntegration (energy.jl:39-91): (θs, ωs) of the mechanism's CState after each of
    `steps` steps of the GP rollout from rest at θ; θ by simdata.rot_angle, ω = CState[10] (0-based).
    batch: the GPs to roll out (pendulum_gps'; else they are fitted here and released)."""
    from . import simdata
    from .projection import predictdynamics_rec

    b = batch if batch is not None else pendulum_gps(theta, nsamples, seed, dtsim, ctx)
    try:
        rec = np.arange(2, int(steps) + 2)  # predictedstates: after step 1 .. steps
        traj, _, _, st = predictdynamics_rec("P1", [[(b, g) for g in range(len(VW_INDICES))]], rest_cstate(theta), int(steps),
                                             VW_INDICES, rec, steps_per_launch=steps_per_launch, ctx=b.ctx)
    finally:
        if batch is None:
            b.close()
    if st[0] != 0:
        raise RuntimeError("singular projection during the rollout")  # the reference throws
    return simdata.rot_angle(traj[0, :, 3:7]), traj[0, :, 10].copy()


def main(argv=None):
    ap = argparse.ArgumentParser(description="examples/energy.jl: energy drift of the GP rollout against explicit Euler")
    ap.add_argument("--steps", type=int, default=100 * 60 * 100, help="the long run (energy.jl:106-107)")
    ap.add_argument("--short-steps", type=int, default=100 * 10, help="the 20 / 10 sample pair (energy.jl:112-114)")
    ap.add_argument("--theta", type=float, default=math.pi / 2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dtsim", type=float, default=1e-4)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="energy.npz")
    a = ap.parse_args(argv)
    from .batch import Context

    ctx = Context(a.device)
    ctx.set_profiling(True)
    res, info = {}, {}
    for name, steps, ns in (("long20", a.steps, 20), ("short20", a.short_steps, 20), ("short10", a.short_steps, 10)):
        ctx.reset_stats()
        b = pendulum_gps(a.theta, ns, a.seed, a.dtsim, ctx)
        t0 = time.perf_counter()
        th, om = gp_variational_integration(steps, a.theta, ns, a.seed, a.dtsim, ctx, batch=b)
        wall = time.perf_counter() - t0
        b.close()
        ks = ctx.kernel_stats("rollout_max_rec")
        te, oe = explicit_euler(steps, DT, a.theta, 0.0)
        res[f"{name}_gp"], res[f"{name}_euler"] = relative_error(th, om, a.theta), relative_error(te, oe, a.theta)
        res[f"{name}_t"] = np.arange(1, steps + 1) / 100
        info[name] = dict(steps=steps, nsamples=ns, wall_s=wall, launches=int(ks["launches"]), kernel_ms=float(ks["ms"]),
                          gp_err_last=float(res[f"{name}_gp"][-1]), gp_err_max=float(np.max(res[f"{name}_gp"])),
                          euler_err_last=float(res[f"{name}_euler"][-1]), euler_err_max=float(np.max(res[f"{name}_euler"])))
        print(json.dumps({name: info[name]}), flush=True)
    ctx.close()
    np.savez_compressed(a.out, info=json.dumps(info), **res)
    print("wrote", a.out)
