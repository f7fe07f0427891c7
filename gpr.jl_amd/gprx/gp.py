"""Host-side mirror of the GaussianProcesses.jl v0.12.4 surface the reference calls
(GP / SEArd / MeanZero / MeanDynamics-style means / optimize! / predict_y / predict_f), with every
evaluation running on the MI355X through the C ABI (include/gprx.h).

Reference call pattern (examples/maximal_coordinates/CPnoise.jl:37-43):
    kernel = SEArd(log.(params[2:end]), log(params[1]))
    mean   = meandynamics ? MeanDynamics(...) : MeanZero()
    gp     = GP(xtrain_old, yi, mean, kernel)                  # logNoise defaults to -2.0
    GaussianProcesses.optimize!(gp, LBFGS(linesearch=BackTracking(order=2)), Optim.Options(time_limit=10.))
and predict_y(gp, obs)[1][1]  (examples/utils/predictdynamics.jl:13).

Prior means: a mean is any object with `mean(X) -> (N,)` and `num_params() == 0` -- the
reference's MeanDynamics has no hyper-parameters (src/mDynamics.jl:29), so μ(X) is evaluated once
per training set and y - μ(X) is what the device sees.  Means with parameters are out of scope.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L
from .batch import GPBatch, Context, default_context


class MeanZero:
    """GaussianProcesses.MeanZero."""

    def num_params(self) -> int:
        return 0

    def mean(self, X) -> np.ndarray:
        return np.zeros(np.asarray(X).shape[1])


class MeanFunction:
    """A θ-independent prior mean given as a callable on one input column (the role of
    GPR.MeanDynamics, src/mDynamics.jl:41-55, whose single-slot cache keyed by the input column
    is kept: consecutive calls at the same column reuse the previous value)."""

    def __init__(self, f):
        self.f = f
        self._key = None
        self._val = None

    def num_params(self) -> int:
        return 0

    def _at(self, x):
        if self._key is None or not np.array_equal(self._key, x):
            self._key = np.array(x, copy=True)
            self._val = float(self.f(x))
        return self._val

    def mean(self, X) -> np.ndarray:
        X = np.asarray(X)
        return np.array([self._at(X[:, t]) for t in range(X.shape[1])])


class MeanDynamics:
    """GPR.MeanDynamics(mechanism, getμ, μID; xtransform) (src/mDynamics.jl:13-55) for the experiment
    mechanisms: the prior mean is output mu_id (1-based, as μID) of one variational-integrator step
    at the input, solved on the device (gprx.mdynamics -> gprx_vi_step).  variant names the
    experiment's input and getμ: "max" (CState inputs, getμ(vωindices)), "min" or "min_sin"
    (minimal coordinates through the experiments' xtransform, the solution's rates).  No
    hyper-parameters (mDynamics.jl:29).  GPEs that carry it roll out in one launch through
    gprx.projection.predictdynamics_md / gprx.rollout.rollout_min_md."""

    VARIANTS = ("max", "min", "min_sin")

    def __init__(self, mech: str, mu_id: int, variant: str = "max", ctx: Context | None = None):
        from .rollout import MECH, NCOORD

        if mech not in MECH:
            raise ValueError(f"Experiment {mech} not supported!")
        if variant not in self.VARIANTS:
            raise ValueError(f"variant must be one of {self.VARIANTS}")
        from .data import VW_INDICES

        nout = len(VW_INDICES[mech]) if variant == "max" else NCOORD[mech]
        if not 1 <= int(mu_id) <= nout:
            raise ValueError(f"mu_id must be in 1..{nout} for {mech} {variant}")
        self.mech, self.mu_id, self.variant, self.ctx = mech, int(mu_id), variant, ctx

    def num_params(self) -> int:
        return 0

    def mean(self, X) -> np.ndarray:
        from . import mdynamics

        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        if self.variant == "max":
            mu = mdynamics.mean_max(self.mech, X, ctx=self.ctx)
        else:
            mu = mdynamics.mean_min(self.mech, X, self.variant == "min_sin", ctx=self.ctx)
        return mu[self.mu_id - 1].copy()


class SEArd:
    """SEArd(ll, lσ): squared-exponential ARD kernel, ll = log length scales, lσ = log σ_f."""

    def __init__(self, ll, lsigma):
        self.ll = np.asarray(ll, dtype=np.float64).copy()
        self.lsigma = float(lsigma)

    def num_params(self) -> int:
        return self.ll.shape[0] + 1

    def get_params(self) -> np.ndarray:
        return np.concatenate([self.ll, [self.lsigma]])

    def set_params(self, hyp):
        hyp = np.asarray(hyp, dtype=np.float64)
        self.ll = hyp[:-1].copy()
        self.lsigma = float(hyp[-1])


class GPE:
    """Exact GP with Gaussian noise (GaussianProcesses.GPE) evaluated on the device.

    Attributes mirror the reference object: x, y, mean, kernel, logNoise, mll, dmll, target,
    dtarget, alpha is kept on the device.
    """

    def __init__(self, x, y, mean, kernel: SEArd, logNoise: float = -2.0, ctx: Context | None = None):
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        if self.x.ndim == 1:
            self.x = self.x[None, :]
        self.dim, self.nobs = self.x.shape
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        assert self.y.shape == (self.nobs,), "y must have one entry per column of x"
        if kernel.ll.shape[0] != self.dim:
            raise ValueError("SEArd needs one length scale per input dimension")
        if mean.num_params() != 0:
            raise NotImplementedError("only parameter-free prior means (MeanZero, MeanDynamics)")
        self.mean = mean
        self.kernel = kernel
        self.logNoise = float(logNoise)
        self.ctx = ctx or default_context()
        self._mu = np.asarray(mean.mean(self.x), dtype=np.float64)  # θ-independent prior mean
        self._batch = GPBatch(1, self.dim, self.nobs, 0, ctx=self.ctx)
        self._batch.set_train(self.x, (self.y - self._mu)[None, :])
        self.mll = -math.inf
        self.dmll = np.zeros(self.dim + 2)
        self.update_mll()  # GPE construction computes the target (initialise_target!)

    # -- parameters ---------------------------------------------------------------------------
    def get_params(self) -> np.ndarray:
        return np.concatenate([[self.logNoise], self.kernel.get_params()])

    def set_params(self, hyp):
        hyp = np.asarray(hyp, dtype=np.float64)
        if hyp.shape != (self.dim + 2,):
            raise ValueError("hyperparameter vector has the wrong length")
        self.logNoise = float(hyp[0])
        self.kernel.set_params(hyp[1:])

    @property
    def target(self) -> float:
        return self.mll

    @property
    def dtarget(self) -> np.ndarray:
        return self.dmll

    # -- evaluation ---------------------------------------------------------------------------
    def _run(self, grad: bool):
        theta = self.get_params()
        if not np.all(np.isfinite(theta)):
            raise ValueError("non-finite hyperparameters")  # ArgumentError in the reference
        r = self._batch.run(theta[None, :], grad=grad)
        st = int(r["status"][0])
        if st == L.NOT_POSITIVE_DEFINITE:
            raise L.NotPositiveDefinite(st, f"pivot {int(r['info'][0])}")
        if st != L.OK:
            L.check(st, self.ctx.h)
        self.mll = float(r["mll"][0])
        if grad:
            self.dmll = r["grad"][0].copy()
        return self.mll

    def update_mll(self):
        return self._run(grad=False)

    def update_mll_and_dmll(self):
        self._run(grad=True)
        return self.mll, self.dmll

    update_target = update_mll
    update_target_and_dtarget = update_mll_and_dmll

    def _test_columns(self, xs):
        xs = np.asarray(xs, dtype=np.float64)
        if xs.ndim == 1:
            xs = xs[:, None]
        if xs.shape[0] != self.dim:
            raise ValueError("test inputs have the wrong dimension")
        return xs

    def predict_f(self, xs, full_cov: bool = False):
        """(μ_f, σ²_f) per test column; full_cov=True: (μ_f, Σ_f) with the joint M x M covariance
        [ext predict_f(gp, x; full_cov)]."""
        xs = self._test_columns(xs)
        self._batch.set_test(xs)
        if full_cov:
            mu, cov = self._batch.predict_cov()
            return mu[0].copy(), cov[0].copy()
        mu, var = self._batch.predict()
        return mu[0].copy(), var[0].copy()

    def predict_y(self, xs, full_cov: bool = False):
        """predict_f + prior mean, variance (full_cov: the covariance's diagonal) + exp(2 logNoise)
        [ext predict_y]."""
        xs = np.asarray(xs, dtype=np.float64)
        if xs.ndim == 1:
            xs = xs[:, None]
        mu, var = self.predict_f(xs, full_cov=full_cov)
        if full_cov:
            var[np.diag_indices_from(var)] += math.exp(2.0 * self.logNoise)
            return mu + self.mean.mean(xs), var
        return mu + self.mean.mean(xs), var + math.exp(2.0 * self.logNoise)

    def rand(self, xs, n: int = 1, rng=None):
        """n draws of the posterior function at the columns of xs, (M, n) [ext rand(gp, x, n)]:
        f-space plus the prior mean.  The standard normals come from `rng` (numpy Generator; default
        a fresh default_rng()) on the host; the covariance, its factor and mu + L z run on the device."""
        xs = self._test_columns(xs)
        rng = rng if rng is not None else np.random.default_rng()
        Z = rng.standard_normal((int(n), xs.shape[1]))
        self._batch.set_test(xs)
        smp, _ = self._batch.sample(Z, raise_on_error=True)
        return (smp[0] + self.mean.mean(xs)[None, :]).T.copy()

    def predict_LOO(self):
        """(μ_i, σ²_i) of every training point predicted from the other N - 1 [ext predict_LOO(gp)],
        from the last factorisation: the prior mean at x is added back here, σ² is in y-space (it
        includes the noise)."""
        r = self._batch.loo(raise_on_error=True)
        return r["mu"][0] + self._mu, r["var"][0].copy()

    def logp_LOO(self) -> float:
        """Sum of the leave-one-out log predictive densities [ext logp_LOO(gp)]."""
        return float(self._batch.loo(raise_on_error=True)["logp"][0])

    def dlogpdtheta_LOO(self) -> np.ndarray:
        """Gradient of logp_LOO with respect to the hyper-parameters, in the order of get_params
        [ext, recalled: dlogpdθ_LOO(gp)]; the prior mean has no parameters here."""
        return self._batch.loo_grad(raise_on_error=True)["grad"][0].copy()

    def _set_folds(self, folds):
        fo = folds_to_ids(folds, self._batch.N)
        self._batch.set_folds(fo, nfolds=len(folds))

    def predict_CVfold(self, folds):
        """(μ_i, σ²_i) of every training point predicted from the points outside its fold [ext
        predict_CVfold(gp, folds)], from the last factorisation.  folds: a list of index vectors
        (0-based) that partition the training points; overlapping or non-covering folds raise
        ValueError.  The prior mean at x is added back here; σ² is the y-space marginal variance (the
        folds' full covariances are not returned)."""
        self._set_folds(folds)
        r = self._batch.cvfold(raise_on_error=True)
        return r["mu"][0] + self._mu, r["var"][0].copy()

    def logp_CVfold(self, folds) -> float:
        """Sum over the folds of log p(y_V | y_-V) [ext logp_CVfold(gp, folds)]."""
        self._set_folds(folds)
        return float(self._batch.cvfold(raise_on_error=True)["logp"][0])

    def predict_y_mean(self, xs):
        """predict_y(gp, obs)[1] without the variance: the rollout call of
        examples/utils/predictdynamics.jl:13 (uses the mean only); skips the O(N^2 M) variance."""
        xs = np.asarray(xs, dtype=np.float64)
        if xs.ndim == 1:
            xs = xs[:, None]
        if xs.shape[0] != self.dim:
            raise ValueError("test inputs have the wrong dimension")
        self._batch.set_test(xs)
        mu, _ = self._batch.predict(variance=False)
        return mu[0] + self.mean.mean(xs)


def folds_to_ids(folds, N: int) -> np.ndarray:
    """GaussianProcesses' folds argument, a list of index vectors (0-based here), as the fold id of
    every point.  ValueError unless the folds partition 0..N-1 (an empty fold is allowed)."""
    fo = np.full(int(N), -1, dtype=np.int32)
    for f, idx in enumerate(folds):
        idx = np.asarray(idx)
        if idx.size == 0:
            continue
        if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"fold {f}: an index vector of integers is needed")
        if idx.min() < 0 or idx.max() >= N:
            raise ValueError(f"fold {f}: index out of range 0..{N - 1}")
        if np.unique(idx).size != idx.size or np.any(fo[idx] >= 0):
            raise ValueError(f"fold {f} overlaps itself or an earlier fold")
        fo[idx] = f
    if len(folds) < 1 or np.any(fo < 0):
        raise ValueError("the folds do not cover every training point")
    return fo


def GP(x, y, mean, kernel, logNoise: float = -2.0, ctx: Context | None = None) -> GPE:
    """GaussianProcesses.GP(x, y, mean, kernel[, logNoise])."""
    return GPE(x, y, mean, kernel, logNoise, ctx=ctx)


def predict_y(gp: GPE, xs, full_cov: bool = False):
    return gp.predict_y(xs, full_cov=full_cov)


def predict_f(gp: GPE, xs, full_cov: bool = False):
    return gp.predict_f(xs, full_cov=full_cov)


def rand(gp: GPE, xs, n: int = 1, rng=None):
    return gp.rand(xs, n, rng)


def predict_LOO(gp: GPE):
    return gp.predict_LOO()


def logp_LOO(gp: GPE) -> float:
    return gp.logp_LOO()


def dlogpdtheta_LOO(gp: GPE) -> np.ndarray:
    return gp.dlogpdtheta_LOO()


def predict_CVfold(gp: GPE, folds):
    return gp.predict_CVfold(folds)


def logp_CVfold(gp: GPE, folds) -> float:
    return gp.logp_CVfold(folds)
