/*
 * gprx.h -- C ABI of the MI355X-native exact-GP (SE-ARD, fp64) hot path for GPR.jl.
 *
 * Plain C: pointers, sizes, status codes.  No torch / HIP types cross this boundary.
 *
 * What each entry point replaces in the reference (amacati/GPR.jl, whose GP arithmetic is
 * delegated to GaussianProcesses.jl v0.12.4, pinned in /root/reference/Manifest.toml):
 *
 *   gprx_gp_create / gprx_batch_set_train
 *       GP(xtrain_old, yi, mean, kernel)            examples/maximal_coordinates/CPnoise.jl:40
 *       (X = reduce(hcat, CState.(traindf.sold)),   CPnoise.jl:26; y = yi - mean(X),
 *        mean from MeanZero or MeanDynamics         src/mDynamics.jl:41-55, theta-independent :29)
 *   gprx_gp_lml        update_mll! inside GP()/optimize! value evaluations   [ext] CPnoise.jl:40-41
 *   gprx_gp_lml_grad   update_mll! + update_dmll! (one LBFGS evaluation)     [ext] CPnoise.jl:41
 *   gprx_gp_predict    predict_f / predict_y(gp, x*)  examples/utils/predictdynamics.jl:13
 *   gprx_gp_predict_cov, gprx_gp_sample   [ext] predict_f(gp, x; full_cov=true), rand(gp, x, n): on
 *                      every GPE (CPnoise.jl:40); the reference's scripts use the mean only
 *   gprx_gp_loo / gprx_batch_loo   [ext] predict_LOO(gp), logp_LOO(gp) (crossvalidation.jl), on every GPE
 *   gprx_gp_loo_grad / gprx_batch_loo_grad   [ext, recalled] dlogpdtheta_LOO(gp) (crossvalidation.jl)
 *   gprx_gp_cvfold / gprx_batch_cvfold   [ext] predict_CVfold(gp, folds), logp_CVfold(gp, folds) (crossvalidation.jl)
 *   gprx_rollout_min   predictdynamicsmin             examples/utils/predictdynamics.jl:30-102
 *   gprx_batch_*       the G per-output GPs of a trial (CPnoise.jl:37-43) and the trial loop
 *                      (examples/parallel/core.jl:28) evaluated as one device batch
 *   gprx_cstate_pack   CState(::Vector{State})      src/CState.jl:25-28
 *   gprx_select_outputs  ytrain = [[s[i] for s in X_curr] for i in vwindices]   CPnoise.jl:28-29
 *
 * Hyper-parameter vector convention (GaussianProcesses get_params(gp) order, d+2 entries):
 *     theta = [ log sigma_n, log ell_1 ... log ell_d, log sigma_f ]
 * built by the callers as SEArd(log.(p[2:end]), log(p[1])) with default logNoise = -2.0
 * (CPnoise.jl:38-40).  Gradients are returned in the same order, with the same sign as
 * GaussianProcesses' gp.dmll (derivative of the log marginal likelihood, not of -mll).
 *
 * Memory: the caller owns every buffer it passes; the library copies on entry.  A batch owns
 * its device workspace (X, y, K/L, L^-1, L^-T, alpha, test points) until destroyed.
 * Threading: a context owns one HIP stream and a mutex; calls on one context serialise, calls on
 * different contexts (e.g. one per Julia thread / per GPU) run concurrently.  All calls block
 * until results are in host memory.
 */
#ifndef GPRX_H
#define GPRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI versions:
 *   1  first release.
 *   2  gprx_opt_options.max_evals <= 0 means "no limit" (Optim's f_calls_limit = 0); under
 *      version 1, 0 was a real cap of zero evaluations.  No signature changed.
 *   3  gprx_batch_set_opt_trace takes the trace buffer's capacity; new gprx_batch_bytes and
 *      gprx_ctx_mem_info (device-batch chunking); gprx_batch_create / gprx_batch_set_test refuse
 *      sizes beyond the kernels' 32-bit buffer addressing (Npad * max(Npad, Mpad) * 8 >= 2^31 - 16). */
#define GPRX_ABI_VERSION 3

/* status codes (mirrors the reference's failure modes) */
#define GPRX_OK 0
#define GPRX_NOT_POSITIVE_DEFINITE 1 /* cholesky! -> PosDefException; Optim then sees +Inf   */
#define GPRX_INVALID_ARGUMENT 2      /* bad sizes, non-finite theta (ArgumentError)          */
#define GPRX_DEVICE_ERROR 3
#define GPRX_OUT_OF_MEMORY 4
#define GPRX_NOT_READY 5 /* predict before any successful factorisation */

/* gprx_batch_run flags */
#define GPRX_WANT_GRAD 1u    /* d mll / d theta (update_dmll!)                          */
#define GPRX_WANT_PREDICT 2u /* predictive mean + variance at the batch's test points    */

/* squared-distance formulation of the SE-ARD kernel (see DESIGN.md "distance modes") */
/* Per-dimension squared distance in the Gram / cross-covariance:
 *   DIRECT   (default): sum_d w_d (a_d - b_d)^2, as GaussianProcesses' cov_ij for StationaryARD
 *            kernels (distij over WeightedSqEuclidean) [ext]
 *   EXPANDED: a^2 + b^2 - 2ab clamped at 0 per dimension, the rounding of the Distances.jl 0.10.5
 *            pairwise(SqEuclidean()) stack that GaussianProcesses keeps for gradients [ext]       */
#define GPRX_DIST_EXPANDED 0
#define GPRX_DIST_DIRECT 1

/* memory kind of pointer arguments */
#define GPRX_MEM_HOST 0
#define GPRX_MEM_DEVICE 1

typedef struct gprx_ctx gprx_ctx;
typedef struct gprx_batch gprx_batch;
typedef struct gprx_gp gprx_gp;

int gprx_abi_version(void);
const char* gprx_status_string(int status);
/* first 16 hex digits of the SHA-256 of the sources the library was built from (the host checks
 * it against the sources it ships with, so a stale prebuilt library is refused)                 */
const char* gprx_build_id(void);
/* number of visible devices (hipGetDeviceCount; 0 when none or on error): hosts map their worker
 * threads / ranks onto devices with it (core.jl:28's threads, jobid mod ndevices)               */
int gprx_device_count(void);

/* ---- context: one device, one stream ------------------------------------------------------ */
int gprx_ctx_create(int device, gprx_ctx** out);
/* also destroys the context's remaining batches / GPs: their handles become invalid */
void gprx_ctx_destroy(gprx_ctx* ctx);
const char* gprx_ctx_last_error(const gprx_ctx* ctx);
int gprx_ctx_set_dist_mode(gprx_ctx* ctx, int mode);
int gprx_ctx_device(const gprx_ctx* ctx);
/* per-kernel timing (HIP events around every launch on the context stream); off by default */
int gprx_ctx_set_profiling(gprx_ctx* ctx, int enable);
/* launch-geometry options (results are identical under every setting; tests cover each path):
 *   GPRX_OPT_LEAF_TILES  recursion nodes of <= value tiles (64 x 64) run fused in one leaf
 *                        kernel; 1: every 64 x 64 diagonal tile on its own; 0 (default) = auto
 *   GPRX_OPT_SMALL_N     recursion nodes of <= value tiles use the 64 x 32 pair-unit GEMM; 0 = auto
 *   GPRX_OPT_GRAPHS      1: replay each evaluation's launch sequence as a hipGraph (default 0)
 *   GPRX_OPT_ACTIVE_DIMS 1 (default): gprx_batch_set_train finds the input dimensions that hold one
 *                        constant over the training points of every slot, and direct-mode
 *                        evaluations leave them out of the Gram and the gradient (their distances
 *                        are exact zeros; their d mll / d log ell is +0).  0 keeps every dimension.
 *                        Read by gprx_batch_set_train.  gprx_ctx_kernel_stats("active_dims") returns
 *                        in *launches the count the latest set_train / evaluation ran with.      */
#define GPRX_OPT_LEAF_TILES 1
#define GPRX_OPT_SMALL_N 2
#define GPRX_OPT_GRAPHS 3
/* id 4 is retired (a launch form that no longer exists) and not reused: GPRX_INVALID_ARGUMENT */
#define GPRX_OPT_ACTIVE_DIMS 5
int gprx_ctx_set_option(gprx_ctx* ctx, int option, int value);
int gprx_ctx_kernel_stats(gprx_ctx* ctx, const char* kernel, double* total_ms, int64_t* launches,
                          double* algo_flops, double* algo_bytes);
int gprx_ctx_reset_stats(gprx_ctx* ctx);
/* free and total device memory of the context's device (hipMemGetInfo), for sizing batches      */
int gprx_ctx_mem_info(gprx_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);

/* ---- batch: B GP slots with equal (d, N); slot b has its own X_b, y_b, theta_b ------------ */
/* M_max: maximum number of test points per slot (0 = no prediction).  d <= 64, N >= 1, and
 * Npad * max(Npad, Mpad) * 8 < 2^31 - 16 (Npad, Mpad: N, M_max rounded up to 64; N <= 16320):
 * the kernels address a matrix panel with 32-bit byte offsets.  Larger sizes: GPRX_INVALID_ARGUMENT. */
int gprx_batch_create(gprx_ctx* ctx, int B, int d, int N, int M_max, gprx_batch** out);
/* Device bytes gprx_batch_create(B, d, N, M_max) allocates (host arithmetic only, no device call;
 * the optimiser's workspace, B * ((10 + 2m)(d+2) + 2m + 16) doubles, comes on top during
 * gprx_batch_optimize).  GPRX_INVALID_ARGUMENT for sizes gprx_batch_create refuses.  Hosts split
 * a rank's trials into device batches that fit the free memory with it (the reference's
 * parallelrun holds no such limit: core.jl:27-67 runs every trial in host RAM).                 */
int gprx_batch_bytes(int B, int d, int N, int M_max, uint64_t* bytes);
void gprx_batch_destroy(gprx_batch* batch);
/* X: d x N column-major per slot (column t = one CState), slot b at X + b*x_slot_stride
 *    (x_slot_stride = 0: all slots share one X, as the G outputs of one trial do);
 * Y: N targets per slot (y - mean(X)), slot b at Y + b*y_slot_stride.                          */
int gprx_batch_set_train(gprx_batch* batch, const double* X, int64_t x_slot_stride, const double* Y,
                         int64_t y_slot_stride, int mem);
/* Xs: d x M column-major per slot, slot b at Xs + b*xs_slot_stride (0 = shared), M <= M_max.   */
int gprx_batch_set_test(gprx_batch* batch, const double* Xs, int M, int64_t xs_slot_stride, int mem);
/* Evaluate every slot at theta[b*(d+2) ...]: Gram build, Cholesky, alpha, log marginal
 * likelihood; optionally its gradient and the predictive mean/variance (f-space: no noise, no
 * prior mean) at the test points.  var == NULL skips the O(N^2 M) variance computation (the
 * rollout pattern of predictdynamics.jl:13, which uses the mean only).  Outputs (host pointers,
 * any may be NULL):
 *   mll[B], grad[B*(d+2)], mu[B*M], var[B*M], status[B], info[B] (1-based failing pivot).
 * Returns GPRX_OK when every slot succeeded, otherwise the first failing slot's status.          */
int gprx_batch_run(gprx_batch* batch, const double* theta, unsigned flags, double* mll, double* grad,
                   double* mu, double* var, int* status, int* info);
/* Predictive mean/variance from the factorisation of the last gprx_batch_run (f-space);
 * var == NULL: mean only.                                                                      */
int gprx_batch_predict(gprx_batch* batch, double* mu, double* var);
int gprx_batch_dims(const gprx_batch* batch, int* B, int* d, int* N, int* M_max);
/* alpha = K^-1 (y - mean) of the last factorisation, alpha[b*N + t] (GPE's gp.alpha; N doubles
 * per slot), for hosts that keep GaussianProcesses' own fields current.  A slot whose status in
 * that evaluation was not GPRX_OK has no alpha: its N entries are NaN.                          */
int gprx_batch_alpha(gprx_batch* batch, double* alpha);

/* ---- joint predictive covariance and posterior samples ------------------------------------- */
/* [ext] predict_f(gp, x; full_cov=true) and rand(gp, x, n) of GaussianProcesses 0.12.4, which every
 * GPE the reference builds carries (examples/maximal_coordinates/CPnoise.jl:40); the reference's
 * own scripts use only the mean (examples/utils/predictdynamics.jl:13).
 *   Sigma = K**(Xs, Xs) - V^T V,  V = L^-1 K*   (f-space: no noise, no prior mean; K** in the
 *   context's distance mode; NOT clamped, unlike var; bitwise symmetric).
 * A slot whose last evaluation failed gets NaN in its mu, cov and samples rows (as
 * gprx_batch_alpha); the other slots are unaffected.  GPRX_NOT_READY before a successful
 * factorisation or with no test points set; GPRX_INVALID_ARGUMENT for a NULL cov, Z or samples,
 * S < 1, Mpad^2 * 8 beyond the 32-bit addressing range (Mpad: M_max rounded up to 64), and, for
 * the sample calls, M > 1024 (a limit of the single-workgroup factorisation).
 * The workspace (gprx_batch_cov_bytes) is allocated by the first of these calls on a batch, not by
 * gprx_batch_create, and freed with the batch; when it cannot be allocated the call returns
 * GPRX_OUT_OF_MEMORY and the batch stays usable.  The launches go straight on the context stream
 * (they are not part of the captured evaluation graphs).                                        */
/* f-space joint posterior at the batch's test points from the last factorisation:
 * mu[B*M] (may be NULL), cov[B*M*M] (slot b at cov + b*M*M, symmetric).                         */
int gprx_batch_predict_cov(gprx_batch* batch, double* mu, double* cov);
/* samples[(b*S + s)*M + m] = mu_b[m] + (L_b z_{b,s})[m],  L_b L_b^T = Sigma_b + jitter_b I.
 * Z: host, S*M standard normals per slot at Z + b*z_slot_stride (0 = shared).  Self-contained:
 * it recomputes mu and Sigma itself.  jitter[B], status[B] may be NULL.
 * The factor of Sigma_b (lower Cholesky, substitution in the panel solves, no explicit inverse):
 * tau_b = (N + M) * 2^-52 * sigma_f^2 is the rounding bound of Sigma's own entries; a pivot fails
 * when it is not finite or <= tau_b.  Attempt 0 adds no jitter, attempts k = 1..8 add 10^k tau_b to
 * the diagonal; the first attempt whose pivots all pass wins and jitter[b] reports its value (0 or
 * 10^k tau_b).  If all nine fail, status[b] = GPRX_NOT_POSITIVE_DEFINITE, jitter[b] and the slot's
 * samples are NaN, and the call returns the first failing slot's status.  This ladder is gprx's own
 * rule: GaussianProcesses.jl was not available to compare its rand() against.                     */
int gprx_batch_sample(gprx_batch* batch, const double* Z, int S, int64_t z_slot_stride, double* samples,
                      double* jitter, int* status);
/* device bytes the two calls allocate on first use, on top of gprx_batch_bytes (host arithmetic):
 * 8 B (Npad Mpad + 2 Mpad^2) for V^T, Sigma and its factor, plus the staging term
 * 8 B 2 Mpad^2 + 12 B (the device Z and sample buffers, Mpad vectors per slot a pass, and the
 * per-slot jitter and status).  GPRX_INVALID_ARGUMENT for a NULL bytes, sizes gprx_batch_create
 * refuses, or Mpad^2 * 8 beyond the addressing range.                                            */
int gprx_batch_cov_bytes(int B, int N, int M_max, uint64_t* bytes);

/* ---- leave-one-out predictions -------------------------------------------------------------- */
/* [ext] predict_LOO(gp) and logp_LOO(gp) of GaussianProcesses 0.12.4 (crossvalidation.jl), which
 * every GPE the reference builds carries (examples/maximal_coordinates/CPnoise.jl:40): the
 * predictive mean and variance at each training point from the other N - 1, its log predictive
 * density and their sum, from the factorisation of the last evaluation (no refit).  With
 * kinv_i = [K^-1]_ii = sum_{k >= i} (L^-1)_ki^2 and alpha = K^-1 y (Rasmussen & Williams 5.10-5.12):
 *   var_i    = 1 / kinv_i                  (y-space: K carries exp(2 log sn) + eps on its diagonal)
 *   mu_i     = y_i - alpha_i / kinv_i      (in the space of the targets given to set_train, y - mean(X))
 *   logp_i   = 0.5 log(kinv_i) - 0.5 alpha_i^2 / kinv_i - 0.5 log(2 pi),   logp[b] = sum_i logp_i
 * GaussianProcesses' source was not available to compare against: the formulas are R&W's and the
 * convention (y-space variance, the prior mean left to the host) is gprx's own.
 * Host outputs, any may be NULL: mu[B*N], var[B*N], logp_i[B*N], logp[B], status[B] (that
 * evaluation's per-slot status).  GPRX_NOT_READY before a successful factorisation;
 * GPRX_INVALID_ARGUMENT for a NULL batch.  A slot whose status in that evaluation was not GPRX_OK
 * gets NaN in its rows and its logp (as gprx_batch_alpha); the other slots are unaffected.  Returns
 * GPRX_OK or the first failing slot's status, as gprx_batch_run.  The results are bitwise
 * reproducible and do not depend on B or on the slot's place in the batch.  The workspace
 * (8 B (4 Npad + 1) bytes) comes from the context's scratch buffer; gprx_batch_bytes is unchanged.
 * The launches go straight on the context stream (stats "loo_diag", "loo_final").                */
int gprx_batch_loo(gprx_batch* batch, double* mu, double* var, double* logp_i, double* logp, int* status);

/* ---- gradient of the leave-one-out log predictive probability ------------------------------- */
/* [ext, recalled: the package source was not available] dlogpdtheta_LOO(gp) of GaussianProcesses'
 * crossvalidation.jl: the gradient of gprx_batch_loo's logp with respect to the hyper-parameters,
 * from the factorisation and theta of the last evaluation (no refit).  With K = Kf + (sn2 + eps) I,
 * q_i = [K^-1]_ii, alpha = K^-1 y, c_i = (1/q_i + alpha_i^2/q_i^2)/2, r_i = alpha_i/q_i,
 * beta = K^-1 r and C = diag(c), Rasmussen & Williams 5.13 in contracted form is
 *   dlogp = sum_kl dK_kl W'_kl,   W' = (beta alpha^T + alpha beta^T)/2 - K^-1 C K^-1
 * with dK/dlog sn = 2 sn2 I, dK/dlog ell_p = Kf o (x_p - x_p')^2 / ell_p^2, dK/dlog sf = 2 Kf: the
 * marginal likelihood gradient's contraction with 2 W' in place of alpha alpha^T - K^-1.
 * Host outputs, any may be NULL: logp[B] (bit for bit gprx_batch_loo's), grad[B*(d+2)] in the order
 * of theta, [log sn, log ell_1..d, log sf] (a dimension that gprx_batch_set_train found constant
 * gets exactly 0, as in the marginal likelihood's gradient), status[B] (that evaluation's per-slot
 * status).  GPRX_NOT_READY before a successful factorisation; GPRX_INVALID_ARGUMENT for a NULL
 * batch.  A slot whose status in that evaluation was not GPRX_OK gets NaN in logp and its gradient
 * row; the other slots are unaffected.  Returns GPRX_OK or the first failing slot's status.  The
 * results are bitwise reproducible and do not depend on B or on the slot's place in the batch.
 * The call overwrites the factorisation workspace Lw (with K^-1 diag(sqrt c)), which nothing reads
 * before the next evaluation rewrites it: predictions, alpha and gprx_batch_loo after it return what
 * they return without it.  The small vectors come from the context's scratch buffer;
 * gprx_batch_bytes is unchanged.  The launches go straight on the context stream (stats
 * "loo_diag", "loo_final", "loo_kinv", "loo_beta", "loo_grad", "loo_grad_final").                 */
int gprx_batch_loo_grad(gprx_batch* batch, double* logp, double* grad, int* status);

/* ---- k-fold cross-validation ---------------------------------------------------------------- */
/* [ext] predict_CVfold(gp, folds) and logp_CVfold(gp, folds) of GaussianProcesses' crossvalidation.jl:
 * the joint prediction of every fold's points from the points of the other folds and its log
 * predictive probability, from the factorisation of the last evaluation (no refit).  For a fold V of
 * m points, Q = [K^-1]_VV and a = alpha_V (K carries exp(2 log sn) + eps; alpha = K^-1 y, y the targets
 * given to set_train), Rasmussen & Williams 5.4.2 in block form:
 *   Sigma_V = Q^-1,  mu_V = y_V - Q^-1 a,  logp_V = -a^T Q^-1 a / 2 + log|Q| / 2 - m log(2 pi) / 2
 * computed with Q = C C^T, w = C^-1 a as
 *   logp_V = -|w|^2 / 2 + sum_i log C_ii - m log(2 pi) / 2,  mu_V = y_V - C^-T w,  var_i = sum_k (C^-1)_ki^2.
 * Folds of one point each give gprx_batch_loo; one fold of all points gives logp = mll.
 *
 * gprx_batch_set_folds: fold_of[N] is the fold id, 0..nfolds-1, of every training point; slot_stride
 * as in gprx_batch_set_train (0: one array shared by all slots, N: one per slot).  The folds are any
 * partition of the points (not contiguous, not equal in size; an empty fold contributes 0 to logp).
 * GPRX_INVALID_ARGUMENT for a NULL argument, a stride other than 0 or N, nfolds < 1, an id out of
 * range or a fold of more than GPRX_CVFOLD_MAX points (one workgroup factors one fold's block, as in
 * gprx_batch_sample).  The call orders each slot's points by fold (stably), builds the fold starts and
 * the table of the 64 x 64 tiles of K^-1 that a fold reaches, and uploads them once; they stay with
 * the batch until the next gprx_batch_set_folds.  It needs no training data and no factorisation.
 * A call that fails (GPRX_OUT_OF_MEMORY for the table included) leaves the batch's folds as they were.
 *
 * gprx_batch_cvfold: host outputs, any may be NULL: mu[B*N] and var[B*N] in the order of the training
 * points (var the y-space marginal variances diag(Sigma_V)), logp_fold[B*nfolds], logp[B] (the sum of
 * the folds' in ascending fold order), status[B].  GPRX_NOT_READY before a successful factorisation
 * or before gprx_batch_set_folds.  A slot whose status in that evaluation was not GPRX_OK gets NaN in
 * all its outputs and keeps that status; the other slots are unaffected.  A fold whose block Q has a
 * pivot that is not finite or <= 0 (no jitter is added: Q is a principal block of K^-1) gives its slot
 * GPRX_NOT_POSITIVE_DEFINITE and NaN at that fold's points, in that fold's logp and in the slot's logp.
 * Returns GPRX_OK or the first failing slot's status.  The results are bitwise reproducible and depend
 * on N, the fold layout and the index alone: not on B or on the slot's place in the batch.
 * Accuracy: Q is as well conditioned as K, but mu and var of a fold go through Q^-1 = C^-T C^-1 after
 * K^-1 was formed, and lose about cond(K)^2 eps for a fold that holds most of the points (for one fold
 * of all points var_i = K_ii is recovered from K^-1: at cond(K) = 1e11 its error is of the order of
 * var itself, with status GPRX_OK).  Small folds at such theta and every fold at moderate cond(K) are
 * accurate to the usual cond(K) eps; logp and logp_fold are well behaved throughout (one fold: mll).
 * No fp64 closed form from K^-1 does better; where the variances of large folds at ill-conditioned
 * theta matter, refit without the fold.
 * The call overwrites the factorisation workspace Lw (with L^-T's rows in fold order, then fold by
 * fold with C and C^-T), which nothing reads before the next evaluation rewrites it: predictions,
 * alpha, gprx_batch_loo and gprx_batch_loo_grad after it return what they return without it.  The
 * rest comes from the context's scratch buffer: 8 B (4096 T + 4 Npad + nfolds + 1) + 4 B (nfolds + 1)
 * bytes, T the largest number of tiles a slot's folds reach (nt for folds within a tile, nt (nt + 1) / 2
 * at most); GPRX_OUT_OF_MEMORY if it cannot be had.  gprx_batch_bytes and gprx_batch_cov_bytes are
 * unchanged.  The launches go straight on the context stream (stats "cv_pack", "cv_kinv", "cv_fold",
 * "cv_final").                                                                                     */
#define GPRX_CVFOLD_MAX 1024
int gprx_batch_set_folds(gprx_batch* batch, const int* fold_of, size_t slot_stride, int nfolds);
int gprx_batch_cvfold(gprx_batch* batch, double* mu, double* var, double* logp_fold, double* logp, int* status);

/* ---- hyper-parameter optimisation on the device ------------------------------------------- */
/* GaussianProcesses.optimize!(gp, LBFGS(linesearch=BackTracking(order=2)), Optim.Options(...))
 * (examples/maximal_coordinates/CPnoise.jl:41 and its 15 siblings) for every slot of a batch:
 * Optim 1.4.1 LBFGS + LineSearches 7.1.1 BackTracking restated as a device state machine, one
 * per slot, advanced in lock-step between evaluations of the whole batch (every evaluation
 * carries the gradient).  Minimises -mll over theta = [log sn, log ell_1..d, log sf]; a failed
 * evaluation (not positive definite, non-finite theta) counts as +Inf, as get_optim_target.   */
#define GPRX_STOP_ITERATIONS 0
#define GPRX_STOP_G_TOL 1
#define GPRX_STOP_X_TOL 2
#define GPRX_STOP_F_TOL 3
#define GPRX_STOP_LINESEARCH 4
#define GPRX_STOP_MAX_EVALS 5
#define GPRX_STOP_TIME_LIMIT 6
#define GPRX_STOP_NAN_GRADIENT 7 /* Optim: "Terminated early due to NaN in gradient"             */
#define GPRX_STOP_CONVERGED 0x100 /* or-ed into stopped[] when assess_convergence succeeded */
typedef struct gprx_opt_options {
  int m;              /* LBFGS history length (Optim: 10)                                        */
  int iterations;     /* Options.iterations (1000)                                               */
  int max_evals;      /* Options.f_calls_limit, the deterministic budget: a soft limit on f calls
                         (the initial evaluation + every line-search trial = the device evaluations),
                         checked after each iteration; <= 0: none (default;
                         Optim's f_calls_limit = 0)                        */
  int ls_iterations;  /* BackTracking.iterations (1000)                                          */
  int scaleinvH0;     /* LBFGS scaleinvH0 (true)                                                 */
  int refit;          /* 1: end with one evaluation of every slot at its minimiser, as optimize!
                         does (set_params! + update_target!); mll/predict then use it (default 1) */
  int successive_f_tol; /* Options.successive_f_tol (1): an exact f repeat converges only after
                           successive_f_tol + 1 successive iterations                          */
  double g_abstol;    /* Options.g_abstol (1e-8); x_abstol = f_abstol = 0 as Optim's defaults     */
  double time_limit;  /* seconds (the experiments use 10); NaN (default) or < 0: none.  Checked
                         between rounds: a slot stops after the iteration that sees it expired  */
  double alphaguess;  /* InitialStatic alpha (1.0)                                               */
  double c_1, rho_hi, rho_lo; /* BackTracking (1e-4, 0.5, 0.1)                                   */
} gprx_opt_options;
void gprx_opt_defaults(gprx_opt_options* opt);
/* theta0[B*(d+2)] start points; outputs (host, any may be NULL): theta_out[B*(d+2)] minimisers,
 * minimum[B] = -mll at the minimiser as Optim reports it, iterations/f_calls/g_calls[B],
 * stopped[B] = GPRX_STOP_* | GPRX_STOP_CONVERGED, rounds = batch evaluations performed
 * (excluding the refit; a round evaluates only the slots whose optimisers are still running, so a
 * ragged batch costs less per round as slots finish).  Returns GPRX_OK, or an error of the evaluations themselves
 * (device / memory); per-slot failures during the search are +Inf answers, not errors.  With
 * refit, a minimiser whose refit fails (not finite: GPRX_INVALID_ARGUMENT; not positive definite:
 * GPRX_NOT_POSITIVE_DEFINITE) is returned as that status (first failing slot), the outputs are
 * still filled, and the batch is left unfactorised (predict answers GPRX_NOT_READY).
 * time_limit is one wall clock for the whole call (all slots), not per GP as Optim's per-call
 * Options(time_limit=10.) at CPnoise.jl:41.  The context's mutex is held for the whole call:
 * other threads sharing the context wait until the optimisation ends.                         */
/* Outputs are written when the call returns GPRX_OK or a refit status after the search.  A call
 * rejected before the search (no training data, options out of range: GPRX_INVALID_ARGUMENT)
 * and a device / memory error write none of them.                                               */
int gprx_batch_optimize(gprx_batch* batch, const double* theta0, const gprx_opt_options* opt, double* theta_out,
                        double* minimum, int* iterations, int* f_calls, int* g_calls, int* stopped, int* rounds);
/* The same optimiser with the objective named.  GPRX_OBJ_MLL is gprx_batch_optimize itself (one body:
 * the same results bit for bit).  GPRX_OBJ_LOO minimises -logp_LOO, the leave-one-out log predictive
 * probability with gprx_batch_loo_grad's gradient: a round evaluates the running slots without the
 * marginal-likelihood gradient (Gram, factorisation, alpha, finalize), runs the six leave-one-out
 * launches for the same slots (stats "loo_diag" .. "loo_grad_final"; the workspace comes from the
 * context's scratch buffer, sized once before the first round) and the state machines take
 * f = -logp, g = -dlogp from those result rows; a failed slot or a non-finite point answers +Inf with a
 * NaN gradient as ever.  minimum[B] is then -logp_LOO at the minimiser.  Arguments, outputs, stop
 * codes, budget, time limit and the refit are gprx_batch_optimize's: with refit the call ends with one
 * evaluation of every slot at its minimiser, marginal-likelihood gradient included, so predict, alpha,
 * gprx_batch_loo and gprx_batch_loo_grad answer for the minimisers.  Any other objective value is
 * GPRX_INVALID_ARGUMENT and writes no output.  A registered trace's rows hold [active, theta, logp,
 * dlogp] in GPRX_OBJ_LOO rounds.                                                                 */
#define GPRX_OBJ_MLL 0 /* -mll: what gprx_batch_optimize minimises */
#define GPRX_OBJ_LOO 1 /* -logp_LOO (gprx_batch_loo_grad's logp and gradient) */
int gprx_batch_optimize_obj(gprx_batch* batch, int objective, const double* theta0, const gprx_opt_options* opt,
                            double* theta_out, double* minimum, int* iterations, int* f_calls, int* g_calls,
                            int* stopped, int* rounds);
/* Diagnostics: record the optimiser's evaluations.  With a host buffer of max_rounds * B * (2(d+2)+2)
 * doubles registered, every later gprx_batch_optimize on this batch writes, for round r < max_rounds
 * and slot b, at trace[(r*B + b) * (2(d+2)+2)]: [active (1/0: evaluated in this round), theta(d+2)
 * as evaluated, mll, dmll(d+2) as answered]; rounds past the last are NaN.  capacity: the buffer's
 * size in doubles; smaller than max_rounds * B * (2(d+2)+2) is GPRX_INVALID_ARGUMENT (nothing is
 * registered).  The buffer must stay valid while registered; max_rounds = 0 unregisters it.  (No
 * reference counterpart: it makes the device optimiser's evaluation sequence comparable with a
 * host restatement's, gprx/optim.py.)                                                           */
int gprx_batch_set_opt_trace(gprx_batch* batch, double* trace, int max_rounds, int64_t capacity);

/* ---- single GP: the GPE surface, a batch of one ------------------------------------------- */
int gprx_gp_create(gprx_ctx* ctx, const double* X, int d, int N, const double* y_minus_mean,
                   gprx_gp** out);
void gprx_gp_destroy(gprx_gp* gp);
int gprx_gp_lml(gprx_gp* gp, const double* theta, double* mll);
int gprx_gp_lml_grad(gprx_gp* gp, const double* theta, double* mll, double* grad);
/* f-space predictive mean (k*^T alpha) and variance (max(k** - |L^-1 k*|^2, 0)) at the
 * factorisation of the last lml call; var may be NULL.                                          */
int gprx_gp_predict(gprx_gp* gp, const double* Xs, int M, double* mu_f, double* var_f);
/* [ext] predict_f(gp, x; full_cov=true): mu_f[M] (may be NULL), cov[M*M]; and rand(gp, x, n) in
 * f-space: samples[S*M] from Z[S*M] host standard normals, jitter (may be NULL) as
 * gprx_batch_sample (whose jitter rule is gprx's own).                                          */
int gprx_gp_predict_cov(gprx_gp* gp, const double* Xs, int M, double* mu, double* cov);
int gprx_gp_sample(gprx_gp* gp, const double* Xs, int M, const double* Z, int S, double* samples, double* jitter);
/* [ext] predict_LOO(gp): mu[N], var[N]; logp_LOO(gp): logp[1]; any may be NULL (gprx_batch_loo on
 * the batch of one, at the factorisation of the last lml call).                                  */
int gprx_gp_loo(gprx_gp* gp, double* mu, double* var, double* logp);
/* [ext, recalled] dlogpdtheta_LOO(gp): logp[1], grad[d+2] in the order of theta; either may be NULL
 * (gprx_batch_loo_grad on the batch of one, at the factorisation of the last lml call).         */
int gprx_gp_loo_grad(gprx_gp* gp, double* logp, double* grad);
/* [ext] predict_CVfold(gp, folds): mu[N], var[N]; logp_CVfold(gp, folds): logp[1], logp_fold[nfolds];
 * any may be NULL (gprx_batch_set_folds / gprx_batch_cvfold on the batch of one, at the factorisation
 * of the last lml call).  fold_of[N]: the fold id of every training point.                      */
int gprx_gp_set_folds(gprx_gp* gp, const int* fold_of, int nfolds);
int gprx_gp_cvfold(gprx_gp* gp, double* mu, double* var, double* logp_fold, double* logp);

/* the single GP's underlying batch of one (slot 0), e.g. for gprx_rollout_min              */
gprx_batch* gprx_gp_batch(gprx_gp* gp);

/* ---- rollout in minimal coordinates (examples/utils/predictdynamics.jl:30-102) ------------ */
#define GPRX_MECH_P1 1 /* pendulum:           q = theta                                  */
#define GPRX_MECH_P2 2 /* double pendulum:    q = (theta1, theta2 relative)              */
#define GPRX_MECH_CP 3 /* cart-pole:          q = (x, theta)                             */
#define GPRX_MECH_FB 4 /* four-bar:           q = (theta1, theta3)                       */
/* predictdynamicsmin for T trajectories in one launch.  A rollout group is the nc GPs of one
 * trial (nc = 1 for P1, else 2; GP g predicts the rate of coordinate g), given as
 * (batches[k], slots[k]) for k = group*nc + g, each factorised by its last gprx_batch_run with
 * MeanZero targets.  Trajectory t uses group traj_group[t] and starts at
 * start[t*2nc ...] = (q_1, qdot_1, ..., q_nc, qdot_nc); the GP input per step is
 * (q, qdot) per coordinate, or (sin q, cos q, qdot) for angles when usesin (input dimension
 * must match).  Each of the `steps` steps predicts the rates at the previous state and advances
 * q by rate*dt, exactly as the reference loop.  final_state[t*2nc ...] = (q_cur, qdot_last);
 * the reference's returned CState is built from q_cur with zero velocities (host side).        */
int gprx_rollout_min(gprx_ctx* ctx, int mech, int usesin, double dt, int steps, int ngroups,
                     gprx_batch* const* batches, const int* slots, int T, const int* traj_group,
                     const double* start, double* final_state);

/* ---- maximal-coordinate physics: projectv! and predictdynamics ----------------------------- */
/* projectv!(vu, wu, mechanism; newtonIter, eps, regularizer)  src/projections/implicitProjection.jl:80-107
 * for T independent mechanism states in one launch: state t is the mechanism's CState
 * cstates[t*13nb ...] (setstates!: positions, quaternions, velocities; the discrete pose follows as
 * x2 = x + v dt, q2 = q * wbar(w) dt/2), the prediction vw_pred[t*6nb ...] = (v_1, w_1, ..., v_nb,
 * w_nb).  Outputs vw_out (the projected twists; NaN for a failed state), iterations[t], status[t]
 * (0 ok, 1 singular KKT matrix: Julia's F \ f throws SingularException).  mech: GPRX_MECH_*, the
 * experiment mechanisms of examples/utils/data/simulations.jl (P1 pendulum, P2 double pendulum,
 * CP cart-pole, FB four-bar).  dt: mechanism.dt (0.01 in the experiments).
 * newton_iter = 0 returns vw_pred unchanged (iterations 0, status 0); eps = 0 runs all newton_iter
 * iterations.  Status 0 does not say that the iteration converged: compare iterations[t] with
 * newton_iter.  A state whose system is not finite (|w| of a body or of its prediction beyond
 * 2/dt, where the reference's sqrt throws a DomainError) is not detected, unlike in
 * gprx_vi_step: it runs all newton_iter iterations on NaNs and returns a NaN row with
 * iterations[t] = newton_iter and status[t] = 0 (measured on an MI355X, asserted by
 * tests/test_hp_physics.py).  The other states of the launch are not affected by it.  This is
 * gprx_projectv's contract alone: what gprx_rollout_max and gprx_rollout_max_md do with such a
 * state in their projection is neither specified nor tested.                                     */
int gprx_projectv(gprx_ctx* ctx, int mech, double dt, int T, const double* cstates, const double* vw_pred,
                  double regularizer, int newton_iter, double eps, double* vw_out, int* iterations, int* status);
/* One variational-integrator step, ConstrainedDynamics 0.7.4 newton!(mechanism) after
 * setstates!(mechanism, CState(x)) -- the prior mean of GPR's MeanDynamics (src/mDynamics.jl:41-60,
 * getmu = CState(mechanism, usesolution=true)) -- for T independent states in one launch, one wave
 * each.  cstates[t*13nb ...]: the current CState; out[t*13nb ...]: the solution CState [x2, q2, v2,
 * w2] per body (NaN row for a failed state).  status[t]: 0 converged (|f| < eps and |ds| < eps), 1
 * not converged within newton_iter iterations, 2 failed (a non-finite system, |w| beyond 2/dt: the
 * reference's DomainError; or a singular one: SingularException).  regularizer: the impulses'
 * regularisation (1e-10 for the four-bar's redundant loop constraints, 0 otherwise).  The host
 * restatement and its documentation: gpr.jl_amd/gprx/vi.py (vi_step).                          */
int gprx_vi_step(gprx_ctx* ctx, int mech, double dt, int T, const double* cstates, double regularizer,
                 int newton_iter, double eps, double* out, int* iterations, int* status);
/* simulate!(mechanism, steps dt, control!, record = true) as the reference makes its datasets
 * (examples/utils/data/simulations.jl: simplependulum2D, doublependulum2D, cartpole, fourbar;
 * examples/parallel/dataframes.jl reads the storage) for T independent trajectories, every step
 * on the device, one wave per trajectory: per step control!, gprx_vi_step's newton!, and the
 * solution CState [x2, q2, v2, w2] becomes the current one (updatestate!).
 * start[t*13nb ...]: the start CState.  Per-trajectory bodies (NULL: the mechanism's nominal
 * ones): mass[t*nb + b]; inertia[(t*nb + b)*9 ...] the body-frame tensor, row-major.  Viscous
 * friction damp[(t*nb + b)*6 ...] = (c_v(3), c_w(3)) (NULL: none): control! reads the current
 * velocities, F = -c_v o v1 (world frame), tau = -c_w o w1 (body frame), constant during the solve,
 * and the step's dynamics rows are
 *     m ((v2 - v1)/dt + g e_z) - F - Gpos_x^T lambda = 0
 *     (sq2 I + [w2 x]) J w2 - (sq1 I - [w1 x]) J w1 - 2 tau - Gpos_phi^T lambda = 0
 * (gpr.jl_amd/gprx/vi.py; gravity 9.81).  The reference's friction is c_w.x of body i = friction[i]
 * (P1, P2, FB); for CP the cart's c_v.y = friction[1] and the pole's c_w.x = friction[2].
 * The trajectory is not stored.  rec[t*R ...]: R non-decreasing 1-based storage indices in
 * [1, steps + 1] (1: the start; j: the state after j - 1 steps, saveToStorage! before each step);
 * out[(t*R + r)*13nb ...] is the CState at rec[t*R + r], and a trajectory stops after its last
 * index.  A failed step (gprx_vi_step status 2) ends its trajectory: the remaining records are NaN
 * and status[t] = 2; a step that does not converge within newton_iter is used as it is, and so is
 * one that stagnates at the rounding floor (|f| < eps, the twist's step < eps, and |ds| no longer
 * falling: at a small dt the multipliers' rounding floor (m/dt)(1e-16/dt) lies above eps, so
 * newton!'s test cannot hold), which ends with status 1 without running the remaining iterations;
 * status[t] (may be NULL) is the OR of the per-step statuses.  The call runs as successive launches
 * of at most steps_per_launch steps (0: the default, 16 for T <= 1024 and 16 / ceil(T / 1024) beyond,
 * which keeps a four-bar launch whose every step runs 100 Newton iterations near 0.2 s; measured
 * with T = 200), state and record cursor carried in device
 * memory; the results do not depend on it.  GPRX_INVALID_ARGUMENT: bad sizes, a decreasing
 * rec or an index out of range.  T = 0 is GPRX_OK.                                                 */
int gprx_simulate(gprx_ctx* ctx, int mech, double dt, int steps, int T, const double* start,
                  const double* mass, const double* inertia, const double* damp, double vi_regularizer,
                  int newton_iter, double eps, int R, const int* rec, int steps_per_launch,
                  double* out, int* status);
/* predictdynamics(mechanism, gps, startobservation, steps, getvw; regularizer)
 * examples/utils/predictdynamics.jl:7-22 for T trajectories in one launch: per step the G GPs'
 * mean predictions at the current CState (predict_y(gp, obs)[1][1], MeanZero), getvw (output g
 * placed at 1-based CState position vw_idx1[g], a velocity or angular-velocity slot), projectv!
 * and updatestate!; one closing updatestate!.  GPs as for gprx_rollout_min: (batches[k],
 * slots[k]) for k = group*G + g, factorised, input dimension 13 nb.  Outputs final_state[t*13nb]
 * (the predicted CState), proj_err[t] (mean projection error per step), status[t] (0 ok, 1
 * singular projection).                                                                          */
int gprx_rollout_max(gprx_ctx* ctx, int mech, double dt, int steps, double regularizer, int ngroups,
                     gprx_batch* const* batches, const int* slots, int G, const int* vw_idx1, int T,
                     const int* traj_group, const double* start, double* final_state, double* proj_err,
                     int* status);

/* ---- rollouts with MeanDynamics GPs: predict_y(gp, obs) = mu(obs) + k*^T alpha ------------------
 * The GPs are (batch, slot) pairs factorised on y - mu(X); mu is one variational-integrator step
 * of the mechanism (src/mDynamics.jl:41-55; gprx_vi_step), solved on the device at every step's
 * state with newton_iter = 100, eps = 1e-10 and gravity 9.81 (gprx_vi_step's callers' values) and
 * the impulses' regularisation vi_regularizer (1e-10 for the four-bar, 0 otherwise).  One launch
 * runs every step of every trajectory.  A physics step that fails (gprx_vi_step status 2: the
 * reference throws) stops its trajectory: status[t] = 2 and a NaN output row; one that does not
 * converge within newton_iter (status 1) is used as it is.  vi_status (may be NULL): the OR of the
 * trajectory's per-step physics statuses.                                                        */
/* predictdynamics (examples/utils/predictdynamics.jl:7-22) with the mean of src/mDynamics.jl:41-55:
 * gprx_rollout_max's arguments and outputs; per step mu_g = GP mean + v2 / w2 of the physics
 * solution at CState position vw_idx1[g] (getmu(vwindices)), then getvw, projectv! and
 * updatestate!.  status[t]: 0 ok, 1 singular projection, 2 failed physics mean.                   */
int gprx_rollout_max_md(gprx_ctx* ctx, int mech, double dt, int steps, double regularizer, double vi_regularizer,
                        int ngroups, gprx_batch* const* batches, const int* slots, int G, const int* vw_idx1,
                        int T, const int* traj_group, const double* start,
                        double* final_state, double* proj_err, int* status, int* vi_status);
/* predictdynamicsmin (examples/utils/predictdynamics.jl:30-102) with the mean of
 * src/mDynamics.jl:41-55: gprx_rollout_min's arguments and outputs; per step the experiments'
 * xtransform builds the CState from the GP input (the angle by atan2(sin, cos) when usesin, the
 * linear velocities by the literal 0.01 finite difference), and the rate of coordinate g is the GP
 * mean plus the physics solution's rate (P1 w1; P2 w1, w2 - w1; CP v1_y, w2; FB w1, w3).
 * status[t]: 0 ok, 2 failed physics mean.                                                        */
int gprx_rollout_min_md(gprx_ctx* ctx, int mech, int usesin, double dt, int steps, double vi_regularizer,
                        int ngroups, gprx_batch* const* batches, const int* slots,
                        int T, const int* traj_group, const double* start,
                        double* final_state, int* status, int* vi_status);

/* ---- recorded rollouts: the trajectory step by step, in bounded launches --------------------------
 * The four rollouts above return the final state only and run every step in one launch.  Each
 * entry point below takes the arguments of its one-launch counterpart plus R, rec,
 * steps_per_launch and traj, keeps the trajectory's state after the steps the caller names
 * (examples/energy.jl keeps all 600 000), and runs as successive launches of at most
 * steps_per_launch steps, the trajectory's state and record cursor carried in device memory, so
 * that no launch holds the device for seconds.
 * rec[t*R ...]: R non-decreasing 1-based storage indices in [1, steps + 1], gprx_simulate's
 * convention: 1 is the start as given, j the trajectory's state after j - 1 steps, before the
 * closing updatestate!.  traj[(t*R + r)*w ...] is the row at rec[t*R + r]:
 *   maximal (w = 13 nb): oldstates = CState(mechanism) of predictdynamics.jl:18, the state the
 *     GPs are evaluated at in step j (energy.jl's predictedstates);
 *   minimal (w = 2 nc): (q_old, qdot_old) per coordinate.
 * R = 0 with rec and traj NULL is allowed: a bounded-launch rollout that records nothing.
 * The final outputs (final_state, proj_err, status, vi_status) are bit for bit those of the
 * one-launch entry point for the same arguments, for every steps_per_launch -- a trajectory always
 * runs all `steps`, wherever its last record lies -- and traj does not depend on
 * steps_per_launch.  A trajectory that stops (status 1, singular projection; status 2, failed
 * physics mean) keeps its one-launch outputs (NaN row, status); its records up to the state the
 * failed step started from are kept and the later ones are NaN; the other trajectories of the call
 * are not affected.
 * steps_per_launch >= 1, or 0 for the default: 0.2 s divided by the time one step of the call's T
 * trajectories takes at the largest shapes the project rolls out (the four-bar, N = 512), lat + T traj
 * from two measurements on an MI355X, T = 100 and T = 3200 (DESIGN.md section 4 has the figures):
 * T = 100 gives 56 steps (maximal), 34 (maximal, MeanDynamics), 224 (minimal, MeanDynamics) and
 * 45 977 (minimal); T = 3200 gives 17, 10, 21 and 6514.
 * GPRX_INVALID_ARGUMENT: what the one-launch call refuses, R < 0, steps_per_launch < 0, a
 * decreasing rec or an index out of range, rec or traj NULL with R > 0.  T = 0 is GPRX_OK.  The
 * records live in the context's scratch buffer until they are copied out: GPRX_OUT_OF_MEMORY when
 * it cannot be grown to T * R * w doubles.                                                         */
int gprx_rollout_min_rec(gprx_ctx* ctx, int mech, int usesin, double dt, int steps, int ngroups,
                         gprx_batch* const* batches, const int* slots, int T, const int* traj_group,
                         const double* start, double* final_state,
                         int R, const int* rec, int steps_per_launch, double* traj);
int gprx_rollout_min_md_rec(gprx_ctx* ctx, int mech, int usesin, double dt, int steps, double vi_regularizer,
                            int ngroups, gprx_batch* const* batches, const int* slots,
                            int T, const int* traj_group, const double* start,
                            double* final_state, int* status, int* vi_status,
                            int R, const int* rec, int steps_per_launch, double* traj);
int gprx_rollout_max_rec(gprx_ctx* ctx, int mech, double dt, int steps, double regularizer, int ngroups,
                         gprx_batch* const* batches, const int* slots, int G, const int* vw_idx1, int T,
                         const int* traj_group, const double* start, double* final_state, double* proj_err,
                         int* status, int R, const int* rec, int steps_per_launch, double* traj);
int gprx_rollout_max_md_rec(gprx_ctx* ctx, int mech, double dt, int steps, double regularizer, double vi_regularizer,
                            int ngroups, gprx_batch* const* batches, const int* slots, int G, const int* vw_idx1,
                            int T, const int* traj_group, const double* start,
                            double* final_state, double* proj_err, int* status, int* vi_status,
                            int R, const int* rec, int steps_per_launch, double* traj);

/* ---- host-side CState helpers (bit-exact copies) ------------------------------------------ */
/* out[13*b + 0..12] = [xc(3), qc.w, qc.x, qc.y, qc.z, vc(3), wc(3)] for body b (CState.jl:20,26) */
int gprx_cstate_pack(int nbodies, const double* xc, const double* qc_wxyz, const double* vc,
                     const double* wc, double* out);
/* Y[k*N + t] = Xcurr[t*d + (idx1[k]-1)]  (1-based indices, as vwindices in the experiments)     */
int gprx_select_outputs(const double* Xcurr, int d, int N, const int* idx1, int G, double* Y);

#ifdef __cplusplus
}
#endif
#endif /* GPRX_H */
