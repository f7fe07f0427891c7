// Internal declarations shared by the HIP kernels (gprx_kernels.hip, gprx_lbfgs.hip,
// gprx_projection.hip) and the C-ABI host code (gprx_api.hip), and the device helpers that more than
// one of the kernel files uses.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <stddef.h>
#include <stdint.h>

namespace gprx {

constexpr int TS = 64;     // tile edge (rows/cols) of every matrix block
constexpr int NTHR = 256;  // threads per workgroup (4 waves)
constexpr int DMAX = 64;   // largest input dimension d supported (FB: 52)

// Device-resident state of one batch of B GP slots with equal (d, N).  Passed to every kernel by
// value.  Matrices are column-major with leading dimension ld = Npad (Npad = ceil(N/64)*64).
//   K    : Gram matrix (lower tiles), reduced in place by the recursive Cholesky's SYRK updates.
//   Lw   : recursion workspace: L21 blocks (strictly lower tiles) and T^T = L11^-1 L21^T blocks
//          (strictly upper tiles).
//   Linv : L^{-1} (lower).      Mt : L^{-T} (upper) = Linv^T, so that every GEMM streams operands
//                                    along contiguous columns.
struct DevBatch {
  int B, d, N, Npad, nt, ntl;  // nt = Npad/64 tiles per edge, ntl = nt(nt+1)/2 lower tiles
  int M, Mpad, mt;             // test points (per slot), padded to 64, mt = Mpad/64
  int dist_mode;               // GPRX_DIST_EXPANDED / GPRX_DIST_DIRECT
  int want_var;                // predictive variance requested (var output non-NULL); 0 skips the
                               // O(N^2 M) variance GEMM (predictdynamics.jl uses the mean only)
  int small_n;                 // recursion nodes of <= small_n tiles use the 64 x 32 pair-unit GEMM
                               // (default, set_geometry in gprx_api.hip: 4 for B >= 32, all nodes
                               // below that, where the 64 x 64 units leave most of the chip idle);
                               // larger: 64 x 64 core
  int da;                      // active dimensions: those not constant over the training points of
                               // every slot (gprx_batch_set_train; d when GPRX_OPT_ACTIVE_DIMS is 0 or
                               // the distance mode is expanded).  A constant dimension adds an exact
                               // +0 to every direct-mode distance, so the Gram and the gradient skip it
  int xs;                      // row stride of Xc: da | 1 (odd: spreads LDS banks)
  int pst;                     // stride of params per slot
  int gps;                     // stride of per-unit gradient partials (da + 2)
  int ngu;                     // gradient partial units per slot (lauum 4-tile units)
  int nlj;                     // lauum jobs per slot (units folded in pairs)
  int nimg;                    // largest number of point-tile images of a lauum unit (LDS size)
  size_t ld, mat;              // ld = Npad, mat = Npad*Npad
  double* X;                   // B x [Npad][d]   (column t = one CState, contiguous d values)
  double* Xc;                  // B x [Npad][xs]  the active dimensions of X, ascending, each minus its
                               //                 mean over the N points, columns da..xs-1 zero
                               //                 (theta-independent; the gradient's distance sums)
  double* Y;                   // B x Npad        (y - mean(X), zero padded)
  double* K;                   // B x mat: lower tiles of K as the Gram wrote them (kept: the gradient
                               //   reads its off-diagonal entries as Kf)
  double* S;                   // B x mat: lower tiles of the trailing matrices the SYRKs update
  double* Lw;                  // B x mat
  double* Linv;                // B x mat
  double* Mt;                  // B x mat
  double* z;                   // B x Npad        z = L^{-1} y
  double* zp;                  // B x 2nt x Npad  per-tile partials of z (see zp_acc4); its unused triangle
                               //                 holds the partials of alpha (ap_row)
  double* alpha;               // B x Npad        alpha = K^{-1} y; until k_alpha writes it, a block's
                               //                 working right-hand side (yw_slot)
  double* params;              // B x pst: [0,d) il2 = exp(-2 log ell), d: sf2, d+1: noise diag
                               //          (sn2 + eps), d+2: sn2, d+3: the dropped dimensions' share of a distance sum
                               //          (+0 or NaN, derive_params)
  double* theta;               // B x (d+2) hyper-parameters [log sn, log ell_1..d, log sf] of the
                               //          evaluation; params derive from it on the device
  double* logdet_part;         // B x nt          sum_r log L_rr per diagonal tile
  double* grad_part;           // B x ngu x gps   per lauum unit: S_p (da, active order), S_f, trace(W)
  double* Xs;                  // B x [Mpad][d]   test points
  double* KsT;                 // B x [Npad][Mpad] K*^T (column-major M x N, ld = Mpad)
  double* mu_part;             // B x nt x Mpad
  double* var_part;            // B x nt x Mpad
  double* out;                 // B x (d+3): mll, grad[d+2]
  double* out_mu;              // B x Mpad
  double* out_var;             // B x Mpad
  int* status;                 // B
  int* info;                   // B
  int* lauum_order;            // nlj x 2 x LU: two units per job, long + short (lauum_plan)
  const int* active;           // B or null: evaluate only the slots with active[s] != 0 (the device
                               //   optimiser's rounds; null = every slot)
  unsigned long long amask;    // bit p: dimension p is active (da bits; a mask, not a list: indexing a
                               // list in the by-value struct would hold all of it in registers)
};

// GEMM operations of the recursive factorisation / inverse / prediction (tile units, see
// gprx_kernels.hip k_gemm):
enum GemmOp : int {
  OP_TRSM = 0,    // Lw[b2,b1]  = K[b2,b1] Linv[b1,b1]^T
  OP_SYRK = 1,    // K[b2,b2]  -= Lw[b2,b1] Lw[b2,b1]^T   (lower tiles)
  OP_TT = 2,      // Lw[b1,b2]  = Mt[b1,b1] Lw[b2,b1]^T   (= T^T, T = L21 L11^-1)
  OP_LINV21 = 3,  // Linv[b2,b1] = -Linv[b2,b2] T ; Mt[b1,b2] = Linv[b2,b1]^T
  OP_PREDVAR = 4  // var_part   = colsum((Linv K*)^2)
};
constexpr int OP_NONE = -1;
struct GemmGeom {
  int op;
  int o, h, n;  // node: offset o, split h, size n (tile units); block1 = [o, o+h), block2 = [o+h, o+n)
  int upd = 0;  // the node lies in an ancestor's trailing block: its tiles are read from S, not K
};
// Output rectangle of an op in tiles: origin (r0, c0), R x C, lower triangle only when tri.
__host__ __device__ inline void op_rect(const GemmGeom& g, int nt, int mt, int& r0, int& c0, int& R, int& C, bool& tri) {
  tri = false;
  switch (g.op) {
    case OP_TRSM:
    case OP_LINV21: r0 = g.o + g.h; c0 = g.o; R = g.n - g.h; C = g.h; break;
    case OP_SYRK: r0 = c0 = g.o + g.h; R = C = g.n - g.h; tri = true; break;
    case OP_TT: r0 = g.o; c0 = g.o + g.h; R = g.h; C = g.n - g.h; break;
    case OP_PREDVAR: r0 = 0; c0 = 0; R = nt; C = mt; break;
    default: r0 = c0 = R = C = 0; break;
  }
}

// Blocks of the recursion: factor_rec (gprx_api.hip) halves a node of more than BLK_TILES tiles (a
// split node) and finishes a smaller one as a block, by whichever kernels.  z is formed by forward
// substitution over the blocks and alpha's products across blocks come from the split nodes' LINV21
// tiles, so the host and the kernels share this one splitting rule.
constexpr int BLK_TILES = 8;
// the block [lo, hi) of tile i among nt tiles
__host__ __device__ inline void blk_range(int nt, int i, int& lo, int& hi) {
  int o = 0, n = nt;
  while (n > BLK_TILES) {
    const int h = n / 2;
    if (i < o + h) {
      n = h;
    } else {
      o += h;
      n -= h;
    }
  }
  lo = o;
  hi = o + n;
}

// Rollouts (k_rollout, k_rollout_max; gprx_projection.hip): one GP of a rollout group, read from a
// batch slot after its factorisation (X: [Npad][d], alpha: Npad, params: il2[d], sf2, ...).
struct RolloutGP {
  const double* X;
  const double* alpha;
  const double* params;
  int N;
  int pad;
};
struct RolloutArgs {
  const RolloutGP* gps;  // ngroups x nc, GP g of a group predicts the rate of coordinate g
  const int* group;      // T: rollout group of each trajectory
  const double* start;   // T x 2nc: (q, qdot) per coordinate (predictdynamicsmin's startobservation)
  double* out;           // T x 2nc: (q_cur, qdot_last) per coordinate
  int T, nc, d, steps;
  int usesin, ang0, ang1;  // obs (sin q, cos q, qdot) for angle coordinates when usesin
  double dt;
};
constexpr int ROLLOUT_DMAX = 6;

// Maximal-coordinate physics of the rollout (gprx_projection.hip): the joint constraints of a
// mechanism as sub-joints (Revolute = T3 + R2, Prismatic = T2 + R3, Cylindrical = T2 + R2), rows of
// each written in the order of the reference's equality constraints.
constexpr int PJ_MAXB = 4;    // bodies (FB)
constexpr int PJ_MAXSUB = 12; // sub-joints
constexpr int PJ_MAXN = 56;   // 6 nb + constraint rows (FB: 24 + 24 = 48)
constexpr int PJ_MAXG = 16;   // GP outputs of one rollout group
struct SubJoint {
  int kind;       // 0 translational, 1 rotational
  int a, b;       // parent (0 = origin) and child body, 1-based
  int rows, row0; // constraint rows (2 or 3) and the first row among all constraint rows
  double pa[3], pb[3];
  double C[3][3]; // rows of the constraint matrix (I3, or the 2 rows normal to the axis)
};
struct MechDev {
  int nb, nd, nsub;  // bodies, constraint rows, sub-joints
  SubJoint sub[PJ_MAXSUB];
  double m[PJ_MAXB];        // body masses and inertia tensors (body frame; the variational
  double J[PJ_MAXB][3][3];  // integrator's dynamics, k_vi_step)
};
struct ProjArgs {
  MechDev mech;
  double dt, reg, eps;
  int iters;          // newtonIter
  int T;              // trajectories
  const double* cs;   // T x 13 nb CStates (the mechanism state: xc, qc, vc, wc per body)
  const double* vw;   // T x 6 nb predicted (v, w) per body (projectv!'s vu, wu)
  double* out;        // T x 6 nb projected (v, w)
  int* iters_out;     // T Newton iterations
  int* status;        // T: 0 ok, 1 singular KKT matrix (Julia's F \ f throws)
};
struct RolloutMaxArgs {
  MechDev mech;
  double dt, reg, eps;
  int iters, steps, T, G, d;
  int vw[PJ_MAXG];      // 0-based CState position of output g (getvw)
  const RolloutGP* gps; // ngroups x G
  const int* group;     // T
  const double* start;  // T x d
  double* out;          // T x d final CStates
  double* perr;         // T mean projection error per step
  int* status;          // T: 0 ok, 1 singular projection, 2 failed physics mean (MeanDynamics)
};
// MeanDynamics GPs (the RolloutMaxMdArgs / RolloutMinMdArgs instantiations of k_rollout_max and
// k_rollout): the variational-integrator step that gives the prior mean at every step's state.  Kept
// apart from the MeanZero structs, so those kernels' arguments are what they were.
struct RolloutViArgs {
  double reg, eps, grav;
  int iters;
  int* status;          // T or null: OR of the per-step physics statuses (ViArgs::status)
};
struct RolloutMaxMdArgs : RolloutMaxArgs {
  RolloutViArgs vi;
};
// predictdynamicsmin with MeanDynamics GPs: RolloutArgs' rollout plus, per step, the experiments'
// xtransform of the features into a CState and one variational-integrator step.  A failed physics
// mean leaves a NaN row in out.
struct RolloutMinMdArgs : RolloutArgs {
  MechDev mech;
  int mech_id;
  double len[2];        // link lengths (gprx/rollout.py LENGTHS)
  int* status;          // T: 0 ok, 2 failed physics mean
  RolloutViArgs vi;
};
// The recording, resumable forms of the four rollouts (the *RecArgs instantiations of k_rollout_max
// and k_rollout): one launch takes steps [step0, step0 + nsteps) of the call's `steps`, writes the
// records whose storage index (1 = the start, j = after j - 1 steps) it reaches, and, unless it is
// the last, stores what the step loop and the closing update read on entry; the next launch takes
// that up again.  The last launch (step0 + nsteps = steps) writes the usual outputs.  The
// one-launch argument structs, and with them those kernels, are what they were.
struct RolloutRec {
  int R, step0, nsteps;
  const int* rec;   // T x R non-decreasing 1-based storage indices (null when R = 0)
  double* traj;     // T x R rows: the CState (13 nb) or (q_old, qdot_old) per coordinate (2 nc)
  int* cursor;      // T: records written so far
  double* carry;    // T x ROLLOUT_CARRY doubles
  int* icarry;      // T x 2: status / failed, OR of the physics statuses
};
struct RolloutMaxRecArgs : RolloutMaxArgs {
  RolloutRec rr;
};
struct RolloutMaxMdRecArgs : RolloutMaxMdArgs {
  RolloutRec rr;
};
struct RolloutRecArgs : RolloutArgs {
  RolloutRec rr;
};
struct RolloutMinMdRecArgs : RolloutMinMdArgs {
  RolloutRec rr;
};
// doubles a trajectory carries from launch to launch.  Maximal: [obs 13 | xk 3 | qk 4 | s 6] per
// body, then the projection-error sum.  Minimal: (q_old, qdot_old, q_cur) per coordinate.
constexpr int ROLLOUT_CARRY = 26 * PJ_MAXB + 1;
// One variational-integrator step (ConstrainedDynamics 0.7.4 newton!, restated in gprx/vi.py) for T
// independent states: the MeanDynamics prior mean (src/mDynamics.jl:41-60).
struct ViArgs {
  MechDev mech;
  double dt, reg, eps, grav;
  int iters;          // newtonIter
  int T;
  const double* cs;   // T x 13 nb current CStates
  double* out;        // T x 13 nb solution CStates [x2, q2, v2, w2] per body (NaN row: failed)
  int* iters_out;     // T Newton iterations
  int* status;        // T: 0 converged, 1 not converged, 2 failed (non-finite / singular system)
};
// Many variational-integrator steps per launch with per-trajectory bodies and viscous friction (the
// datasets' simulate!, examples/utils/data/simulations.jl): steps [step0, step0 + nsteps) of every
// trajectory.  cs, cursor and status carry a trajectory from one launch to the next.
struct SimArgs {
  MechDev mech;         // the joints; its m / J are the bodies where mass / inertia are null
  double dt, reg, eps, grav;
  int iters;            // newtonIter
  int T, R;             // trajectories, records per trajectory
  int step0, nsteps;    // cs holds storage index step0 + 1 on entry
  const double* mass;     // T x nb or null
  const double* inertia;  // T x nb x 9 (row-major 3 x 3, body frame) or null
  const double* damp;     // T x nb x 6 (c_v, c_w per body: F = -c_v o v1, tau = -c_w o w1) or null
  const int* rec;       // T x R non-decreasing 1-based storage indices
  double* cs;           // T x 13 nb: the current CStates
  int* cursor;          // T: records written so far (R: the trajectory has ended)
  int* status;          // T: OR of the per-step statuses; 2 = a failed step ended the trajectory
  double* out;          // T x R x 13 nb recorded CStates (NaN after a failed step)
};
void launch_project(const ProjArgs& a, hipStream_t s);
void launch_vi_step(const ViArgs& a, hipStream_t s);
void launch_simulate(const SimArgs& a, hipStream_t s);
void launch_rollout_max(const RolloutMaxArgs& a, int dist_mode, hipStream_t s);
void launch_rollout_max_md(const RolloutMaxMdArgs& a, int dist_mode, hipStream_t s);
void launch_rollout(const RolloutArgs& a, int dist_mode, hipStream_t s);
void launch_rollout_min_md(const RolloutMinMdArgs& a, int dist_mode, hipStream_t s);
void launch_rollout_max_rec(const RolloutMaxRecArgs& a, int dist_mode, hipStream_t s);
void launch_rollout_max_md_rec(const RolloutMaxMdRecArgs& a, int dist_mode, hipStream_t s);
void launch_rollout_rec(const RolloutRecArgs& a, int dist_mode, hipStream_t s);
void launch_rollout_min_md_rec(const RolloutMinMdRecArgs& a, int dist_mode, hipStream_t s);

// ---- device helpers that use no device global, shared by gprx_kernels.hip and gprx_projection.hip
// (gprx_device.h holds the ones that do and belongs to gprx_kernels.hip alone) --------------------
// Squared distance along one input dimension.
//  EXPANDED: Distances.jl 0.10.5 _pairwise!(r, SqEuclidean(), a, b) on the 1-row views that
//            GaussianProcesses' StationaryARD KernelData builds: max(a^2 + b^2 - 2(ab), 0).
//            (s - 2t with t = fl(ab) equals fma(-2, t, s): 2t is exact.)
//  DIRECT  : (a - b)^2.
// Every file is compiled with -ffp-contract=off so everything else rounds exactly as written.
// sqd2: the expanded form with the squares precomputed.
__device__ __forceinline__ double sqd2(double a, double a2, double b, double b2) {
  const double v = fma(-2.0, a * b, a2 + b2);
  return v > 0.0 ? v : 0.0;
}
// r + d(a, b) w.  Expanded mode keeps the Distances.jl stack's rounding (d, then w d, then +; 6 fp64
// ops per element and dimension).  Direct mode is distij's s += (a-b)^2 w with the accumulation
// fused (3 ops): a rounding-level reordering, like the reference's own @simd sum.  (k_gram and
// k_pred_cross go one step further in direct mode: coordinates pre-scaled by 1/ell, 2 ops.)
template <int MODE>
__device__ __forceinline__ double wacc(double r, double a, double a2, double b, double b2, double w) {
  if (MODE == 0) return r + sqd2(a, a2, b, b2) * w;
  const double t = a - b;
  return __builtin_fma(t * t, w, r);
}

// The place of active dimension p among the active ones, in ascending order: its column of Xc and
// its entry of a gradient partial row.
__device__ __forceinline__ int act_rank(unsigned long long amask, int p) { return __popcll(amask & ((1ull << p) - 1ull)); }

// one lane's value on every lane (lane uniform); the sum over the wave's 64 lanes on every lane
__device__ __forceinline__ double readlane_d(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// hyper-parameters -> kernel parameters for one slot, exactly as SEArd / GPE derive them:
//   il2 = exp(-2 log ell), sf2 = exp(2 log sf), noise = exp(2 logNoise) + eps();
// a non-finite theta is an ArgumentError (status GPRX_INVALID_ARGUMENT = 2, parameters 1).
// The one derivation every evaluation uses (k_params for gprx_batch_run, k_lbfgs for the device
// optimiser), so both see the same device exp().
__device__ inline void derive_params(const DevBatch& b, int slot) {
  const int d = b.d, np = d + 2;
  const double* th = b.theta + (size_t)slot * np;
  double* P = b.params + (size_t)slot * b.pst;
  bool finite = true;
  for (int q = 0; q < np; ++q) finite = finite && isfinite(th[q]);
  for (int p = 0; p < d; ++p) P[p] = finite ? exp(-2.0 * th[1 + p]) : 1.0;
  P[d] = finite ? exp(2.0 * th[d + 1]) : 1.0;
  const double sn2 = finite ? exp(2.0 * th[0]) : 1.0;
  P[d + 1] = sn2 + DBL_EPSILON;
  P[d + 2] = sn2;
  // What the dropped (constant) dimensions add to every direct-mode distance sum, the value the
  // Gram starts its sums from: +0, unless a scaled constant c sqrt(il2 / 2) overflows or is 0 * Inf;
  // then c s - c s is NaN for every pair, as the sum over all dimensions would have it.
  double r0 = 0.0;
  for (int p = 0; p < d; ++p)
    if (!((b.amask >> p) & 1) && !isfinite(b.X[(size_t)slot * b.Npad * d + p] * sqrt(0.5 * P[p]))) r0 = NAN;
  P[d + 3] = r0;
  b.status[slot] = finite ? 0 : 2;
  b.info[slot] = 0;
}

// Device LBFGS (gprx_lbfgs.hip): one optimiser state machine per slot, advanced between two
// evaluations of the batch.  n = d + 2 parameters in GaussianProcesses order, m history pairs.
constexpr int LB_NI = 16;  // ints of state per slot
constexpr int LB_NS = 16;  // scalar doubles of state per slot
__host__ __device__ inline size_t lb_ws_doubles(int n, int m) { return (size_t)(10 + 2 * m) * n + 2 * m + LB_NS; }
// stop reasons (GPRX_STOP_* in gprx.h); result_i[3] = reason | 0x100 when converged
enum LbStop : int {
  LB_STOP_ITERATIONS = 0, LB_STOP_G_TOL = 1, LB_STOP_X_TOL = 2, LB_STOP_F_TOL = 3, LB_STOP_LINESEARCH = 4,
  LB_STOP_MAX_EVALS = 5, LB_STOP_TIME_LIMIT = 6, LB_STOP_NAN_GRADIENT = 7
};
struct LbArgs {
  double* ws;            // B x lb_ws_doubles(n, m)
  int* iws;              // B x LB_NI
  const double* theta0;  // B x n
  int* active;           // B: slot requested an evaluation / is not finished
  double* result;        // B x (n + 1): x, f(x) = -mll
  int* result_i;         // B x 4: iterations, f calls, g calls, stop | converged
  int n, m, max_evals, iterations, ls_iterations, scaleinvH0, successive_f_tol, time_up;
  double g_abstol, alphaguess, c_1, rho_hi, rho_lo;
};
constexpr int LB_LDS_MAX = 160 * 1024;
size_t lbfgs_lds_bytes(int n, int m);

// kernel launchers (gprx_kernels.hip); every launcher is asynchronous on `s`
void set_kernel_attributes();  // once per device (gprx_ctx_create), before any launch
void set_lbfgs_attributes();   // gprx_lbfgs.hip, called by set_kernel_attributes
void launch_params(const DevBatch& b, hipStream_t s);
void launch_gram(const DevBatch& b, hipStream_t s);
void launch_center(const DevBatch& b, hipStream_t s);
// flags[B][d] (ints): 1 where dimension p of a slot is not one constant over its N training points
void launch_const_flags(const DevBatch& b, int* flags, hipStream_t s);
void launch_diag(const DevBatch& b, int jt, int upd, hipStream_t s);
void launch_leaf(const DevBatch& b, int o, int n, int upd, hipStream_t s);
// a whole 8-tile node (top leaf, TRSM, SYRK + TT, bottom leaf, LINV21) in one launch (k_node8; B >= 32)
void launch_node8(const DevBatch& b, int o, int upd, hipStream_t s);
// one launch; with g2.op != OP_NONE the units of g2 are appended to g's (independent ops)
void launch_gemm(const DevBatch& b, const GemmGeom& g, hipStream_t s, const GemmGeom& g2 = GemmGeom{OP_NONE, 0, 0, 0});
// around a block [o, o + n): its right-hand side Yw before it, its rows of z after it
void launch_rhs(const DevBatch& b, int o, int n, hipStream_t s);
void launch_znode(const DevBatch& b, int o, int n, hipStream_t s);
void launch_alpha(const DevBatch& b, hipStream_t s);
void launch_lauum_grad(const DevBatch& b, hipStream_t s);
// k_lauum_grad's job table: units of 4 output tiles, folded in pairs; LU ints per unit (see
// lauum_plan in gprx_kernels.hip).  Returns the jobs per slot; *nunits the units, *nimg the
// largest image count; out (nullable) receives jobs x 2 x LU ints.
constexpr int LU = 24;
int lauum_plan(int nt, int d, int* nunits, int* nimg, int* out);
void launch_finalize(const DevBatch& b, int want_grad, hipStream_t s);
void launch_pred_cross(const DevBatch& b, hipStream_t s);
void launch_pred_final(const DevBatch& b, hipStream_t s);
// joint predictive covariance and samples (gprx_predcov.h).  VT: B x [Npad][Mpad] (K*^T's layout);
// Sig: B x [M][M] compact; F: the factor, ld = M, slot stride fs doubles; Z / smp: [S][M] per slot
// at strides zs (0 = shared) / ss; jit[B], st[B] as k_cov_chol writes them
void launch_pred_whiten(const DevBatch& b, double* VT, hipStream_t s);
void launch_pred_cov(const DevBatch& b, const double* VT, double* Sig, hipStream_t s);
void launch_cov_chol(const DevBatch& b, const double* Sig, double* F, size_t fs, double* jit, int* st, hipStream_t s);
void launch_cov_sample(const DevBatch& b, const double* F, size_t fs, const double* Z, size_t zs, double* smp, size_t ss,
                       int S, const int* st, hipStream_t s);
// leave-one-out predictions (gprx_loo.h).  kinv, mu, var, lp: B x Npad; logp: B
void launch_loo_diag(const DevBatch& b, double* kinv, hipStream_t s);
void launch_loo_final(const DevBatch& b, const double* kinv, double* mu, double* var, double* lp, double* logp, hipStream_t s);
// gradient of the leave-one-out log predictive probability (gprx_loograd.h).  bpart: B x nt x Npad;
// beta: B x Npad; gpart: B x ngu x gps; out: B x (d + 3) = [logp, grad[d + 2]]
void launch_loo_kinv(const DevBatch& b, const double* kinv, double* bpart, hipStream_t s);
void launch_loo_beta(const DevBatch& b, const double* bpart, double* beta, hipStream_t s);
void launch_loo_grad(const DevBatch& b, const double* beta, double* gpart, hipStream_t s);
void launch_loo_grad_final(const DevBatch& b, const double* gpart, const double* logp, double* out, hipStream_t s);
// k-fold cross-validation (gprx_cvfold.h).  The fold layout of a batch as gprx_batch_set_folds builds
// it on the host: one table of ints per layout (lstride = 0: one layout shared by all slots), the
// parts in this order.  "Packed order" lists the points fold after fold, each fold's points in
// ascending index (a stable sort by fold id), so a fold is a contiguous range of packed positions.
//   perm   [Npad]      the point at a packed position (-1 for the positions >= N)
//   fstart [F + 1]     packed position of a fold's first point
//   foff   [F + 1]     sum of m_g^2 over the folds g before f: the fold's m x m square in Lw
//   rowlo  [nt]        the first tile column a fold reaches from tile row ti of the packed K^-1
//   rowoff [nt + 1]    index of tile (ti, rowlo[ti]) among the slot's tiles; rowoff[nt] = their number
//   kmin   [nt]        64 floor(min perm / 64) over the tile row's points: the packed rows are 0 before it
//   jobs   [2 njmax]   (ti, tj) of tile j, rows ascending and columns ascending within a row; -1 beyond
struct CvArgs {
  const int* tab;
  size_t lstride;  // ints between the layouts of two slots, or 0
  int F, njmax;
  double* tiles;   // B x njmax x [64][64] column-major tiles of the packed K^-1 (the folds' Q blocks)
  double* r;       // B x Npad  r = Q^-1 a per fold, packed order
  double* pvar;    // B x Npad  diag(Q^-1), packed order
  double* lpf;     // B x F     log p(y_V | y_-V)
  int* fst;        // B x F     0, or 1: the fold's block is not positive definite
  double* mu;      // B x Npad  the outputs in point order
  double* var;     // B x Npad
  double* logp;    // B
  int* st;         // B         0, 1 (a fold failed), or the status of the slot's failed evaluation
};
__host__ __device__ inline size_t cv_tab_ints(int Npad, int nt, int F, int njmax) {
  return (size_t)Npad + 2 * (size_t)(F + 1) + 3 * (size_t)nt + 1 + 2 * (size_t)njmax;
}
constexpr int CVFOLD_MAX = 1024;  // GPRX_CVFOLD_MAX: one workgroup factors one fold's block
void launch_cv_pack(const DevBatch& b, const CvArgs& a, hipStream_t s);
void launch_cv_kinv(const DevBatch& b, const CvArgs& a, hipStream_t s);
void launch_cv_fold(const DevBatch& b, const CvArgs& a, hipStream_t s);
void launch_cv_final(const DevBatch& b, const CvArgs& a, hipStream_t s);
void launch_lbfgs(const LbArgs& a, const DevBatch& db, int init, hipStream_t s);  // gprx_lbfgs.hip
void launch_lbfgs_final(const LbArgs& a, const DevBatch& db, hipStream_t s);

}  // namespace gprx
