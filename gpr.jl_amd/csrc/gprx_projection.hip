// gprx_projection.hip -- maximal-coordinate rollout physics on the device (gfx950, fp64).
//
// projectv! (src/projections/implicitProjection.jl:80-107): Newton iteration on the KKT system
//     F = [I + reg  G^T; G  reg I],  f(s) = [-s_u + s_v + G^T lambda ; g(x3(s), q3(s))],
//     s <- s - F \ f(s)   until |f| < eps and |ds| < eps (or newtonIter iterations),
// with the joint constraints g and their velocity Jacobians G = dg/d(v, w) of ConstrainedDynamics
// 0.7.4 [ext, restated in oracle/projection_oracle.py]:
//     x3 = xk + v dt,  q3 = qk * wbar(w) * dt / 2,  wbar(w) = (sqrt(4/dt^2 - w.w), w)
//     translational: g = C R(qa3)^T (xb3 + R(qb3) pb - xa3) - C pa
//     rotational:    g = C Im(qa3^-1 * qb3)
// One wave (projectv) or one workgroup (the rollout) runs one trajectory's solve with F in LDS
// (n = 6 nb + nd <= 48 rows); each sub-joint's rows and Jacobian blocks are built by one lane of
// wave 0; the LU is LAPACK dgetf2's
// right-looking partial pivoting (first maximal |pivot|, reciprocal scaling, rank-1 update) and
// dgetrs' unit-lower / upper substitutions, as Julia's F \ f.
//
// predictdynamics (examples/utils/predictdynamics.jl:7-22) for many trajectories: one 256-thread
// workgroup per trajectory runs every step on the device -- the G GPs' mean predictions at the
// current CState (the training points split over the workgroup), getvw, the projection (its LU
// update over the whole workgroup), the projection error and updatestate!.
//
// predictdynamicsmin (:30-102), the rollout in minimal coordinates (k_rollout), is here too: with
// MeanDynamics GPs each of its steps runs the variational-integrator solve below.
#include "gprx_internal.h"
#include <type_traits>

namespace gprx {

namespace {

struct Qd {
  double w, x, y, z;
};
__device__ __forceinline__ Qd qmul(const Qd& p, const Qd& q) {
  return Qd{p.w * q.w - (p.x * q.x + p.y * q.y + p.z * q.z), p.w * q.x + q.w * p.x + (p.y * q.z - p.z * q.y),
            p.w * q.y + q.w * p.y + (p.z * q.x - p.x * q.z), p.w * q.z + q.w * p.z + (p.x * q.y - p.y * q.x)};
}
__device__ __forceinline__ Qd qconj(const Qd& q) { return Qd{q.w, -q.x, -q.y, -q.z}; }
// R(q) p = (q0^2 - |qv|^2) p + 2 qv (qv.p) + 2 q0 qv x p
__device__ __forceinline__ void rot(const Qd& q, const double* p, double* o) {
  const double c = q.w * q.w - (q.x * q.x + q.y * q.y + q.z * q.z);
  const double d = q.x * p[0] + q.y * p[1] + q.z * p[2];
  const double cx = q.y * p[2] - q.z * p[1], cy = q.z * p[0] - q.x * p[2], cz = q.x * p[1] - q.y * p[0];
  o[0] = c * p[0] + 2.0 * q.x * d + 2.0 * q.w * cx;
  o[1] = c * p[1] + 2.0 * q.y * d + 2.0 * q.w * cy;
  o[2] = c * p[2] + 2.0 * q.z * d + 2.0 * q.w * cz;
}
// d (R(q) p) / dq, 3 x 4 (columns w, x, y, z)
__device__ __forceinline__ void drot(const Qd& q, const double* p, double (&J)[3][4]) {
  const double qv[3] = {q.x, q.y, q.z};
  const double cx = q.y * p[2] - q.z * p[1], cy = q.z * p[0] - q.x * p[2], cz = q.x * p[1] - q.y * p[0];
  const double cr[3] = {cx, cy, cz};
  const double d = q.x * p[0] + q.y * p[1] + q.z * p[2];
  // -2 q0 [p]x
  const double sk[3][3] = {{0.0, -p[2], p[1]}, {p[2], 0.0, -p[0]}, {-p[1], p[0], 0.0}};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    J[i][0] = 2.0 * q.w * p[i] + 2.0 * cr[i];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      J[i][1 + j] = -2.0 * p[i] * qv[j] + (i == j ? 2.0 * d : 0.0) + 2.0 * qv[i] * p[j] - 2.0 * q.w * sk[i][j];
  }
}
// Lmat(p): p * q = Lmat(p) q ; Rmat(q): p * q = Rmat(q) p
__device__ __forceinline__ void lmat(const Qd& p, double (&M)[4][4]) {
  M[0][0] = p.w; M[0][1] = -p.x; M[0][2] = -p.y; M[0][3] = -p.z;
  M[1][0] = p.x; M[1][1] = p.w;  M[1][2] = -p.z; M[1][3] = p.y;
  M[2][0] = p.y; M[2][1] = p.z;  M[2][2] = p.w;  M[2][3] = -p.x;
  M[3][0] = p.z; M[3][1] = -p.y; M[3][2] = p.x;  M[3][3] = p.w;
}
__device__ __forceinline__ void rmat(const Qd& q, double (&M)[4][4]) {
  M[0][0] = q.w; M[0][1] = -q.x; M[0][2] = -q.y; M[0][3] = -q.z;
  M[1][0] = q.x; M[1][1] = q.w;  M[1][2] = q.z;  M[1][3] = -q.y;
  M[2][0] = q.y; M[2][1] = -q.z; M[2][2] = q.w;  M[2][3] = q.x;
  M[3][0] = q.z; M[3][1] = q.y;  M[3][2] = -q.x; M[3][3] = q.w;
}
// getq3: ((qk * wbar(w)) * dt) / 2
__device__ __forceinline__ Qd wbar_step(const Qd& qk, const double* w, double dt) {
  const Qd wb{sqrt(4.0 / (dt * dt) - (w[0] * w[0] + w[1] * w[1] + w[2] * w[2])), w[0], w[1], w[2]};
  const Qd r = qmul(qk, wb);
  return Qd{r.w * dt / 2.0, r.x * dt / 2.0, r.y * dt / 2.0, r.z * dt / 2.0};
}
// d q3 / d w (4 x 3) = Lmat(qk) [-w^T / s ; I] dt / 2
__device__ __forceinline__ void dq3(const Qd& qk, const double* w, double dt, double (&D)[4][3]) {
  const double s = sqrt(4.0 / (dt * dt) - (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]));
  double L[4][4];
  lmat(qk, L);
  double Wp[4][3] = {{-w[0] / s, -w[1] / s, -w[2] / s}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) t += L[i][k] * Wp[k][j];
      D[i][j] = t * (dt / 2.0);
    }
}

// Per-trajectory mechanism state and the KKT workspace in LDS.
struct PState {
  double xk[PJ_MAXB][3], qk[PJ_MAXB][4];  // discrete pose (x2, q2)
  double xc[PJ_MAXB][3], qc[PJ_MAXB][4], vc[PJ_MAXB][3], wc[PJ_MAXB][3];
  double s[PJ_MAXN], su[6 * PJ_MAXB], f[PJ_MAXN], ds[PJ_MAXN];
  int status, it;
};
// The Newton matrix F and the LU's working copy A live in dynamic LDS sized for the mechanism
// (2 n (n + 1) doubles, n = 6 nb + nd; row i at i (n + 1)), so a small mechanism's workgroups are
// not limited to the largest one's LDS footprint.
__device__ __forceinline__ double* pj_lds() {
  extern __shared__ __attribute__((aligned(16))) double pj_dyn[];
  return pj_dyn;
}
#define PJ_F (pj_lds())
#define PJ_A (pj_lds() + (size_t)(ldf - 1) * ldf)
__host__ __device__ inline size_t pj_lds_bytes(int nb, int nd) {
  const size_t n = 6 * (size_t)nb + nd;
  return 2 * n * (n + 1) * sizeof(double);
}
// the variational-integrator step's dynamic LDS: its Newton matrix (n x (n + 1)) and Gpos (nd x 6 nb)
__host__ __device__ inline size_t vi_lds_doubles(int nb, int nd) {
  const size_t n = 6 * (size_t)nb + nd;
  return n * (n + 1) + (size_t)nd * 6 * nb;
}
__device__ __forceinline__ Qd ldq(const double* q) { return Qd{q[0], q[1], q[2], q[3]}; }

// x3, q3 of body b (1-based; 0 = origin) at the current solution s
__device__ __forceinline__ void pose3(const PState& P, int b, double dt, double* x, Qd& q) {
  if (b == 0) {
    x[0] = x[1] = x[2] = 0.0;
    q = Qd{1.0, 0.0, 0.0, 0.0};
    return;
  }
  const double* v = P.s + 6 * (b - 1);
  const double* w = v + 3;
  for (int k = 0; k < 3; ++k) x[k] = P.xk[b - 1][k] + v[k] * dt;
  q = wbar_step(ldq(P.qk[b - 1]), w, dt);
}

// One sub-joint's constraint rows (into f[n6 + row0 ..] when want_g) and, when want_jac, its
// Jacobian blocks into F (G rows and the transposed G^T columns).  Called by one lane.
__device__ void subjoint(PState& P, const SubJoint& J, int n6, int ldf, double dt, bool want_g, bool want_jac,
                         bool sym = true) {
  double xa[3], xb[3];
  Qd qa, qb;
  pose3(P, J.a, dt, xa, qa);
  pose3(P, J.b, dt, xb, qb);
  const Qd qac = qconj(qa);
  const int R = J.rows;
  double gm[3];  // the 3-vector before C
  double Gv_b[3][3], Gw_b[3][3], Gv_a[3][3], Gw_a[3][3];
  const double* wb = P.s + 6 * (J.b - 1) + 3;
  double Db[4][3];
  dq3(ldq(P.qk[J.b - 1]), wb, dt, Db);
  double Da[4][3];
  if (J.a > 0) dq3(ldq(P.qk[J.a - 1]), P.s + 6 * (J.a - 1) + 3, dt, Da);
  if (J.kind == 0) {  // translational
    double rpb[3], y[3], e[3];
    rot(qb, J.pb, rpb);
    for (int k = 0; k < 3; ++k) y[k] = xb[k] + rpb[k] - xa[k];
    rot(qac, y, e);
    for (int k = 0; k < 3; ++k) gm[k] = e[k] - J.pa[k];
    if (want_jac) {
      double RaT[3][3];  // R(qa)^T: column j = R(qa^-1) e_j
      for (int j = 0; j < 3; ++j) {
        const double ej[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
        double c[3];
        rot(qac, ej, c);
        for (int i = 0; i < 3; ++i) RaT[i][j] = c[i];
      }
      double Jb[3][4];
      drot(qb, J.pb, Jb);
      double M[3][3];  // RaT drot(qb, pb) Db
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double t = 0.0;
          for (int k = 0; k < 3; ++k) {
            double u = 0.0;
            for (int m = 0; m < 4; ++m) u += Jb[k][m] * Db[m][j];
            t += RaT[i][k] * u;
          }
          M[i][j] = t;
        }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          Gv_b[i][j] = RaT[i][j] * dt;
          Gw_b[i][j] = M[i][j];
          Gv_a[i][j] = -RaT[i][j] * dt;
        }
      if (J.a > 0) {
        double Ja[3][4];
        drot(qac, y, Ja);
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            double t = 0.0;
            for (int m = 0; m < 4; ++m) t += Ja[i][m] * (m == 0 ? 1.0 : -1.0) * Da[m][j];
            Gw_a[i][j] = t;
          }
      }
    }
  } else {  // rotational
    const Qd r = qmul(qac, qb);
    gm[0] = r.x;
    gm[1] = r.y;
    gm[2] = r.z;
    if (want_jac) {
      double L[4][4];
      lmat(qac, L);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double t = 0.0;
          for (int m = 0; m < 4; ++m) t += L[1 + i][m] * Db[m][j];
          Gw_b[i][j] = t;
          Gv_b[i][j] = 0.0;
          Gv_a[i][j] = 0.0;
        }
      if (J.a > 0) {
        double Rq[4][4];
        rmat(qb, Rq);
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            double t = 0.0;
            for (int m = 0; m < 4; ++m) t += Rq[1 + i][m] * (m == 0 ? 1.0 : -1.0) * Da[m][j];
            Gw_a[i][j] = t;
          }
      }
    }
  }
  for (int r = 0; r < R; ++r) {
    const int row = n6 + J.row0 + r;
    if (want_g) {
      double t = 0.0;
      for (int k = 0; k < 3; ++k) t += J.C[r][k] * gm[k];
      P.f[row] = t;
    }
    if (want_jac) {
      for (int side = 0; side < 2; ++side) {
        const int body = side ? J.a : J.b;
        if (body == 0) continue;
        const int c0 = 6 * (body - 1);
        for (int j = 0; j < 3; ++j) {
          double tv = 0.0, tw = 0.0;
          for (int k = 0; k < 3; ++k) {
            tv += J.C[r][k] * (side ? Gv_a[k][j] : Gv_b[k][j]);
            tw += J.C[r][k] * (side ? Gw_a[k][j] : Gw_b[k][j]);
          }
          PJ_F[row * ldf + c0 + j] = tv;
          PJ_F[row * ldf + c0 + 3 + j] = tw;
          if (sym) {
            PJ_F[(c0 + j) * ldf + row] = tv;
            PJ_F[(c0 + 3 + j) * ldf + row] = tw;
          }
        }
      }
    }
  }
}

// f(s) upper part: -su + s_v + G^T lambda (G read from F's lower-left block), lanes over columns
__device__ __forceinline__ void residual_upper(PState& P, int n6, int nd, int ldf, int l) {
  if (l < n6) {
    double t = 0.0;
    for (int r = 0; r < nd; ++r) t += PJ_F[(n6 + r) * ldf + l] * P.s[n6 + r];
    P.f[l] = (-P.su[l] + P.s[l]) + t;
  }
}

template <int NW>
__device__ __forceinline__ void pj_sync() {
  if constexpr (NW == 1) {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// A x = b by LAPACK dgetf2's right-looking LU with partial pivoting (first maximal |pivot|,
// reciprocal scaling, rank-1 update spread over the NW waves, one element per thread) and dgetrs'
// unit-lower / upper substitutions, as Julia's F \ f.  A (n x n, row stride ldf) in LDS is
// overwritten; b: lane l < n holds b_l on entry and x_l on exit (the same on every wave).  Returns
// true for an exactly singular pivot (b is then undefined).  All NW * 64 threads call.
template <int NW>
__device__ bool lu_solve(double* A, int n, int ldf, double& b) {
  constexpr int NT = 64 * NW;
  const int tid = threadIdx.x & (NT - 1), l = tid & 63;
  const bool w0 = tid < 64;
  bool singular = false;
  for (int k = 0; k < n; ++k) {
    // pivot: first row of maximal |a_ik|, i >= k (idamax)
    double v = (l >= k && l < n) ? fabs(A[l * ldf + k]) : -1.0;
    int idx = l;
    for (int o = 1; o < 64; o <<= 1) {
      const double v2 = __shfl_xor(v, o);
      const int i2 = __shfl_xor(idx, o);
      if (v2 > v || (v2 == v && i2 < idx)) {
        v = v2;
        idx = i2;
      }
    }
    const int p = idx;
    if (p != k) {  // swap rows k and p of A and of the right-hand side
      if (NW > 1) pj_sync<NW>();  // every wave has read column k
      for (int j = tid; j < n; j += NT) {
        const double t = A[k * ldf + j];
        A[k * ldf + j] = A[p * ldf + j];
        A[p * ldf + j] = t;
      }
      const double bk = readlane_d(b, k), bp = readlane_d(b, p);
      if (l == k) b = bp;
      if (l == p) b = bk;
    }
    pj_sync<NW>();
    const double akk = A[k * ldf + k];
    if (akk == 0.0) singular = true;
    const int m = n - 1 - k;
    if (akk != 0.0 && m > 0) {
      if (w0 && l > k && l < n)
        A[l * ldf + k] = fabs(akk) >= DBL_MIN ? A[l * ldf + k] * (1.0 / akk) : A[l * ldf + k] / akk;
      pj_sync<NW>();
      // trailing update A[i][j] -= l_i A[k][j], i, j in (k, n): element e = (i - k - 1) m + (j - k - 1)
      const int si = NT / m, sj = NT - si * m;
      int i = tid / m, j = tid - i * m;
      for (int e = tid; e < m * m; e += NT) {
        const int gi = k + 1 + i, gj = k + 1 + j;
        A[gi * ldf + gj] = A[gi * ldf + gj] - A[gi * ldf + k] * A[k * ldf + gj];
        i += si;
        j += sj;
        if (j >= m) {
          j -= m;
          ++i;
        }
      }
    }
    pj_sync<NW>();
  }
  if (singular) return true;
  // forward substitution (unit lower), then backward (upper), as dgetrs / dtrsm
  for (int k = 0; k < n; ++k) {
    const double bk = readlane_d(b, k);
    if (bk != 0.0 && l > k && l < n) b = b - bk * A[l * ldf + k];
  }
  for (int k = n - 1; k >= 0; --k) {
    const double ukk = A[k * ldf + k];
    double bk = readlane_d(b, k);
    if (bk != 0.0) {
      bk = bk / ukk;
      if (l == k) b = bk;
      if (l < k) b = b - bk * A[l * ldf + k];
    }
  }
  return false;
}

// projectv! on NW waves (all NW * 64 threads call).  P.s holds the predicted (v, w) per body on
// entry (lambda = 0 appended); leaves the projected (v, w) in P.s[0 .. 6nb).  P.xk / P.qk set.
// Wave 0 builds the constraints, Jacobians and residuals (one lane per sub-joint / row); the LU's
// trailing update is spread over every thread, one element each; pivot search, the right-hand
// side and the substitutions run redundantly on every wave (the same values), so no broadcast is
// needed.  Each element sees the same operations in the same order for any NW.
template <int NW>
__device__ void project(PState& P, const MechDev& M, double dt, double reg, double eps, int iters) {
  constexpr int NT = 64 * NW;
  const int tid = threadIdx.x & (NT - 1), l = tid & 63;
  const bool w0 = tid < 64;
  const int nb = M.nb, nd = M.nd, n6 = 6 * nb, n = n6 + nd, ldf = n + 1;
  for (int i = tid; i < n * ldf; i += NT) PJ_F[i] = 0.0;
  pj_sync<NW>();
  if (w0) {
    if (l < n6) P.su[l] = P.s[l];
    if (l >= n6 && l < n) P.s[l] = 0.0;
  }
  pj_sync<NW>();
  if (w0 && l < M.nsub) subjoint(P, M.sub[l], n6, ldf, dt, false, true);  // updateF!
  pj_sync<NW>();
  if (w0 && l < n) PJ_F[l * ldf + l] = (l < n6 ? 1.0 : 0.0) + reg;        // F += I * regularizer
  if (tid == 0) {
    P.status = 0;
    P.it = 0;
  }
  pj_sync<NW>();
  for (int it = 1; it <= iters; ++it) {
    if (w0 && l < M.nsub) subjoint(P, M.sub[l], n6, ldf, dt, true, true);  // updateF! + g(mechanism)
    pj_sync<NW>();
    if (w0) residual_upper(P, n6, nd, ldf, l);
    pj_sync<NW>();
    // ---- ds = F \ f: LU with partial pivoting of a working copy A (F keeps the Newton matrix;
    // its G blocks are rebuilt by the next updateF!)
    for (int i = tid; i < n * ldf; i += NT) PJ_A[i] = PJ_F[i];
    double b = l < n ? P.f[l] : 0.0;
    pj_sync<NW>();
    if (lu_solve<NW>(PJ_A, n, ldf, b)) {  // Julia's F \ f throws SingularException: the trajectory stops
      if (tid == 0) P.status = 1;
      pj_sync<NW>();
      return;
    }
    // s -= ds, updateMechanism!
    if (w0 && l < n) {
      P.ds[l] = b;
      P.s[l] = P.s[l] - b;
    }
    pj_sync<NW>();
    // convergence: |f(s_new)| (with the iteration's G) and |ds|
    if (w0 && l < M.nsub) subjoint(P, M.sub[l], n6, ldf, dt, true, false);
    pj_sync<NW>();
    if (w0) residual_upper(P, n6, nd, ldf, l);
    pj_sync<NW>();
    const double fv = l < n ? P.f[l] : 0.0, dv = l < n ? P.ds[l] : 0.0;
    const double nf = sqrt(wave_sum(fv * fv)), nds = sqrt(wave_sum(dv * dv));
    if (tid == 0) P.it = it;
    pj_sync<NW>();
    if (nf < eps && nds < eps) break;
  }
}

// setstates! (+ discretizestate!, setsolution!) from a CState
__device__ void set_states(PState& P, const double* cs, int nb, double dt, int l) {
  if (l < nb) {
    const double* c = cs + 13 * l;
    for (int k = 0; k < 3; ++k) {
      P.xc[l][k] = c[k];
      P.vc[l][k] = c[7 + k];
      P.wc[l][k] = c[10 + k];
      P.xk[l][k] = c[k] + c[7 + k] * dt;
    }
    for (int k = 0; k < 4; ++k) P.qc[l][k] = c[3 + k];
    const Qd q = wbar_step(ldq(P.qc[l]), P.wc[l], dt);
    P.qk[l][0] = q.w;
    P.qk[l][1] = q.x;
    P.qk[l][2] = q.y;
    P.qk[l][3] = q.z;
  }
}
// updatestate! with the solution (v, w) in P.s
__device__ void update_state(PState& P, int nb, double dt, int l) {
  if (l < nb) {
    const double* v = P.s + 6 * l;
    const double* w = v + 3;
    for (int k = 0; k < 3; ++k) {
      P.xc[l][k] = P.xk[l][k];
      P.vc[l][k] = v[k];
      P.wc[l][k] = w[k];
      P.xk[l][k] = P.xk[l][k] + v[k] * dt;
    }
    for (int k = 0; k < 4; ++k) P.qc[l][k] = P.qk[l][k];
    const Qd q = wbar_step(ldq(P.qk[l]), w, dt);
    P.qk[l][0] = q.w;
    P.qk[l][1] = q.x;
    P.qk[l][2] = q.y;
    P.qk[l][3] = q.z;
  }
}
__device__ __forceinline__ double cstate_at(const PState& P, int i) {
  const int b = i / 13, k = i - 13 * b;
  if (k < 3) return P.xc[b][k];
  if (k < 7) return P.qc[b][k - 3];
  if (k < 10) return P.vc[b][k - 7];
  return P.wc[b][k - 10];
}

// ---- one variational-integrator step: ConstrainedDynamics 0.7.4 newton! (restated in gprx/vi.py,
// which documents the equations): per body, with the current state (x1, q1, v1, w1) and the discrete
// pose x2 = x1 + v1 dt, q2 = q1 wbar(w1) dt/2, Newton on s = (v2, w2 per body, lambda) for
//     m ((v2 - v1)/dt + g e_z) - Gpos_x^T lambda = 0
//     sq2 J w2 + w2 x J w2 - (sq1 J w1 - w1 x J w1) - Gpos_phi^T lambda = 0,  sq = sqrt(4/dt^2 - w.w)
//     g(x3, q3) = 0,  x3 = x2 + v2 dt,  q3 = q2 wbar(w2) dt/2
// Gpos = dg/d(x, phi) at pose 2 (phi: q -> q (1, phi)), fixed during the solve; the constraint rows'
// velocity Jacobian is the projection's (subjoint).  One wave per state; the Newton matrix is
// rebuilt in LDS every iteration and factored in place (lu_solve).
// R(q) as gprx/vi.py rotmat (unit quaternions)
__device__ __forceinline__ void rotm(const Qd& q, double (&R)[3][3]) {
  const double w = q.w, x = q.x, y = q.y, z = q.z;
  R[0][0] = w * w + x * x - y * y - z * z;
  R[0][1] = 2.0 * (x * y - w * z);
  R[0][2] = 2.0 * (x * z + w * y);
  R[1][0] = 2.0 * (x * y + w * z);
  R[1][1] = w * w - x * x + y * y - z * z;
  R[1][2] = 2.0 * (y * z - w * x);
  R[2][0] = 2.0 * (x * z - w * y);
  R[2][1] = 2.0 * (y * z + w * x);
  R[2][2] = w * w - x * x - y * y + z * z;
}
__device__ __forceinline__ void pose2(const PState& P, int b, double* x, Qd& q) {
  if (b == 0) {
    x[0] = x[1] = x[2] = 0.0;
    q = Qd{1.0, 0.0, 0.0, 0.0};
    return;
  }
  for (int k = 0; k < 3; ++k) x[k] = P.xk[b - 1][k];
  q = ldq(P.qk[b - 1]);
}
// one sub-joint's rows of Gpos = dg/d(x_1, phi_1, ..., x_nb, phi_nb) at pose 2 (gprx/vi.py jac_phi)
// into G (row-major, nd x n6); called by one lane
__device__ void subjoint_pose_jac(const PState& P, const SubJoint& J, int n6, double* G) {
  double xa[3], xb[3];
  Qd qa, qb;
  pose2(P, J.a, xa, qa);
  pose2(P, J.b, xb, qb);
  double Bx_b[3][3], Bp_b[3][3], Bx_a[3][3], Bp_a[3][3];  // the 3 x 3 blocks before C
  if (J.kind == 0) {  // translational: g = C (R(qa)^T (xb + R(qb) pb - xa) - pa)
    double Ra[3][3], Rb[3][3];
    rotm(qa, Ra);
    rotm(qb, Rb);
    double y[3], u[3];
    for (int i = 0; i < 3; ++i) y[i] = xb[i] + (Rb[i][0] * J.pb[0] + Rb[i][1] * J.pb[1] + Rb[i][2] * J.pb[2]) - xa[i];
    for (int i = 0; i < 3; ++i) u[i] = Ra[0][i] * y[0] + Ra[1][i] * y[1] + Ra[2][i] * y[2];
    const double spb[3][3] = {{0.0, -J.pb[2], J.pb[1]}, {J.pb[2], 0.0, -J.pb[0]}, {-J.pb[1], J.pb[0], 0.0}};
    const double su[3][3] = {{0.0, -u[2], u[1]}, {u[2], 0.0, -u[0]}, {-u[1], u[0], 0.0}};
    double RbS[3][3];  // R(qb) (-2 [pb]x)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) RbS[i][j] = -2.0 * (Rb[i][0] * spb[0][j] + Rb[i][1] * spb[1][j] + Rb[i][2] * spb[2][j]);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        Bx_b[i][j] = Ra[j][i];
        Bp_b[i][j] = Ra[0][i] * RbS[0][j] + Ra[1][i] * RbS[1][j] + Ra[2][i] * RbS[2][j];
        Bx_a[i][j] = -Ra[j][i];
        Bp_a[i][j] = 2.0 * su[i][j];
      }
  } else {  // rotational: g = C Im(qa^-1 qb); d/dphi_b = Lmat(rq)[1:,1:], d/dphi_a = -Rmat(rq)[1:,1:]
    const Qd r = qmul(qconj(qa), qb);
    const double rv[3] = {r.x, r.y, r.z};
    const double sr[3][3] = {{0.0, -rv[2], rv[1]}, {rv[2], 0.0, -rv[0]}, {-rv[1], rv[0], 0.0}};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        Bx_b[i][j] = 0.0;
        Bx_a[i][j] = 0.0;
        Bp_b[i][j] = (i == j ? r.w : 0.0) + sr[i][j];
        Bp_a[i][j] = -((i == j ? r.w : 0.0) - sr[i][j]);
      }
  }
  for (int rr = 0; rr < J.rows; ++rr) {
    double* g = G + (size_t)(J.row0 + rr) * n6;
    for (int side = 0; side < 2; ++side) {
      const int body = side ? J.a : J.b;
      if (body == 0) continue;
      const int c0 = 6 * (body - 1);
      for (int j = 0; j < 3; ++j) {
        double tx = 0.0, tp = 0.0;
        for (int k = 0; k < 3; ++k) {
          tx += J.C[rr][k] * (side ? Bx_a[k][j] : Bx_b[k][j]);
          tp += J.C[rr][k] * (side ? Bp_a[k][j] : Bp_b[k][j]);
        }
        g[c0 + j] = tx;
        g[c0 + 3 + j] = tp;
      }
    }
  }
}
// Where the step reads its bodies.  MechBodies: the launch-wide mechanism's nominal masses and
// inertias and no external force (k_vi_step, the MeanDynamics rollouts).  TrajBodies: one
// trajectory's own, in LDS, and the external force of the current step, ext[6 b + c] = F_c (world
// frame, c < 3) or 2 tau_(c-3) (body frame) (k_simulate).
struct MechBodies {
  const MechDev& M;
  static constexpr bool forced = false, stall_stop = false;
  __device__ __forceinline__ double m(int b) const { return M.m[b]; }
  __device__ __forceinline__ double J(int b, int i, int k) const { return M.J[b][i][k]; }
  __device__ __forceinline__ double ext(int) const { return 0.0; }
};
struct TrajBodies {
  const double* mm;            // nb
  const double (*JJ)[3][3];    // nb
  const double* fx;            // 6 nb
  static constexpr bool forced = true, stall_stop = true;
  __device__ __forceinline__ double m(int b) const { return mm[b]; }
  __device__ __forceinline__ double J(int b, int i, int k) const { return JJ[b][i][k]; }
  __device__ __forceinline__ double ext(int j) const { return fx[j]; }
};
// the dynamics rows of the residual, lane j < n6: body b = j / 6
template <class Bodies>
__device__ __forceinline__ double vi_dyn_row(const PState& P, const Bodies& B, const double (*mom1)[3], const double* G,
                                             int n6, int nd, double dt, double grav, int j) {
  const int b = j / 6, c = j - 6 * b;
  const double* v2 = P.s + 6 * b;
  const double* w2 = v2 + 3;
  double d;
  if (c < 3) {
    d = B.m(b) * ((v2[c] - P.vc[b][c]) / dt + (c == 2 ? grav : 0.0));
  } else {
    const int k = c - 3;
    double Jw[3];
    for (int i = 0; i < 3; ++i) Jw[i] = B.J(b, i, 0) * w2[0] + B.J(b, i, 1) * w2[1] + B.J(b, i, 2) * w2[2];
    const double sq2 = sqrt(4.0 / (dt * dt) - (w2[0] * w2[0] + w2[1] * w2[1] + w2[2] * w2[2]));
    const double cr = k == 0 ? w2[1] * Jw[2] - w2[2] * Jw[1] : (k == 1 ? w2[2] * Jw[0] - w2[0] * Jw[2] : w2[0] * Jw[1] - w2[1] * Jw[0]);
    d = (sq2 * Jw[k] + cr) - mom1[b][k];
  }
  if constexpr (Bodies::forced) d = d - B.ext(j);  // - F, - 2 tau
  double t = 0.0;
  for (int r = 0; r < nd; ++r) t += G[(size_t)r * n6 + j] * P.s[n6 + r];
  return d - t;
}
// [v]x (i, j) and v[i] by selects: a register array indexed by a lane-dependent value would live in
// scratch memory
__device__ __forceinline__ double sel3(const double* v, int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : v[2]); }
__device__ __forceinline__ double skew_at(const double* v, int i, int j) {
  if (i == j) return 0.0;
  const double x = sel3(v, 3 - i - j);
  return (j - i == 1 || j - i == -2) ? -x : x;
}

// The Newton solve of one variational-integrator step on NW waves (all NW * 64 threads call; P.xc /
// qc / vc / wc and the discrete pose P.xk / qk set by set_states).  Leaves the solution (v2, w2 per
// body, lambda) in P.s and returns the status: 0 converged, 1 not converged within iters, 2 failed
// (a non-finite or singular system; P.s is then undefined); it: the iterations taken.  The Newton
// matrix A (n x (n + 1)) and Gpos (nd x n6) live in dynamic LDS, pj_lds() onwards.
// The whole workgroup runs it, as project<NW>: wave 0 builds the rows (one lane per sub-joint /
// inertia entry / residual row), the zeroing, the -Gpos^T block and lu_solve's trailing update are
// spread over every thread, and the finiteness test, the right-hand side, the substitutions and
// the norms run redundantly on every wave from the same LDS values, so every wave takes the same
// branch without a broadcast.  Each element sees the same operations in the same order for any
// NW (k_vi_step's NW = 1 included).  Ends with a barrier: the caller may reuse the dynamic LDS.
// B: the bodies' masses and inertias and the external force (MechBodies / TrajBodies above), constant
// during the solve, so the Newton matrix has no term of it; TrajBodies also ends a stagnated solve.
template <int NW, class Bodies>
__device__ int vi_newton(PState& P, double (*mom1)[3], const MechDev& M, const Bodies& B, double dt, double reg, double eps,
                         double grav, int iters, int& it) {
  constexpr int NT = 64 * NW;
  const int tid = threadIdx.x & (NT - 1), l = tid & 63;
  const bool w0 = tid < 64;
  const int nb = M.nb, nd = M.nd, n6 = 6 * nb, n = n6 + nd, ldf = n + 1;
  double* A = PJ_F;                         // the Newton matrix, rebuilt and factored each iteration
  double* G = PJ_F + (size_t)n * ldf;       // Gpos (nd x n6), fixed
  if (w0 && l < nb) {  // (sq1 I - [w1 x]) J w1; setsolution!: (v2, w2) start at the current velocities
    const double* w1 = P.wc[l];
    double Jw[3];
    for (int i = 0; i < 3; ++i) Jw[i] = B.J(l, i, 0) * w1[0] + B.J(l, i, 1) * w1[1] + B.J(l, i, 2) * w1[2];
    const double sq1 = sqrt(4.0 / (dt * dt) - (w1[0] * w1[0] + w1[1] * w1[1] + w1[2] * w1[2]));
    const double cr[3] = {w1[1] * Jw[2] - w1[2] * Jw[1], w1[2] * Jw[0] - w1[0] * Jw[2], w1[0] * Jw[1] - w1[1] * Jw[0]};
    for (int i = 0; i < 3; ++i) {
      mom1[l][i] = sq1 * Jw[i] - cr[i];
      P.s[6 * l + i] = P.vc[l][i];
      P.s[6 * l + 3 + i] = w1[i];
    }
  }
  if (w0 && l >= n6 && l < n) P.s[l] = 0.0;
  for (int i = tid; i < nd * n6; i += NT) G[i] = 0.0;
  pj_sync<NW>();
  if (w0 && l < M.nsub) subjoint_pose_jac(P, M.sub[l], n6, G);
  pj_sync<NW>();
  int status = 1;
  it = 0;
  [[maybe_unused]] double nds_prev = INFINITY;
  for (int k = 1; k <= iters; ++k) {
    // ---- the Newton matrix and the residual at the current solution
    for (int i = tid; i < n * ldf; i += NT) A[i] = 0.0;
    pj_sync<NW>();
    if (w0) {
      if (l < M.nsub) {
        subjoint(P, M.sub[l], n6, ldf, dt, true, true, false);  // g(x3, q3) and dg/d(v2, w2)
      } else if (l < M.nsub + 9 * nb) {  // d/dw2 [(sq2 I + [w2 x]) J w2] (gprx/vi.py)
        const int e = l - M.nsub, b = e / 9, i = (e - 9 * b) / 3, kk = e - 9 * b - 3 * i;
        const double* w2 = P.s + 6 * b + 3;
        double Jw[3];
        for (int q = 0; q < 3; ++q) Jw[q] = B.J(b, q, 0) * w2[0] + B.J(b, q, 1) * w2[1] + B.J(b, q, 2) * w2[2];
        const double sq2 = sqrt(4.0 / (dt * dt) - (w2[0] * w2[0] + w2[1] * w2[1] + w2[2] * w2[2]));
        const double swJ = skew_at(w2, i, 0) * B.J(b, 0, kk) + skew_at(w2, i, 1) * B.J(b, 1, kk) + skew_at(w2, i, 2) * B.J(b, 2, kk);
        A[(6 * b + 3 + i) * ldf + 6 * b + 3 + kk] = ((sq2 * B.J(b, i, kk) + swJ) - skew_at(Jw, i, kk)) - sel3(Jw, i) * w2[kk] / sq2;
      } else if (l < M.nsub + 12 * nb) {
        const int e = l - M.nsub - 9 * nb, b = e / 3, c = e - 3 * b;
        A[(6 * b + c) * ldf + 6 * b + c] = B.m(b) / dt;
      }
    }
    for (int e = tid; e < n6 * nd; e += NT) {  // -Gpos^T (upper right), -reg I (lower right)
      const int j = e / nd, r = e - j * nd;
      A[j * ldf + n6 + r] = -G[(size_t)r * n6 + j];
    }
    if (w0 && l < nd && reg != 0.0) A[(n6 + l) * ldf + n6 + l] = -reg;
    pj_sync<NW>();
    if (w0 && l < n6) P.f[l] = vi_dyn_row(P, B, mom1, G, n6, nd, dt, grav, l);
    pj_sync<NW>();
    // a system that is not finite (|w| beyond 2/dt: the reference's sqrt throws a DomainError) or is
    // singular (SingularException) fails the state.  Every wave scans the whole matrix.
    bool fin = l < n ? isfinite(P.f[l]) : true;
    for (int i = l; i < n * ldf; i += 64) fin = fin && isfinite(A[i]);
    if (__any(!fin)) {
      status = 2;
      break;
    }
    double bvec = l < n ? P.f[l] : 0.0;
    if (lu_solve<NW>(A, n, ldf, bvec) || __any(l < n && !isfinite(bvec))) {
      status = 2;
      break;
    }
    if (w0 && l < n) {
      P.ds[l] = bvec;
      P.s[l] = P.s[l] - bvec;
    }
    it = k;
    pj_sync<NW>();
    // ---- convergence: |f(s_new)| and |ds|
    if (w0 && l < M.nsub) subjoint(P, M.sub[l], n6, ldf, dt, true, false, false);
    pj_sync<NW>();
    if (w0 && l < n6) P.f[l] = vi_dyn_row(P, B, mom1, G, n6, nd, dt, grav, l);
    pj_sync<NW>();
    const double fv = l < n ? P.f[l] : 0.0, dv = l < n ? P.ds[l] : 0.0;
    const double nf = sqrt(wave_sum(fv * fv)), nds = sqrt(wave_sum(dv * dv));
    if (nf < eps && nds < eps) {
      status = 0;
      break;
    }
    if constexpr (Bodies::stall_stop) {
      // Stagnation at the rounding floor: the residual and the twist's step are below eps and |ds|, which
      // the multipliers' step dominates, no longer falls.  At a small dt the multipliers' floor,
      // (m / dt) (1e-16 / dt), lies above eps and newton!'s test can never hold; further iterations only
      // move the last bits.  The step ends with status 1 (newton!'s test not met) and is used as it is.
      const double tv = l < n6 ? P.ds[l] : 0.0;
      const double ntw = sqrt(wave_sum(tv * tv));
      if (nf < eps && ntw < eps && nds >= nds_prev) break;
      nds_prev = nds;
    }
  }
  pj_sync<NW>();
  return status;
}

}  // namespace

// ---- projectv! for T independent mechanism states: one wave each ------------------------------
// Contract (include/gprx.h, gprx_projectv): status 1 and a NaN row for an exactly singular KKT
// matrix.  A non-finite system (|w| beyond 2/dt: sqrt of a negative number) is NOT detected --
// project<NW> has no finiteness test, unlike vi_newton: NaN compares false in the pivot search, in
// the zero-pivot test and in the convergence test, so the state runs all a.iters iterations and
// returns a NaN row with iterations = a.iters and status 0.  With NaNs the butterfly's pivot row p
// may differ from lane to lane.  On the lanes l < n, the only ones that touch A, it stays below n;
// a lane l >= n may end with p >= n, but it swaps nothing, and readlane of a lane <= 63 is valid.
// The state's wave touches no other state's memory.
// This holds for k_project (NW = 1), where it is measured.  It is not a statement about the
// rollouts: in project<4> a lane-dependent p makes `if (p != k) pj_sync<NW>()` a barrier inside
// divergent control flow, and no test gives k_rollout_max a non-finite state.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_project(ProjArgs a) {
  __shared__ PState P;
  const int t = blockIdx.x, l = threadIdx.x;
  const int nb = a.mech.nb, n6 = 6 * nb;
  set_states(P, a.cs + (size_t)t * 13 * nb, nb, a.dt, l);
  if (l < n6) P.s[l] = a.vw[(size_t)t * n6 + l];
  __builtin_amdgcn_wave_barrier();
  project<1>(P, a.mech, a.dt, a.reg, a.eps, a.iters);
  __builtin_amdgcn_wave_barrier();
  if (l < n6) a.out[(size_t)t * n6 + l] = P.status ? NAN : P.s[l];
  if (l == 0) {
    a.iters_out[t] = P.it;
    a.status[t] = P.status;
  }
}

// ---- one variational-integrator step for T independent states: one wave each --------------------
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_vi_step(ViArgs a) {
  __shared__ PState P;
  __shared__ double mom1[PJ_MAXB][3];
  const int t = blockIdx.x, l = threadIdx.x;
  const int nb = a.mech.nb;
  set_states(P, a.cs + (size_t)t * 13 * nb, nb, a.dt, l);
  int it;
  const int status = vi_newton<1>(P, mom1, a.mech, MechBodies{a.mech}, a.dt, a.reg, a.eps, a.grav, a.iters, it);
  double* o = a.out + (size_t)t * 13 * nb;
  for (int i = l; i < 13 * nb; i += 64) {
    const int b = i / 13, k = i - 13 * b;
    double v;
    if (k < 3) v = P.xk[b][k];
    else if (k < 7) v = P.qk[b][k - 3];
    else v = P.s[6 * b + (k - 7)];  // v2 (7..9), w2 (10..12)
    o[i] = status == 2 ? NAN : v;
  }
  if (l == 0) {
    a.iters_out[t] = it;
    a.status[t] = status;
  }
}

// ---- simulate!: many variational-integrator steps of T independent trajectories, one wave each ----
// The datasets' simulations (examples/utils/data/simulations.jl; examples/parallel/dataframes.jl reads
// their storage): per step control! (viscous friction from the current velocities: F = -c_v o v1 in
// the world frame, tau = -c_w o w1 in the body frame), newton!, and the next CState [x2, q2, v2, w2]
// -- what k_vi_step writes, taken up by set_states exactly as a host loop over k_vi_step hands it
// back, so S steps here equal S launches of one step bit for bit.  The bodies are the trajectory's
// own (mass / inertia: the datasets' dm, dJ), read once into LDS.  The trajectory is not stored: rec
// lists the storage indices wanted (1 = the start, j = after j - 1 steps: saveToStorage! before
// each step), and the trajectory ends after its last one.  A failed step (status 2) ends it with
// NaN in the remaining records; one that only runs out of iterations is used as it is (the
// MeanDynamics rollouts' contract).  One launch takes steps [step0, step0 + nsteps); cs, cursor and
// status carry the trajectory to the next launch.  Every loop is bounded by nsteps, R or iters.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_simulate(SimArgs a) {
  __shared__ PState P;
  __shared__ double mom1[PJ_MAXB][3];
  __shared__ double cs[13 * PJ_MAXB];
  __shared__ double bm[PJ_MAXB], bJ[PJ_MAXB][3][3], bc[6 * PJ_MAXB], ext[6 * PJ_MAXB];
  const int t = blockIdx.x, l = threadIdx.x;
  const int nb = a.mech.nb, n6 = 6 * nb, d = 13 * nb, R = a.R;
  int r = a.cursor[t];
  if (r >= R) return;  // the trajectory has ended (the same on every lane)
  const int* rec = a.rec + (size_t)t * R;
  double* gcs = a.cs + (size_t)t * d;
  double* out = a.out + (size_t)t * R * d;
  for (int i = l; i < d; i += 64) cs[i] = gcs[i];
  if (l < nb) bm[l] = a.mass ? a.mass[(size_t)t * nb + l] : a.mech.m[l];
  for (int i = l; i < 9 * nb; i += 64) {
    const int b = i / 9, e = i - 9 * b;
    bJ[b][e / 3][e % 3] = a.inertia ? a.inertia[(size_t)t * 9 * nb + i] : a.mech.J[b][e / 3][e % 3];
  }
  if (l < n6) bc[l] = a.damp ? a.damp[(size_t)t * n6 + l] : 0.0;
  pj_sync<1>();
  const TrajBodies B{bm, bJ, ext};
  const int kend = a.step0 + a.nsteps;
  int st = 0, next = rec[r];
  bool failed = false;
  for (int k = a.step0;; ++k) {  // cs is the state of storage index k + 1
    while (r < R && next <= k + 1) {
      for (int i = l; i < d; i += 64) out[(size_t)r * d + i] = cs[i];
      ++r;
      if (r < R) next = rec[r];
    }
    if (r >= R || k >= kend) break;
    set_states(P, cs, nb, a.dt, l);
    pj_sync<1>();
    if (l < n6) {  // control!: F = -c_v o v1, and 2 tau = -2 c_w o w1 as the rotational row takes it
      const int b = l / 6, c = l - 6 * b;
      ext[l] = c < 3 ? -(bc[l] * P.vc[b][c]) : 2.0 * -(bc[l] * P.wc[b][c - 3]);
    }
    pj_sync<1>();
    int it;
    const int s = vi_newton<1>(P, mom1, a.mech, B, a.dt, a.reg, a.eps, a.grav, a.iters, it);
    if (s == 2) {  // the same on every lane
      failed = true;
      break;
    }
    st |= s;
    for (int i = l; i < d; i += 64) {  // the solution CState, as k_vi_step writes it
      const int b = i / 13, c = i - 13 * b;
      cs[i] = c < 3 ? P.xk[b][c] : (c < 7 ? P.qk[b][c - 3] : P.s[6 * b + (c - 7)]);
    }
    pj_sync<1>();
  }
  if (failed) {
    for (; r < R; ++r)
      for (int i = l; i < d; i += 64) out[(size_t)r * d + i] = NAN;
  } else {
    for (int i = l; i < d; i += 64) gcs[i] = cs[i];
  }
  if (l == 0) {
    a.cursor[t] = r;
    a.status[t] = failed ? 2 : (a.status[t] | st);
  }
}

// ---- predictdynamics: one workgroup per trajectory, every step on the device --------------------
// The MeanDynamics form (MD; predict_y = mu(obs) + k*^T alpha, src/mDynamics.jl:41-55) adds the physics
// mean per step: a second LDS PState set from obs (what the stepwise path hands gprx_vi_step), the
// variational-integrator solve on the whole workgroup (vi_newton), and v2 / w2 of its solution at
// CState position vw[g] added to GP g's mean (getmu(vwindices)).  The solve's matrix shares the
// dynamic LDS with the projection's F / A (they run one after the other); the second PState and
// mom1 follow it there.  A failed physics step (status 2: the reference throws) stops the
// trajectory with status 2; one that only runs out of iterations (status 1) is used as it is, as
// the stepwise path uses it.
// One template over the argument type: with RolloutMaxArgs (MeanZero) the instructions are those
// of the kernel before the MeanDynamics form existed (compared in the disassembly; a shared
// __device__ body called by two kernels changed its register allocation).  The MeanDynamics form
// drops the four-waves-per-SIMD hint: in the 128 registers that leaves, the solve spills to scratch.
__host__ __device__ inline size_t md_mat_doubles(int nb, int nd) {
  const size_t n = 6 * (size_t)nb + nd, pj = 2 * n * (n + 1), vi = vi_lds_doubles(nb, nd);
  return pj > vi ? pj : vi;
}
template <class Args>
constexpr bool is_md = std::is_base_of_v<RolloutMaxMdArgs, Args> || std::is_base_of_v<RolloutMinMdArgs, Args>;
// The recording, resumable forms (RolloutRec, gprx_internal.h): what they add stands in `if constexpr
// (is_rec<Args>)`, so the one-launch instantiations keep their instructions (compared in the
// disassembly) and each step body is stated once.
template <class Args>
constexpr bool is_rec = std::is_same_v<Args, RolloutMaxRecArgs> || std::is_same_v<Args, RolloutMaxMdRecArgs> ||
                        std::is_same_v<Args, RolloutRecArgs> || std::is_same_v<Args, RolloutMinMdRecArgs>;
// The records a launch has reached: rows of w doubles, row(i) the i-th, for every record whose storage
// index is at most `idx`; the whole workgroup calls (r and next are the same on every thread).
template <int NT, class Row>
__device__ __forceinline__ void rec_write(const RolloutRec& rr, int t, int w, int idx, int& r, int& next, Row row) {
  while (r < rr.R && next <= idx) {
    double* o = rr.traj + ((size_t)t * rr.R + r) * w;
    for (int i = threadIdx.x; i < w; i += NT) o[i] = row(i);
    ++r;
    if (r < rr.R) next = rr.rec[(size_t)t * rr.R + r];
  }
}
// NaN in every record from the cursor on: the trajectory has stopped
template <int NT>
__device__ __forceinline__ void rec_nan(const RolloutRec& rr, int t, int w, int& r) {
  for (; r < rr.R; ++r) {
    double* o = rr.traj + ((size_t)t * rr.R + r) * w;
    for (int i = threadIdx.x; i < w; i += NT) o[i] = NAN;
  }
}
// the steps of a launch: all of them, or [step0, step0 + nsteps) of a recorded form
template <class Args>
__device__ __forceinline__ int step_first(const Args& a) {
  if constexpr (is_rec<Args>) return a.rr.step0;
  else return 0;
}
template <class Args>
__device__ __forceinline__ int step_end(const Args& a) {
  if constexpr (is_rec<Args>) return a.rr.step0 + a.rr.nsteps < a.steps ? a.rr.step0 + a.rr.nsteps : a.steps;
  else return a.steps;
}
template <int MODE, class Args>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(is_md<Args> ? 1 : 4, is_md<Args> ? 2 : 4)))
void k_rollout_max(Args a) {
  constexpr bool MD = is_md<Args>, REC = is_rec<Args>;
  constexpr int NT = 256, NW = NT / 64;
  __shared__ PState P;
  __shared__ double obs[13 * PJ_MAXB];
  __shared__ double red[NW][PJ_MAXG];
  __shared__ double perr_s;
  const int t = blockIdx.x, tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int nb = a.mech.nb, n6 = 6 * nb, d = a.d, G = a.G;
  const RolloutGP* gp = a.gps + (size_t)a.group[t] * G;
  const double* st0 = a.start + (size_t)t * d;
  [[maybe_unused]] PState* Q = nullptr;            // the physics mean's state and (sq1 I - [w1 x]) J w1
  [[maybe_unused]] double (*mom1)[3] = nullptr;
  [[maybe_unused]] int vis = 0;
  if constexpr (MD) {
    Q = reinterpret_cast<PState*>(pj_lds() + md_mat_doubles(nb, a.mech.nd));
    mom1 = reinterpret_cast<double (*)[3]>(Q + 1);
  }
  if (w == 0) set_states(P, st0, nb, a.dt, l);
  for (int i = tid; i < d; i += NT) obs[i] = st0[i];
  if constexpr (MD) {
    // setstates! leaves the start's own velocities as the solution, which the closing updatestate!
    // uses when steps = 0 (the MeanZero form, kept as it was, leaves P.s unset in that case)
    if (tid < n6) P.s[tid] = st0[13 * (tid / 6) + 7 + tid % 6];
  }
  if (tid == 0) {
    perr_s = 0.0;
    P.status = 0;
  }
  __syncthreads();
  [[maybe_unused]] int rcur = 0, rnext = 0;  // the record cursor and the storage index it waits for
  if constexpr (REC) {
    if (a.rr.step0 > 0) {
      // What the loop and the closing update read on entry, as the last launch left it, over the
      // start's: the CState (obs, and in P), the discrete pose, the solution twists, the error sum
      // and the statuses.  The pose is carried, not rebuilt by set_states: that is the same algebra,
      // not the same roundings.
      const double* cy = a.rr.carry + (size_t)t * ROLLOUT_CARRY;
      for (int i = tid; i < d; i += NT) {
        const double v = cy[i];
        const int b = i / 13, k = i - 13 * b;
        obs[i] = v;
        if (k < 3) P.xc[b][k] = v;
        else if (k < 7) P.qc[b][k - 3] = v;
        else if (k < 10) P.vc[b][k - 7] = v;
        else P.wc[b][k - 10] = v;
      }
      for (int i = tid; i < 3 * nb; i += NT) P.xk[i / 3][i % 3] = cy[d + i];
      for (int i = tid; i < 4 * nb; i += NT) P.qk[i / 4][i % 4] = cy[d + 3 * nb + i];
      for (int i = tid; i < n6; i += NT) P.s[i] = cy[d + 7 * nb + i];
      if (tid == 0) {
        perr_s = cy[d + 7 * nb + n6];
        P.status = a.rr.icarry[2 * t];
      }
      if constexpr (MD) vis = a.rr.icarry[2 * t + 1];
      rcur = a.rr.cursor[t];
      __syncthreads();
    }
    if (rcur < a.rr.R) rnext = a.rr.rec[(size_t)t * a.rr.R + rcur];
  }
  for (int step = step_first(a); step < step_end(a) && P.status == 0; ++step) {
    // obs is the CState after `step` steps, storage index step + 1 (it changes after the next barrier)
    if constexpr (REC) rec_write<NT>(a.rr, t, d, step + 1, rcur, rnext, [&](int i) { return obs[i]; });
    // ---- mu_g = sum_j sf2 exp(-r_j / 2) alpha_j at the current CState (predict_y means)
    for (int g = 0; g < G; ++g) {
      const RolloutGP Gp = gp[g];
      const double sf2 = Gp.params[d];
      double sacc = 0.0;
      for (int j = tid; j < Gp.N; j += NT) {
        const double* x = Gp.X + (size_t)j * d;
        double r = 0.0;
        for (int p = 0; p < d; ++p) {
          const double o = obs[p];
          if (MODE == 0) {
            const double v = fma(-2.0, x[p] * o, x[p] * x[p] + o * o);
            r = r + (v > 0.0 ? v : 0.0) * Gp.params[p];
          } else {
            const double df = x[p] - o;
            r = __builtin_fma(df * df, Gp.params[p], r);
          }
        }
        sacc = fma(sf2 * exp(-r * 0.5), Gp.alpha[j], sacc);
      }
      sacc = wave_sum(sacc);
      if (l == 0) red[w][g] = sacc;
    }
    __syncthreads();
    if constexpr (MD) {  // the physics mean at obs
      if (w == 0) set_states(*Q, obs, nb, a.dt, l);
      __syncthreads();
      int vit;
      const int vs = vi_newton<NW>(*Q, mom1, a.mech, MechBodies{a.mech}, a.dt, a.vi.reg, a.vi.eps, a.vi.grav, a.vi.iters, vit);
      vis |= vs;
      if (vs == 2) {  // the same on every wave
        if (tid == 0) P.status = 2;
        __syncthreads();
        break;
      }
    }
    if (w == 0) {
      // getvw: mu_g at CState position vw[g], zero elsewhere; (v, w) per body into P.s
      if (l < n6) P.s[l] = 0.0;
      __builtin_amdgcn_wave_barrier();
      if (l < G) {
        double mu = red[0][l];
        for (int q = 1; q < NW; ++q) mu += red[q][l];
        const int pos = a.vw[l], b = pos / 13, k = pos - 13 * b;  // k in 7..12
        if constexpr (MD) mu += Q->s[6 * b + (k - 7)];
        P.s[6 * b + (k - 7)] = mu;
      }
    }
    __syncthreads();
    project<NW>(P, a.mech, a.dt, a.reg, a.eps, a.iters);  // the whole workgroup
    if (w == 0) {
      // projection error |(v, w)_const - (v, w)_pred| (predictdynamics.jl:16), then updatestate!
      const double dv = l < n6 ? P.s[l] - P.su[l] : 0.0;
      const double e = sqrt(wave_sum(dv * dv));
      if (l == 0) perr_s += e;
      update_state(P, nb, a.dt, l);
      __builtin_amdgcn_wave_barrier();
      for (int i = l; i < d; i += 64) obs[i] = cstate_at(P, i);
    }
    __syncthreads();
  }
  if constexpr (REC) {
    // the state the loop ended at, index step_end + 1 (the next launch's first, or the last of all); a
    // trajectory that stopped has NaN from the failed step onward and keeps its one-launch outputs
    if (P.status == 0) {
      rec_write<NT>(a.rr, t, d, step_end(a) + 1, rcur, rnext, [&](int i) { return obs[i]; });
    } else {
      rec_nan<NT>(a.rr, t, d, rcur);
    }
    if (step_end(a) < a.steps) {
      double* cy = a.rr.carry + (size_t)t * ROLLOUT_CARRY;
      for (int i = tid; i < d; i += NT) cy[i] = obs[i];
      for (int i = tid; i < 3 * nb; i += NT) cy[d + i] = P.xk[i / 3][i % 3];
      for (int i = tid; i < 4 * nb; i += NT) cy[d + 3 * nb + i] = P.qk[i / 4][i % 4];
      for (int i = tid; i < n6; i += NT) cy[d + 7 * nb + i] = P.s[i];
      if (tid == 0) {
        cy[d + 7 * nb + n6] = perr_s;
        a.rr.cursor[t] = rcur;
        a.rr.icarry[2 * t] = P.status;
        a.rr.icarry[2 * t + 1] = vis;
      }
      return;
    }
  }
  if (w == 0) {
    update_state(P, nb, a.dt, l);  // the closing updatestate! (predictdynamics.jl:20)
    __builtin_amdgcn_wave_barrier();
    for (int i = l; i < d; i += 64) a.out[(size_t)t * d + i] = P.status ? NAN : cstate_at(P, i);
    if (l == 0) {
      a.perr[t] = P.status ? NAN : perr_s / (a.steps > 0 ? a.steps : 1);
      a.status[t] = P.status;
      if constexpr (MD)
        if (a.vi.status) a.vi.status[t] = vis;
    }
  }
}
// ---- the minimal coordinates' CState (predictdynamicsmin with MeanDynamics GPs) ------------------
// The experiments' xtransform (examples/minimal_coordinates/*noise.jl, restated in
// gprx/mdynamics.py xtransform, whose operation order this keeps) for body b: the CState of the
// mechanism at the minimal coordinates (a0, a1) with rates (r0, r1), the linear velocities by the
// reference's literal 0.01 finite difference of the positions (not dt).
static __device__ __forceinline__ void min_cstate_body(int mech, int b, double a0, double r0, double a1, double r1, double l1, double l2, double* c) {
  const double h = 0.01;
  double x = 0.0, y, z, yn, zn, th, w;  // position (x, y, z), the advanced (yn, zn), angle about x and its rate
  if (mech == 1) {  // P1
    th = a0;
    w = r0;
    const double tn = th + w * h;
    y = 0.5 * sin(th) * l1;
    z = -0.5 * cos(th) * l1;
    yn = 0.5 * sin(tn) * l1;
    zn = -0.5 * cos(tn) * l1;
  } else if (mech == 2) {  // P2: a1 relative to link 1
    const double n1 = a0 + r0 * h, n2 = a1 + r1 * h;
    if (b == 0) {
      th = a0;
      w = r0;
      y = 0.5 * sin(a0) * l1;
      z = -0.5 * cos(a0) * l1;
      yn = 0.5 * sin(n1) * l1;
      zn = -0.5 * cos(n1) * l1;
    } else {
      th = a0 + a1;
      w = r0 + r1;
      y = sin(a0) * l1 + 0.5 * sin(a0 + a1) * l2;
      z = -cos(a0) * l1 - 0.5 * cos(a0 + a1) * l2;
      yn = sin(n1) * l1 + 0.5 * sin(n1 + n2) * l2;
      zn = -cos(n1) * l1 - 0.5 * cos(n1 + n2) * l2;
    }
  } else if (mech == 3) {  // CP: the cart at (0, a0, 0) moving with r0, the pole at angle a1
    if (b == 0) {
      for (int k = 0; k < 13; ++k) c[k] = 0.0;
      c[1] = a0;
      c[3] = 1.0;
      c[8] = r0;
      return;
    }
    th = a1;
    w = r1;
    const double tn = w * h + th;
    y = a0 + 0.5 * sin(th) * l1;
    z = -0.5 * cos(th) * l1;
    yn = a0 + r0 * h + 0.5 * sin(tn) * l1;
    zn = -0.5 * cos(tn) * l1;
  } else {  // FB: links 1 and 4 turn with a0, links 2 and 3 with a1
    const double na = 0.01 * r0 + a0, nb = 0.01 * r1 + a1;
    const bool first = b == 0 || b == 3;
    th = first ? a0 : a1;
    w = first ? r0 : r1;
    if (b == 0 || b == 2) {
      const double t = b == 0 ? a0 : a1, tn = b == 0 ? na : nb;
      y = 0.5 * sin(t) * l1;
      z = -0.5 * cos(t) * l1;
      yn = 0.5 * sin(tn) * l1;
      zn = -0.5 * cos(tn) * l1;
    } else {
      const double p = b == 1 ? a0 : a1, q = b == 1 ? a1 : a0, pn = b == 1 ? na : nb, qn = b == 1 ? nb : na;
      y = sin(p) * l1 + 0.5 * sin(q) * l1;
      z = -cos(p) * l1 - 0.5 * cos(q) * l1;
      yn = sin(pn) * l1 + 0.5 * sin(qn) * l1;
      zn = -cos(pn) * l1 - 0.5 * cos(qn) * l1;
    }
  }
  c[0] = x;
  c[1] = y;
  c[2] = z;
  c[3] = cos(th / 2.0);
  c[4] = sin(th / 2.0);
  c[5] = 0.0;
  c[6] = 0.0;
  c[7] = (x - x) / h;
  c[8] = (yn - y) / h;
  c[9] = (zn - z) / h;
  c[10] = w;
  c[11] = 0.0;
  c[12] = 0.0;
}

// ---- predictdynamicsmin (examples/utils/predictdynamics.jl:30-102): one workgroup per trajectory ---
// `steps` rounds of  obs = f(q_old, qdot_old);  qdot_cur_g = mu_g(obs) for each of the nc GPs;
// (q_old, qdot_old) = (q_cur, qdot_cur);  q_cur += qdot_cur dt.  The step chain is serial, so the
// rollout is latency-bound: one launch instead of steps x nc predict calls.  mu_g = sum_j sf2
// exp(-r_j/2) alpha_j with r_j summed as distij does (il2-weighted; k_pred_cross sums coordinates
// pre-scaled by sqrt(il2/2) instead), so a rollout step reproduces gprx_batch_predict's mean up to
// rounding: the distance sums', the exp's (libm's here, k_pred_cross's table exp_sf) and the order of
// the final sum.  The state updates use explicit round-to-nearest mul/add (no fma contraction), as the
// reference's Julia arithmetic.  Every thread keeps the coordinates (the same values).
// One template over the argument type, as k_rollout_max: with RolloutArgs (MeanZero) the instructions
// are those of the kernel before the MeanDynamics form existed.  With RolloutMinMdArgs
// (src/mDynamics.jl:41-55) each step adds the physics mean: the CState of the features
// (min_cstate_body; the angle is atan2(sin, cos) when usesin), set_states and vi_newton on the whole
// workgroup, and the rates read from the solution (gprx/mdynamics.py MIN_IDX / mean_min) added to the
// GP means.  A failed physics step (status 2: the reference throws) stops the trajectory.
__device__ __forceinline__ double pick3(const double (&e)[3], int i) {
  return i == 0 ? e[0] : (i == 1 ? e[1] : (i == 2 ? e[2] : 0.0));
}
// entry i of a record, (q_old, qdot_old) per coordinate, from copies of the four values (selects: a
// register array indexed by a lane-dependent value, or one a lambda refers to, would live in scratch memory)
__device__ __forceinline__ double min_row(double q0, double v0, double q1, double v1, int i) {
  return (i & 1) ? (i >> 1 ? v1 : v0) : (i >> 1 ? q1 : q0);
}

template <int MODE, class Args>
__global__ __launch_bounds__(256) void k_rollout(Args a) {
  constexpr bool MD = is_md<Args>, REC = is_rec<Args>;
  constexpr int NT = 256, NW = NT / 64, U = 4;  // U training points per thread in flight
  __shared__ double red[2][NW][2];
  [[maybe_unused]] __shared__ PState Q;  // the physics mean's state, (sq1 I - [w1 x]) J w1 and CState
  [[maybe_unused]] __shared__ double mom1[PJ_MAXB][3];
  [[maybe_unused]] __shared__ double cs[13 * PJ_MAXB];
  const int t = blockIdx.x, tid = threadIdx.x, nc = a.nc, d = a.d;
  const RolloutGP* gp = a.gps + (size_t)a.group[t] * nc;
  double qo[2], vo[2], qc[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    qo[c] = c < nc ? a.start[(size_t)t * 2 * nc + 2 * c] : 0.0;
    vo[c] = c < nc ? a.start[(size_t)t * 2 * nc + 2 * c + 1] : 0.0;
    qc[c] = __dadd_rn(qo[c], __dmul_rn(a.dt, vo[c]));
  }
  const bool s0 = a.usesin && a.ang0, s1 = a.usesin && a.ang1;
  const int w0 = s0 ? 3 : 2;
  [[maybe_unused]] int vis = 0;
  bool failed = false;
  [[maybe_unused]] int rcur = 0, rnext = 0;  // the record cursor and the storage index it waits for
  if constexpr (REC) {
    if (a.rr.step0 > 0) {  // the coordinates and the statuses as the last launch left them
      const double* cy = a.rr.carry + (size_t)t * ROLLOUT_CARRY;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        qo[c] = cy[3 * c];
        vo[c] = cy[3 * c + 1];
        qc[c] = cy[3 * c + 2];
      }
      rcur = a.rr.cursor[t];
      failed = a.rr.icarry[2 * t] != 0;
      vis = a.rr.icarry[2 * t + 1];
    }
    if (rcur < a.rr.R) rnext = a.rr.rec[(size_t)t * a.rr.R + rcur];
  }
  for (int step = step_first(a); step < step_end(a); ++step) {
    if constexpr (REC) {
      if (failed) break;  // the trajectory has stopped in an earlier launch (the same on every thread)
      // (q_old, qdot_old) is the state after `step` steps, storage index step + 1
      const double q0 = qo[0], v0 = vo[0], q1 = qo[1], v1 = vo[1];
      rec_write<NT>(a.rr, t, 2 * nc, step + 1, rcur, rnext, [=](int i) { return min_row(q0, v0, q1, v1, i); });
    }
    double e0[3], e1[3];
    e0[0] = s0 ? sin(qo[0]) : qo[0];
    e0[1] = s0 ? cos(qo[0]) : vo[0];
    e0[2] = s0 ? vo[0] : 0.0;
    e1[0] = s1 ? sin(qo[1]) : qo[1];
    e1[1] = s1 ? cos(qo[1]) : vo[1];
    e1[2] = s1 ? vo[1] : 0.0;
    double ov[ROLLOUT_DMAX], ov2[ROLLOUT_DMAX];
#pragma unroll
    for (int p = 0; p < ROLLOUT_DMAX; ++p) {
      ov[p] = p < w0 ? pick3(e0, p) : pick3(e1, p - w0);
      ov2[p] = ov[p] * ov[p];
    }
    // ---- mu_g = sum_j sf2 exp(-r_j / 2) alpha_j at the features
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (g >= nc) break;
      const RolloutGP G = gp[g];
      double il2[ROLLOUT_DMAX];
#pragma unroll
      for (int p = 0; p < ROLLOUT_DMAX; ++p) il2[p] = p < d ? G.params[p] : 0.0;
      const double sf2 = G.params[d];
      double s = 0.0;
      // points j = tid + NT k in increasing k (the same order as a plain strided loop), U at a time
      for (int j0 = tid; j0 < G.N; j0 += U * NT) {
        double xv[U][ROLLOUT_DMAX], al[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = j0 + u * NT;
          const bool ok = j < G.N;
          const double* x = G.X + (size_t)(ok ? j : 0) * d;
#pragma unroll
          for (int p = 0; p < ROLLOUT_DMAX; ++p) xv[u][p] = p < d ? x[p] : 0.0;
          al[u] = ok ? G.alpha[j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          double r = 0.0;
#pragma unroll
          for (int p = 0; p < ROLLOUT_DMAX; ++p)
            if (p < d) r = wacc<MODE>(r, xv[u][p], xv[u][p] * xv[u][p], ov[p], ov2[p], il2[p]);
          if (j0 + u * NT < G.N) s = fma(sf2 * exp(-r * 0.5), al[u], s);
        }
      }
      acc[g] = wave_sum(s);
    }
    const int par = step & 1;
    if ((tid & 63) == 0) {
      red[par][tid >> 6][0] = acc[0];
      red[par][tid >> 6][1] = acc[1];
    }
    [[maybe_unused]] double phys[2];
    if constexpr (MD) {  // the physics mean: CState of the features, one variational-integrator step
      const int nb = a.mech.nb;
      const double a0 = s0 ? atan2(e0[0], e0[1]) : e0[0], r0 = s0 ? e0[2] : e0[1];
      const double a1 = s1 ? atan2(e1[0], e1[1]) : e1[0], r1 = s1 ? e1[2] : e1[1];
      if (tid < nb) min_cstate_body(a.mech_id, tid, a0, r0, a1, r1, a.len[0], a.len[1], cs + 13 * tid);
      __syncthreads();
      if (tid < 64) set_states(Q, cs, nb, a.dt, tid);
      __syncthreads();
      int vit;
      const int vs = vi_newton<NW>(Q, mom1, a.mech, MechBodies{a.mech}, a.dt, a.vi.reg, a.vi.eps, a.vi.grav, a.vi.iters, vit);
      vis |= vs;
      if (vs == 2) {  // the same on every wave
        failed = true;
        break;
      }
      // the solution's rates (0-based CState positions 13 b + k, k >= 7, at Q.s[6 b + k - 7]):
      // P1 [11]; P2 (w1, w2 - w1) of bodies 1 and 2; CP [9, 24]; FB [11, 37] (1-based)
      if (a.mech_id == 2) {
        phys[0] = Q.s[3];
        phys[1] = Q.s[9] - Q.s[3];
      } else if (a.mech_id == 3) {
        phys[0] = Q.s[1];
        phys[1] = Q.s[9];
      } else {
        phys[0] = Q.s[3];
        phys[1] = a.mech_id == 4 ? Q.s[15] : 0.0;
      }
    }
    // red[par] is rewritten two steps later, after this step's reads; Q and mom1 by the next step, whose
    // writes follow this barrier and this step's reads of them precede it
    __syncthreads();
    double pred[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      double v = red[par][0][g];
#pragma unroll
      for (int w = 1; w < NW; ++w) v += red[par][w][g];
      if constexpr (MD) v += phys[g];  // (a coordinate past nc has mean and rate 0 and is not written)
      pred[g] = v;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      qo[c] = qc[c];
      vo[c] = pred[c];
      qc[c] = __dadd_rn(qc[c], __dmul_rn(pred[c], a.dt));
    }
  }
  if constexpr (REC) {
    // the state the loop ended at, index step_end + 1; NaN from a failed step onward
    const double q0 = qo[0], v0 = vo[0], q1 = qo[1], v1 = vo[1];
    if (!failed) rec_write<NT>(a.rr, t, 2 * nc, step_end(a) + 1, rcur, rnext, [=](int i) { return min_row(q0, v0, q1, v1, i); });
    else rec_nan<NT>(a.rr, t, 2 * nc, rcur);
    if (step_end(a) < a.steps) {
      if (tid == 0) {
        double* cy = a.rr.carry + (size_t)t * ROLLOUT_CARRY;
        for (int c = 0; c < 2; ++c) {
          cy[3 * c] = qo[c];
          cy[3 * c + 1] = vo[c];
          cy[3 * c + 2] = qc[c];
        }
        a.rr.cursor[t] = rcur;
        a.rr.icarry[2 * t] = failed ? 2 : 0;
        a.rr.icarry[2 * t + 1] = vis;
      }
      return;
    }
  }
  if (tid == 0) {
    for (int c = 0; c < nc; ++c) {
      a.out[(size_t)t * 2 * nc + 2 * c] = failed ? NAN : qc[c];
      a.out[(size_t)t * 2 * nc + 2 * c + 1] = failed ? NAN : vo[c];
    }
    if constexpr (MD) {
      a.status[t] = failed ? 2 : 0;
      if (a.vi.status) a.vi.status[t] = vis;
    }
  }
}

void launch_project(const ProjArgs& a, hipStream_t s) {
  if (a.T > 0) hipLaunchKernelGGL(k_project, dim3(a.T), dim3(64), pj_lds_bytes(a.mech.nb, a.mech.nd), s, a);
}
void launch_vi_step(const ViArgs& a, hipStream_t s) {
  if (a.T > 0) hipLaunchKernelGGL(k_vi_step, dim3(a.T), dim3(64), vi_lds_doubles(a.mech.nb, a.mech.nd) * sizeof(double), s, a);
}
void launch_simulate(const SimArgs& a, hipStream_t s) {
  if (a.T > 0) hipLaunchKernelGGL(k_simulate, dim3(a.T), dim3(64), vi_lds_doubles(a.mech.nb, a.mech.nd) * sizeof(double), s, a);
}
template <class Args>
static void launch_rollout_max_t(const Args& a, int dist_mode, hipStream_t s) {
  if (a.T <= 0) return;
  // MeanDynamics: [the larger of the projection's F / A and the solve's matrix + Gpos | the solve's PState | mom1]
  const size_t lds = is_md<Args> ? md_mat_doubles(a.mech.nb, a.mech.nd) * sizeof(double) + sizeof(PState) + sizeof(double) * 3 * PJ_MAXB
                                 : pj_lds_bytes(a.mech.nb, a.mech.nd);
  if (dist_mode == 0) hipLaunchKernelGGL((k_rollout_max<0, Args>), dim3(a.T), dim3(256), lds, s, a);
  else hipLaunchKernelGGL((k_rollout_max<1, Args>), dim3(a.T), dim3(256), lds, s, a);
}
void launch_rollout_max(const RolloutMaxArgs& a, int dist_mode, hipStream_t s) { launch_rollout_max_t(a, dist_mode, s); }
void launch_rollout_max_md(const RolloutMaxMdArgs& a, int dist_mode, hipStream_t s) { launch_rollout_max_t(a, dist_mode, s); }
void launch_rollout_max_rec(const RolloutMaxRecArgs& a, int dist_mode, hipStream_t s) { launch_rollout_max_t(a, dist_mode, s); }
void launch_rollout_max_md_rec(const RolloutMaxMdRecArgs& a, int dist_mode, hipStream_t s) { launch_rollout_max_t(a, dist_mode, s); }
// 256 threads per trajectory for every T (measured: 512 is 0.04 ms faster for 100 trajectories, 256 is
// 1.4x faster for 3200; a fixed size keeps each trajectory's sums independent of T)
template <class Args>
static void launch_rollout_min(const Args& a, int dist_mode, size_t lds, hipStream_t s) {
  if (a.T <= 0) return;
  if (dist_mode == 0) hipLaunchKernelGGL((k_rollout<0, Args>), dim3(a.T), dim3(256), lds, s, a);
  else hipLaunchKernelGGL((k_rollout<1, Args>), dim3(a.T), dim3(256), lds, s, a);
}
void launch_rollout(const RolloutArgs& a, int dist_mode, hipStream_t s) { launch_rollout_min(a, dist_mode, 0, s); }
void launch_rollout_min_md(const RolloutMinMdArgs& a, int dist_mode, hipStream_t s) {
  launch_rollout_min(a, dist_mode, vi_lds_doubles(a.mech.nb, a.mech.nd) * sizeof(double), s);
}
void launch_rollout_rec(const RolloutRecArgs& a, int dist_mode, hipStream_t s) { launch_rollout_min(a, dist_mode, 0, s); }
void launch_rollout_min_md_rec(const RolloutMinMdRecArgs& a, int dist_mode, hipStream_t s) {
  launch_rollout_min(a, dist_mode, vi_lds_doubles(a.mech.nb, a.mech.nd) * sizeof(double), s);
}

}  // namespace gprx
