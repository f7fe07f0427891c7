// gprx_kernels.hip -- CDNA4 (gfx950) kernels of the exact SE-ARD GP hot path, fp64.
//
// Algorithm (restating GaussianProcesses.jl v0.12.4 update_cK!/update_mll!/update_dmll!/predict_f
// as used by examples/maximal_coordinates/*noise.jl; see DESIGN.md for the kernel map):
//   K = sf2 * exp(-r/2) + (sn2 + eps) I,  r_ij = sum_p il2_p * dist_p(x_i, x_j)          (gram)
//   recursive Cholesky + triangular inverse on 64x64 tiles (host recursion, gprx_api.hip):
//     [A11 .; A21 A22]: rec(A11) -> L11, L11^-1 ; L21 = A21 L11^-T (TRSM) ;
//     A22 -= L21 L21^T (SYRK) ; rec(A22) ; T^T = L11^-T L21^T (TT) ; L21^-1 = -L22^-1 T (LINV21)
//     leaves: 64x64 Cholesky + inverse in one workgroup (diag)
//   alpha = L^-T (L^-1 y)                                                            (alpha)
//   K^-1  = L^-T L^-1 tile by tile, fused with the gradient reduction of
//           W = alpha alpha^T - K^-1 against dK/dtheta (K^-1 never written to HBM)   (lauum_grad)
//   mll, dmll                                                                        (finalize)
//   mu* = k*^T alpha,  var* = max(sf2 - |L^-1 k*|^2, 0)                             (pred_*)
// The rollouts (k_rollout, k_rollout_max) and their physics are in gprx_projection.hip.
//
// Dense products: one wave computes a 64x32 block with v_mfma_f64_16x16x4_f64 (4x2 16x16
// accumulators), operands streamed straight from L2 one 16-deep stage ahead (fp64 MFMA is 64
// cycles per instruction per SIMD; a 4x2 register tile needs 0.75 fragment loads per MFMA).  A
// workgroup = 4 waves = two vertically adjacent 64x64 tiles sharing their B panel.  Each wave has
// its own K range, so triangular operands are skipped at tile granularity.
// Workgroup -> (slot, unit) mapping keeps every slot's units on one XCD (blocks b, b+8, ... share
// an XCD), so the panels of a slot stay in that XCD's L2.
#include "gprx_internal.h"
#include <algorithm>
#include <array>
#include <cstdlib>
#include <vector>
// This file is one translation unit cut along its banners.  It includes its parts once each, in this
// order:
//   gprx_device.h, gprx_cores.h, gprx_stamps.h                  here, before the first kernel (lane
//                                                               primitives, wave MFMA cores, stamps)
//   gprx_gemm.h, gprx_factor.h                                  after the Gram and single-tile kernels
//   gprx_predcov.h, gprx_loo.h, gprx_loograd.h, gprx_cvfold.h   last, after the launchers
// No other file includes them: they share the device globals and there is no relocatable device
// code in this build.
#include "gprx_device.h"
#include "gprx_cores.h"
#include "gprx_stamps.h"

namespace gprx {

// ============================================================================================
// Gram: lower tiles of K (noise on the diagonal).  grid = B * ntl, 256 threads, each thread
// a 4x4 register block; X tiles in dynamic LDS as [p][64].
// ============================================================================================
// Coordinate images in LDS, dimension-major with row stride CS = 66 doubles: the tile loads write
// them with the dimension as the fast index across lanes, and a stride of 64 put every dimension of
// a point in one bank (26-way conflicts on each ds_write_b64); 66 spreads them over the banks and
// keeps the 16-B alignment of the inner loop's ds_read_b128.
constexpr int CS = TS + 2;
// (the waves per SIMD the registers must allow are stated: 8 in direct mode, 5 in expanded mode, which
// the kernel met unasked until the active-dimension staging tipped the scheduler's estimate)
template <int MODE>
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(MODE == 1 ? 8 : 5))) void k_gram(DevBatch db) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ __attribute__((aligned(16))) double tab[128];  // exp_sf's sf2 2^(j/64) table (static: a
                                                            // known LDS address, no base add)
  // Only the da active dimensions are staged and summed (DevBatch::da, amask; in ascending order, so
  // the chain below keeps its order).  A dropped dimension holds one constant per slot: its scaled
  // difference is an exact +0 and fma(0, 0, r) == r, so K keeps every bit.  Expanded mode runs with
  // da == d, every dimension active (a^2 + b^2 - 2ab is no exact zero).
  const int d = db.d, da = db.da, tid = threadIdx.x;
  double* xi = sm;
  double* xj = xi + da * CS;
  double* pw = xj + da * CS;
  int slot, t, i = 0, j = 0;
  if (!map_slot(db, db.ntl, slot, t)) return;
  {  // t-th lower tile in column-major order
    int c = 0, u = t;
    while (u >= db.nt - c) {
      u -= db.nt - c;
      ++c;
    }
    j = c;
    i = c + u;
  }
  const double* X = db.X + (size_t)slot * db.Npad * d;
  const double* P = db.params + (size_t)slot * db.pst;
  {  // thread -> (dimension p = tid mod 32 + 32 k, rows tid / 32 + 8 m): no per-element division,
     // 16 loads in flight per thread, coalesced over the 32 dimensions of a point row
    // buffer loads: the lane's byte offset in a VGPR, the row step and tile base in SGPRs, so no
    // per-load address arithmetic (64-bit global addresses cost 2-3 VALU per load here)
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(X, db.Npad * d * (int)sizeof(double));
    const int bi = i * TS * d * (int)sizeof(double), bj = j * TS * d * (int)sizeof(double);
    const int os = 8 * d * (int)sizeof(double);
    for (int pf = tid & 31; pf < d; pf += 32) {  // pf: the dimension in X and P; p: its image row
      if (!((db.amask >> pf) & 1)) continue;
      const int p = act_rank(db.amask, pf);
      double vi[TS / 8], vj[TS / 8];
      const int o0 = ((tid >> 5) * d + pf) * (int)sizeof(double);
#pragma unroll
      for (int m = 0; m < TS / 8; ++m) {
        vi[m] = buffer_load_f64(xr, o0, bi + m * os);
        vj[m] = buffer_load_f64(xr, o0, bj + m * os);
      }
      // direct mode: coordinates pre-scaled by 1/(sqrt(2) ell_p) = sqrt(il2_p / 2), so that the
      // sums are r/2, the exponent's magnitude (0.5 il2_p is exact: as accurate as scaling by
      // 1/ell_p); each thread scales its own dimension (no staging barrier)
      const double s = MODE == 1 ? sqrt(0.5 * P[pf]) : 1.0;
#pragma unroll
      for (int m = 0; m < TS / 8; ++m) {
        const int r = (tid >> 5) + 8 * m;
        xi[p * CS + r] = vi[m] * s;
        xj[p * CS + r] = vj[m] * s;
      }
    }
  }
  for (int e = tid; e < d + 4; e += NTHR) pw[e] = P[e];
  if (tid < 64) {  // sf2 (hi_j + lo_j) as hi + lo: the product's rounding error by fma, plus sf2 lo_j
    const double s2 = P[d], h = g_exp2tab[2 * tid], lo = g_exp2tab[2 * tid + 1];
    const double th = s2 * h;
    tab[2 * tid] = th;
    tab[2 * tid + 1] = fma(s2, h, -th) + s2 * lo;
  }
  __syncthreads();
  const double noise = pw[d + 1];
  const ExpK ek = g_expk;
  const int rb = tid & 15, cb = tid >> 4;
  double rr[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) rr[a][b] = 0.0;
  for (int p = 0; p < da; ++p) {
    const double2 u0 = *(const double2*)(xi + p * CS + 4 * rb);
    const double2 u1 = *(const double2*)(xi + p * CS + 4 * rb + 2);
    const double2 v0 = *(const double2*)(xj + p * CS + 4 * cb);
    const double2 v1 = *(const double2*)(xj + p * CS + 4 * cb + 2);
    const double av[4] = {u0.x, u0.y, u1.x, u1.y};
    const double bv[4] = {v0.x, v0.y, v1.x, v1.y};
    const double w = pw[p];  // expanded mode only, where p is the dimension itself
    double a2[4], b2[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      a2[a] = av[a] * av[a];
      b2[a] = bv[a] * bv[a];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (MODE == 0) {
          rr[a][b] = wacc<0>(rr[a][b], av[a], a2[a], bv[b], b2[b], w);
        } else {  // r += (a/ell - b/ell)^2: 2 fp64 ops per element and dimension
          const double t = av[a] - bv[b];
          rr[a][b] = __builtin_fma(t, t, rr[a][b]);
        }
      }
  }
  {  // the dropped dimensions' share of every sum (derive_params): +0, which leaves the sums (all
     // >= +0) as they are, or NaN
    const double r0 = pw[d + 3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) rr[a][b] += r0;
  }
  double* K = db.K + (size_t)slot * db.mat;
  // buffer stores over the tile (base uniform): the lane's byte offset in a VGPR (column step
  // added per store), no 64-bit address arithmetic per store
  const __amdgpu_buffer_rsrc_t kr = buffer_rsrc(K + (size_t)j * TS * db.ld + i * TS, 0x7ffffff0);
  const int ldb = (int)db.ld * (int)sizeof(double), lof = 4 * cb * ldb + 4 * rb * (int)sizeof(double);
  if (i != j && (i + 1) * TS <= db.N) {  // off-diagonal tile inside N x N (block-uniform): no tests
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      double kv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) kv[a] = exp_sf(MODE == 1 ? -rr[a][b] : -rr[a][b] * 0.5, ek, tab);
      buffer_store_f64x2(kr, lof + b * ldb, kv[0], kv[1]);
      buffer_store_f64x2(kr, lof + b * ldb + 16, kv[2], kv[3]);
    }
    return;
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int gj = j * TS + 4 * cb + b;
    double kv[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {  // branch-free: padded points (finite coordinates) are selected away
      const int gi = i * TS + 4 * rb + a;
      const double fv = exp_sf(MODE == 1 ? -rr[a][b] : -rr[a][b] * 0.5, ek, tab);
      const bool pad = gi >= db.N || gj >= db.N;
      kv[a] = (gi == gj) ? (pad ? 1.0 : fv + noise) : (pad ? 0.0 : fv);
    }
    buffer_store_f64x2(kr, lof + b * ldb, kv[0], kv[1]);
    buffer_store_f64x2(kr, lof + b * ldb + 16, kv[2], kv[3]);
  }
}

// Centred copy of the training points, active dimensions only: Xc[t][q] = X[t][p] - mean_t X[t][p],
// p = act[q], for t < N, q < da, and 0 elsewhere (padded points, padded columns up to the stride
// xs).  grid = B, once per gprx_batch_set_train.
__global__ __launch_bounds__(NTHR) void k_center(DevBatch db) {
  __shared__ double mean[DMAX];
  __shared__ double red[4];
  __shared__ int act[DMAX];  // act[q]: the q-th active dimension
  const int slot = blockIdx.x, tid = threadIdx.x, d = db.d, xs = db.xs, da = db.da;
  const double* X = db.X + (size_t)slot * db.Npad * d;
  double* Xc = db.Xc + (size_t)slot * db.Npad * xs;
  if (tid < d && ((db.amask >> tid) & 1)) act[act_rank(db.amask, tid)] = tid;
  __syncthreads();
  for (int q = 0; q < da; ++q) {
    const int p = act[q];
    double s = 0.0;
    for (int t = tid; t < db.N; t += NTHR) s += X[(size_t)t * d + p];
    s = wave_sum(s);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) mean[q] = (((red[0] + red[1]) + red[2]) + red[3]) / db.N;
  }
  __syncthreads();
  for (int e = tid; e < db.Npad * xs; e += NTHR) {
    const int t = e / xs, q = e - t * xs;
    Xc[e] = (t < db.N && q < da) ? X[(size_t)t * d + act[q]] - mean[q] : 0.0;
  }
}

// ============================================================================================
// Leaf of the recursion: Cholesky of the 64x64 diagonal tile jt (already reduced by the SYRK
// updates of its ancestors) and its inverse, one workgroup (4 waves) per slot, blocked by 16:
// the 16x16 diagonal blocks are factored and inverted in registers by wave 0 (lane = row /
// column, pivots and row values broadcast by readlane), the panel TRSM / trailing SYRK and the
// off-diagonal blocks of the inverse run on the MFMA pipe from an LDS image of the tile.
// 4 + 3 barrier-separated phases per panel instead of 128 steps.
//   panel P (c0 = 16P):  D = chol(A_PP), Dinv = D^-1               (wave 0)
//                        A_iP <- A_iP Dinv^T  (i > P)              (TRSM, one wave per block)
//                        A_ij -= A_iP A_jP^T  (i >= j > P)          (SYRK)
//   inverse:  X_PP = Dinv_P ;  X_ij = -Dinv_i sum_{k=j}^{i-1} L_ik X_kj   by sub-diagonal i - j
// Failure (first pivot <= 0 or NaN, as LAPACK dpotrf) records status 1 and the 1-based global
// pivot index and continues with pivot 1.  Writes Linv[jt,jt] = L_jj^-1 and Mt[jt,jt] = L_jj^-T
// (full tiles, explicit zeros) and the tile's sum_c log L_cc.
// 16x16x4 f64 MFMA operand maps (gfx950): A lane l = A[l&15][l>>4], B lane l = B[l>>4][l&15],
// D lane l reg q = D[(l>>4) + 4q][l&15].
// ============================================================================================
constexpr int FS = TS + 1;  // LDS column stride of the tile images
// LDS of the diagonal routine (the caller's): T[c*FS + r] = A[r][c], then L (lower); Xi[c*FS + r]
// = X[r][c] = (L^-1)[r][c] (the inverse stays there until the next call); cbs: [256] scratch.
// t_ready: T already holds the tile's lower triangle (zeros above), written by the caller; else
// it is read from Ksrc (K, or S when a SYRK updated it).
__device__ __forceinline__ void diag_tile_fast(const DevBatch& db, int slot, int jt, double* T, double* Xi, double* cbs,
                                               bool t_ready, const double* Ksrc, bool store = true);
__device__ __forceinline__ void diag_store(const DevBatch& db, int slot, int jt, const double* Xi, double* cbs);
__global__ __launch_bounds__(NTHR) void k_diag_f(DevBatch db, int jt, int upd) {
  __shared__ double T[TS * FS], Xi[TS * FS];
  __shared__ __attribute__((aligned(16))) double cbs[256];
  if (slot_active(db, blockIdx.x)) diag_tile_fast(db, blockIdx.x, jt, T, Xi, cbs, false, upd ? db.S : db.K);
}
__device__ __forceinline__ void diag_tile_fast(const DevBatch& db, int slot, int jt, double* T, double* Xi, double* cbs,
                                               bool t_ready, const double* Ksrc, bool store) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lk = l >> 4;
  const size_t ld = db.ld;
  const double* A = Ksrc + (size_t)slot * db.mat + (size_t)jt * TS * ld + jt * TS;
  if (!t_ready) {  // all 16 loads of a thread in flight before the LDS stores (one latency, not 16)
    double v[TS * TS / NTHR];
#pragma unroll
    for (int k = 0; k < TS * TS / NTHR; ++k) {
      const int e = tid + k * NTHR, r = e & 63, c = e >> 6;
      v[k] = (r >= c) ? A[(size_t)c * ld + r] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < TS * TS / NTHR; ++k) {
      const int e = tid + k * NTHR, r = e & 63, c = e >> 6;
      T[c * FS + r] = v[k];
    }
  }
  for (int e = tid; e < TS * TS; e += NTHR) Xi[(e >> 6) * FS + (e & 63)] = 0.0;
  __syncthreads();
  int fail = -1;
  double lsum = 0.0;  // wave 0: sum log l_jj
  for (int P = 0; P < 4; ++P) {
    const int c0 = 16 * P;
    if (w == 0) {
      // ---- factor and invert the diagonal block together, by elimination on 16 lanes: lane i
      //      holds row i of the block (a[k] = A[c0+i][c0+k], becoming L) and column i of its
      //      inverse (y[m] = X[m][i], starting from the identity).  Step j scales column j of L and
      //      row j of X by 1/l_jj, then L[m][j] (lane m's a[j]) is broadcast to the row of 16 lanes
      //      by DPP (row_newbcast: no LDS round trip) and updates both A (a[m] -= L[i][j] L[m][j])
      //      and X (X[m][i] -= L[m][j] X[j][i]).  The operations and their order are those of the
      //      column-by-column factor followed by the row-oriented forward substitution, so the
      //      results are bit-identical to that form. ----
      double a[16], y[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        a[k] = T[(c0 + k) * FS + c0 + lr];
        y[k] = (k == lr) ? 1.0 : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double p = readlane_d(a[j], j);
        const double pk = (p > 0.0) ? p : 1.0;
        if (!(p > 0.0) && fail < 0) fail = c0 + j;
        double ljj, rj;
        sqrt_rsqrt(pk, ljj, rj);
        a[j] = (lr > j) ? a[j] * rj : (lr == j ? ljj : 0.0);
        y[j] = y[j] * rj;
#pragma unroll
        for (int m = j + 1; m < 16; ++m) {
          const double b = row_bcast16(a[j], m);  // L[m][j]
          a[m] = fma(-a[j], b, a[m]);
          y[m] = fma(-b, y[j], y[m]);
        }
      }
      double (&x)[16] = y;
      if (l < 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k) T[(c0 + k) * FS + c0 + l] = (k <= l) ? a[k] : 0.0;  // row l of L_PP
      }
      __builtin_amdgcn_wave_barrier();
      if (l < 16) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Xi[(c0 + l) * FS + c0 + r] = x[r];    // column l of Dinv
      }
    }
    __syncthreads();
    // ---- TRSM: block row i > P:  A_iP <- A_iP Dinv^T   (D[r][c] = sum_k A_iP[r][k] Dinv[c][k]) ----
    {
      const int i = P + 1 + w;
      if (i < 4) {
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = 4 * s + lk;
          const double av = T[(c0 + k) * FS + 16 * i + lr];   // A_iP[lr][k]
          const double bv = Xi[(c0 + k) * FS + c0 + lr];      // B[k][j=lr] = Dinv[lr][k]
          acc = mfma(av, bv, acc);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) T[(c0 + lr) * FS + 16 * i + lk + 4 * q] = acc[q];  // D[lk+4q][lr]
      }
    }
    __syncthreads();
    // ---- SYRK: A_ij -= A_iP A_jP^T for P < j <= i < 4 ----
    {
      const int m = 3 - P;  // trailing blocks per edge
      for (int t = w; t < m * (m + 1) / 2; t += 4) {
        int u = t, j = 0;
        while (u >= m - j) {
          u -= m - j;
          ++j;
        }
        const int bj = P + 1 + j, bi = bj + u;
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = 4 * s + lk;
          const double av = T[(c0 + k) * FS + 16 * bi + lr];  // A_iP[lr][k]
          const double bv = T[(c0 + k) * FS + 16 * bj + lr];  // B[k][lr] = A_jP[lr][k]
          acc = mfma(av, bv, acc);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          double* pp = &T[(16 * bj + lr) * FS + 16 * bi + lk + 4 * q];
          *pp = *pp - acc[q];
        }
      }
    }
    __syncthreads();
  }
  // ---- off-diagonal blocks of the inverse, by sub-diagonal s = i - j ----
  for (int sd = 1; sd < 4; ++sd) {
    const int j = w, i = w + sd;
    if (i < 4) {
      // Y = sum_{k=j}^{i-1} L_ik X_kj
      d4 y = (d4){0.0, 0.0, 0.0, 0.0};
      for (int kb = j; kb < i; ++kb)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = 4 * s + lk;
          const double av = T[(16 * kb + k) * FS + 16 * i + lr];    // L_ik[lr][k]
          const double bv = Xi[(16 * j + lr) * FS + 16 * kb + k];   // X_kj[k][lr]
          y = mfma(av, bv, y);
        }
      // X_ij = -Dinv_i Y ; Y's D layout (reg q = Y[lk+4q][lr]) is the B operand of k-chunk q
      d4 x = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double av = Xi[(16 * i + 4 * s + lk) * FS + 16 * i + lr];  // Dinv_i[lr][4s+lk]
        x = mfma(av, y[s], x);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) Xi[(16 * j + lr) * FS + 16 * i + lk + 4 * q] = -x[q];
    }
    __syncthreads();
  }
  if (w == 0) {  // fail: uniform over wave 0; sum log l_jj from the diagonal of T, one per lane
    lsum = wave_sum(log(T[l * FS + l]));
    if (l == 0) {
      db.logdet_part[(size_t)slot * db.nt + jt] = lsum;
      if (fail >= 0 && db.status[slot] == 0) {
        db.status[slot] = 1;
        db.info[slot] = jt * TS + fail + 1;
      }
    }
  }
  if (store) diag_store(db, slot, jt, Xi, cbs);
}
// The diagonal routine's results to HBM: Linv[jt,jt], Mt[jt,jt] and the tile's z partial, from the
// inverse image Xi (LDS).  The fused leaf issues them after its TRSM tasks' loads: issued first, the
// stores sat ahead of those loads in the in-order counter and zp_diag's barriers drained them.
__device__ __forceinline__ void diag_store(const DevBatch& db, int slot, int jt, const double* Xi, double* cbs) {
  const int tid = threadIdx.x;
  const size_t ld = db.ld;
  double* Li = db.Linv + (size_t)slot * db.mat + (size_t)jt * TS * ld + jt * TS;
  double* Mj = db.Mt + (size_t)slot * db.mat + (size_t)jt * TS * ld + jt * TS;
  for (int e = tid; e < TS * TS; e += NTHR) {
    const int r = e & 63, c = e >> 6;
    const double v = (r >= c) ? Xi[c * FS + r] : 0.0;
    Li[(size_t)c * ld + r] = v;                              // Linv[r][c]
    Mj[(size_t)c * ld + r] = (c >= r) ? Xi[r * FS + c] : 0.0;  // Mt[r][c] = X[c][r]
  }
  zp_diag(db, slot, jt, Xi, 1, FS, cbs);
}

}  // namespace gprx

// Here rather than at the top: non-template kernels land in the code object in definition order,
// and k_center and k_diag_f precede the GEMM and fused-node kernels there.
#include "gprx_gemm.h"
#include "gprx_factor.h"

namespace gprx {

// ============================================================================================
// z = L^-1 y by forward substitution over the blocks, alpha = L^-T z.  Around every block [lo, lo + n)
// of the recursion (blk_range; factor_rec launches them):
//   k_rhs   : Yw = y + sum_{h < 2 lo} zp_row(h), the partials -L[i,tj] z[tj] the split nodes' TRSMs
//             wrote left of the block.  The first block's is a copy of y, launched all the same:
//             Yw carries nothing from one evaluation to the next.                      grid = B * n
//   k_znode : z = sum_{h = 2 lo}^{2(i+1)-1} zp_row(h), the block's own partials.          grid = B * n
// and once per evaluation
//   k_alpha : alpha = Mt z inside each block + the split nodes' LINV21 partials ap.     grid = B * nt
// The partials are summed in a fixed order: thread group pt takes every fourth row, then the four
// groups' sums in order.
// ============================================================================================
__device__ __forceinline__ double zp_sum(const DevBatch& db, int slot, int i, int h0, int h1, double (&part)[4][TS]) {
  const int r = threadIdx.x & 63, pt = threadIdx.x >> 6;
  double acc = 0.0;
  for (int h = h0 + pt; h < h1; h += 4) acc += zp_row(db, slot, h)[i * TS + r];
  part[pt][r] = acc;
  __syncthreads();
  return ((part[0][r] + part[1][r]) + part[2][r]) + part[3][r];
}
__global__ __launch_bounds__(NTHR) void k_rhs(DevBatch db, int lo, int n) {
  __shared__ double part[4][TS];
  int slot, u;
  if (!map_slot(db, n, slot, u)) return;
  const int i = lo + u, r = threadIdx.x & 63;
  const double s = zp_sum(db, slot, i, 0, 2 * lo, part);
  const size_t e = (size_t)slot * db.Npad + i * TS + r;
  if (threadIdx.x < TS) yw_slot(db, slot)[i * TS + r] = lo ? db.Y[e] + s : db.Y[e];
}
__global__ __launch_bounds__(NTHR) void k_znode(DevBatch db, int lo, int n) {
  __shared__ double part[4][TS];
  int slot, u;
  if (!map_slot(db, n, slot, u)) return;
  const int i = lo + u, r = threadIdx.x & 63;
  const double s = zp_sum(db, slot, i, 2 * lo, 2 * (i + 1), part);
  if (threadIdx.x < TS) db.z[(size_t)slot * db.Npad + i * TS + r] = s;
}
__global__ __launch_bounds__(NTHR) void k_alpha(DevBatch db) {
  __shared__ double part[4][TS];
  int slot, i;
  if (!map_slot(db, db.nt, slot, i)) return;
  const int r = threadIdx.x & 63, pt = threadIdx.x >> 6;
  int blo, bhi;
  blk_range(db.nt, i, blo, bhi);
  // the partials from below the block first: their loads are in flight under the Mt stream
  __shared__ double apart[4][TS];
  {
    double a = 0.0;
    for (int ti = bhi + pt; ti < db.nt; ti += 4) a += ap_row(db, slot, ti)[i * TS + r];
    apart[pt][r] = a;
  }
  const size_t ld = db.ld;
  // lane: rows 2 rp, 2 rp + 1 of the tile row (one 16-B load), columns of parity cp: one load
  // instruction reads two whole 512-B column segments.  The column range [k0, end of the block) is
  // split in 4 contiguous quarters of whole 16-column groups (wave-uniform, so z comes in by scalar
  // loads).
  const int rp = r & 31, cp = r >> 5, w = __builtin_amdgcn_readfirstlane(pt);
  const double* A = db.Mt + (size_t)slot * db.mat + i * TS + 2 * rp + (size_t)cp * ld;
  const double* v = db.z + (size_t)slot * db.Npad;
  const int k0 = i * TS, k1 = bhi * TS;
  const int ng = (k1 - k0) / 16, g0 = (ng * w) / 4, g1 = (ng * (w + 1)) / 4;
  typedef double d2 __attribute__((ext_vector_type(2)));
  d2 acc[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
  // group gq + 1's loads are issued before group gq's arithmetic (16 loads in flight per lane)
  d2 m[8];
  if (g0 < g1) {
#pragma unroll
    for (int u = 0; u < 8; ++u) m[u] = *(const d2*)(A + (size_t)(k0 + 16 * g0 + 2 * u) * ld);
  }
  for (int gq = g0; gq < g1; ++gq) {
    const int kk = k0 + 16 * gq;
    d2 mn[8];
    if (gq + 1 < g1) {
#pragma unroll
      for (int u = 0; u < 8; ++u) mn[u] = *(const d2*)(A + (size_t)(kk + 16 + 2 * u) * ld);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double zv = cp ? v[kk + 2 * u + 1] : v[kk + 2 * u];
      acc[u & 3].x = fma(m[u].x, zv, acc[u & 3].x);
      acc[u & 3].y = fma(m[u].y, zv, acc[u & 3].y);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) m[u] = mn[u];
  }
  double s0 = (acc[0].x + acc[1].x) + (acc[2].x + acc[3].x), s1 = (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y);
  s0 = sum_xor32(s0);  // the other column parity
  s1 = sum_xor32(s1);
  if (cp == 0) {
    part[pt][2 * rp] = s0;
    part[pt][2 * rp + 1] = s1;
  }
  __syncthreads();
  if (pt == 0) {
    double s = ((part[0][r] + part[1][r]) + part[2][r]) + part[3][r];
    if (bhi < db.nt) s += ((apart[0][r] + apart[1][r]) + apart[2][r]) + apart[3][r];
    db.alpha[(size_t)slot * db.Npad + i * TS + r] = s;
  }
}

// ============================================================================================
// K^-1 lower tiles = Mt_i Mt_j^T (K range [i, nt)), fused with the gradient partial sums
//   G_rc = wt_rc * (alpha_r alpha_c - Kinv_rc) * Kf_rc    (wt = 1/2 on the diagonal, as
//                                                        dmll_kern! weights ααinvcKI[j,j]/2)
//   S_p = sum G_rc (x_pr - x_pc)^2,  S_f = sum G_rc,  T = sum_diag W_rr
// One gradient partial row per unit of 4 tiles.  Kf is K's lower tile (ti, tj) exactly as the Gram
// wrote it (the factorisation's SYRKs write S, never K), read once per output tile; only entries
// with gi > gj are used, so the noise on the diagonal is never seen: G_rr uses sf2 analytically.
//
// The distance sums are expanded per wave tile (rows r, columns c):
//   S_p = sum_r x_pr^2 R_r + sum_c x_pc^2 C_c - 2 sum_r x_pr Q_rp,   Q = G Xc  (64 x da)
// over the da active dimensions only (DevBatch::da: a dimension that is constant has S_p = 0).  Each
// S_p is its own MFMA column and its own reductions, so it does not depend on which others are there.
// with R / C the row / column sums of G.  Q runs on the MFMA pipe with G straight from the
// accumulators as the B operand (the swapped-operand C layout of mma_64x32_s1 is exactly a B
// fragment), so the epilogue costs ~2d MFMAs + a few dozen cross-lane sums per wave instead of
// 32 d distance evaluations and d wave reductions.  x is the centred copy Xc (per-dimension mean
// removed; S_p is translation invariant), which keeps the expansion's cancellation at the
// rounding level of the points' spread, as for the reference's own a^2 + b^2 - 2ab distances.
// LDS: the unit's point tiles as raw [point][xs] images (LDS-DMA, issued after the MFMA loop),
// per-wave partials and alpha of the image points.
// ============================================================================================
__device__ __forceinline__ void dma_tile(double* lds, const double* src, int ndbl) {
  // ndbl doubles (even) from src to lds, 16 B per lane, one wave-instruction per KiB;
  // the LDS destination of each instruction is wave-uniform (M0), lane i writes base + 16 i
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nch = ndbl >> 1;
  for (int c0 = w * 64; c0 < nch; c0 += NTHR) {
    if (c0 + l < nch)
      __builtin_amdgcn_global_load_lds((const void*)(src + 2 * (c0 + l)),
                                       (__attribute__((address_space(3))) void*)(lds + 2 * c0), 16, 0, 0);
  }
}
constexpr int SPW = DMAX + 2;  // per-wave partial row: S_p (d), S_f, T
// LDS of a lauum workgroup: per-wave partials, alpha of the image points, then nimg point-tile
// images [64][xs] (16-B aligned: the small arrays hold an even count)
static_assert((4 * SPW + 5 * TS) % 2 == 0, "lauum LDS image base alignment");
__host__ __device__ inline size_t lauum_lds_dbl(int xs, int nimg) {
  return (size_t)4 * SPW + 5 * TS + (size_t)nimg * TS * xs;
}
// Unit = 4 output tiles of the lower triangle, one per wave, each with its own K range [ti, nt)
// (register-direct operands: the waves share no panel, only the unit's point-tile images for the
// epilogue).  Job table entry per unit (LU ints):
//   [0] unit id (-1: none)  [1] nimg  [2..6] image tiles  [7..10] ti per wave (-1: idle)
//   [11..14] tj  [15..18] image of ti  [19..22] image of tj
// The plan (lauum_plan) takes the lower tiles in row order, four consecutive tiles per unit: the
// waves' K ranges differ by at most one tile (99% of the wave time is MFMA work at nt = 32,
// against 92% for 2 x 2 units, whose diagonal units leave a wave idle and whose second tile row
// has 64 less K).  Such a unit needs up to 5 images (row tiles and column tiles); where 5 images
// would cost a workgroup per CU against 4 (d > 26 at two per CU, d > 63 at one), the plan falls
// back to 2 x 2 units.
__device__ __forceinline__ void lauum_unit(const DevBatch& db, int slot, const int* ju);
__device__ __forceinline__ void lauum_body(const DevBatch& db) {
  int slot, job;
  if (!map_slot(db, db.nlj, slot, job)) return;
  const int* jb = db.lauum_order + (size_t)job * 2 * LU;
  GTS_L(0);
  const int nu = jb[LU] >= 0 ? 2 : 1;  // block-uniform: the folded short unit
  // every workgroup takes its long unit first (staggering the order between the two workgroups
  // of a CU measured no gain: DESIGN.md, "Gradient jobs staggered")
  lauum_unit(db, slot, jb);
  if (nu == 2) {
    __syncthreads();  // the first unit's LDS images and partials are consumed
    lauum_unit(db, slot, jb + LU);
  }
}
// One gradient unit, stated once for k_lauum_grad and k_loo_grad (gprx_loograd.h): wave w forms its
// tile m of (ti, tj) = (ju[7 + w], ju[11 + w]) with product(acc, ti, tj, ld, so), the workgroup brings
// in the unit's point images by LDS-DMA, and the epilogue of the banner above reduces
//   G_rc = wt_rc * W_rc * Kf_rc,   W_rc = wf(alpha_r, alpha_c, gi, gj, m_rc)   (gi, gj: global row, column)
// to the unit's partial row part[slot][ju[0]][0 .. da + 1] = [S_p of the da active dimensions, S_f, T].
// Only the two callables differ between the kernels; with lauum_unit's k_lauum_grad compiles to the
// instructions it had when this text stood in lauum_unit (an epilogue cut out on its own did not: its
// main loop waited on coarser load counts and ran 1% slower, profiles/shared_epilogue_ab.txt).
// Every wave of the workgroup calls (the barriers are workgroup-uniform); an idle wave (ti < 0) adds
// zeros.  Reduction order, fixed: a lane's elements in (a, b, q) order, the lanes by wave_sum /
// row_sum16 / xor 16, 32, then the four waves' rows in order.  The diagnostic builds' marks (GTS_*,
// GPRX_STAMPS) ride along in both kernels; their scripts launch the evaluation alone.
template <class PF, class WF>
__device__ __forceinline__ void grad_unit(const DevBatch& db, int slot, const int* ju, double* part, PF product, WF wf) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  // d: the active dimensions (Xc's columns, the S_p of a partial row)
  const int d = db.da, tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xs = db.xs, xt = TS * xs;  // point-tile image: [64][xs]
  const int nimg = ju[1];
  double* sp = sm;                      // [4][SPW]
  double* als = sp + 4 * SPW;           // [nimg][64] alpha of the image points
  double* img = als + 5 * TS;           // [nimg][64][xs]
  const double* X = db.Xc + (size_t)slot * db.Npad * xs;
  const double* al = db.alpha + (size_t)slot * db.Npad;
  const int ti = ju[7 + w], tj = ju[11 + w];
  const bool active = ti >= 0;
  const int l = tid & 63, lr = l & 15, lk = l >> 4;
  d4 acc[QM][QN];
  acc4_zero(acc);
  const size_t ld = db.ld, so = (size_t)slot * db.mat;
#ifdef GPRX_STAMPS
  const Stamp st0 = stamp_now();
#endif
  [[maybe_unused]] const int gu = (ju - db.lauum_order) % (2 * LU) == 0 ? 0 : 1;  // the job's first or second unit
  GTS_L(1 + 3 * gu);
  if (active) product(acc, ti, tj, ld, so);  // wave-uniform
  GTS_L(2 + 3 * gu);
#ifdef GPRX_STAMPS
  if (active && (ju - db.lauum_order) % (2 * LU) == 0) {  // the job's first (long) unit
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp_store(0, st0, stamp_now());
  }
#endif
  // the unit's point images by LDS-DMA after the main loop: issued before it, they sit ahead of
  // the first stage's loads in the wave's in-order load counter and delay the first MFMA
  for (int i = 0; i < nimg; ++i) dma_tile(img + i * xt, X + (size_t)ju[2 + i] * xt, xt);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-DMA landed
  __syncthreads();                                   // ... and every other wave's
  GTS_D(gu, 4);
  double sf = 0.0, tr = 0.0;
  double* spw = sp + w * SPW;
  for (int e = l; e < SPW; e += 64) spw[e] = 0.0;
  const double* P = db.params + (size_t)slot * db.pst;
  for (int e = tid; e < nimg * TS; e += NTHR) als[e] = al[ju[2 + (e >> 6)] * TS + (e & 63)];
  __syncthreads();
  GTS_D(gu, 5);
  if (active) {
    const double sf2 = P[db.d];
    const int ir = ju[15 + w], ic = ju[19 + w];
    const double* xr = img + ir * xt;  // [r][xs]
    const double* xc = img + ic * xt;  // [c][xs]
    const double* ar = als + ir * TS;
    const double* ac = als + ic * TS;
    // G in place of acc, with Kf read from K's lower tile (ti, tj) as the Gram wrote it (the same
    // kernel values the factorisation used); only gi > gj is used: the diagonal (Kf + noise) is
    // never loaded, G_rr = W_rr sf2 / 2 analytically
    const double* Kf = db.K + so + (size_t)(tj * TS) * ld + ti * TS;
    const size_t ldk = ld;
#pragma unroll
    for (int a = 0; a < QM; ++a) {
      double kf[QN][4];
#pragma unroll
      for (int b = 0; b < QN; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) kf[b][q] = Kf[(size_t)(16 * b + lk + 4 * q) * ldk + 16 * a + lr];
#pragma unroll
      for (int b = 0; b < QN; ++b) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = 16 * a + lr, c = 16 * b + lk + 4 * q;
          const int gi = ti * TS + r, gj = tj * TS + c;
          double G = 0.0;
          if (gi < db.N && gj < db.N && gi >= gj) {
            const double W = wf(ar[r], ac[c], gi, gj, acc[a][b][q]);
            if (gi == gj) {
              G = 0.5 * (W * sf2);
              tr += W;
            } else {
              G = W * kf[b][q];
            }
            sf += G;
          }
          acc[a][b][q] = G;
        }
      }
    }
    GTS_D(gu, 6);
    // row sums R (row 16a + lr over the tile's 64 columns), column sums C (column 16b + lk + 4q
    // over the 64 rows)
    double R[QM], Cs[QN][4];
#pragma unroll
    for (int a = 0; a < QM; ++a) {
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < QN; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) s += acc[a][b][q];
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      R[a] = s;
    }
#pragma unroll
    for (int b = 0; b < QN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        Cs[b][q] = row_sum16((acc[0][b][q] + acc[1][b][q]) + (acc[2][b][q] + acc[3][b][q]));
      }
    const int H = (d + 15) >> 4;
#pragma unroll 1
    for (int h = 0; h < H; ++h) {
      // A operand: x of column point c = 16b + 4q + lk, dimension pA = 16h + lr (clamped to a
      // finite image value for pA >= d: those Q columns and t2 lanes are never stored)
      const int pA = 16 * h + lr, pAc = pA < d ? pA : d - 1;
      double xa[QN][4];
      double t2 = 0.0;  // sum_c x_{pA,c}^2 C_c over this lane's 16 columns
#pragma unroll
      for (int b = 0; b < QN; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          xa[b][q] = xc[(16 * b + 4 * q + lk) * xs + pAc];
          t2 = fma(xa[b][q] * xa[b][q], Cs[b][q], t2);
        }
      double t13[4] = {0.0, 0.0, 0.0, 0.0};  // dims p = 16h + lk + 4q'
#pragma unroll
      for (int a = 0; a < QM; ++a) {
        d4 Q = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int b = 0; b < QN; ++b)
#pragma unroll
          for (int q = 0; q < 4; ++q) Q = mfma(xa[b][q], acc[a][b][q], Q);
        // lane: row r = 16a + lr; Q[q'] = Q[r][16h + lk + 4q']
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int p = 16 * h + lk + 4 * qq;
          const double x = xr[(16 * a + lr) * xs + (p < d ? p : d - 1)];
          t13[qq] = fma(x, fma(x, R[a], -2.0 * Q[qq]), t13[qq]);
        }
      }
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) t13[qq] = row_sum16(t13[qq]);
      t2 += __shfl_xor(t2, 16);
      t2 += __shfl_xor(t2, 32);
      if (lr == 0) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int p = 16 * h + lk + 4 * qq;
          if (p < d) spw[p] = t13[qq];
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (lk == 0 && pA < d) spw[pA] += t2;
      __builtin_amdgcn_wave_barrier();
    }
  }
  GTS_D(gu, 7);
  sf = wave_sum(sf);
  tr = wave_sum(tr);
  if (l == 0) {
    spw[d] = sf;
    spw[d + 1] = tr;
  }
  __syncthreads();
  double* out = part + ((size_t)slot * db.ngu + ju[0]) * db.gps;
  for (int e = tid; e < d + 2; e += NTHR)
    out[e] = ((sp[e] + sp[SPW + e]) + sp[2 * SPW + e]) + sp[3 * SPW + e];
  GTS_L(3 + 3 * gu);
}
__device__ __forceinline__ void lauum_unit(const DevBatch& db, int slot, const int* ju) {
  grad_unit(
      db, slot, ju, db.grad_part,
      [&db](d4 (&acc)[QM][QN], int ti, int tj, size_t ld, size_t so) {  // diagonal tiles form only their lower blocks
        const int nt = db.nt;
        const double* Ap = db.Mt + so + (size_t)ti * TS * ld + ti * TS;
        // global addressing here: the buffer-load form (k_gemm's) measured 0.15 ms slower in this kernel
        // (11.60 / 11.66 / 11.53 against 11.41 / 11.47 / 11.44 ms, same box, bit-identical output)
        if (ti == tj) mma_64x64_m<TRI_AB_FIRST>(acc, Ap, ld, Ap, ld, (nt - ti) * TS);
        else mma_64x64_m<TRI_A_FIRST>(acc, Ap, ld, db.Mt + so + (size_t)ti * TS * ld + tj * TS, ld, (nt - ti) * TS);
      },
      [](double alr, double alc, int, int, double m) { return alr * alc - m; });
}
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_lauum_grad(DevBatch db) {
  lauum_body(db);
}
// workgroups per CU that an LDS size allows (2 at most: the kernel's VGPRs)
static int lauum_wgs(size_t bytes) {
  const size_t cu = 160 * 1024;
  return bytes > cu ? 0 : (int)std::min<size_t>(2, cu / bytes);
}
int lauum_plan(int nt, int d, int* nunits, int* nimg, int* out) {
  const int xs = d | 1;
  const size_t b4 = lauum_lds_dbl(xs, 4) * sizeof(double), b5 = lauum_lds_dbl(xs, 5) * sizeof(double);
  const bool rows = lauum_wgs(b5) >= lauum_wgs(b4) && lauum_wgs(b5) > 0;
  // units in decreasing K order (K = nt - first row), each as its 4 (ti, tj) (ti = -1: idle wave)
  std::vector<std::array<int, 8>> us;
  if (rows) {
    std::vector<std::pair<int, int>> t;
    for (int i = 0; i < nt; ++i)
      for (int j = 0; j <= i; ++j) t.push_back({i, j});
    for (size_t k = 0; k < t.size(); k += 4) {
      std::array<int, 8> u;
      for (int w = 0; w < 4; ++w) {
        const bool in = k + w < t.size();
        u[w] = in ? t[k + w].first : -1;
        u[4 + w] = in ? t[k + w].second : -1;
      }
      us.push_back(u);
    }
  } else {
    for (int pr = 0; pr < nt; pr += 2)
      for (int pc = 0; pc <= pr; pc += 2) {
        std::array<int, 8> u;
        for (int w = 0; w < 4; ++w) {
          const int i = pr + (w >> 1), j = pc + (w & 1);
          const bool in = i < nt && j <= i;
          u[w] = in ? i : -1;
          u[4 + w] = in ? j : -1;
        }
        us.push_back(u);
      }
  }
  const int n = (int)us.size(), nj = (n + 1) / 2;
  *nunits = n;
  *nimg = 0;
  auto fill = [&](int* e, int id) {  // one LU-int entry of unit id (-1: none)
    for (int k = 0; k < LU; ++k) e[k] = -1;
    if (id < 0) return;
    const std::array<int, 8>& u = us[id];
    int img[8], ni = 0;
    auto slot_of = [&](int tile) {
      for (int k = 0; k < ni; ++k)
        if (img[k] == tile) return k;
      img[ni] = tile;
      return ni++;
    };
    e[0] = id;
    for (int w = 0; w < 4; ++w) {
      e[7 + w] = u[w];
      e[11 + w] = u[4 + w];
      if (u[w] >= 0) {
        e[15 + w] = slot_of(u[w]);
        e[19 + w] = slot_of(u[4 + w]);
      }
    }
    e[1] = ni;  // <= 5: at most 2 row tiles (2 x 2: 2 rows, 2 columns) and 4 column tiles
    for (int k = 0; k < ni && k < 5; ++k) e[2 + k] = img[k];
    if (ni > 5) e[1] = -1;  // not reached; lauum_plan returns -1
    *nimg = std::max(*nimg, ni);
  };
  std::vector<int> tmp(2 * LU);
  for (int j = 0; j < nj; ++j) {
    const int a = j, b = (n - 1 - j != j) ? n - 1 - j : -1;  // the j-th longest + the j-th shortest
    int* e = out ? out + (size_t)j * 2 * LU : tmp.data();
    fill(e, a);
    fill(e + LU, b);
    if (e[1] < 0 || (b >= 0 && e[LU + 1] < 0)) return -1;
  }
  return nj;
}

// The unit partial rows gp[ngu][gps] of a slot (grad_unit's: S_p of the da active dimensions, S_f,
// T) reduced into out[1 .. d + 2] = the gradient in GaussianProcesses order [log sn, log ell_1..d,
// log sf], for k_finalize and k_loo_grad_final.  Deterministic: 4 waves x 64 lanes stride the units,
// one parameter at a time, wave_sum, then the four waves in order.  Called by the whole workgroup in
// workgroup-uniform control flow (two barriers a parameter).
__device__ __forceinline__ void grad_reduce(const DevBatch& db, int slot, const double* gp, double* out) {
  __shared__ double pr[4];
  const int tid = threadIdx.x, d = db.d;
  const double* P = db.params + (size_t)slot * db.pst;
  // a partial row holds the S of the da active dimensions; a dropped (constant) dimension's
  // distances are all 0 and so is its derivative, exactly (NaN where the distances are: P[d + 3])
  const int da = db.da;
  if (da < d)
    for (int e = tid; e < d; e += NTHR) out[2 + e] = P[d + 3];  // ordered before thread 0's by the barriers below
  int pn = 0;  // thread 0: the next dimension to look at
  for (int q = 0; q < da + 2; ++q) {
    double tot = 0.0;
    for (int t = tid; t < db.ngu; t += NTHR) tot += gp[(size_t)t * db.gps + q];
    tot = wave_sum(tot);
    __syncthreads();
    if ((tid & 63) == 0) pr[tid >> 6] = tot;
    __syncthreads();
    if (tid == 0) {
      tot = ((pr[0] + pr[1]) + pr[2]) + pr[3];
      int p = 0;
      if (q < da) {  // the q-th active dimension
        while (pn < d - 1 && !((db.amask >> pn) & 1)) ++pn;
        p = pn < d - 1 ? pn++ : pn;
      }
      if (q < da) out[2 + p] = P[p] * tot;       // d / d log ell_p = il2_p * S_p
      else if (q == da) out[2 + d] = 2.0 * tot;  // d / d log sf    = 2 S_f
      else out[1] = P[d + 2] * tot;             // d / d log sn    = sn2 T  (T = tr(W))
    }
  }
}

// ============================================================================================
// Per slot: mll = -(y.alpha + logdet + N log 2pi)/2 ; gradient (d+2) in GaussianProcesses order
// [log sn, log ell_1..d, log sf].  grid = B
// ============================================================================================
__global__ __launch_bounds__(NTHR) void k_finalize(DevBatch db, int want_grad) {
  __shared__ double red[4];
  const int slot = blockIdx.x, tid = threadIdx.x, d = db.d;
  if (!slot_active(db, slot)) return;
  const double* y = db.Y + (size_t)slot * db.Npad;
  const double* al = db.alpha + (size_t)slot * db.Npad;
  double s = 0.0;
  for (int k = tid; k < db.N; k += NTHR) s = fma(y[k], al[k], s);
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  double* out = db.out + (size_t)slot * (d + 3);
  if (tid == 0) {
    const double ya = ((red[0] + red[1]) + red[2]) + red[3];
    double ldt = 0.0;
    for (int k = 0; k < db.nt; ++k) ldt += db.logdet_part[(size_t)slot * db.nt + k];
    const double log2pi = 1.8378770664093453;  // log(2pi), Julia's log2π
    out[0] = -((ya + 2.0 * ldt) + log2pi * db.N) / 2.0;
  }
  if (want_grad) grad_reduce(db, slot, db.grad_part + (size_t)slot * db.ngu * db.gps, out);
}

// ============================================================================================
// Prediction.
//   pred_cross: K*^T tile (64 test x 64 train) + partial means over the train tile.
//               grid = B * nt * mt
//   (pred_var : OP_PREDVAR of k_gemm, V = Linv K*, column sums of V^2)
//   pred_final: mu = sum mu_part, var = max(sf2 - sum var_part, 0).       grid = B
// ============================================================================================
template <int MODE>
__global__ __launch_bounds__(NTHR) void k_pred_cross(DevBatch db) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ __attribute__((aligned(16))) double tab[128];  // exp_sf's table, as k_gram
  const int d = db.d, tid = threadIdx.x;
  double* xt = sm;
  double* xs = sm + d * CS;
  double* pw = sm + 2 * d * CS;
  int slot, t;
  if (!map_slot(db, db.nt * db.mt, slot, t)) return;
  const int ch = t / db.mt, mtile = t - ch * db.mt;
  const double* X = db.X + (size_t)slot * db.Npad * d;
  const double* Xq = db.Xs + (size_t)slot * db.Mpad * d;
  const double* P = db.params + (size_t)slot * db.pst;
  double* sc = pw + DMAX + 4;  // as k_gram (sqrt(il2 / 2): the sums are r/2)
  if (MODE == 1) {
    for (int e = tid; e < d; e += NTHR) sc[e] = sqrt(0.5 * P[e]);
    __syncthreads();
  }
  {  // as k_gram: no per-element division, buffer loads
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(X, db.Npad * d * (int)sizeof(double));
    const __amdgpu_buffer_rsrc_t qr = buffer_rsrc(Xq, db.Mpad * d * (int)sizeof(double));
    const int bi = ch * TS * d * (int)sizeof(double), bj = mtile * TS * d * (int)sizeof(double);
    const int os = 8 * d * (int)sizeof(double);
    for (int p = tid & 31; p < d; p += 32) {
      const double s = MODE == 1 ? sc[p] : 1.0;
      double vi[TS / 8], vj[TS / 8];
      const int o0 = ((tid >> 5) * d + p) * (int)sizeof(double);
#pragma unroll
      for (int m = 0; m < TS / 8; ++m) {
        vi[m] = buffer_load_f64(xr, o0, bi + m * os);
        vj[m] = buffer_load_f64(qr, o0, bj + m * os);
      }
#pragma unroll
      for (int m = 0; m < TS / 8; ++m) {
        const int r = (tid >> 5) + 8 * m;
        xt[p * CS + r] = vi[m] * s;
        xs[p * CS + r] = vj[m] * s;
      }
    }
  }
  for (int e = tid; e < d + 3; e += NTHR) pw[e] = P[e];
  if (tid < 64) {  // as k_gram
    const double s2 = P[d], h = g_exp2tab[2 * tid], lo = g_exp2tab[2 * tid + 1];
    const double th = s2 * h;
    tab[2 * tid] = th;
    tab[2 * tid + 1] = fma(s2, h, -th) + s2 * lo;
  }
  __syncthreads();
  const ExpK ek = g_expk;
  // thread: 4 test points (4mb..) x 4 train points (4rb..)
  const int mb = tid & 15, rb = tid >> 4;
  double rr[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) rr[a][b] = 0.0;
  for (int p = 0; p < d; ++p) {
    const double2 u0 = *(const double2*)(xt + p * CS + 4 * rb);
    const double2 u1 = *(const double2*)(xt + p * CS + 4 * rb + 2);
    const double2 v0 = *(const double2*)(xs + p * CS + 4 * mb);
    const double2 v1 = *(const double2*)(xs + p * CS + 4 * mb + 2);
    const double av[4] = {u0.x, u0.y, u1.x, u1.y};
    const double bv[4] = {v0.x, v0.y, v1.x, v1.y};
    const double wgt = pw[p];
    double a2[4], b2[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      a2[a] = av[a] * av[a];
      b2[a] = bv[a] * bv[a];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (MODE == 0) {
          rr[a][b] = wacc<0>(rr[a][b], av[a], a2[a], bv[b], b2[b], wgt);
        } else {  // as k_gram
          const double t = av[a] - bv[b];
          rr[a][b] = __builtin_fma(t, t, rr[a][b]);
        }
      }
  }
  double* KsT = db.KsT + (size_t)slot * db.Npad * db.Mpad;
  const double* al = db.alpha + (size_t)slot * db.Npad;
  const bool inner = (ch + 1) * TS <= db.N && (mtile + 1) * TS <= db.M;  // block-uniform
  double mp[4] = {0.0, 0.0, 0.0, 0.0};  // this thread's share of the partial means
#pragma unroll
  for (int a = 0; a < 4; ++a) {  // train point gt
    const int gt = ch * TS + 4 * rb + a;
    const double alt = al[gt];
    double kv[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int gm = mtile * TS + 4 * mb + b;
      const double fv = exp_sf(MODE == 1 ? -rr[a][b] : -rr[a][b] * 0.5, ek, tab);  // padded points: finite, selected away
      kv[b] = (inner || (gt < db.N && gm < db.M)) ? fv : 0.0;
      mp[b] = fma(kv[b], alt, mp[b]);
    }
    double* o = KsT + (size_t)gt * db.Mpad + mtile * TS + 4 * mb;
    *(double2*)o = make_double2(kv[0], kv[1]);
    *(double2*)(o + 2) = make_double2(kv[2], kv[3]);
  }
  // the tile's partial means mu_part[ch][m] = sum_{t in tile ch} K*^T[t][m] alpha_t (k_pred_final adds
  // the tiles): the 4 train points of the thread, then the 4 row groups of the wave, then the waves
  double* mup = sc + DMAX;  // [4 waves][64 test points]
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    mp[b] = sum_xor32(sum_xor16(mp[b]));
  }
  if ((tid & 63) < 16) {
#pragma unroll
    for (int b = 0; b < 4; ++b) mup[(tid >> 6) * TS + 4 * mb + b] = mp[b];
  }
  __syncthreads();
  if (tid < TS)
    db.mu_part[((size_t)slot * db.nt + ch) * db.Mpad + mtile * TS + tid] = ((mup[tid] + mup[TS + tid]) + mup[2 * TS + tid]) + mup[3 * TS + tid];
}


__global__ __launch_bounds__(NTHR) void k_pred_final(DevBatch db) {
  const int slot = blockIdx.x;
  const double sf2 = db.params[(size_t)slot * db.pst + db.d];
  for (int m = threadIdx.x; m < db.Mpad; m += NTHR) {
    double mu = 0.0, s = 0.0;
    for (int k = 0; k < db.nt; ++k) {
      mu += db.mu_part[((size_t)slot * db.nt + k) * db.Mpad + m];
      if (db.want_var) s += db.var_part[((size_t)slot * db.nt + k) * db.Mpad + m];
    }
    const double v = sf2 - s;
    db.out_mu[(size_t)slot * db.Mpad + m] = mu;
    db.out_var[(size_t)slot * db.Mpad + m] = db.want_var ? (v > 0.0 ? v : 0.0) : 0.0;
  }
}


// Which dimensions of a slot are one constant: flags[slot][p] = 1 unless every training point t < N
// holds the bits of the slot's first point in dimension p.  Mixed +0 / -0 differ in bits, and a
// non-finite value never counts as constant (its difference is NaN, not 0).  grid = B, once per
// gprx_batch_set_train; the host forms the batch's active list from the flags of all slots.
__global__ __launch_bounds__(NTHR) void k_const_flags(DevBatch db, int* flags) {
  __shared__ int nc[DMAX];
  const int slot = blockIdx.x, tid = threadIdx.x, d = db.d;
  const double* X = db.X + (size_t)slot * db.Npad * d;
  if (tid < DMAX) nc[tid] = 0;
  __syncthreads();
  for (int e = tid; e < db.N * d; e += NTHR) {
    const int p = e % d;
    const double v = X[e];
    if (__double_as_longlong(v) != __double_as_longlong(X[p]) || !isfinite(v)) nc[p] = 1;  // every writer stores 1
  }
  __syncthreads();
  if (tid < d) flags[(size_t)slot * d + tid] = nc[tid];
}
// (defined here: non-template kernels land in the code object in definition order)

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
static size_t gram_lds(int d) { return (size_t)(2 * d * CS + DMAX + 4) * sizeof(double); }  // + k_gram's static table
static size_t lauum_lds(const DevBatch& b) { return lauum_lds_dbl(b.xs, b.nimg) * sizeof(double); }
static size_t cross_lds(int d) { return (size_t)(2 * d * CS + 2 * DMAX + 4 + 4 * TS) * sizeof(double); }  // + the static table

// Dynamic-LDS limits above the 64 KB default, for the current device.  Called once per device by
// gprx_ctx_create (std::call_once per device index) before any launch, so concurrent contexts on
// other threads never launch a kernel whose attribute is not yet set.
static void set_predcov_attributes();  // gprx_predcov.h
static void set_loograd_attributes();  // gprx_loograd.h
void set_kernel_attributes() {
  for (const void* f : {(const void*)k_gram<0>, (const void*)k_gram<1>})
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gram_lds(DMAX));
  (void)hipFuncSetAttribute((const void*)k_lauum_grad, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  for (const void* f : {(const void*)k_pred_cross<0>, (const void*)k_pred_cross<1>})
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cross_lds(DMAX));
  for (const void* f : {(const void*)k_leaf9, (const void*)k_node8})
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)leaf9_lds_bytes());
  for (const void* f : {(const void*)k_gemm<REV_A>, (const void*)k_gemm<REV_B>, (const void*)k_gemm<TRI_A_FIRST>})
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)linv21_lds_bytes());
  set_lbfgs_attributes();
  set_predcov_attributes();
  set_loograd_attributes();
}

void launch_gram(const DevBatch& b, hipStream_t s) {
  if (b.dist_mode == 0) hipLaunchKernelGGL(k_gram<0>, dim3(grid_blocks(b.B, b.ntl)), dim3(NTHR), gram_lds(b.da), s, b);
  else hipLaunchKernelGGL(k_gram<1>, dim3(grid_blocks(b.B, b.ntl)), dim3(NTHR), gram_lds(b.da), s, b);
}
__global__ __launch_bounds__(64) void k_params(DevBatch b) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot < b.B) derive_params(b, slot);
}
void launch_params(const DevBatch& b, hipStream_t s) { hipLaunchKernelGGL(k_params, dim3((b.B + 63) / 64), dim3(64), 0, s, b); }
void launch_center(const DevBatch& b, hipStream_t s) { hipLaunchKernelGGL(k_center, dim3(b.B), dim3(NTHR), 0, s, b); }
void launch_const_flags(const DevBatch& b, int* flags, hipStream_t s) {
  hipLaunchKernelGGL(k_const_flags, dim3(b.B), dim3(NTHR), 0, s, b, flags);
}
void launch_diag(const DevBatch& b, int jt, int upd, hipStream_t s) {
  hipLaunchKernelGGL(k_diag_f, dim3(b.B), dim3(NTHR), 0, s, b, jt, upd);
}
void launch_leaf(const DevBatch& b, int o, int n, int upd, hipStream_t s) {
  if (n == 4) {
    hipLaunchKernelGGL(k_leaf9, dim3(b.B), dim3(2 * NTHR), leaf9_lds_bytes(), s, b, o, upd);
    return;
  }
  hipLaunchKernelGGL(k_leaf, dim3(b.B), dim3(NTHR), 0, s, b, o, n, upd);
}
void launch_node8(const DevBatch& b, int o, int upd, hipStream_t s) {
  hipLaunchKernelGGL(k_node8, dim3(b.B), dim3(2 * NTHR), leaf9_lds_bytes(), s, b, o, upd);
}
void launch_gemm(const DevBatch& b, const GemmGeom& g, hipStream_t s, const GemmGeom& g2) {
  if (g.op != OP_PREDVAR && g.n <= b.small_n) {  // small node: pair units, 64 x 32 waves
    int T = pair_op_units(g, b.nt, b.mt);
    if (g2.op != OP_NONE) T += pair_op_units(g2, b.nt, b.mt);
    hipLaunchKernelGGL(k_gemm_p, dim3(grid_blocks(b.B, T)), dim3(NTHR), 0, s, b, g, g2);
    return;
  }
  int T = op_units(g, b.nt, b.mt);
  if (g2.op != OP_NONE) T += op_units(g2, b.nt, b.mt);
  if (n8_plan(g, g2)) T = 2;  // gemm_body's fixed plan
  const size_t lds = (g.op == OP_LINV21 || g2.op == OP_LINV21) ? linv21_lds_bytes() : 0;
  if (g.op == OP_PREDVAR) hipLaunchKernelGGL(k_gemm_pv, dim3(grid_blocks(b.B, T)), dim3(NTHR), lds, s, b, g, g2);
  else if (g.op == OP_TRSM) hipLaunchKernelGGL(k_gemm<REV_B>, dim3(grid_blocks(b.B, T)), dim3(NTHR), lds, s, b, g, g2);
  else if (g.op == OP_LINV21) hipLaunchKernelGGL(k_gemm<REV_A>, dim3(grid_blocks(b.B, T)), dim3(NTHR), lds, s, b, g, g2);
  else hipLaunchKernelGGL(k_gemm<TRI_A_FIRST>, dim3(grid_blocks(b.B, T)), dim3(NTHR), lds, s, b, g, g2);
}
void launch_rhs(const DevBatch& b, int o, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_rhs, dim3(grid_blocks(b.B, n)), dim3(NTHR), 0, s, b, o, n);
}
void launch_znode(const DevBatch& b, int o, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_znode, dim3(grid_blocks(b.B, n)), dim3(NTHR), 0, s, b, o, n);
}
void launch_alpha(const DevBatch& b, hipStream_t s) {
  hipLaunchKernelGGL(k_alpha, dim3(grid_blocks(b.B, b.nt)), dim3(NTHR), 0, s, b);
}
void launch_lauum_grad(const DevBatch& b, hipStream_t s) {
  hipLaunchKernelGGL(k_lauum_grad, dim3(grid_blocks(b.B, b.nlj)), dim3(NTHR), lauum_lds(b), s, b);
}
void launch_finalize(const DevBatch& b, int want_grad, hipStream_t s) {
  hipLaunchKernelGGL(k_finalize, dim3(b.B), dim3(NTHR), 0, s, b, want_grad);
}
void launch_pred_cross(const DevBatch& b, hipStream_t s) {
  const dim3 grid(grid_blocks(b.B, b.nt * b.mt));
  if (b.dist_mode == 0) hipLaunchKernelGGL(k_pred_cross<0>, grid, dim3(NTHR), cross_lds(b.d), s, b);
  else hipLaunchKernelGGL(k_pred_cross<1>, grid, dim3(NTHR), cross_lds(b.d), s, b);
}
void launch_pred_final(const DevBatch& b, hipStream_t s) {
  hipLaunchKernelGGL(k_pred_final, dim3(b.B), dim3(NTHR), 0, s, b);
}

}  // namespace gprx

// Last: the joint-covariance kernels follow every evaluation kernel in the code object.
#include "gprx_predcov.h"
// ... and the leave-one-out kernels.
#include "gprx_loo.h"
// ... and the gradient of their log predictive probability.
#include "gprx_loograd.h"
// ... and k-fold cross-validation.
#include "gprx_cvfold.h"
