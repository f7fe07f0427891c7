// gprx_loograd.h -- gradient of the leave-one-out log predictive probability (gprx_batch_loo_grad)
// from the factorisation of the last evaluation: k_loo_kinv, k_loo_beta, k_loo_grad,
// k_loo_grad_final and their launchers.
//
// With K = Kf + (sn2 + eps) I, q_i = [K^-1]_ii, alpha = K^-1 y and
//   logp = sum_i [ log(q_i)/2 - alpha_i^2 / (2 q_i) - log(2 pi)/2 ]                  (R&W 5.10-5.12)
//   c_i  = (1/q_i + alpha_i^2/q_i^2) / 2  (> 0),   r_i = alpha_i / q_i,   beta = K^-1 r,
// dK^-1 = -K^-1 dK K^-1 gives Rasmussen & Williams 5.13 in contracted form:
//   dlogp = sum_kl dK_kl W'_kl,   W' = (beta alpha^T + alpha beta^T)/2 - K^-1 C K^-1,   C = diag(c)
// (the marginal likelihood: dLML = sum_kl dK_kl (alpha alpha^T - K^-1)_kl / 2).  For
// theta = [log sn, log ell_1..d, log sf]:  dK/dlog sn = 2 sn2 I,  dK/dlog ell_p = Kf o (x_p - x_p')^2/ell_p^2,
// dK/dlog sf = 2 Kf.  So the gradient is the LML gradient's contraction (k_lauum_grad's epilogue and
// k_finalize's formulas) with W_loo = 2 W' = beta alpha^T + alpha beta^T - 2 P P^T in place of
// W = alpha alpha^T - K^-1, over the lower triangle with weight 1/2 on the diagonal;
// P = K^-1 diag(sqrt c), K^-1 C K^-1 = P P^T.
//
//   k_loo_diag      (gprx_loo.h) q                                                       runs first
//   k_loo_final     (gprx_loo.h) logp, which k_loo_grad_final copies bit for bit
//   k_loo_kinv      K^-1's lower tiles = Mt_i Mt_j^T (k_lauum_grad's product and unit plan), stored as
//                   the full square P in Lw, and the per-tile partials of beta
//   k_loo_beta      beta = the partials of a row tile added in ascending column-tile order
//   k_loo_grad      M = P P^T lower tiles (K = Npad, the plain core) + the ARD epilogue on W_loo
//   k_loo_grad_final  the unit partials in k_finalize's order -> grad[d+2], logp beside it
//
// Lw is free after an evaluation: only the factorisation reads it (gprx_gemm.h, gprx_factor.h) and
// every evaluation rewrites what it reads, so P needs no buffer of its own.
// No atomics, no spinning; every workgroup barrier is in workgroup-uniform control flow; every
// reduction order depends on (N, index) alone, not on B, the slot or the block that ran it.
//
// A part of gprx_kernels.hip, included there after gprx_loo.h and by no other file (the parts and their
// order are listed at its includes).
#pragma once

namespace gprx {

// sqrt(c_i) and r_i of point i (0 for a padded point), v = 1/q and alpha/q as k_loo_final forms them
__device__ __forceinline__ void loo_cr(const DevBatch& db, int slot, const double* kinv, int i, double& sc, double& r) {
  sc = 0.0;
  r = 0.0;
  if (i < db.N) {
    const double q = kinv[(size_t)slot * db.Npad + i], a = db.alpha[(size_t)slot * db.Npad + i];
    const double v = 1.0 / q, aq = a / q;
    sc = sqrt(0.5 * (v + aq * aq));
    r = aq;
  }
}

// ============================================================================================
// loo_kinv: one lower tile (ti, tj) of K^-1 per wave, k_lauum_grad's units and job table
// (db.lauum_order).  Kinv_rc = sum_{k >= 64 ti} Mt[r][k] Mt[c][k].  Like k_lauum_grad the product
// relies on Mt's padded part only for being finite (the Gram pads K with the identity, so it is the
// identity): every element with a padded row or column is replaced by 0 by a select before it is used.
//
// Stores, P = K^-1 diag(sqrt c) as a full square matrix (ld = Npad) in Lw:
//   (ti, tj)  P[r][c] = Kinv_rc sqrt(c_c)      straight from the accumulators (16 lanes = 128 B of a column)
//   (tj, ti)  P[c][r] = Kinv_rc sqrt(c_r)      through the wave's [16][65] LDS buffer, one 16-column block
//                                              at a time (accq_store_t's form: 128-B row segments)
// A diagonal tile holds its blocks b <= a (TRI_AB_FIRST); its blocks b > a are the transposed stores
// of the blocks a > b.  Rows and columns >= N are exact zeros (a select, and sqrt c = 0 there).
//
// beta partials bp[x][y][i] = sum_{j in tile y} Kinv[64 x + i][j] r_j  (x, y < nt):
//   (ti, tj): bp[ti][tj][r] = sum_c Kinv_rc r_c   a lane's 16 columns in (b, q) order, then lanes ^16, ^32
//             bp[tj][ti][c] = sum_r Kinv_rc r_r   a lane's 4 row blocks in order, then the row of 16 lanes
//   a diagonal tile adds the two (the second over the blocks a > b only) into bp[ti][ti].
// The waves of a workgroup share nothing: no workgroup barrier.   grid = grid_blocks(B, nlj)
// ============================================================================================
constexpr int LKW = 16 * (TS + 1) + 5 * TS;  // doubles of LDS per wave: tb, sqrt c and r of the row / column points, cw
__device__ __forceinline__ void loo_kinv_unit(const DevBatch& db, int slot, const int* ju, const double* kinv, double* bpart,
                                              double* wl) {
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ti = ju[7 + w], tj = ju[11 + w];
  if (ti < 0) return;  // wave-uniform; no workgroup barrier below
  const int l = tid & 63, lr = l & 15, lk = l >> 4;
  const int nt = db.nt, N = db.N;
  const size_t ld = db.ld, so = (size_t)slot * db.mat;
  const bool diag = ti == tj;
  double* tb = wl;                  // [16][TS + 1]
  double* scr = tb + 16 * (TS + 1);  // sqrt c of the row points
  double* scc = scr + TS;           // ... of the column points
  double* rr = scc + TS;            // r of the row points
  double* rc = rr + TS;             // ... of the column points
  double* cw = rc + TS;             // a 64-vector on its way between lanes
  d4 acc[QM][QN];
  acc4_zero(acc);
  {
    const double* Ap = db.Mt + so + (size_t)ti * TS * ld + ti * TS;
    if (diag) mma_64x64_m<TRI_AB_FIRST>(acc, Ap, ld, Ap, ld, (nt - ti) * TS);
    else mma_64x64_m<TRI_A_FIRST>(acc, Ap, ld, db.Mt + so + (size_t)ti * TS * ld + tj * TS, ld, (nt - ti) * TS);
  }
  {
    double s, r;
    loo_cr(db, slot, kinv, ti * TS + l, s, r);
    scr[l] = s;
    rr[l] = r;
    loo_cr(db, slot, kinv, tj * TS + l, s, r);
    scc[l] = s;
    rc[l] = r;
  }
  __builtin_amdgcn_wave_barrier();
  // padded rows and columns: exact zeros, whatever Mt holds there
#pragma unroll
  for (int a = 0; a < QM; ++a)
#pragma unroll
    for (int b = 0; b < QN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int gi = ti * TS + 16 * a + lr, gj = tj * TS + 16 * b + lk + 4 * q;
        acc[a][b][q] = (gi < N && gj < N) ? acc[a][b][q] : 0.0;
      }
  // ---- beta partials ----
  double R[QM], Cs[QN][4];
#pragma unroll
  for (int a = 0; a < QM; ++a) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < QN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) s = fma(acc[a][b][q], rc[16 * b + lk + 4 * q], s);  // a diagonal tile's b > a: zeros
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    R[a] = s;
  }
#pragma unroll
  for (int b = 0; b < QN; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < QM; ++a)
        if (!diag || a > b) s = fma(acc[a][b][q], rr[16 * a + lr], s);
      Cs[b][q] = row_sum16(s);
    }
  double* bp_rc = bpart + (((size_t)slot * nt + ti) * nt + tj) * TS;
  double* bp_cr = bpart + (((size_t)slot * nt + tj) * nt + ti) * TS;
  if (lk == 0) {
#pragma unroll
    for (int a = 0; a < QM; ++a) cw[16 * a + lr] = R[a];
  }
  __builtin_amdgcn_wave_barrier();
  const double rowpart = cw[l];
  __builtin_amdgcn_wave_barrier();
  if (lr == 0) {
#pragma unroll
    for (int b = 0; b < QN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) cw[16 * b + lk + 4 * q] = Cs[b][q];
  }
  __builtin_amdgcn_wave_barrier();
  const double colpart = cw[l];
  __builtin_amdgcn_wave_barrier();
  if (diag) {
    bp_rc[l] = rowpart + colpart;
  } else {
    bp_rc[l] = rowpart;
    bp_cr[l] = colpart;
  }
  // ---- P, tile (ti, tj): columns scaled by sqrt c of the column point ----
  double* Pd = db.Lw + so + (size_t)(tj * TS) * ld + ti * TS;
#pragma unroll
  for (int b = 0; b < QN; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 16 * b + lk + 4 * q;
      const double s = scc[c];
#pragma unroll
      for (int a = 0; a < QM; ++a)
        if (!diag || a >= b) Pd[(size_t)c * ld + 16 * a + lr] = acc[a][b][q] * s;
    }
  // ---- P, tile (tj, ti): the transpose, columns (the row points) scaled by their sqrt c ----
  double* Pt = db.Lw + so + (size_t)(ti * TS) * ld + tj * TS;
  const int c16 = l & 15, r4 = l >> 4;
#pragma unroll
  for (int b = 0; b < QN; ++b) {
    const int rmin = diag ? 16 * (b + 1) : 0;  // wave-uniform
#pragma unroll
    for (int a = 0; a < QM; ++a)
#pragma unroll
      for (int q = 0; q < 4; ++q) tb[(lk + 4 * q) * (TS + 1) + 16 * a + lr] = acc[a][b][q] * scr[16 * a + lr];  // tb[c][r]
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < TS; r += 4)
      if (r >= rmin) Pt[(size_t)(r + r4) * ld + 16 * b + c16] = tb[c16 * (TS + 1) + r + r4];
    __builtin_amdgcn_wave_barrier();
  }
}
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_loo_kinv(DevBatch db, const double* kinv,
                                                                                              double* bpart) {
  __shared__ __attribute__((aligned(16))) double lw[4 * LKW];
  int slot, job;
  if (!map_slot(db, db.nlj, slot, job)) return;
  const int* jb = db.lauum_order + (size_t)job * 2 * LU;
  double* wl = lw + (threadIdx.x >> 6) * LKW;
  loo_kinv_unit(db, slot, jb, kinv, bpart, wl);
  if (jb[LU] >= 0) loo_kinv_unit(db, slot, jb + LU, kinv, bpart, wl);  // the folded short unit (per-wave LDS only)
}

// ============================================================================================
// loo_beta: beta[64 x + i] = sum_{y = 0}^{nt - 1} bp[x][y][i], y ascending.  Padded points: 0 (their
// rows of K^-1 were stored as zeros).   grid = grid_blocks(B, nt), 64 threads
// ============================================================================================
__global__ __launch_bounds__(TS) void k_loo_beta(DevBatch db, const double* bpart, double* beta) {
  int slot, x;
  if (!map_slot(db, db.nt, slot, x)) return;
  const int nt = db.nt, l = threadIdx.x;
  const double* bp = bpart + ((size_t)slot * nt + x) * nt * TS;
  double s = 0.0;
  for (int y = 0; y < nt; ++y) s += bp[(size_t)y * TS + l];
  beta[(size_t)slot * db.Npad + x * TS + l] = s;
}

// ============================================================================================
// loo_grad: M's lower tiles = P_i P_j^T over K = Npad (mma_64x64_sq, the plain 64 x 64 core; a diagonal
// tile forms its blocks b <= a only), one tile per wave in k_lauum_grad's units, followed by
// k_lauum_grad's epilogue: grad_unit (gprx_kernels.hip) with this kernel's product and its W, so that
//   G_rc = wt_rc (beta_r alpha_c + alpha_r beta_c - 2 M_rc) Kf_rc     (wt = 1/2 on the diagonal)
// Kf from db.K as the Gram wrote it, only gi > gj read, G_rr with sf2 analytically, row and column
// sums and Q = G Xc on the MFMA pipe, the da active dimensions only, the trace kept for sn.
// LDS: lauum_unit's layout and size (beta comes from global memory), so two workgroups fit a CU
// wherever k_lauum_grad's do.  One partial row per unit: gpart[slot][unit][gps].
// grid = grid_blocks(B, nlj)
// ============================================================================================
__device__ __forceinline__ void loo_grad_unit(const DevBatch& db, int slot, const int* ju, const double* beta, double* gpart) {
  const double* be = beta + (size_t)slot * db.Npad;
  grad_unit(
      db, slot, ju, gpart,
      [&db](d4 (&acc)[QM][QN], int ti, int tj, size_t ld, size_t so) {
        const double* Pi = db.Lw + so + ti * TS;
        if (ti == tj) mma_64x64_sq<true>(acc, Pi, ld, Pi, ld, db.Npad);
        else mma_64x64_sq<false>(acc, Pi, ld, db.Lw + so + tj * TS, ld, db.Npad);
      },
      [be](double alr, double alc, int gi, int gj, double m) { return (be[gi] * alc + alr * be[gj]) - 2.0 * m; });
}
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_loo_grad(DevBatch db, const double* beta,
                                                                                              double* gpart) {
  int slot, job;
  if (!map_slot(db, db.nlj, slot, job)) return;
  const int* jb = db.lauum_order + (size_t)job * 2 * LU;
  const int nu = jb[LU] >= 0 ? 2 : 1;  // block-uniform: the folded short unit
  loo_grad_unit(db, slot, jb, beta, gpart);
  if (nu == 2) {
    __syncthreads();  // the first unit's LDS images and partials are consumed
    loo_grad_unit(db, slot, jb + LU, beta, gpart);
  }
}

// ============================================================================================
// loo_grad_final: out[slot] = [logp, d logp / d (log sn, log ell_1..d, log sf)], the unit partials
// reduced by grad_reduce (gprx_kernels.hip), as k_finalize reduces the marginal likelihood's (threads
// stride the units, wave_sum, the four waves in order): il2_p S_p, 2 S_f, sn2 tr(W_loo).  An inactive (constant)
// dimension gets exactly 0 (NaN where its distances are: params[d + 3]).  logp is k_loo_final's, copied.
// A slot whose last evaluation did not end with status 0 gets NaN throughout.   grid = B
// ============================================================================================
__global__ __launch_bounds__(NTHR) void k_loo_grad_final(DevBatch db, const double* gpart, const double* logp, double* out_all) {
  const int slot = blockIdx.x, tid = threadIdx.x, d = db.d;
  if (!slot_active(db, slot)) return;  // block-uniform, before the first barrier: the slot's row stays as it is
  double* out = out_all + (size_t)slot * (d + 3);
  if (db.status[slot] != 0) {  // block-uniform
    for (int e = tid; e < d + 3; e += NTHR) out[e] = __builtin_nan("");
    return;
  }
  if (tid == 0) out[0] = logp[slot];
  grad_reduce(db, slot, gpart + (size_t)slot * db.ngu * db.gps, out);
}

static void set_loograd_attributes() {
  (void)hipFuncSetAttribute((const void*)k_loo_grad, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}
void launch_loo_kinv(const DevBatch& b, const double* kinv, double* bpart, hipStream_t s) {
  hipLaunchKernelGGL(k_loo_kinv, dim3(grid_blocks(b.B, b.nlj)), dim3(NTHR), 0, s, b, kinv, bpart);
}
void launch_loo_beta(const DevBatch& b, const double* bpart, double* beta, hipStream_t s) {
  hipLaunchKernelGGL(k_loo_beta, dim3(grid_blocks(b.B, b.nt)), dim3(TS), 0, s, b, bpart, beta);
}
void launch_loo_grad(const DevBatch& b, const double* beta, double* gpart, hipStream_t s) {
  hipLaunchKernelGGL(k_loo_grad, dim3(grid_blocks(b.B, b.nlj)), dim3(NTHR), lauum_lds(b), s, b, beta, gpart);
}
void launch_loo_grad_final(const DevBatch& b, const double* gpart, const double* logp, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_loo_grad_final, dim3(b.B), dim3(NTHR), 0, s, b, gpart, logp, out);
}

}  // namespace gprx
