// gprx_loo.h -- leave-one-out predictions from the factorisation of the last evaluation: k_loo_diag
// (kinv = diag(K^-1) from one sweep of L^-1's lower triangle), k_loo_final (mu, var, logp_i per point
// and logp per slot, Rasmussen & Williams 5.10-5.12), and their launchers.
//
// A part of gprx_kernels.hip, included there once and by no other file (the parts and their order
// are listed at its includes).
#pragma once

namespace gprx {

// ============================================================================================
// loo_diag: kinv[slot][i] = [K^-1]_ii = sum_{k >= i} Linv[k, i]^2 for i < N (0 for the padded
// i >= N): column i of Linv from its diagonal down, which is contiguous.  Column strip j (the 64
// columns of tile column j) has the tiles (j..nt-1, j); a workgroup takes the strips lo = p and
// hi = nt - 1 - p one after the other (nt + 1 tiles whatever p; the middle strip of an odd nt
// alone), so every workgroup of a launch reads the same number of tiles.
//
// Only tiles on and below the diagonal are read.  Nothing is assumed about what the strictly upper
// part of a diagonal tile or the padded rows k >= N hold: those elements are loaded with their
// tile and replaced by 0 by a select (never multiplied), so a NaN there does not reach the sum.
//
// Wave w owns the strip's columns 16 w .. 16 w + 15.  Lane l = 32 cp + rp loads rows 2 rp, 2 rp + 1
// (one 16-B load) of the columns 16 w + 2 u + cp, u = 0..7: a load instruction reads two whole
// 512-B column segments of the tile.  The next tile's 8 loads are issued before this tile's
// arithmetic (16 loads in flight per lane).
//
// Reduction order, fixed: a lane adds the squares of its two rows of a column tile after tile down
// the strip (two fma chains per column, even and odd row), then even + odd, then the column's 32
// lanes by the xor tree 16, 8, 4, 2, 1.  A column belongs to one wave, so no sum crosses waves.
// The order depends on (N, i) alone: not on B, the slot, or the block that ran it.  No atomics.
// grid = grid_blocks(B, (nt + 1) / 2)
// ============================================================================================
__host__ __device__ inline int loo_units(int nt) { return (nt + 1) / 2; }
__global__ __launch_bounds__(NTHR) void k_loo_diag(DevBatch db, double* kinv) {
  int slot, p;
  if (!map_slot(db, loo_units(db.nt), slot, p)) return;  // a masked slot: before the first load
  typedef double d2 __attribute__((ext_vector_type(2)));
  const int l = threadIdx.x & 63, rp = l & 31, cp = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nt = db.nt, N = db.N;
  const size_t ld = db.ld;
  const int lo = p, hi = nt - 1 - p;
  const int ns = lo != hi ? 2 : 1;
#pragma unroll 1
  for (int k = 0; k < ns; ++k) {
    const int j = k ? lo : hi;
    const int c0 = 16 * w + cp;  // this lane's column of the strip for u = 0; + 2 u
    // element (row 64 ti + 2 rp, column 64 j + c0 + 2 u) = A[64 ti + 2 u ld]
    const double* A = db.Linv + (size_t)slot * db.mat + (size_t)(j * TS + c0) * ld + 2 * rp;
    d2 acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = d2{0.0, 0.0};
    d2 m[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) m[u] = *(const d2*)(A + (size_t)j * TS + (size_t)(2 * u) * ld);
#pragma unroll 1
    for (int ti = j; ti < nt; ++ti) {
      d2 mn[8];
      if (ti + 1 < nt) {
#pragma unroll
        for (int u = 0; u < 8; ++u) mn[u] = *(const d2*)(A + (size_t)(ti + 1) * TS + (size_t)(2 * u) * ld);
      }
      if (ti == j || (ti + 1) * TS > N) {  // wave-uniform: the diagonal tile, the tile with padded rows
        const int r0 = ti * TS + 2 * rp;   // global row of .x
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int col = j * TS + c0 + 2 * u;
          const double x = (r0 >= col && r0 < N) ? m[u].x : 0.0;
          const double y = (r0 + 1 >= col && r0 + 1 < N) ? m[u].y : 0.0;
          acc[u].x = fma(x, x, acc[u].x);
          acc[u].y = fma(y, y, acc[u].y);
        }
      } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          acc[u].x = fma(m[u].x, m[u].x, acc[u].x);
          acc[u].y = fma(m[u].y, m[u].y, acc[u].y);
        }
      }
      if (ti + 1 < nt) {
#pragma unroll
        for (int u = 0; u < 8; ++u) m[u] = mn[u];
      }
    }
    double* o = kinv + (size_t)slot * db.Npad + j * TS + c0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      double s = acc[u].x + acc[u].y;
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off);  // within the column's 32 lanes
      if (rp == 0) o[2 * u] = s;
    }
  }
}

// ============================================================================================
// loo_final: for i < N, from kinv and alpha (alpha = K^-1 y, y the targets given to set_train):
//   var_i  = 1 / kinv_i                          (K carries the noise and eps on its diagonal)
//   mu_i   = y_i - alpha_i / kinv_i
//   lp_i   = 0.5 log(kinv_i) - 0.5 alpha_i^2 / kinv_i - 0.5 log(2 pi)
// and logp[slot] = sum_i lp_i: thread t adds its points t, t + 256, ... in ascending order, then the
// 256 partial sums by a halving tree in LDS; every addition is a two-sum whose error terms are
// carried along and added at the end, so the sum is the rounded exact sum of the lp_i to about one
// ulp whatever N.  Points i >= N are neither written nor summed.  A slot whose last evaluation
// did not end with status 0 gets NaN in all four outputs.
// mu, var, lp: B x Npad (row stride Npad).  grid = B
// ============================================================================================
__device__ __forceinline__ void two_sum_acc(double& s, double& e, double v, double ve) {
  const double t = s + v, bp = t - s;
  e += ((s - (t - bp)) + (v - bp)) + ve;
  s = t;
}
// The workgroup's NTHR partial sums (s, e) added by a halving tree in LDS, every addition a two-sum
// with the error terms carried; thread 0 returns the sum, s + e of the root.  Called by the whole
// workgroup in workgroup-uniform control flow.  (k_loo_final, k_cv_final)
__device__ __forceinline__ double two_sum_block(double s, double e) {
  __shared__ double ps[NTHR], pe[NTHR];
  const int tid = threadIdx.x;
  ps[tid] = s;
  pe[tid] = e;
  __syncthreads();
  for (int h = NTHR / 2; h > 0; h >>= 1) {
    if (tid < h) {
      two_sum_acc(s, e, ps[tid + h], pe[tid + h]);
      ps[tid] = s;
      pe[tid] = e;
    }
    __syncthreads();
  }
  return s + e;
}
__global__ __launch_bounds__(NTHR) void k_loo_final(DevBatch db, const double* kinv, double* mu, double* var, double* lp,
                                                    double* logp) {
  const int slot = blockIdx.x, tid = threadIdx.x, N = db.N;
  if (!slot_active(db, slot)) return;  // block-uniform, before the first barrier: the slot's rows stay as they are
  const size_t ro = (size_t)slot * db.Npad;
  if (db.status[slot] != 0) {  // block-uniform
    const double nan = __builtin_nan("");
    for (int i = tid; i < N; i += NTHR) mu[ro + i] = var[ro + i] = lp[ro + i] = nan;
    if (tid == 0) logp[slot] = nan;
    return;
  }
  const double hl2pi = 0.91893853320467274178;  // 0.5 log(2 pi)
  double s = 0.0, e = 0.0;
  for (int i = tid; i < N; i += NTHR) {
    const double q = kinv[ro + i], a = db.alpha[ro + i];
    const double v = 1.0 / q, aq = a / q;
    const double t = (0.5 * log(q) - 0.5 * (a * aq)) - hl2pi;
    var[ro + i] = v;
    mu[ro + i] = db.Y[ro + i] - aq;
    lp[ro + i] = t;
    two_sum_acc(s, e, t, 0.0);
  }
  const double tot = two_sum_block(s, e);
  if (tid == 0) logp[slot] = tot;
}

void launch_loo_diag(const DevBatch& b, double* kinv, hipStream_t s) {
  hipLaunchKernelGGL(k_loo_diag, dim3(grid_blocks(b.B, loo_units(b.nt))), dim3(NTHR), 0, s, b, kinv);
}
void launch_loo_final(const DevBatch& b, const double* kinv, double* mu, double* var, double* lp, double* logp, hipStream_t s) {
  hipLaunchKernelGGL(k_loo_final, dim3(b.B), dim3(NTHR), 0, s, b, kinv, mu, var, lp, logp);
}

}  // namespace gprx
