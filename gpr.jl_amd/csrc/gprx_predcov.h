// gprx_predcov.h -- the joint predictive covariance and posterior samples: k_pred_whiten (V^T =
// K*^T L^-T stored), k_pred_cov (Sigma = K** - V^T V, lower tiles and their mirrors), k_cov_chol
// (lower Cholesky of Sigma with the jitter ladder) and k_cov_sample (mu + L z), and their launchers.
//
// A part of gprx_kernels.hip, included there once and by no other file (the parts and their order
// are listed at its includes).
#pragma once

namespace gprx {

// ============================================================================================
// pred_whiten: V^T = K*^T L^-T in K*^T's layout (M x N column-major, ld = Mpad).  Output tile
// (tm, tn) = K*^T[tm, 0..tn] Linv[tn, 0..tn]^T on one wave: A = a K*^T tile (the accumulator row is
// the test index, so a 16-lane store is 128 contiguous bytes), B = an L^-1 row tile, K = (tn + 1)
// tiles.  Units of 2 training x 2 test tiles as OP_PREDVAR; K grows with the training tile, so a
// workgroup computes the unit with the longest K range and then its mirror (gemm_unit's fold).
// Test points >= M and training points >= N are stored as exact zeros.
// grid = grid_blocks(B, whiten_units)
// ============================================================================================
__host__ __device__ inline int whiten_units(int nt, int mt) {
  const int RU = (nt + 1) / 2, CU = (mt + 1) / 2;
  return ((RU + 1) / 2) * CU;
}
__device__ __forceinline__ void whiten_tile(const DevBatch& db, double* VT, int slot, int tn, int tm) {
  const size_t po = (size_t)slot * db.Npad * db.Mpad;
  d4 acc[QM][QN];
  acc4_zero(acc);
  mma_64x64(acc, db.KsT + po + tm * TS, (size_t)db.Mpad, db.Linv + (size_t)slot * db.mat + tn * TS, db.ld, (tn + 1) * TS);
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  double* o = VT + po + (size_t)(tn * TS) * db.Mpad + tm * TS;
  const bool inner = (tn + 1) * TS <= db.N && (tm + 1) * TS <= db.M;  // wave-uniform
#pragma unroll
  for (int a = 0; a < QM; ++a)
#pragma unroll
    for (int b = 0; b < QN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = 16 * a + lr, n = 16 * b + lk + 4 * q;
        const bool in = inner || (tm * TS + m < db.M && tn * TS + n < db.N);
        o[(size_t)n * db.Mpad + m] = in ? acc[a][b][q] : 0.0;
      }
}
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_pred_whiten(DevBatch db, double* VT) {
  const int RU = (db.nt + 1) / 2, CU = (db.mt + 1) / 2;
  int slot, u;
  if (!map_block(blockIdx.x, db.B, whiten_units(db.nt, db.mt), slot, u)) return;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wr = w >> 1, wc = w & 1;
  const int f = u / CU, pj = u - f * CU;
  const int lo = f, hi = RU - 1 - f;
  const int np = lo != hi ? 2 : 1;
#pragma unroll 1
  for (int k = 0; k < np; ++k) {  // ONE call site of the core (see gemm_unit)
    const int tn = 2 * (k ? lo : hi) + wr, tm = 2 * pj + wc;
    if (tn >= db.nt || tm >= db.mt) continue;  // wave-uniform: partial unit
    whiten_tile(db, VT, slot, __builtin_amdgcn_readfirstlane(tn), __builtin_amdgcn_readfirstlane(tm));
  }
}

// ============================================================================================
// pred_cov: Sigma = K** - V^T V, one lower 64 x 64 tile (ti >= tj) per single-wave workgroup: a
// SYRK over K = Npad on the stored V^T, K** formed in the epilogue with k_pred_cross's arithmetic
// (MODE 1: coordinates pre-scaled by sqrt(il2 / 2), r/2 summed by fma; MODE 0: the expanded
// distance; exp_sf with the staged sf2 table).  Sigma is stored compact (M x M column-major, ld =
// M, slot b at Sig + b M M).  Each value is computed once, for i >= j, and written to (i, j) and
// (j, i): bitwise symmetric.  Not clamped.
// grid = grid_blocks(B, mt (mt + 1) / 2), 64 threads; dynamic LDS 2 * 64 * (d | 1) doubles
// ============================================================================================
static size_t predcov_lds(int d) { return (size_t)2 * TS * (d | 1) * sizeof(double); }
template <int MODE>
__global__ __launch_bounds__(64) void k_pred_cov(DevBatch db, const double* VT, double* Sig) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ __attribute__((aligned(16))) double tab[128];  // exp_sf's table, as k_pred_cross
  __shared__ double pw[DMAX];
  const int d = db.d, ds = d | 1, l = threadIdx.x;
  int slot, t;
  if (!map_block(blockIdx.x, db.B, db.mt * (db.mt + 1) / 2, slot, t)) return;
  int ti, tj;
  quad_tri(t, ti, tj);
  ti = __builtin_amdgcn_readfirstlane(ti);
  tj = __builtin_amdgcn_readfirstlane(tj);
  const double* P = db.params + (size_t)slot * db.pst;
  const double* Xq = db.Xs + (size_t)slot * db.Mpad * d;
  double* xi = sm;
  double* xj = sm + TS * ds;
  for (int p = l; p < d; p += 64) pw[p] = P[p];
  __syncthreads();
  for (int e = l; e < TS * d; e += 64) {  // point r = e / d, dimension p: contiguous reads
    const int r = e / d, p = e - r * d;
    const double s = MODE == 1 ? sqrt(0.5 * pw[p]) : 1.0;
    xi[r * ds + p] = Xq[(size_t)(ti * TS) * d + e] * s;
    xj[r * ds + p] = Xq[(size_t)(tj * TS) * d + e] * s;
  }
  {
    const double s2 = P[d], h = g_exp2tab[2 * l], lo = g_exp2tab[2 * l + 1];
    const double th = s2 * h;
    tab[2 * l] = th;
    tab[2 * l + 1] = fma(s2, h, -th) + s2 * lo;
  }
  __syncthreads();
  const ExpK ek = g_expk;
  const double* V = VT + (size_t)slot * db.Npad * db.Mpad;
  d4 acc[QM][QN];
  acc4_zero(acc);
  mma_64x64(acc, V + ti * TS, (size_t)db.Mpad, V + tj * TS, (size_t)db.Mpad, db.Npad);
  const int lr = l & 15, lk = l >> 4;
  const int M = db.M;
  double* S = Sig + (size_t)slot * M * M;
  const bool diag = ti == tj;
#pragma unroll
  for (int a = 0; a < QM; ++a)
#pragma unroll
    for (int b = 0; b < QN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int il = 16 * a + lr, jl = 16 * b + lk + 4 * q;
        const int i = ti * TS + il, j = tj * TS + jl;
        if (i >= M || j >= M || (diag && jl > il)) continue;
        const double* pa = xi + il * ds;
        const double* pb = xj + jl * ds;
        double rr = 0.0;
        for (int p = 0; p < d; ++p) {
          const double av = pa[p], bv = pb[p];
          if (MODE == 0) {
            rr = wacc<0>(rr, av, av * av, bv, bv * bv, pw[p]);
          } else {
            const double dt = av - bv;
            rr = __builtin_fma(dt, dt, rr);
          }
        }
        const double v = exp_sf(MODE == 1 ? -rr : -rr * 0.5, ek, tab) - acc[a][b][q];
        S[(size_t)j * M + i] = v;
        if (i != j) S[(size_t)i * M + j] = v;
      }
}

// ============================================================================================
// cov_chol: lower Cholesky of the M x M Sigma of a slot, one workgroup per slot, blocked
// right-looking (CB columns a step): the diagonal block factored in LDS, the panel below it solved
// by forward substitution against the block (no explicit inverse: Sigma is routinely near-singular),
// the trailing lower triangle updated by fma chains.  tau = (N + M) eps sf2 bounds the rounding of
// Sigma's own entries; a pivot that is not finite or <= tau fails the attempt.  Attempt 0 factors
// Sigma itself, attempts k = 1..8 Sigma + 10^k tau I; every attempt starts from the untouched Sigma
// (the factor is built in F).  jit[slot]: the jitter of the attempt that passed (NaN: none did),
// st[slot]: 0, GPRX_NOT_POSITIVE_DEFINITE, or the status of the slot's failed evaluation.
// Every branch around a barrier is workgroup-uniform (the pivots are read from LDS by all threads).
// grid = B
// ============================================================================================
constexpr int CB = 16;      // columns per step (the panel solve keeps a row of CB values in registers)
constexpr int CJ = 8;       // trailing columns per pass of a thread's row
constexpr int COV_ATT = 9;  // attempts: 0 (no jitter), 1..8
struct CovArgs {
  const double* Sig;  // B x [M][M] compact
  double* F;          // B x [M][M] factor (ld = M), slot stride fs
  size_t fs;
  const double* Z;    // [S][M] per slot at Z + slot zs (zs = 0: shared)
  size_t zs;
  double* smp;        // [S][M] per slot at smp + slot ss
  size_t ss;
  double* jit;        // B
  int* st;            // B
  int S;
};
__global__ __launch_bounds__(NTHR) void k_cov_chol(DevBatch db, CovArgs a) {
  __shared__ double D[CB][CB + 1];
  const int slot = blockIdx.x, tid = threadIdx.x, M = db.M;
  const int est = db.status[slot];
  if (est != 0) {  // block-uniform: the slot's last evaluation failed
    if (tid == 0) {
      a.jit[slot] = __builtin_nan("");
      a.st[slot] = est;
    }
    return;
  }
  const double* Sg = a.Sig + (size_t)slot * M * M;
  double* F = a.F + (size_t)slot * a.fs;
  const double sf2 = db.params[(size_t)slot * db.pst + db.d];
  const double tau = ((double)(db.N + M) * DBL_EPSILON) * sf2;
  double p10 = 1.0, jit = 0.0;
  bool ok = false;
#pragma unroll 1
  for (int att = 0; att < COV_ATT && !ok; ++att) {
    if (att > 0) {
      p10 *= 10.0;
      jit = p10 * tau;
    }
    __syncthreads();  // the previous attempt's reads of F
    for (int e = tid; e < M * M; e += NTHR) {
      const int c = e / M, r = e - c * M;
      F[e] = r > c ? Sg[e] : (r == c ? Sg[e] + jit : 0.0);
    }
    __syncthreads();
    ok = true;
#pragma unroll 1
    for (int k0 = 0; k0 < M && ok; k0 += CB) {
      const int nb = M - k0 < CB ? M - k0 : CB;
      for (int e = tid; e < nb * nb; e += NTHR) {
        const int c = e / nb, r = e - c * nb;
        D[r][c] = F[(size_t)(k0 + c) * M + k0 + r];
      }
      __syncthreads();
#pragma unroll 1
      for (int c = 0; c < nb && ok; ++c) {
        const double p = D[c][c];  // the same value in every thread
        if (!(isfinite(p) && p > tau)) {
          ok = false;
          break;
        }
        const double s = sqrt(p);
        __syncthreads();  // every thread has read the pivot
        if (tid == 0) D[c][c] = s;
        if (tid > c && tid < nb) D[tid][c] = D[tid][c] / s;
        __syncthreads();
        const int w = nb - 1 - c;  // trailing block: rows and columns c+1..nb-1, lower part
        for (int e = tid; e < w * w; e += NTHR) {
          const int cc = c + 1 + e / w, r = c + 1 + e % w;
          if (r >= cc) D[r][cc] = fma(-D[r][c], D[cc][c], D[r][cc]);
        }
        __syncthreads();
      }
      if (!ok) break;
      for (int e = tid; e < nb * nb; e += NTHR) {
        const int c = e / nb, r = e - c * nb;
        F[(size_t)(k0 + c) * M + k0 + r] = D[r][c];
      }
      const int r0 = k0 + CB;  // rows below the block (only after a full block: nb == CB)
      for (int r = r0 + tid; r < M; r += NTHR) {  // L21 row r: x L11^T = a by substitution
        double x[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) {
          double v = F[(size_t)(k0 + c) * M + r];
#pragma unroll
          for (int p = 0; p < c; ++p) v = fma(-x[p], D[c][p], v);
          x[c] = v / D[c][c];
        }
#pragma unroll
        for (int c = 0; c < CB; ++c) F[(size_t)(k0 + c) * M + r] = x[c];
      }
      __syncthreads();  // the panel is visible to the workgroup; D is free again
      for (int jb = r0; jb < M; jb += CJ) {  // A22 -= L21 L21^T, lower part, CJ columns a pass
        for (int r = jb + tid; r < M; r += NTHR) {
          double v[CJ];
#pragma unroll
          for (int j = 0; j < CJ; ++j) v[j] = (jb + j <= r) ? F[(size_t)(jb + j) * M + r] : 0.0;
#pragma unroll 4
          for (int p = 0; p < CB; ++p) {
            const double lrp = F[(size_t)(k0 + p) * M + r];
#pragma unroll
            for (int j = 0; j < CJ; ++j)
              if (jb + j <= r) v[j] = fma(-lrp, F[(size_t)(k0 + p) * M + jb + j], v[j]);
          }
#pragma unroll
          for (int j = 0; j < CJ; ++j)
            if (jb + j <= r) F[(size_t)(jb + j) * M + r] = v[j];
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    a.jit[slot] = ok ? jit : __builtin_nan("");
    a.st[slot] = ok ? 0 : 1;  // GPRX_NOT_POSITIVE_DEFINITE
  }
}

// cov_sample: smp[s][m] = mu[m] + sum_{p <= m} L[m][p] z[s][p]; NaN rows for a slot without a factor.
// grid = (B, ceil(S M / NTHR))
__global__ __launch_bounds__(NTHR) void k_cov_sample(DevBatch db, CovArgs a) {
  const int slot = blockIdx.x, M = db.M;
  const int e = blockIdx.y * NTHR + threadIdx.x;
  if (e >= a.S * M) return;
  const int s = e / M, m = e - s * M;
  double* o = a.smp + (size_t)slot * a.ss + e;
  if (a.st[slot] != 0) {
    *o = __builtin_nan("");
    return;
  }
  const double* F = a.F + (size_t)slot * a.fs;
  const double* z = a.Z + (size_t)slot * a.zs + (size_t)s * M;
  double v = 0.0;
  for (int p = 0; p <= m; ++p) v = fma(F[(size_t)p * M + m], z[p], v);
  *o = db.out_mu[(size_t)slot * db.Mpad + m] + v;
}

static void set_predcov_attributes() {
  for (const void* f : {(const void*)k_pred_cov<0>, (const void*)k_pred_cov<1>})
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)predcov_lds(DMAX));
}
void launch_pred_whiten(const DevBatch& b, double* VT, hipStream_t s) {
  hipLaunchKernelGGL(k_pred_whiten, dim3(grid_blocks(b.B, whiten_units(b.nt, b.mt))), dim3(NTHR), 0, s, b, VT);
}
void launch_pred_cov(const DevBatch& b, const double* VT, double* Sig, hipStream_t s) {
  const dim3 grid(grid_blocks(b.B, b.mt * (b.mt + 1) / 2));
  if (b.dist_mode == 0) hipLaunchKernelGGL(k_pred_cov<0>, grid, dim3(64), predcov_lds(b.d), s, b, VT, Sig);
  else hipLaunchKernelGGL(k_pred_cov<1>, grid, dim3(64), predcov_lds(b.d), s, b, VT, Sig);
}
void launch_cov_chol(const DevBatch& b, const double* Sig, double* F, size_t fs, double* jit, int* st, hipStream_t s) {
  CovArgs a{Sig, F, fs, nullptr, 0, nullptr, 0, jit, st, 0};
  hipLaunchKernelGGL(k_cov_chol, dim3(b.B), dim3(NTHR), 0, s, b, a);
}
void launch_cov_sample(const DevBatch& b, const double* F, size_t fs, const double* Z, size_t zs, double* smp, size_t ss,
                       int S, const int* st, hipStream_t s) {
  CovArgs a{nullptr, const_cast<double*>(F), fs, Z, zs, smp, ss, nullptr, const_cast<int*>(st), S};
  hipLaunchKernelGGL(k_cov_sample, dim3(b.B, ((size_t)S * b.M + NTHR - 1) / NTHR), dim3(NTHR), 0, s, b, a);
}

}  // namespace gprx
