// gprx_cvfold.h -- k-fold cross-validation (gprx_batch_cvfold) from the factorisation of the last
// evaluation: k_cv_pack, k_cv_kinv, k_cv_fold, k_cv_final and their launchers.
//
// For a fold V of m points, Q = [K^-1]_VV and a = alpha_V (K carries sn2 + eps; alpha = K^-1 y, y the
// targets given to set_train), Rasmussen & Williams 5.4.2 in block form:
//   Sigma_V = Q^-1,   mu_V = y_V - Q^-1 a,   log p(y_V | y_-V) = -a^T Q^-1 a / 2 + log|Q| / 2 - m log(2 pi) / 2
// and with Q = C C^T, w = C^-1 a:
//   logp_V = -|w|^2 / 2 + sum_i log C_ii - m log(2 pi) / 2,   mu_V = y_V - C^-T w,   var_i = sum_k (C^-1)_ki^2.
//
//   k_cv_pack   the rows of Mt = L^-T in packed (fold) order into Lw, every element L^-T defines as
//               zero and every padded row or column an exact 0
//   k_cv_kinv   the lower 64 x 64 tiles of (packed)(packed)^T that a fold reaches, one per wave, into
//               the workspace (the folds' Q blocks; never all of K^-1)
//   k_cv_fold   one workgroup per (slot, fold): Q's lower triangle gathered into the fold's m x m
//               square of Lw, factored there, then w, logp_V, r = C^-T w and the column norms of C^-1
//   k_cv_final  mu and var back in point order, logp = sum_V logp_V, the slot's status
//
// Lw is free after an evaluation (see gprx_loograd.h): k_cv_pack fills it, k_cv_kinv reads it, and
// k_cv_fold then reuses it fold by fold (sum_V m_V^2 <= N^2).  The tiles keep Q, Lw keeps C (lower
// triangle of a fold's square) and C^-T (strictly upper), the workspace keeps r: what a gradient
// would start from.
// No atomics, no spinning; every workgroup barrier is in workgroup-uniform control flow; every
// reduction order depends on (N, the fold layout, index) alone, not on B, the slot or the block.
//
// A part of gprx_kernels.hip, included there last and by no other file (the parts and their order
// are listed at its includes).
#pragma once

namespace gprx {

// the parts of a slot's layout table (CvArgs in gprx_internal.h)
struct CvTab {
  const int *perm, *fstart, *foff, *rowlo, *rowoff, *kmin, *jobs;
};
__device__ __forceinline__ CvTab cv_tab(const DevBatch& db, const CvArgs& a, int slot) {
  CvTab t;
  t.perm = a.tab + (size_t)slot * a.lstride;
  t.fstart = t.perm + db.Npad;
  t.foff = t.fstart + a.F + 1;
  t.rowlo = t.foff + a.F + 1;
  t.rowoff = t.rowlo + db.nt;
  t.kmin = t.rowoff + db.nt + 1;
  t.jobs = t.kmin + db.nt;
  return t;
}

// ============================================================================================
// cv_pack: Lw[r'][k] = Mt[perm[r']][k] where L^-T has an element (perm[r'] <= k < N), else exactly 0
// (a select: the other triangle of Mt and its padding are never read).  A workgroup takes the 64
// columns k of one column strip; a thread its rows r' = tid, tid + 256, ...: the stores of a column
// are contiguous, the loads a gather within the column.   grid = grid_blocks(B, nt)
// ============================================================================================
__global__ __launch_bounds__(NTHR) void k_cv_pack(DevBatch db, CvArgs a) {
  int slot, j;
  if (!map_slot(db, db.nt, slot, j)) return;  // a masked slot: before the first load
  if (db.status[slot] != 0) return;           // a failed slot: its Mt is not read
  const CvTab t = cv_tab(db, a, slot);
  const int N = db.N, Npad = db.Npad;
  const size_t ld = db.ld, so = (size_t)slot * db.mat;
  for (int rp = threadIdx.x; rp < Npad; rp += NTHR) {
    const int p = t.perm[rp];
    const double* src = db.Mt + so + (p >= 0 ? p : 0);
    double* dst = db.Lw + so + rp;
#pragma unroll 8
    for (int c = 0; c < TS; ++c) {
      const int k = j * TS + c;
      double v = 0.0;
      if (p >= 0 && p <= k && k < N) v = src[(size_t)k * ld];
      dst[(size_t)k * ld] = v;
    }
  }
}

// ============================================================================================
// cv_kinv: tile j = (ti, tj) of the slot's job table, T_rc = sum_k P[64 ti + r][k] P[64 tj + c][k]
// with P the packed matrix in Lw, by k_loo_grad's product (mma_64x64_sq: the plain 64 x 64 core, a
// diagonal tile its blocks b <= a only).  The zeros of P are exact, so the sum starts at the first
// column in which both row tiles can hold anything, k0 = max(kmin[ti], kmin[tj]), and runs to Npad.
// One tile per wave, stored column-major [c][r] at tiles[slot][j]; of a diagonal tile only the blocks
// b <= a are stored (k_cv_fold reads the lower triangle only).  The waves share nothing.
// grid = grid_blocks(B, ceil(njmax / 4))
// ============================================================================================
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_cv_kinv(DevBatch db, CvArgs a) {
  int slot, unit;
  if (!map_slot(db, (a.njmax + 3) / 4, slot, unit)) return;
  if (db.status[slot] != 0) return;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int job = 4 * unit + w;
  if (job >= a.njmax) return;  // wave-uniform; no workgroup barrier below
  const CvTab t = cv_tab(db, a, slot);
  const int ti = __builtin_amdgcn_readfirstlane(t.jobs[2 * job]), tj = __builtin_amdgcn_readfirstlane(t.jobs[2 * job + 1]);
  if (ti < 0) return;
  const int ka = t.kmin[ti], kb = t.kmin[tj];
  const int k0 = __builtin_amdgcn_readfirstlane(ka > kb ? ka : kb);
  const size_t ld = db.ld, so = (size_t)slot * db.mat;
  const double* Pi = db.Lw + so + (size_t)k0 * ld + ti * TS;
  d4 acc[QM][QN];
  acc4_zero(acc);
  if (ti == tj) mma_64x64_sq<true>(acc, Pi, ld, Pi, ld, db.Npad - k0);
  else mma_64x64_sq<false>(acc, Pi, ld, db.Lw + so + (size_t)k0 * ld + tj * TS, ld, db.Npad - k0);
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  double* T = a.tiles + ((size_t)slot * a.njmax + job) * (TS * TS);
#pragma unroll
  for (int b = 0; b < QN; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 16 * b + lk + 4 * q;
#pragma unroll
      for (int aa = 0; aa < QM; ++aa)
        if (ti != tj || aa >= b) T[c * TS + 16 * aa + lr] = acc[aa][b][q];
    }
}

// ============================================================================================
// cv_fold: one workgroup per (slot, fold).  The fold's points are the packed positions s0 .. s0 + m - 1
// (m <= CVFOLD_MAX); F is its m x m column-major square in Lw (offset foff).
//   gather   F's lower triangle = Q, element (i, j) from tile (floor((s0+i)/64), floor((s0+j)/64));
//            ws = a = alpha of the fold's points (LDS)
//   factor   k_cov_chol's blocked right-looking Cholesky, CB columns a step: the diagonal block in
//            LDS, the panel by forward substitution against it, the trailing triangle by fma chains.
//            A pivot that is not finite or <= 0 fails the fold (no jitter).  The right-hand side
//            rides along as one more row: after a step's block, thread 0 substitutes ws over the
//            block's columns and the workgroup takes the block's columns out of the rest of ws, so
//            w = C^-1 a when the factor is done.  sum log C_ii is added pivot by pivot, in order.
//   logp_V   = (-|w|^2 / 2 + sum log C_ii) - m log(2 pi) / 2, |w|^2 one fma chain in ascending order
//   r        = C^-T w by backward substitution, column by column from the last (one barrier a column)
//   var_i    = sum_{k >= i} X_ki^2, X = C^-1: thread i forms column i by forward substitution in
//            ascending k and keeps it in F's strictly upper triangle (X_ki at (i, k)), one fma chain;
//            a wave walks its 64 columns together, so C's elements are read once per wave.
// A fold of one point divides by its pivot alone.  Every branch around a barrier is workgroup-uniform
// (pivots are read from LDS by all threads).  An empty fold: logp_V = 0.
// grid = grid_blocks(B, F)
// ============================================================================================
__global__ __launch_bounds__(NTHR) void k_cv_fold(DevBatch db, CvArgs a) {
  __shared__ double D[CB][CB + 1];
  __shared__ double ws[CVFOLD_MAX], us[CVFOLD_MAX];
  __shared__ int tb[CVFOLD_MAX / TS + 2];  // rowoff - rowlo of the fold's tile rows
  int slot, f;
  if (!map_slot(db, a.F, slot, f)) return;
  if (db.status[slot] != 0) return;  // k_cv_final writes the failed slot's NaN
  const int tid = threadIdx.x;
  const CvTab t = cv_tab(db, a, slot);
  const int s0 = t.fstart[f], m = t.fstart[f + 1] - s0;
  double* lpf = a.lpf + (size_t)slot * a.F + f;
  int* fst = a.fst + (size_t)slot * a.F + f;
  if (m <= 0) {  // block-uniform
    if (tid == 0) {
      *lpf = 0.0;
      *fst = 0;
    }
    return;
  }
  double* F = db.Lw + (size_t)slot * db.mat + t.foff[f];
  const double* tiles = a.tiles + (size_t)slot * a.njmax * (TS * TS);
  const size_t ro = (size_t)slot * db.Npad;
  const int tr0 = s0 >> 6, tr1 = (s0 + m - 1) >> 6;
  for (int e = tid; e <= tr1 - tr0; e += NTHR) tb[e] = t.rowoff[tr0 + e] - t.rowlo[tr0 + e];
  for (int i = tid; i < m; i += NTHR) ws[i] = db.alpha[ro + t.perm[s0 + i]];
  __syncthreads();
  for (int e = tid; e < m * m; e += NTHR) {
    const int c = e / m, r = e - c * m;
    if (r >= c) {
      const int pr = s0 + r, pc = s0 + c;
      F[e] = tiles[(size_t)(tb[(pr >> 6) - tr0] + (pc >> 6)) * (TS * TS) + (pc & 63) * TS + (pr & 63)];
    }
  }
  __syncthreads();
  bool ok = true;
  double sld = 0.0;  // the same value in every thread
#pragma unroll 1
  for (int k0 = 0; k0 < m && ok; k0 += CB) {
    const int nb = m - k0 < CB ? m - k0 : CB;
    for (int e = tid; e < nb * nb; e += NTHR) {
      const int c = e / nb, r = e - c * nb;
      if (r >= c) D[r][c] = F[(size_t)(k0 + c) * m + k0 + r];
    }
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < nb && ok; ++c) {
      const double p = D[c][c];  // the same value in every thread
      if (!(isfinite(p) && p > 0.0)) {
        ok = false;
        break;
      }
      const double s = sqrt(p);
      sld += log(s);
      __syncthreads();  // every thread has read the pivot
      if (tid == 0) D[c][c] = s;
      if (tid > c && tid < nb) D[tid][c] = D[tid][c] / s;
      __syncthreads();
      const int wd = nb - 1 - c;  // trailing block: rows and columns c+1..nb-1, lower part
      for (int e = tid; e < wd * wd; e += NTHR) {
        const int cc = c + 1 + e / wd, r = c + 1 + e % wd;
        if (r >= cc) D[r][cc] = fma(-D[r][c], D[cc][c], D[r][cc]);
      }
      __syncthreads();
    }
    if (!ok) break;
    for (int e = tid; e < nb * nb; e += NTHR) {
      const int c = e / nb, r = e - c * nb;
      if (r >= c) F[(size_t)(k0 + c) * m + k0 + r] = D[r][c];
    }
    if (tid == 0) {  // the right-hand side's row over the block's columns
      for (int c = 0; c < nb; ++c) {
        double v = ws[k0 + c];
        for (int p = 0; p < c; ++p) v = fma(-ws[k0 + p], D[c][p], v);
        ws[k0 + c] = v / D[c][c];
      }
    }
    const int r0 = k0 + CB;  // rows below the block (only after a full block: nb == CB)
    for (int r = r0 + tid; r < m; r += NTHR) {  // C21 row r: x C11^T = q by substitution
      double x[CB];
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        double v = F[(size_t)(k0 + c) * m + r];
#pragma unroll
        for (int p = 0; p < c; ++p) v = fma(-x[p], D[c][p], v);
        x[c] = v / D[c][c];
      }
#pragma unroll
      for (int c = 0; c < CB; ++c) F[(size_t)(k0 + c) * m + r] = x[c];
    }
    __syncthreads();  // the panel and w's block are visible to the workgroup; D is free again
    for (int r = r0 + tid; r < m; r += NTHR) {  // the rest of the right-hand side
      double v = ws[r];
#pragma unroll 4
      for (int p = 0; p < CB; ++p) v = fma(-ws[k0 + p], F[(size_t)(k0 + p) * m + r], v);
      ws[r] = v;
    }
    for (int jb = r0; jb < m; jb += CJ) {  // Q22 -= C21 C21^T, lower part, CJ columns a pass
      for (int r = jb + tid; r < m; r += NTHR) {
        double v[CJ];
#pragma unroll
        for (int j = 0; j < CJ; ++j) v[j] = (jb + j <= r) ? F[(size_t)(jb + j) * m + r] : 0.0;
#pragma unroll 4
        for (int p = 0; p < CB; ++p) {
          const double lrp = F[(size_t)(k0 + p) * m + r];
#pragma unroll
          for (int j = 0; j < CJ; ++j)
            if (jb + j <= r) v[j] = fma(-lrp, F[(size_t)(k0 + p) * m + jb + j], v[j]);
        }
#pragma unroll
        for (int j = 0; j < CJ; ++j)
          if (jb + j <= r) F[(size_t)(jb + j) * m + r] = v[j];
      }
    }
    __syncthreads();
  }
  if (!ok) {  // block-uniform
    const double nan = __builtin_nan("");
    for (int i = tid; i < m; i += NTHR) a.r[ro + s0 + i] = a.pvar[ro + s0 + i] = nan;
    if (tid == 0) {
      *lpf = nan;
      *fst = 1;  // GPRX_NOT_POSITIVE_DEFINITE
    }
    return;
  }
  if (tid == 0) {
    const double hl2pi = 0.91893853320467274178;  // 0.5 log(2 pi)
    double ww = 0.0;
    for (int i = 0; i < m; ++i) ww = fma(ws[i], ws[i], ww);
    *lpf = (sld - 0.5 * ww) - (double)m * hl2pi;
    *fst = 0;
  }
  __syncthreads();  // w has been read
  // r = C^-T w: us[k] = ws[k] / C_kk, then ws[i] -= C_ki us[k] for i < k
#pragma unroll 1
  for (int k = m - 1; k >= 0; --k) {
    const double uk = ws[k] / F[(size_t)k * m + k];  // every thread: ws[k] is final since the last barrier
    if (tid == 0) us[k] = uk;
    for (int i = tid; i < k; i += NTHR) ws[i] = fma(-F[(size_t)i * m + k], uk, ws[i]);
    __syncthreads();
  }
  for (int i = tid; i < m; i += NTHR) a.r[ro + s0 + i] = us[i];
  // var: column i of X = C^-1 in ascending k; the wave's first column i0 bounds the walk
  const int nset = (m + NTHR - 1) / NTHR;
  for (int set = 0; set < nset; ++set) {
    const int i = set * NTHR + tid;
    const int i0 = __builtin_amdgcn_readfirstlane(i - (tid & 63));
    if (i0 >= m) continue;  // wave-uniform; no barrier below
    const bool mine = i < m;
    double acc = 0.0, xd = 0.0;  // xd = X_ii, kept in a register: (i, i) holds C_ii
#pragma unroll 1
    for (int k = i0; k < m; ++k) {
      double s = (k == i) ? 1.0 : 0.0;
      const double* Ck = F + k;  // row k of C: element (k, l) at Ck[l m]
      for (int l = i0; l < k; ++l) {
        const double ckl = Ck[(size_t)l * m];  // the same address in every lane
        if (mine && l >= i) s = fma(-ckl, l == i ? xd : F[(size_t)l * m + i], s);  // X_li at (i, l) for l > i
      }
      if (mine && k >= i) {
        const double x = s / Ck[(size_t)k * m];
        if (k > i) F[(size_t)k * m + i] = x;
        else xd = x;
        acc = fma(x, x, acc);
      }
    }
    if (mine) a.pvar[ro + s0 + i] = acc;
  }
}

// ============================================================================================
// cv_final: mu_i = y_i - r, var_i back in point order (i = perm of the packed position), and
// logp[slot] = sum_V logp_V by k_loo_final's sum: thread t adds its folds t, t + 256, ... in ascending
// order, then the 256 partial sums by two_sum_block (gprx_loo.h).  A fold that failed leaves NaN at its points and in logp and the status 1; a slot
// whose evaluation failed reads NaN everywhere and keeps that status.   grid = B
// ============================================================================================
__global__ __launch_bounds__(NTHR) void k_cv_final(DevBatch db, CvArgs a) {
  const int slot = blockIdx.x, tid = threadIdx.x, N = db.N;
  if (!slot_active(db, slot)) return;  // block-uniform, before the first barrier
  const size_t ro = (size_t)slot * db.Npad;
  const int est = db.status[slot];
  if (est != 0) {  // block-uniform
    const double nan = __builtin_nan("");
    for (int i = tid; i < N; i += NTHR) a.mu[ro + i] = a.var[ro + i] = nan;
    for (int f = tid; f < a.F; f += NTHR) a.lpf[(size_t)slot * a.F + f] = nan;
    if (tid == 0) {
      a.logp[slot] = nan;
      a.st[slot] = est;
    }
    return;
  }
  const CvTab t = cv_tab(db, a, slot);
  for (int rp = tid; rp < N; rp += NTHR) {
    const int i = t.perm[rp];
    a.mu[ro + i] = db.Y[ro + i] - a.r[ro + rp];
    a.var[ro + i] = a.pvar[ro + rp];
  }
  double s = 0.0, e = 0.0;
  int b = 0;
  for (int f = tid; f < a.F; f += NTHR) {
    two_sum_acc(s, e, a.lpf[(size_t)slot * a.F + f], 0.0);
    b |= a.fst[(size_t)slot * a.F + f];
  }
  b = __syncthreads_or(b);  // any fold of the slot failed
  const double tot = two_sum_block(s, e);
  if (tid == 0) {
    a.logp[slot] = b ? __builtin_nan("") : tot;
    a.st[slot] = b ? 1 : 0;
  }
}

void launch_cv_pack(const DevBatch& b, const CvArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cv_pack, dim3(grid_blocks(b.B, b.nt)), dim3(NTHR), 0, s, b, a);
}
void launch_cv_kinv(const DevBatch& b, const CvArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cv_kinv, dim3(grid_blocks(b.B, (a.njmax + 3) / 4)), dim3(NTHR), 0, s, b, a);
}
void launch_cv_fold(const DevBatch& b, const CvArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cv_fold, dim3(grid_blocks(b.B, a.F)), dim3(NTHR), 0, s, b, a);
}
void launch_cv_final(const DevBatch& b, const CvArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cv_final, dim3(b.B), dim3(NTHR), 0, s, b, a);
}

}  // namespace gprx
