// gprx_factor.h -- the fused factorisation kernels: k_leaf and leaf9_body / k_leaf9 / k_node8.
// Uses FS, diag_tile_fast and diag_store of the single-tile routine, which gprx_kernels.hip
// defines above the include (k_diag_f keeps its place among the kernels).
//
// A part of gprx_kernels.hip, included there once and by no other file (the parts and their order
// are listed at its includes).
#pragma once

namespace gprx {

// ============================================================================================
// Fused leaf node: Cholesky + inverse of the n <= 4 diagonal tiles o..o+n-1 (a 256x256 block at
// most) in ONE workgroup per slot, replacing ~4n latency-bound launches of the recursion.
//   for k: diag(o+k); Lw[i,k] = K[i,k] Linv[k,k]^T (i > k); K[i,j] -= Lw[i,k] Lw[j,k]^T (i >= j > k)
//   then the off-diagonal inverse tiles by sub-diagonal s = i - j:
//     X = sum_{t=j}^{i-1} L[i,t] Linv[t,j]  (per wave quarter, in LDS),  Linv[i,j] = -Linv[i,i] X
// Each 64x64 tile task is split into four 64x16 column quarters, one per wave.  The X of a task is
// only re-read by the wave that computed it (its own 16 columns, kept in the wave's LDS buffer), so
// a wave-level barrier replaces a workgroup barrier between the two products.
// ============================================================================================
__device__ __forceinline__ void leaf_body(const DevBatch& db, int o, int n, int upd) {
  // every 64 x 64 tile task is split into four 64 x 16 column quarters, one per wave (wave w:
  // columns 16w..16w+15 of every tile of a step), so a step with fewer tiles than waves keeps
  // all four SIMDs busy; quarter-transposed stores through the wave's LDS buffer
  __shared__ double tbs[4 * 16 * (TS + 1)];
  __shared__ double zq[6][4][TS];  // n <= 4: z partials of the off-diagonal L^-1 quarters [tile][wave][row]
  __shared__ double dT[TS * FS], dXi[TS * FS];  // the diagonal routine's tile and inverse images
  __shared__ __attribute__((aligned(16))) double dcb[256];
  const int slot = blockIdx.x;
  if (!slot_active(db, slot)) return;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), cq = 16 * w;
  double* tb = tbs + w * 16 * (TS + 1);
  const size_t ld = db.ld, so = (size_t)slot * db.mat;
  // the leaf's tiles: from K (or S, upd) in step 0; every later step reads what this leaf's own
  // SYRK wrote to S
  double* S = db.S + so;
  const double* K0 = (upd ? db.S : db.K) + so;
  double* Lw = db.Lw + so;
  double* Li = db.Linv + so;
  double* Mt = db.Mt + so;
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  LEAF_TS(0);
  for (int k = 0; k < n; ++k) {
    const int tk = o + k, m = n - 1 - k;
    const double* xi = dXi;  // Linv[tk,tk] in LDS, read by the TRSM tasks below
    const double* K = k > 0 ? S : K0;
    diag_tile_fast(db, slot, tk, dT, dXi, dcb, k > 0, upd ? db.S : db.K, false);  // k > 0: the SYRK below left the tile in dT
    __syncthreads();
    LEAF_TS(1 + 3 * k);
    for (int t = 0; t < m; ++t) {  // TRSM: L[ti,tk] = K[ti,tk] Linv[tk,tk]^T
      const int ti = tk + 1 + t;
      d4 acc[QM];
#pragma unroll
      for (int a = 0; a < QM; ++a) acc[a] = (d4){0.0, 0.0, 0.0, 0.0};
      mma_64x16(acc, K + (size_t)tk * TS * ld + ti * TS, ld, xi + cq, FS, TS);
      accq_store(Lw + (size_t)(tk * TS + cq) * ld + ti * TS, ld, acc, 1.0);
    }
    diag_store(db, slot, tk, dXi, dcb);  // after the TRSM loads (dXi stays until the next diagonal)
    __syncthreads();
    LEAF_TS(2 + 3 * k);
    for (int c = 0; c < m; ++c)  // SYRK (lower trailing tiles)
      for (int a0 = 0; a0 < m - c; ++a0) {
        const int tj = tk + 1 + c, ti = tj + a0;
        const double* Cs = K + (size_t)(tj * TS + cq) * ld + ti * TS;
        double* Ct = S + (size_t)(tj * TS + cq) * ld + ti * TS;
        d4 acc[QM];  // -C - L L^T, stored negated
#pragma unroll
        for (int a = 0; a < QM; ++a)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[a][q] = -Cs[(size_t)(lk + 4 * q) * ld + 16 * a + lr];
        mma_64x16(acc, Lw + (size_t)tk * TS * ld + ti * TS, ld, Lw + (size_t)tk * TS * ld + tj * TS + cq, ld, TS);
        if (c == 0 && a0 == 0) {  // the next diagonal tile: straight into the diagonal routine's LDS
#pragma unroll
          for (int a = 0; a < QM; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int r = 16 * a + lr, cc = cq + lk + 4 * q;
              dT[cc * FS + r] = r >= cc ? -acc[a][q] : 0.0;
            }
        } else {
          accq_store(Ct, ld, acc, -1.0);
        }
      }
    __syncthreads();
    LEAF_TS(3 + 3 * k);
  }
  // off-diagonal inverse tiles by sub-diagonal s:  X = sum_{k=tj}^{ti-1} L[ti,k] Linv[k,tj] (kept
  // transposed in the wave's LDS buffer), Linv[ti,tj] = -Linv[ti,ti] X.  Wave w's quarter of
  // Linv[ti,tj] needs only its own quarter of X: no barrier between the two products.
  int kz = 0;  // off-diagonal tile index in (s, t) order
  for (int s = 1; s < n; ++s) {
    for (int t = 0; t < n - s; ++t, ++kz) {
      const int tj = o + t, ti = tj + s;
      double* Xt = Mt + (size_t)(ti * TS) * ld + tj * TS;  // Mt[tj,ti]
      d4 acc[QM];
#pragma unroll
      for (int a = 0; a < QM; ++a) acc[a] = (d4){0.0, 0.0, 0.0, 0.0};
      mma_64x16(acc, Lw + (size_t)tj * TS * ld + ti * TS, ld, Mt + (size_t)tj * TS * ld + tj * TS + cq, ld, s * TS);
      // this wave's quarter of X stays in its LDS buffer, transposed (tb[c][r] = X[r][cq + c]):
      // the second product reads it from there instead of a global round trip
#pragma unroll
      for (int a = 0; a < QM; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) tb[(lk + 4 * q) * (TS + 1) + 16 * a + lr] = acc[a][q];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int a = 0; a < QM; ++a) acc[a] = (d4){0.0, 0.0, 0.0, 0.0};
      mma_64x16_ldsb(acc, Li + (size_t)ti * TS * ld + ti * TS, ld, tb);
      __builtin_amdgcn_wave_barrier();  // the reads of X precede accq_store_t's writes to tb
      if (n <= 4) {  // this quarter's z partial, from the registers: sum_c Linv[r][cq + c] y[cq + c]
        const double* yq = yw_slot(db, slot) + tj * TS + cq;
        double yv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) yv[q] = yq[lk + 4 * q];
#pragma unroll
        for (int a = 0; a < QM; ++a) {
          double zt = 0.0;
#pragma unroll
          for (int q = 0; q < 4; ++q) zt = fma(-acc[a][q], yv[q], zt);
          zt = sum_xor32(sum_xor16(zt));
          if (lk == 0) zq[kz][w][16 * a + lr] = zt;
        }
      }
      accq_store(Li + (size_t)(tj * TS + cq) * ld + ti * TS, ld, acc, -1.0);
      accq_store_t(Xt + cq, ld, acc, -1.0, tb);
    }
    __syncthreads();
    LEAF_TS(12 + s);
  }
  // z partials of the off-diagonal L^-1 tiles of this leaf (the diagonal tiles' come from
  // diag_tile_fast).  n <= 4: the four quarters' partials from zq, summed in wave order.
  if (n <= 4) {
    const int r = threadIdx.x & 63;
    for (int k = threadIdx.x >> 6; k < n * (n - 1) / 2; k += 4) {
      int s = 1, t = k;
      while (t >= n - s) {
        t -= n - s;
        ++s;
      }
      const int tj = o + t, ti = tj + s;
      zp_row(db, slot, 2 * tj)[ti * TS + r] = ((zq[k][0][r] + zq[k][1][r]) + zq[k][2][r]) + zq[k][3][r];
      zp_row(db, slot, 2 * tj + 1)[ti * TS + r] = 0.0;
    }
    LEAF_TS(16);
    return;
  }
  // larger leaves: read the tiles back from L2 (this workgroup wrote them); 16 tiles per round
  // (the [4][16][65] buffer)
  __threadfence_block();
  {
    const int r = threadIdx.x & 63, qc = threadIdx.x >> 6;  // 4 quarters of 16 columns
    const int nod = n * (n - 1) / 2;
    for (int k0 = 0; k0 < nod; k0 += 16) {
      int k = 0;
      for (int s = 1; s < n; ++s)
        for (int t = 0; t < n - s; ++t, ++k) {
          if (k < k0 || k >= k0 + 16) continue;
          const int tj = o + t, ti = tj + s;
          const double* Lt = Li + (size_t)(tj * TS) * ld + ti * TS;
          const double* y = yw_slot(db, slot) + tj * TS;
          double acc = 0.0;
#pragma unroll
          for (int c = 16 * qc; c < 16 * qc + 16; ++c) acc = fma(Lt[(size_t)c * ld + r], y[c], acc);
          tbs[(4 * (k - k0) + qc) * TS + r] = acc;
        }
      __syncthreads();
      k = 0;
      for (int s = 1; s < n; ++s)
        for (int t = 0; t < n - s; ++t, ++k)
          if (qc == 0 && k >= k0 && k < k0 + 16) {
            const int tj = o + t, ti = tj + s;
            const double* pk = tbs + 4 * (k - k0) * TS;
            zp_row(db, slot, 2 * tj)[ti * TS + r] = ((pk[r] + pk[TS + r]) + pk[2 * TS + r]) + pk[3 * TS + r];
            zp_row(db, slot, 2 * tj + 1)[ti * TS + r] = 0.0;
          }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(NTHR) void k_leaf(DevBatch db, int o, int n, int upd) { leaf_body(db, o, n, upd); }
// ============================================================================================
// Workgroup-local hand-offs of the fused leaf (k_leaf9): progress words and counter barriers in
// LDS, polled by the waiting waves.  Every wait is bounded (2^24 polls, about half a second): a
// hand-off that never comes ends the kernel with status GPRX_DEVICE_ERROR (3) for the slot instead
// of a hung launch.
// ============================================================================================
__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void l9_release() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); }
__device__ __forceinline__ void l9_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }
__device__ __forceinline__ void lds_publish(int* p, int v) {
  // the writer's LDS and global stores are complete before the word changes
  l9_release();
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
constexpr int LW_SPIN = 1 << 24;
__device__ __forceinline__ void lw_timeout(const DevBatch& db, int slot) {
  if ((threadIdx.x & 63) == 0) db.status[slot] = 3;
}
// poll the LDS word *p until done(word), at most LW_SPIN times (then the slot's status; the caller
// goes on).  Only the loop: the callers keep their own fences and atomics.
template <class Pred>
__device__ __forceinline__ void lds_spin_until(const int* p, Pred done, const DevBatch& db, int slot) {
  for (int it = 0; !done(lds_load(p)); ++it) {
    if (it > LW_SPIN) {
      lw_timeout(db, slot);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}
__device__ __forceinline__ void lds_wait_gt(const int* p, int v, const DevBatch& db, int slot) {
  lds_spin_until(p, [v](int x) { return x > v; }, db, slot);
  l9_acquire();
}
__device__ __forceinline__ void lds_wait_ge(const int* p, int v, const DevBatch& db, int slot) {
  lds_spin_until(p, [v](int x) { return x >= v; }, db, slot);
  l9_acquire();
}
// ---- k_leaf9's diagonal wave: the diagonal routine of diag_tile_fast on one wave.  The 16 x 16
// factor+inverse is an unscaled elimination (no square root inside the 16-step loop: the columns
// are scaled by 1/sqrt(p_j) once at the end) with v_fmac_f64 taking the DPP row broadcast
// directly, one instruction per update instead of a 64-bit broadcast move and an fma.  A single
// wave issues one VALU instruction per ~4.5 cycles here, so the instruction count sets the time
// (scratch/factbench: 4346 -> about 3500 cycles per 16 x 16 block).  The TRSM, SYRK and inverse
// blocks of a panel are issued as one batch (all operand reads, then the MFMA chains interleaved,
// then the stores) instead of block after block.  The inverse image's upper blocks are never
// written (no reader touches them), and the tile's diagonal goes to ldiag[64] for the
// log-determinant, which a task wave sums.
// LDS writes of this wave complete and visible to its later reads (the compiler keeps the order)
__device__ __forceinline__ void wave_sync() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
template <int M>
__device__ __forceinline__ void fmac_bcast(double& acc, double src, double f) {
  // acc += src[lane M of this row] * f.  A VALU write followed by a DPP read of the same register
  // needs two wait states, which the compiler does not insert around inline assembly.  The only
  // DPP source is a step's pivot column u[.][j], last written by the previous step's update for
  // m = j; volatile keeps the updates in program order, so at least three updates (its X partner
  // and the m = j+1 pair) separate that write from the first read.
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(f), "i"(M));
}
template <int J, int M>
__device__ __forceinline__ void fact_updates(double (&a)[16], double (&y)[16], double au, double fa, double fy) {
  if constexpr (M < 16) {
    fmac_bcast<M>(a[M], au, fa);  // a[m] -= u[m][j] u[i][j] / p_j   (fa = -u[i][j] / p_j)
    fmac_bcast<M>(y[M], au, fy);  // W^-1[m][i] -= (u[m][j] / p_j) W^-1[j][i]   (fy = -W^-1[j][i] / p_j)
    fact_updates<J, M + 1>(a, y, au, fa, fy);
  }
}
template <int J>
__device__ __forceinline__ double row_bcast_c(double v) { return __builtin_amdgcn_mov_dpp(v, 0x150 + J, 0xF, 0xF, true); }
// Step J of the unscaled elimination A = U D^-1 U^T (U = L D^1/2, D = diag(p)): lane i holds row i
// of U (a) and column i of W^-1 (y; W = U D^-1 unit lower) and d = its running diagonal, so the
// next pivot is one DPP broadcast away and the step's critical path is the reciprocal of p_J (no
// square root: the columns are scaled by 1/sqrt(p_J) once, after the last step).
template <int J>
__device__ __forceinline__ void fact_step(double (&a)[16], double (&y)[16], double& d, double& pv, int lr, int& fl) {
  if constexpr (J < 16) {
    const double au = a[J], yu = y[J];
    const double p = row_bcast_c<J>(d);
    const double pk = (p > 0.0) ? p : 1.0;
    fl = (fl < 0 && !(p > 0.0)) ? J : fl;  // the first pivot <= 0 or NaN (continue with 1)
    pv = (lr == J) ? pk : pv;
    const double r0 = __builtin_amdgcn_rcp(pk);
    const double e = fma(-pk, r0, 1.0);
    const double ip = fma(r0, fma(e, e, e), r0);  // 1/p to the rounding level (error e^3)
    d = fma(-au * au, ip, d);
    fact_updates<J, J + 1>(a, y, au, -au * ip, -yu * ip);
    fact_step<J + 1>(a, y, d, pv, lr, fl);
  }
}
template <int J>
__device__ __forceinline__ void fact_scale(double (&a)[16], double (&y)[16], double rl, double sl, int lr) {
  if constexpr (J < 16) {
    const double rJ = row_bcast_c<J>(rl);  // 1/sqrt(p_J)
    a[J] = (lr > J) ? a[J] * rJ : (lr == J ? sl : 0.0);
    y[J] = y[J] * rJ;
    fact_scale<J + 1>(a, y, rl, sl, lr);
  }
}
// Panel P of the diagonal wave: the TRSM and SYRK blocks below and right of the 16 x 16 block P.
// The block's inverse Dinv_P[r][c] is read from the inverse image's diagonal block,
// Xi[(16 P + c) * FS + 16 P + r].
template <int P>
__device__ __forceinline__ void w1_panel(double* T, const double* Xi, int lr, int lk) {
  constexpr int NT = 3 - P;  // trailing blocks
  if constexpr (NT > 0) {
    constexpr int c0 = 16 * P;
    // TRSM: A_iP <- A_iP Dinv^T, i = P+1 .. 3
    double bv[4], av[NT][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bv[s] = Xi[(c0 + 4 * s + lk) * FS + c0 + lr];
#pragma unroll
      for (int i = 0; i < NT; ++i) av[i][s] = T[(c0 + 4 * s + lk) * FS + 16 * (P + 1 + i) + lr];
    }
    d4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < NT; ++i) acc[i] = mfma(av[i][s], bv[s], acc[i]);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) T[(c0 + lr) * FS + 16 * (P + 1 + i) + lk + 4 * q] = acc[i][q];
    wave_sync();
    // SYRK: A_ij -= A_iP A_jP^T for P < j <= i < 4
    double pv[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int s = 0; s < 4; ++s) pv[i][s] = T[(c0 + 4 * s + lk) * FS + 16 * (P + 1 + i) + lr];
    constexpr int NB = NT * (NT + 1) / 2;
    d4 sacc[NB], old[NB];
#pragma unroll
    for (int b = 0, j = 0; j < NT; ++j)
#pragma unroll
      for (int i = j; i < NT; ++i, ++b) {
#pragma unroll
        for (int q = 0; q < 4; ++q) old[b][q] = T[(16 * (P + 1 + j) + lr) * FS + 16 * (P + 1 + i) + lk + 4 * q];
        sacc[b] = (d4){0.0, 0.0, 0.0, 0.0};
      }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int b = 0, j = 0; j < NT; ++j)
#pragma unroll
        for (int i = j; i < NT; ++i, ++b) sacc[b] = mfma(pv[i][s], pv[j][s], sacc[b]);
#pragma unroll
    for (int b = 0, j = 0; j < NT; ++j)
#pragma unroll
      for (int i = j; i < NT; ++i, ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) T[(16 * (P + 1 + j) + lr) * FS + 16 * (P + 1 + i) + lk + 4 * q] = old[b][q] - sacc[b][q];
    wave_sync();
  }
}
// off-diagonal inverse blocks of sub-diagonal SD: X_ij = -Dinv_i sum_{k=j}^{i-1} L_ik X_kj, j = 0 .. 3-SD
template <int SD>
__device__ __forceinline__ void w1_inverse(const double* T, double* Xi, int lr, int lk) {
  constexpr int NJ = 4 - SD;
  d4 y[NJ], x[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) y[j] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < SD; ++kk) {
    double av[NJ][4], bv[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int i = j + SD, kb = j + kk;
        av[j][s] = T[(16 * kb + 4 * s + lk) * FS + 16 * i + lr];   // L_ik[lr][k]
        bv[j][s] = Xi[(16 * j + lr) * FS + 16 * kb + 4 * s + lk];  // X_kj[k][lr]
      }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < NJ; ++j) y[j] = mfma(av[j][s], bv[j][s], y[j]);
  }
  double dv[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s) dv[j][s] = Xi[(16 * (j + SD) + 4 * s + lk) * FS + 16 * (j + SD) + lr];  // Dinv_i[lr][4s+lk]
#pragma unroll
  for (int j = 0; j < NJ; ++j) x[j] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int j = 0; j < NJ; ++j) x[j] = mfma(dv[j][s], y[j][s], x[j]);
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) Xi[(16 * j + lr) * FS + 16 * (j + SD) + lk + 4 * q] = -x[j][q];
  wave_sync();
}
// the tile's failure (first pivot <= 0 or NaN), as diag_tile_fast records it
__device__ __forceinline__ void w1_status(const DevBatch& db, int slot, int jt, int fail, int l) {
  if (fail >= 0 && l == 0 && db.status[slot] == 0) {
    db.status[slot] = 1;
    db.info[slot] = jt * TS + fail + 1;
  }
}
__device__ __forceinline__ void diag_w1(const DevBatch& db, int slot, int jt, double* T, double* Xi, double* ldiag) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  int fail = -1;
  D_TS1(0);
  for (int P = 0; P < 4; ++P) {
    const int c0 = 16 * P;
    double a[16], y[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      a[k] = T[(c0 + k) * FS + c0 + lr];
      y[k] = (k == lr) ? 1.0 : 0.0;
    }
    double d = T[(c0 + lr) * FS + c0 + lr], pv = 1.0;
    int fl = -1;
    fact_step<0>(a, y, d, pv, lr, fl);
    fl = __builtin_amdgcn_readfirstlane(fl);
    if (fail < 0 && fl >= 0) fail = c0 + fl;
    {
      double sl, rl;
      sqrt_rsqrt(pv, sl, rl);  // lane i: sqrt(p_i), 1/sqrt(p_i)
      fact_scale<0>(a, y, rl, sl, lr);
    }
    if (l < 16) {
#pragma unroll
      for (int k = 0; k < 16; ++k) T[(c0 + k) * FS + c0 + l] = (k <= l) ? a[k] : 0.0;  // row l of L_PP
      ldiag[c0 + l] = a[l];
    }
    __builtin_amdgcn_wave_barrier();
    if (l < 16) {
#pragma unroll
      for (int r = 0; r < 16; ++r) Xi[(c0 + l) * FS + c0 + r] = y[r];  // column l of Dinv
    }
    wave_sync();
    D_TS1(1 + 2 * P);
    switch (P) {
      case 0: w1_panel<0>(T, Xi, lr, lk); break;
      case 1: w1_panel<1>(T, Xi, lr, lk); break;
      case 2: w1_panel<2>(T, Xi, lr, lk); break;
      default: break;
    }
    D_TS1(2 + 2 * P);
  }
  w1_inverse<1>(T, Xi, lr, lk);
  w1_inverse<2>(T, Xi, lr, lk);
  w1_inverse<3>(T, Xi, lr, lk);
  D_TS1(9);
  w1_status(db, slot, jt, fail, l);
}

struct Leaf9Sync {
  int tk;          // task-wave barrier counter (monotonic, 7 per barrier)
  int ch;          // chain-wave barrier counter (4 per barrier)
  int diag_done;   // diagonal tiles factored and inverted
  int tile_ready;  // diagonal tiles handed to wave 0 (tile 0 at the start)
  int xfree;       // steps whose readers of dX[k & 1] are done
  int crit;        // critical SYRK items done (monotonic over the steps)
};
constexpr int L9_TW = 7;
// Phase-A items go round L9_HW = 6 task waves, the three off the chain first: 5, 6, 7, 1, 2, 3.
// Wave 4 is the diagonal wave's SIMD-mate (waves w and w + 4 of a workgroup share a SIMD,
// scratch/hwid_probe.hip), and the fp64 VALU of the diagonal routine shares that SIMD's one fp64
// pipe with the mate's MFMAs: without items on wave 4 (it keeps its chain quarter, while wave 0
// waits), node8 2.741 -> 2.723 ms per step at B = 240 and 2.998 -> 2.957 ms for CP at B = 1014
// against all seven task waves (same box, two pairs each; the same items, so bit-identical).
constexpr int L9_HW = 6;
// Phase B (the SYRK items and the Y items of the next inverse row) runs while the diagonal wave
// waits for the next chain, so its round robin keeps wave 4 (L9_HWB = 7): otherwise its SIMD idles
// through phase B.
constexpr int L9_HWB = 7;
// phase B of step k (m = n - 1 - k trailing tiles per edge): the SYRK tiles the next step needs,
// column k + 1 below the diagonal and the next diagonal tile, are its first nc tiles in the
// column-major enumeration that skips (k + 1, k + 1)
__host__ __device__ constexpr int l9_crit_tiles(int m) { return m <= 0 ? 0 : (m - 1) + (m >= 2 ? 1 : 0); }
__device__ __forceinline__ void lds_count(int* p) {  // one more item done (its stores before the count)
  l9_release();
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// The diagonal tile's four store quarters go to waves 1, 5, 6, 7.
__device__ __forceinline__ int l9_store_wave(int e) { return e > 0 ? 4 + e : 1; }
__device__ __forceinline__ int l9_wave_of(int e) {
  const int r = e % L9_HW;
  return r < 3 ? 5 + r : r - 2;
}
__device__ __forceinline__ void ctr_barrier(int* ctr, int& gen, int nw, const DevBatch& db, int slot) {
  gen += nw;
  l9_release();
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  lds_spin_until(ctr, [gen](int x) { return x >= gen; }, db, slot);
  l9_acquire();
}
// acc[a] += sum_k Lx[16a + lk + 4q][k] b(k) for a triangular Lx (lower; LDS image Lx[c * FS + r]):
// chunk s (k = 4s .. 4s + 3) reaches only the blocks a >= s / 4.  b[s] is lane (lr, lk)'s B operand
// of chunk s.
__device__ __forceinline__ void lmma_tri(d4 (&acc)[QM], const double* Lx, const double (&b)[16]) {
  const int l = threadIdx.x & 63, llo = (l >> 4) * FS + (l & 15);
#pragma unroll
  for (int s = 0; s < 16; ++s)
#pragma unroll
    for (int a = s >> 2; a < QM; ++a) acc[a] = mfma(Lx[4 * s * FS + 16 * a + llo], b[s], acc[a]);
}

__device__ __forceinline__ void leaf9_body(const DevBatch& db, int o, int upd) {
  constexpr int n = 4;
  extern __shared__ __attribute__((aligned(16))) double l9a[];
  double* dT = l9a;                  // wave 0's tile image
  double* dXb = dT + TS * FS;        // two inverse images
  double* Tc = dXb + 2 * TS * FS;    // the chain's L(k+1,k), Tc[c * FS + r] = L[r][c]
  double(*zq)[4][TS] = (double(*)[4][TS])(Tc + TS * FS);  // z partials: 6 off-diagonal tiles
  double(*zqd)[4][TS] = zq + 6;                            // ... and the 4 diagonal tiles
  double* ldiag = (double*)(zqd + 4);  // [2][64]: the diagonal of L_kk (log-determinant)
  Leaf9Sync& sy = *(Leaf9Sync*)(ldiag + 2 * TS);
  const int slot = blockIdx.x;
  if (slot >= db.B || !slot_active(db, slot)) return;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const size_t ld = db.ld, so = (size_t)slot * db.mat;
  // 32-bit element offsets within a slot's matrix: a uniform part plus one of three lane parts
  const int ldi = (int)ld;
  const int lo = lk * ldi + lr;   // row + lr, column + lk
  const int lo2 = lr * ldi + lk;  // row + lk, column + lr
  const int llo = lk * FS + lr;   // LDS images: row + lr, column + lk
  double* S = db.S + so;
  const double* K0 = (upd ? db.S : db.K) + so;
  double* Lw = db.Lw + so;
  double* Li = db.Linv + so;
  double* Mt = db.Mt + so;
  const double* Y = yw_slot(db, slot);
  {  // tile o into wave 0's image (all eight waves, all loads in flight first)
    const double* A = K0 + (size_t)o * TS * ld + o * TS;
    double v[TS * TS / (2 * NTHR)];
#pragma unroll
    for (int k = 0; k < TS * TS / (2 * NTHR); ++k) {
      const int e = threadIdx.x + k * 2 * NTHR, r = e & 63, c = e >> 6;
      v[k] = (r >= c) ? A[(size_t)c * ld + r] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < TS * TS / (2 * NTHR); ++k) {
      const int e = threadIdx.x + k * 2 * NTHR, r = e & 63, c = e >> 6;
      dT[c * FS + r] = v[k];
    }
    if (threadIdx.x == 0) {
      sy.tk = 0;
      sy.ch = 0;
      sy.diag_done = 0;
      sy.tile_ready = 1;
      sy.xfree = 0;
      sy.crit = 0;
    }
  }
  __syncthreads();
  if (wave == 0) {  // ---- wave 0: the diagonal tiles
    L9_TS(0);
    for (int k = 0; k < n; ++k) {
      lds_wait_gt(&sy.tile_ready, k, db, slot);
      if (k >= 2) lds_wait_gt(&sy.xfree, k - 2, db, slot);  // step k-2's readers of dX[k & 1] done
      L9_TS(1 + 2 * k);
      diag_w1(db, slot, o + k, dT, dXb + (k & 1) * TS * FS, ldiag + (k & 1) * TS);
      L9_TS(2 + 2 * k);
      lds_publish(&sy.diag_done, k + 1);
    }
  } else {  // ---- the task waves
    // chain quarter of this wave (-1: off the chain): waves 4, 1, 2, 3 -> 0, 1, 2, 3
    const int cw = wave == 4 ? 0 : (wave <= 3 ? wave : -1);
    const int cq = 16 * (cw < 0 ? 0 : cw);
    int gen = 0, cgen = 0;
    d4 yh[2][QM];       // held Y items (inverse row of the next step)
#pragma unroll
    for (int h = 0; h < 2; ++h) acc_zero4(yh[h]);
    // the chain's first operand of step k, A(o+k+1, o+k) rows cq.., staged in the idle inverse
    // image dX[(k+1) & 1] (its step k-1 readers are past their barrier; wave 0 writes it again only
    // after this chain hands tile k+1 over), Bs[c * FS + r] = A[r][c], this wave's rows only
    auto preload = [&](int k) {
      const double* Kc = k > 0 ? S : K0;
      const int kk = o + k, k1 = kk + 1;
      double* Bs = dXb + ((k + 1) & 1) * TS * FS;
      double v[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) v[s] = Kc[(kk * TS + 4 * s) * ldi + k1 * TS + cq + lo];
#pragma unroll
      for (int s = 0; s < 16; ++s) Bs[4 * s * FS + cq + llo] = v[s];
    };
    if (cw >= 0) preload(0);
    // phase B (and the held inverse items): round-robin position, waves 4, 1, 2, 3 first (wave 4
    // alone on its SIMD while wave 0 waits; waves 5-7 share SIMDs with the older waves 1-3, which
    // win issue arbitration: a younger wave's first item took 18-20 us against 10-11 us in the
    // leaf timeline), so the critical items land on the waves that run them fastest
    const int rw = wave == 4 ? 0 : (wave <= 3 ? wave : wave - 1);
    int ncrit = 0;  // critical SYRK items of the steps so far (sy.crit's target)
    int nc4p = 0;   // critical items of the previous step's phase B (the held items' offset)
    for (int k = 0; k < n; ++k) {
      const int kk = o + k;
      const double* Kc = k > 0 ? S : K0;
      const double* dX = dXb + (k & 1) * TS * FS;
      // items of Y(k, j) held since the previous step: e = 4 j + c, phase-B item g = nc4p + e on
      // wave l9_wave_of(g); this wave's h-th one is g = g0 + 7 h (g0: its first g >= nc4p)
      const int nyp = 4 * k;  // Y(k, j), j < k
      const int g0p = nc4p + ((rw - nc4p) % L9_HWB + L9_HWB) % L9_HWB;
      lds_wait_gt(&sy.diag_done, k, db, slot);
      if (wave == 5) L9_TS(9 + 4 * k);
      // ---- phase A: the chain; the held inverse items of row k; the diagonal tile's stores; the
      //      other TRSMs of column k
      if (k < n - 1 && cw >= 0) {
        const int k1 = kk + 1;
        d4 cp[QM];  // -A(k1, k1) rows cq.. (blocks a <= cw): loaded under the first product
#pragma unroll
        for (int a = 0; a < QM; ++a)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            cp[a][q] = -Kc[(k1 * TS + 16 * a + 4 * q) * ldi + k1 * TS + cq + lo];  // upper blocks: masked below
        double bp[16];
        {
          const double* Bs = dXb + ((k + 1) & 1) * TS * FS;
#pragma unroll
          for (int s = 0; s < 16; ++s) bp[s] = Bs[4 * s * FS + cq + llo];
        }
        d4 u[QM];
        acc_zero4(u);
        lmma_tri(u, dX, bp);  // L(k1, kk) rows cq.. (transposed)
#pragma unroll
        for (int a = 0; a < QM; ++a)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            Lw[(kk * TS + 16 * a + 4 * q) * ldi + k1 * TS + cq + lo] = u[a][q];
            Tc[(16 * a + 4 * q) * FS + cq + llo] = u[a][q];
          }
        ctr_barrier(&sy.ch, cgen, 4, db, slot);
        // S(k1, k1) rows cq.. = A - L L^T: M = L from Tc, B operand = this wave's own rows of L
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const double b = u[s >> 2][s & 3];
#pragma unroll
          for (int a = 0; a < QM; ++a)
            cp[a] = mfma(Tc[4 * s * FS + 16 * a + llo], b, cp[a]);
        }
#pragma unroll
        for (int a = 0; a < QM; ++a)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int x = 16 * a + lk + 4 * q;  // column; row cq + lr
            dT[(16 * a + 4 * q) * FS + cq + llo] = (cq + lr >= x) ? -cp[a][q] : 0.0;
          }
        ctr_barrier(&sy.ch, cgen, 4, db, slot);
        if (cw == 0) lds_publish(&sy.tile_ready, k + 2);
        if (wave == 4) L9_TS(10 + 4 * k);
      }
      // held items: X(k, j) = -Linv_kk Y(k, j), columns cq.. of tile (kk, o + j)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int e = g0p + L9_HWB * h - nc4p;
        if (rw >= 0 && e < nyp) {
          const int j = e >> 2, c = e & 3, tj = o + j, xq = 16 * c;
          double b[16];
#pragma unroll
          for (int s = 0; s < 16; ++s) b[s] = yh[h][s >> 2][s & 3];
          d4 x[QM];
          acc_zero4(x);
          lmma_tri(x, dX, b);
          const double yv = Y[tj * TS + xq + lr];
#pragma unroll
          for (int a = 0; a < QM; ++a) {
            double zt[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const double v = -x[a][q];  // Linv(kk, tj)[16a + lk + 4q][xq + lr]
              Li[(tj * TS + xq) * ldi + kk * TS + 16 * a + 4 * q + lo2] = v;
              Mt[(kk * TS + 16 * a + 4 * q) * ldi + tj * TS + xq + lo] = v;  // Mt(tj, kk)^T
              zt[q] = row_sum16(v * yv);
            }
            if (lr == 0) {
              const int kz = k * (k - 1) / 2 + j;
#pragma unroll
              for (int q = 0; q < 4; ++q) zq[kz][c][16 * a + lk + 4 * q] = zt[q];
            }
          }
        }
      }
      // general phase-A items after the held ones: e = nyp.. : the diagonal tile's stores (4
      // column quarters), then TRSM T(i, kk) rows (4 quarters per tile, i = kk + 2 ..)
      {
        const int nt1 = n - 2 - k > 0 ? n - 2 - k : 0;
        const int na = 4 + 4 * nt1;
        bool waited = false;
        for (int e = 0; e < na; ++e) {
          if ((e < 4 ? l9_store_wave(e) : l9_wave_of(nyp + e - 4)) != wave) continue;
          const int c = e & 3, xq = 16 * c;
          if (e >= 4 && !waited) {  // S(ti, kk): the previous step's critical items
            lds_wait_ge(&sy.crit, ncrit, db, slot);
            waited = true;
          }
          if (e < 4) {  // columns xq.. of the diagonal tile: Linv, Mt = Linv^T, z partial
            double* Lc = Li + (size_t)kk * TS * ld + kk * TS;
            double* Mc = Mt + (size_t)kk * TS * ld + kk * TS;
            const int r = l;
            double t = 0.0;
#pragma unroll 4
            for (int cc = xq; cc < xq + 16; ++cc) {
              const double xv = r >= cc ? dX[cc * FS + r] : 0.0;
              Lc[(size_t)cc * ld + r] = xv;
              Mc[(size_t)cc * ld + r] = (cc >= r) ? dX[r * FS + cc] : 0.0;
              t = fma(xv, Y[kk * TS + cc], t);
            }
            zqd[k][c][r] = t;
            if (c == 0) {  // the tile's log-determinant part from wave 0's copy of the diagonal
              const double lsum = wave_sum(log(ldiag[(k & 1) * TS + l]));
              if (l == 0) db.logdet_part[(size_t)slot * db.nt + kk] = lsum;
            }
          } else {  // T(ti, kk) rows xq..: L(ti, kk)[xq + lr][x] = sum_k A[xq + lr][k] Linv_kk[x][k]
            const int ti = kk + 2 + ((e - 4) >> 2);
            double b[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) b[s] = Kc[(kk * TS + 4 * s) * ldi + ti * TS + xq + lo];
            d4 u[QM];
            acc_zero4(u);
            lmma_tri(u, dX, b);
#pragma unroll
            for (int a = 0; a < QM; ++a)
#pragma unroll
              for (int q = 0; q < 4; ++q) Lw[(kk * TS + 16 * a + 4 * q) * ldi + ti * TS + xq + lo] = u[a][q];
          }
        }
      }
      ctr_barrier(&sy.tk, gen, L9_TW, db, slot);
      if (wave == 5) {
        lds_publish(&sy.xfree, k + 1);  // every reader of dX[k & 1] in step k is past the barrier
        L9_TS(11 + 4 * k);
      }
      if (k == n - 1) break;
      // ---- phase B (round 5: no closing barrier): items in the order the next step needs them,
      //      g = 0.. on wave l9_wave_of(g):
      //        the critical SYRK rows (column kk+1 below the diagonal and tile (kk+2, kk+2): the next
      //        step's chain and TRSMs read them, after sy.crit counts them);
      //        Y(k+1, j), j <= k (held for the next phase A);
      //        the other SYRK rows (read only after the next phase A's barrier).
      //      The chain waves then wait for the critical count and stage the next chain operand.
      {
        const int k1 = kk + 1;
        const int ny = 4 * (k + 1);
        const int m = n - 1 - k;  // trailing tiles per edge
        const int nsy = m * (m + 1) / 2 - 1;
        const int nc4 = 4 * l9_crit_tiles(m);
        [[maybe_unused]] int nb = 0;
        W_TS(8 * k);
        // SYRK row item e (tile e / 4 of the enumeration, quarter e % 4)
        auto syrk_item = [&](int e) {
          const int c = e & 3, xq = 16 * c;
          int u = (e >> 2) + 1, cc = 0;  // lower trailing tile u (column-major), skipping (k1, k1)
          while (u >= m - cc) {
            u -= m - cc;
            ++cc;
          }
          const int tj = k1 + cc, ti = tj + u;
          // S(ti, tj) rows xq..: OUT[x][xq + lr] = S[xq + lr][x], M = L(tj, kk), N = L(ti, kk) rows xq..
          // (a diagonal tile's blocks above the diagonal are formed and stored too: no reader uses them)
          d4 acc[QM];
          // row-packed core: block a holds OUT rows 32 (a / 2) + (a % 2) + 2 lk + 8 q
          const int lop = 2 * lk * ldi + lr;
#pragma unroll
          for (int a = 0; a < QM; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q)
              acc[a][q] = -Kc[(tj * TS + 32 * (a >> 1) + (a & 1) + 8 * q) * ldi + ti * TS + xq + lop];
          mma_rd_pk(acc, Lw + (size_t)kk * TS * ld + tj * TS, ld, Lw + (size_t)kk * TS * ld + ti * TS + xq, ld, TS);
#pragma unroll
          for (int a = 0; a < QM; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q)
              S[(tj * TS + 32 * (a >> 1) + (a & 1) + 8 * q) * ldi + ti * TS + xq + lop] = -acc[a][q];
          W_TS(8 * k + 1 + (nb < 5 ? nb++ : 5));
        };
        for (int g = rw < 0 ? nc4 : rw; g < nc4; g += L9_HWB) {
          syrk_item(g);
          lds_count(&sy.crit);
        }
        const int g0 = nc4 + ((rw - nc4) % L9_HWB + L9_HWB) % L9_HWB;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int e = g0 + L9_HWB * h - nc4;
          if (rw >= 0 && e < ny) {
            const int j = e >> 2, c = e & 3, tj = o + j, xq = 16 * c;
            // Y(k1, tj)[:, xq..] = sum_{m=tj}^{kk} L(k1, m) Linv(m, tj): M = Lw row k1, N = Mt row tj
            // (Linv(m, tj)^T); Linv(tj, tj)'s columns xq.. are zero above row xq: K starts at xq
            acc_zero4(yh[h]);
            mma_rd(yh[h], Lw + (size_t)(tj * TS + xq) * ld + k1 * TS, ld, Mt + (size_t)(tj * TS + xq) * ld + tj * TS + xq, ld,
                   (k1 - tj) * TS - xq);
            W_TS(8 * k + 1 + (nb < 5 ? nb++ : 5));
          }
        }
        for (int g = rw < 0 ? 4 * nsy + ny : nc4 + ny + ((rw - nc4 - ny) % L9_HWB + L9_HWB) % L9_HWB; g < 4 * nsy + ny; g += L9_HWB)
          syrk_item(g - ny);
        W_TS(8 * k + 7);
        ncrit += nc4;
        nc4p = nc4;
      }
      if (wave == 5) L9_TS(12 + 4 * k);
      if (cw >= 0 && k + 1 < n - 1) {
        lds_wait_ge(&sy.crit, ncrit, db, slot);  // S(kk+2, kk+1) and S(kk+2, kk+2) for the chain
        preload(k + 1);
      }
    }
  }
  __syncthreads();
  if (wave == 0) L9_TS(25);
  // z partials: the diagonal tiles' and the off-diagonal tiles' quarters summed in quarter order
  for (int e = threadIdx.x; e < (n + 6) * TS; e += 2 * NTHR) {
    const int t = e >> 6, r = e & 63;
    int ti, tj;
    double v;
    if (t < n) {
      ti = tj = o + t;
      v = ((zqd[t][0][r] + zqd[t][1][r]) + zqd[t][2][r]) + zqd[t][3][r];
    } else {
      const int kz = t - n;
      int k = 1;
      while (k * (k + 1) / 2 <= kz) ++k;
      ti = o + k;
      tj = o + (kz - k * (k - 1) / 2);
      v = ((zq[kz][0][r] + zq[kz][1][r]) + zq[kz][2][r]) + zq[kz][3][r];
    }
    zp_row(db, slot, 2 * tj)[ti * TS + r] = v;
    zp_row(db, slot, 2 * tj + 1)[ti * TS + r] = 0.0;
  }
}
constexpr size_t leaf9_lds_bytes() {
  return (4 * TS * FS + 10 * 4 * TS + 2 * TS) * sizeof(double) + sizeof(Leaf9Sync);
}
// k_node8's LINV21 epilogue puts its eight waves' transpose buffers in the leaf's LDS
static_assert(leaf9_lds_bytes() >= 2 * linv21_lds_bytes(), "k_node8: LINV21 transpose buffers exceed the leaf's LDS");
__global__ __launch_bounds__(2 * NTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_leaf9(DevBatch db, int o, int upd) {
  leaf9_body(db, o, upd);
}
// A whole 8-tile recursion node (512 x 512) in one launch, one 8-wave workgroup per slot, a
// workgroup barrier between the phases: the top leaf (leaf9_body), TRSM and SYRK + TT, the bottom
// leaf (tiles updated into S) and LINV21 (L^-1_21 = -L22^-1 T) -- five launches of the recursion
// with the same tile work.  The GEMM phases run the slot's units on the two halves of the
// workgroup (gemm_unit); LINV21's transposed Mt store uses the leaf's LDS, dead after its barrier.
// Round 5: the node's second half joined the first (it was a launch of its own, k_node9b), so each
// slot goes on to its bottom leaf when its own SYRK + TT is done instead of every slot waiting for
// the slowest one at the launch boundary: 2.84-2.89 -> 2.79-2.82 ms per step for the four nodes.
__global__ __launch_bounds__(2 * NTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_node8(DevBatch db, int o, int upd) {
  const int slot = blockIdx.x;
  if (slot >= db.B || !slot_active(db, slot)) return;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = wave >> 2, w = wave & 3;
  const GemmGeom none{OP_NONE, 0, 0, 0};
  N_TS(0);
  N_TS(6);
  N_TS(7);
  leaf9_body(db, o, upd);
  __syncthreads();
  N_TS(1);
  gemm_unit<false, REV_B, false>(db, GemmGeom{OP_TRSM, o, 4, 8, upd}, none, slot, half, w, 2);
  __syncthreads();
  N_TS(2);
  gemm_unit<false, TRI_A_FIRST, false>(db, GemmGeom{OP_SYRK, o, 4, 8, upd}, GemmGeom{OP_TT, o, 4, 8, upd}, slot, half, w, 2);
  __syncthreads();
  N_TS(3);
  leaf9_body(db, o + 4, 1);
  __syncthreads();
  N_TS(4);
  gemm_unit<false, REV_A, false>(db, GemmGeom{OP_LINV21, o, 4, 8, upd}, none, slot, half, w, 2);
  N_TS(5);
}

}  // namespace gprx
