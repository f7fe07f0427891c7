// gprx_cores.h -- the wave-level MFMA cores (operand fragments, operand addressing, every mma_* loop)
// and the accumulator helpers.
//
// A part of gprx_kernels.hip, included there once and by no other file (the parts and their order
// are listed at its includes).
#pragma once

namespace gprx {

// ---------------------------------------------------------------------------------------------
// Wave GEMM core:  acc[a][b] += A(64 x K) * B(32 x K)^T
//   A rows r0..r0+63 with element (r, k) at A[r + k*lda] (column-major; rows contiguous); B rows
//   c0..c0+31 likewise.  The MFMA is issued with the operands swapped (A-op <- B rows, B-op <- A
//   rows) so that lane&15 indexes the output ROW: acc[a][b] lane l, reg q holds
//       C[16a + (l&15)][16b + (l>>4) + 4q]
//   (f64 16x16x4 C/D map: row = (lane>>4) + 4 reg, col = lane & 15; verified on gfx950), which
//   makes stores into column-major C contiguous over 16 lanes.
//   K is a multiple of 16, taken in 16-deep register stages.
// ---------------------------------------------------------------------------------------------
constexpr int WM = 4, WN = 2;
struct Frag {
  double a[4][WM], b[4][WN];
};
__device__ __forceinline__ void frag_load(Frag& f, const double* pa, const double* pb, size_t sa, size_t sb) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int a = 0; a < WM; ++a) f.a[s][a] = pa[s * sa + 16 * a];
#pragma unroll
    for (int b = 0; b < WN; ++b) f.b[s][b] = pb[s * sb + 16 * b];
  }
}
__device__ __forceinline__ void frag_mma(d4 (&acc)[WM][WN], const Frag& f) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
      for (int b = 0; b < WN; ++b) acc[a][b] = mfma(f.b[s][b], f.a[s][a], acc[a][b]);
}
// single register stage (no prefetch): latency is hidden by occupancy instead (4 waves/SIMD)
__device__ __forceinline__ void mma_64x32_s1(d4 (&acc)[WM][WN], const double* __restrict__ A, size_t lda,
                                             const double* __restrict__ B, size_t ldb, int K) {
  // K is wave-uniform but derived from threadIdx.x >> 6; make that provable, otherwise hipcc
  // builds a divergent loop and moves all accumulator registers VGPR<->AGPR every stage.
  const int nst = __builtin_amdgcn_readfirstlane(K >> 4);
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const double* pa = A + lr + (size_t)lk * lda;
  const double* pb = B + lr + (size_t)lk * ldb;
  const size_t sa = 4 * lda, sb = 4 * ldb;
  for (int it = 0; it < nst; ++it) {
    Frag f;
    frag_load(f, pa + (size_t)it * 4 * sa, pb + (size_t)it * 4 * sb, sa, sb);
    frag_mma(acc, f);
  }
}

// ---------------------------------------------------------------------------------------------
// 64 x 64 wave core (k_gemm, k_lauum_grad): acc[a][b] += A(64 x K) B(64 x K)^T, same operand and
// C maps as mma_64x32_s1 (acc[a][b] lane l reg q = C[16a + (l&15)][16b + (l>>4) + 4q]), 16 MFMAs
// per 8 fragment loads, two register stages of depth 8 (Q4SD = 2 MFMA sub-steps) in ping-pong,
// ~210 VGPRs: two waves per SIMD.  Scheduling barriers pin the two halves of an iteration (stage
// it+1's loads with stage it's MFMAs, stage it+2's loads with stage it+1's MFMAs): without them the
// compiler sinks the prefetch next to the other stage's loads and waits on vmcnt(0) before the
// first MFMA, serialising load and compute.  Inside a half, group barriers interleave one load per
// two MFMAs (round 2: every GEMM 2-3% faster than with the loads issued as one burst before the
// MFMAs, step 43.25 -> 42.7 ms at B=240, same-box A/B).  Measured on MI355X before the interleave
// (scratch/big_core_bench.hip, 192 batched 1024 x 1024 panels, 2 waves/SIMD): 70.9 / 68.5 / 64.2
// TF/s at K = 1024 / 512 / 256, against 64.5 / 67.4 / 63.0 for depth-16 stages without the
// barriers (and 60.2 / 57.4 / 52.7 for depth 16 with them: 25 spills).
// ---------------------------------------------------------------------------------------------
constexpr int QM = 4, QN = 4, Q4SD = 2;
struct Frag4 {
  double a[Q4SD][QM], b[Q4SD][QN];
};
// NB < QN: only the first NB 16-column blocks of B (the prediction's last, partly padded test tile)
template <int NB = QN>
__device__ __forceinline__ void frag4_mma(d4 (&acc)[QM][QN], const Frag4& f) {
#pragma unroll
  for (int s = 0; s < Q4SD; ++s)
#pragma unroll
    for (int a = 0; a < QM; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[a][b] = mfma(f.b[s][b], f.a[s][a], acc[a][b]);
}
// mma_64x64 with triangular operand tiles and lower-only outputs skipped at 16 x 16-block
// granularity.  A 64-K tile of the K loop is 8 stages (k = 8s..8s+7), i.e. 4 loop trips of 2 stages.
//   TRI_A_FIRST  A's first K tile is upper triangular (explicit zeros below the diagonal): row block
//                a is zero for k < 16a, so trip t of that tile needs rows a <= t (lauum: A = Mt[ti, ti:];
//                TT: A = Mt[ti, ti:]).
//   TRI_AB_FIRST the same with B = A (a diagonal output tile of the lauum), and only the output blocks
//                b <= a are formed (the caller ignores the upper ones): trip t needs blocks a, b <= t.
//   REV_A, REV_B the K walk reversed from a lower-triangular last tile of A / of B (mma_64x64_pm).
// The peeled trips carry compile-time masks; skipped products are exact zeros, so the sums are
// bit-identical to the full core's.  Shared panels (B = A) load the fragments once.
// (the values name the k_gemm<PM> instances in profiles)
enum CoreMode { PLAIN = 0, TRI_A_FIRST = 1, TRI_AB_FIRST = 2, REV_A = 6, REV_B = 7 };
// Operand addressing: element (row, k) at base[row + k ld]; lane (lr, lk) of sub-step s of stage st
// reads k = 8 st + 4 s + lk of rows 16 a + lr (a 16-row block reads 128 contiguous bytes).  Round 5:
// buffer loads, the lane's byte offset in a VGPR (fixed), the stage and sub-step offsets in SGPRs
// and the row block in the instruction's offset field, so the K loop has no VALU address
// arithmetic (64-bit global addresses needed a v_lshl_add_u64 per address per stage, and every
// VALU instruction takes issue cycles from the other wave's MFMAs on gfx950: the core pattern on an
// L2-resident panel ran at 76.4 TF/s with global loads and 77.6 with buffer loads,
// scratch/mfma_pattern.hip, profiles/r05_mfma_valu_pattern.txt).
struct CorePtr {
  __amdgpu_buffer_rsrc_t r;  // over the operand from its tile origin
  int vo;                    // this lane's byte offset: row lr, column lk
  int o;                     // byte offset of stage 0, sub-step 0 (wave-uniform)
  int st, sub;               // stage / sub-step strides in bytes (negative: a backward walk)
};
__device__ __forceinline__ CorePtr core_ptr(const double* X, size_t ld) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const int L = (int)ld * (int)sizeof(double);
  return CorePtr{buffer_rsrc(X, 0x7ffffff0), lr * (int)sizeof(double) + lk * L, 0, 8 * L, 4 * L};
}
__device__ __forceinline__ CorePtr core_rev(CorePtr c, int nst) {  // stages and sub-steps backward
  c.o += (nst - 1) * c.st + c.sub;
  c.st = -c.st;
  c.sub = -c.sub;
  return c;
}
// The same walk through 64-bit global addresses (the round-4 form): k_node8 keeps it, since its
// GEMM phases sit beside the fused leaf's state and the buffer form's SGPR resources pushed that
// kernel from 8 to 58 spilled VGPRs.
struct CorePtrG {
  const double* p;  // this lane's address of stage 0, sub-step 0, row block 0
  ptrdiff_t st;     // stage stride
  ptrdiff_t sub;    // sub-step stride
};
__device__ __forceinline__ CorePtrG core_ptr_g(const double* X, size_t ld) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const ptrdiff_t L = (ptrdiff_t)ld;
  return CorePtrG{X + lr + lk * L, 8 * L, 4 * L};
}
__device__ __forceinline__ CorePtrG core_rev(CorePtrG c, int nst) {
  c.p += (ptrdiff_t)(nst - 1) * c.st + c.sub;
  c.st = -c.st;
  c.sub = -c.sub;
  return c;
}
template <int A0, int A1, int B0, int B1, bool SAME>
__device__ __forceinline__ void frag4_load_r(Frag4& f, const CorePtrG& A, const CorePtrG& B, int st) {
  constexpr int L0 = SAME ? (A0 < B0 ? A0 : B0) : A0, L1 = SAME ? (A1 > B1 ? A1 : B1) : A1;
  const double* pa = A.p + (ptrdiff_t)st * A.st;
  const double* pb = B.p + (ptrdiff_t)st * B.st;
#pragma unroll
  for (int s = 0; s < Q4SD; ++s) {
#pragma unroll
    for (int a = L0; a < L1; ++a) f.a[s][a] = pa[s * A.sub + 16 * a];
    if constexpr (!SAME) {
#pragma unroll
      for (int b = B0; b < B1; ++b) f.b[s][b] = pb[s * B.sub + 16 * b];
    }
  }
}
template <bool BUF>
__device__ __forceinline__ auto core_addr(const double* X, size_t ld) {
  if constexpr (BUF) return core_ptr(X, ld);
  else return core_ptr_g(X, ld);
}
template <int A0, int A1, int B0, int B1, bool SAME>
__device__ __forceinline__ void frag4_load_r(Frag4& f, const CorePtr& A, const CorePtr& B, int st) {
  constexpr int L0 = SAME ? (A0 < B0 ? A0 : B0) : A0, L1 = SAME ? (A1 > B1 ? A1 : B1) : A1;
  const int oa = A.o + st * A.st, ob = B.o + st * B.st;
#pragma unroll
  for (int s = 0; s < Q4SD; ++s) {
#pragma unroll
    for (int a = L0; a < L1; ++a) f.a[s][a] = buffer_load_f64(A.r, A.vo + 128 * a, oa + s * A.sub);
    if constexpr (!SAME) {
#pragma unroll
      for (int b = B0; b < B1; ++b) f.b[s][b] = buffer_load_f64(B.r, B.vo + 128 * b, ob + s * B.sub);
    }
  }
}
template <int A0, int A1, int B0, int B1, bool SAME, bool LOWER>
__device__ __forceinline__ void frag4_mma_r(d4 (&acc)[QM][QN], const Frag4& f) {
#pragma unroll
  for (int s = 0; s < Q4SD; ++s)
#pragma unroll
    for (int a = A0; a < A1; ++a)
#pragma unroll
      for (int b = B0; b < B1; ++b) {
        if (LOWER && b > a) continue;
        acc[a][b] = mfma(SAME ? f.a[s][b] : f.b[s][b], f.a[s][a], acc[a][b]);
      }
}
// the prediction variance's core (k_gemm_pv): NB < QN: only the first NB 16-column blocks of B
// (the last, partly padded test tile); operands through CorePtr like the triangular cores
template <int NB = QN>
__device__ __forceinline__ void mma_64x64(d4 (&acc)[QM][QN], const double* __restrict__ A, size_t lda,
                                          const double* __restrict__ B, size_t ldb, int K) {
  const int nst = __builtin_amdgcn_readfirstlane(K / (4 * Q4SD));  // even: K is whole 64-tiles
  if (nst <= 0) return;
  const CorePtr pa = core_ptr(A, lda), pb = core_ptr(B, ldb);
  Frag4 f0, f1;
  frag4_load_r<0, QM, 0, NB, false>(f0, pa, pb, 0);
  for (int it = 0; it < nst; it += 2) {
    __builtin_amdgcn_sched_barrier(0);
    frag4_load_r<0, QM, 0, NB, false>(f1, pa, pb, it + 1);
    frag4_mma<NB>(acc, f0);
#pragma unroll
    for (int g = 0; g < Q4SD * (QM + NB); ++g) {
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // one VMEM read
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // two MFMAs
    }
    __builtin_amdgcn_sched_barrier(0);
    const int n2 = (it + 2 < nst) ? it + 2 : nst - 1;
    frag4_load_r<0, QM, 0, NB, false>(f0, pa, pb, n2);
    frag4_mma<NB>(acc, f1);
#pragma unroll
    for (int g = 0; g < Q4SD * (QM + NB); ++g) {
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}
// masks of trip T (0..3) of the triangular tile; T = 4: the dense trips
template <int MODE, int T>
struct TripMask {
  static constexpr bool first = MODE == TRI_A_FIRST || MODE == TRI_AB_FIRST || MODE == REV_A || MODE == REV_B;
  static constexpr bool dense = T >= 4 || (first && T == 3);
  static constexpr int a0 = (!dense && MODE == REV_A) ? 3 - T : 0;
  static constexpr int a1 = (!dense && (MODE == TRI_A_FIRST || MODE == TRI_AB_FIRST)) ? T + 1 : QM;
  static constexpr int b0 = (!dense && MODE == REV_B) ? 3 - T : 0;
  static constexpr int b1 = (!dense && MODE == TRI_AB_FIRST) ? T + 1 : QN;
};
template <int MODE, int T, class CP>
__device__ __forceinline__ void core_load(Frag4& f, const CP& A, const CP& B, int st) {
  constexpr bool same = MODE == TRI_AB_FIRST;
  using M = TripMask<MODE, T>;
  frag4_load_r<M::a0, M::a1, M::b0, M::b1, same>(f, A, B, st);
}
template <int MODE, int T>
__device__ __forceinline__ void core_mma(d4 (&acc)[QM][QN], const Frag4& f) {
  using M = TripMask<MODE, T>;
  constexpr bool same = MODE == TRI_AB_FIRST;
  frag4_mma_r<M::a0, M::a1, M::b0, M::b1, same, same>(acc, f);
}
// group barriers of a dense half trip: its loads spread evenly over its MFMAs (one load per two
// MFMAs; shared panels: 8 loads, 20 MFMAs)
template <int MODE>
__device__ __forceinline__ void core_groups() {
  constexpr bool same = MODE == TRI_AB_FIRST;
  constexpr int la = Q4SD * QM, lb = same ? 0 : Q4SD * QN;
  constexpr int nl = la + lb, nm = Q4SD * (same ? 10 : QM * QN), q = nm / nl, r = nm % nl;
#pragma unroll
  for (int g = 0; g < r; ++g) {
    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, q + 1, 0);
  }
#pragma unroll
  for (int g = r; g < nl; ++g) {
    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, q, 0);
  }
}
// one peeled trip T of the triangular tile, stages st and st + 1; the prefetch of stage st + 2
// uses trip T2's masks (NX: whether there is a next stage at all)
#define GPRX_TRIP(M, T, T2, st, NX)                  \
  {                                                  \
    __builtin_amdgcn_sched_barrier(0);               \
    core_load<M, T>(f1, pa, pb, (st) + 1);      \
    core_mma<M, T>(acc, f0);                         \
    __builtin_amdgcn_sched_barrier(0);               \
    if (NX) core_load<M, T2>(f0, pa, pb, (st) + 2); \
    core_mma<M, T>(acc, f1);                         \
  }
// k_lauum_grad's core (MODE: TRI_A_FIRST or TRI_AB_FIRST), operands through global addresses
template <int MODE>
__device__ __forceinline__ void mma_64x64_m(d4 (&acc)[QM][QN], const double* __restrict__ A, size_t lda,
                                            const double* __restrict__ B, size_t ldb, int K) {
  static_assert(MODE == TRI_A_FIRST || MODE == TRI_AB_FIRST, "the triangular tile is the first one");
  const int nst = __builtin_amdgcn_readfirstlane(K / (4 * Q4SD));  // multiple of 8: K is whole 64-tiles
  if (nst <= 0) return;
  const CorePtrG pa = core_ptr_g(A, lda), pb = core_ptr_g(B, ldb);
  Frag4 f0, f1;
  core_load<MODE, 0>(f0, pa, pb, 0);
  GPRX_TRIP(MODE, 0, 1, 0, true)
  GPRX_TRIP(MODE, 1, 2, 2, true)
  GPRX_TRIP(MODE, 2, 3, 4, true)
  int it = 6;
  for (; it < nst; it += 2) {
    __builtin_amdgcn_sched_barrier(0);
    core_load<MODE, 4>(f1, pa, pb, it + 1);
    core_mma<MODE, 4>(acc, f0);
    core_groups<MODE>();
    __builtin_amdgcn_sched_barrier(0);
    const int n2 = (it + 2 < nst) ? it + 2 : nst - 1;
    core_load<MODE, 4>(f0, pa, pb, n2);
    core_mma<MODE, 4>(acc, f1);
    core_groups<MODE>();
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_sched_barrier(0);
}
// k_loo_grad's and k_cv_kinv's core: the plain 64 x 64 product over whole 64-tiles of K, operands
// through global addresses; SAME: B = A, a diagonal tile, which forms its blocks b <= a only
template <bool SAME>
__device__ __forceinline__ void mma_64x64_sq(d4 (&acc)[QM][QN], const double* __restrict__ A, size_t lda,
                                             const double* __restrict__ B, size_t ldb, int K) {
  constexpr int MODE = SAME ? TRI_AB_FIRST : PLAIN;  // trip 4: the dense masks (SAME: B = A, blocks b <= a)
  const int nst = __builtin_amdgcn_readfirstlane(K / (4 * Q4SD));  // even: K is whole 64-tiles
  if (nst <= 0) return;
  const CorePtrG pa = core_ptr_g(A, lda), pb = core_ptr_g(B, ldb);
  Frag4 f0, f1;
  core_load<MODE, 4>(f0, pa, pb, 0);
  for (int it = 0; it < nst; it += 2) {
    __builtin_amdgcn_sched_barrier(0);
    core_load<MODE, 4>(f1, pa, pb, it + 1);
    core_mma<MODE, 4>(acc, f0);
    core_groups<MODE>();
    __builtin_amdgcn_sched_barrier(0);
    const int n2 = (it + 2 < nst) ? it + 2 : nst - 1;
    core_load<MODE, 4>(f0, pa, pb, n2);
    core_mma<MODE, 4>(acc, f1);
    core_groups<MODE>();
    __builtin_amdgcn_sched_barrier(0);
  }
  __builtin_amdgcn_sched_barrier(0);
}
// k_gemm's core: ONE copy of the dense loop and at most one peeled prefix per kernel instance (a
// second inlined copy of the loop, or a second peeled prefix / tail, makes the register allocator
// spill 150-700 VGPRs).  The instance's op (PM) has its triangular tile peeled in front of the
// loop: TT walks K forward from its upper-triangular first tile (Mt[ti,ti]); TRSM and LINV21 walk
// K backward from their lower-triangular last tile (Linv[tj,tj], Linv[ti,ti]: reversed trip T
// needs the row / column blocks >= 3 - T).  tri: this wave's op is PM's.
template <int PM, bool BUF = true>
__device__ __forceinline__ void mma_64x64_pm(d4 (&acc)[QM][QN], Frag4& f0, const double* __restrict__ A, size_t lda,
                                             const double* __restrict__ B, size_t ldb, int K, bool tri, bool pre, bool nxt,
                                             const double* nA, const double* nB, int nK) {
  // pre: f0 already holds this tile's first stage (loaded by the previous tile's last iteration);
  // nxt: the last iteration loads the next tile's first stage (operands nA, nB, K range nK, the
  // same op and walk) into f0 instead of re-reading its own last stage, so the next tile's first
  // MFMAs do not wait for a load issued after this tile's epilogue (round 5)
  const int nst = __builtin_amdgcn_readfirstlane(K / (4 * Q4SD));
  if (nst <= 0) return;
  auto pa = core_addr<BUF>(A, lda), pb = core_addr<BUF>(B, ldb);
  Frag4 f1;
  int it = 0;
  if (tri) {
    if constexpr (PM == REV_A || PM == REV_B) {  // stage j reads the k of stage nst - 1 - j
      pa = core_rev(pa, nst);
      pb = core_rev(pb, nst);
    }
    if (!pre) core_load<PM, 0>(f0, pa, pb, 0);
    GPRX_TRIP(PM, 0, 1, 0, true)
    GPRX_TRIP(PM, 1, 2, 2, true)
    GPRX_TRIP(PM, 2, 3, 4, true)
    it = 6;
  } else {
    if (!pre) core_load<PLAIN, 4>(f0, pa, pb, 0);
  }
  [[maybe_unused]] auto na = pa, nb = pb;
  if constexpr (BUF) {
    if (nxt) {
      const int nn = __builtin_amdgcn_readfirstlane(nK / (4 * Q4SD));
      na = core_addr<BUF>(nA, lda);
      nb = core_addr<BUF>(nB, ldb);
      if constexpr (PM == REV_A || PM == REV_B) {
        if (tri) {
          na = core_rev(na, nn);
          nb = core_rev(nb, nn);
        }
      }
    }
  }
  for (; it < nst; it += 2) {
    __builtin_amdgcn_sched_barrier(0);
    core_load<PLAIN, 4>(f1, pa, pb, it + 1);
    core_mma<PLAIN, 4>(acc, f0);
    core_groups<PLAIN>();
    __builtin_amdgcn_sched_barrier(0);
    const int n2 = (it + 2 < nst) ? it + 2 : nst - 1;
    if constexpr (BUF) {
      const bool nx = nxt && it + 2 >= nst;  // wave-uniform: scalar selects, no branch
      CorePtr la = pa, lb = pb;
      la.r = nx ? na.r : pa.r;
      la.o = nx ? na.o : pa.o + n2 * pa.st;
      la.sub = nx ? na.sub : pa.sub;
      lb.r = nx ? nb.r : pb.r;
      lb.o = nx ? nb.o : pb.o + n2 * pb.st;
      lb.sub = nx ? nb.sub : pb.sub;
      core_load<PLAIN, 4>(f0, la, lb, 0);
    } else {
      core_load<PLAIN, 4>(f0, pa, pb, n2);
    }
    core_mma<PLAIN, 4>(acc, f1);
    core_groups<PLAIN>();
    __builtin_amdgcn_sched_barrier(0);
  }
}
#undef GPRX_TRIP
// 64 x 16 wave core (the fused leaf's column-quarter tasks): acc[a] += A(64 x K) B(16 x K)^T,
// lane l reg q = C[16a + (l&15)][(l>>4) + 4q]; 4 MFMAs per 5 fragment loads, stages of depth 16
// in ping-pong (the same barriers as mma_64x64, groups of 5 loads and 4 MFMAs interleaved: leaf
// 2.18 -> 2.09 ms at B=240, same-box A/B).  K: whole 64-tiles.
struct Frag16 {
  double a[4][QM], b[4];
};
__device__ __forceinline__ void frag16_load(Frag16& f, const double* pa, const double* pb, size_t sa, size_t sb) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int a = 0; a < QM; ++a) f.a[s][a] = pa[s * sa + 16 * a];
    f.b[s] = pb[s * sb];
  }
}
__device__ __forceinline__ void frag16_mma(d4 (&acc)[QM], const Frag16& f) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int a = 0; a < QM; ++a) acc[a] = mfma(f.b[s], f.a[s][a], acc[a]);
}
__device__ __forceinline__ void mma_64x16(d4 (&acc)[QM], const double* __restrict__ A, size_t lda,
                                          const double* __restrict__ B, size_t ldb, int K) {
  const int nst = __builtin_amdgcn_readfirstlane(K >> 4);  // even: K is whole 64-tiles
  if (nst <= 0) return;
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const double* pa = A + lr + (size_t)lk * lda;
  const double* pb = B + lr + (size_t)lk * ldb;
  const size_t sa = 4 * lda, sb = 4 * ldb;
  Frag16 f0, f1;
  frag16_load(f0, pa, pb, sa, sb);
  for (int it = 0; it < nst; it += 2) {
    __builtin_amdgcn_sched_barrier(0);
    frag16_load(f1, pa + (size_t)(it + 1) * 4 * sa, pb + (size_t)(it + 1) * 4 * sb, sa, sb);
    frag16_mma(acc, f0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x020, 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    const int n2 = (it + 2 < nst) ? it + 2 : nst - 1;
    frag16_load(f0, pa + (size_t)n2 * 4 * sa, pb + (size_t)n2 * 4 * sb, sa, sb);
    frag16_mma(acc, f1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x020, 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}
// mma_64x16 with the B operand from the wave's LDS buffer: B(j, k) = tb[j * (TS + 1) + k] (a
// column quarter kept transposed in LDS by the producer), K = 64 (one tile)
__device__ __forceinline__ void mma_64x16_ldsb(d4 (&acc)[QM], const double* __restrict__ A, size_t lda, const double* tb) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const double* pa = A + lr + (size_t)lk * lda;
  const double* pb = tb + lr * (TS + 1) + lk;
  const size_t sa = 4 * lda;
#pragma unroll
  for (int st = 0; st < TS / 16; ++st) {
    double a[4][QM], b[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int q = 0; q < QM; ++q) a[s][q] = pa[(size_t)(4 * st + s) * sa + 16 * q];
      b[s] = pb[16 * st + 4 * s];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < QM; ++q) acc[q] = mfma(b[s], a[s][q], acc[q]);
  }
}
__device__ __forceinline__ void acc4_zero(d4 (&acc)[QM][QN]) {
#pragma unroll
  for (int a = 0; a < QM; ++a)
#pragma unroll
    for (int b = 0; b < QN; ++b) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
}
__device__ __forceinline__ void acc_zero(d4 (&acc)[WM][WN]) {
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
}
__device__ __forceinline__ void acc_zero4(d4 (&acc)[QM]) {
#pragma unroll
  for (int a = 0; a < QM; ++a) acc[a] = (d4){0.0, 0.0, 0.0, 0.0};
}
// Row-block core over global operands: acc[a] lane (lr, lk) reg q += sum_k M[16a + lk + 4q][k]
// N[lr][k] (M, N column-major, K a multiple of 16).  Operands
// one 16-deep stage ahead in registers, as mma_64x16 (whose MFMA operands are the other way round).
__device__ __forceinline__ void frag16_load_rd(Frag16& f, const double* pa, const double* pb, size_t sa, size_t sb) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int a = 0; a < QM; ++a) f.a[s][a] = pa[s * sa + 16 * a];
    f.b[s] = pb[s * sb];
  }
}
__device__ __forceinline__ void frag16_mma_rd(d4 (&acc)[QM], const Frag16& f) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int a = 0; a < QM; ++a) acc[a] = mfma(f.a[s][a], f.b[s], acc[a]);
}
__device__ __forceinline__ void mma_rd(d4 (&acc)[QM], const double* __restrict__ M, size_t ldm, const double* __restrict__ N,
                                       size_t ldn, int K) {
  const int nst = __builtin_amdgcn_readfirstlane(K >> 4);
  if (nst <= 0) return;
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const double* pa = M + lr + (size_t)lk * ldm;
  const double* pb = N + lr + (size_t)lk * ldn;
  const size_t sa = 4 * ldm, sb = 4 * ldn;
  Frag16 f0, f1;
  frag16_load_rd(f0, pa, pb, sa, sb);
  int it = 0;
  for (; it + 1 < nst; it += 2) {
    __builtin_amdgcn_sched_barrier(0);
    frag16_load_rd(f1, pa + (size_t)(it + 1) * 4 * sa, pb + (size_t)(it + 1) * 4 * sb, sa, sb);
    frag16_mma_rd(acc, f0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x020, 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    const int n2 = (it + 2 < nst) ? it + 2 : it + 1;
    frag16_load_rd(f0, pa + (size_t)n2 * 4 * sa, pb + (size_t)n2 * 4 * sb, sa, sb);
    frag16_mma_rd(acc, f1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x020, 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (it < nst) frag16_mma_rd(acc, f0);
}
// Row-packed mma_rd, for products whose output row order is free (the leaf's SYRK items): block a =
// (h = a / 2, p = a % 2) holds rows 32 h + 2 i + p (i = lk + 4 q in the C layout), so a lane's two
// rows 32 h + 2 lr, + 1 of an M column arrive by one 16-B load: 8 A loads per 16-deep stage instead
// of 16.  Every output element sums its k in mma_rd's order: the same results.
struct Frag16p {
  double2 a[4][2];
  double b[4];
};
__device__ __forceinline__ void frag16p_load_rd(Frag16p& f, const double* pa, const double* pb, size_t sa, size_t sb) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int h = 0; h < 2; ++h) f.a[s][h] = *(const double2*)(pa + s * sa + 32 * h);
    f.b[s] = pb[s * sb];
  }
}
__device__ __forceinline__ void frag16p_mma_rd(d4 (&acc)[QM], const Frag16p& f) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      acc[2 * h] = mfma(f.a[s][h].x, f.b[s], acc[2 * h]);
      acc[2 * h + 1] = mfma(f.a[s][h].y, f.b[s], acc[2 * h + 1]);
    }
}
// M's rows in pairs (16-B aligned: M's offset and ldm even)
__device__ __forceinline__ void mma_rd_pk(d4 (&acc)[QM], const double* __restrict__ M, size_t ldm, const double* __restrict__ N,
                                          size_t ldn, int K) {
  const int nst = __builtin_amdgcn_readfirstlane(K >> 4);
  if (nst <= 0) return;
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const double* pa = M + 2 * lr + (size_t)lk * ldm;
  const double* pb = N + lr + (size_t)lk * ldn;
  const size_t sa = 4 * ldm, sb = 4 * ldn;
  Frag16p f0, f1;
  frag16p_load_rd(f0, pa, pb, sa, sb);
  int it = 0;
  for (; it + 1 < nst; it += 2) {
    __builtin_amdgcn_sched_barrier(0);
    frag16p_load_rd(f1, pa + (size_t)(it + 1) * 4 * sa, pb + (size_t)(it + 1) * 4 * sb, sa, sb);
    frag16p_mma_rd(acc, f0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (it + 2 < nst) frag16p_load_rd(f0, pa + (size_t)(it + 2) * 4 * sa, pb + (size_t)(it + 2) * 4 * sb, sa, sb);
    frag16p_mma_rd(acc, f1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (it < nst) frag16p_mma_rd(acc, f0);
}
// 64 x 16 column-quarter stores (C layout of mma_64x16, quarter columns 16w..): C[r + c ld] =
// sgn acc, C -= acc, and the transposed Ct[c + r ld] through the wave's [16][65] LDS buffer (four
// 128-B row segments per store instruction)
__device__ __forceinline__ void accq_store(double* C, size_t ld, const d4 (&acc)[QM], double sgn) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
#pragma unroll
  for (int a = 0; a < QM; ++a)
#pragma unroll
    for (int q = 0; q < 4; ++q) C[(size_t)(lk + 4 * q) * ld + 16 * a + lr] = sgn * acc[a][q];
}
__device__ __forceinline__ void accq_store_t(double* Ct, size_t ld, const d4 (&acc)[QM], double sgn, double* tb) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
#pragma unroll
  for (int a = 0; a < QM; ++a)
#pragma unroll
    for (int q = 0; q < 4; ++q) tb[(lk + 4 * q) * (TS + 1) + 16 * a + lr] = sgn * acc[a][q];  // tb[c][r]
  __builtin_amdgcn_wave_barrier();
  const int c = l & 15, r4 = l >> 4;
#pragma unroll
  for (int r = 0; r < TS; r += 4) Ct[(size_t)(r + r4) * ld + c] = tb[c * (TS + 1) + r + r4];
  __builtin_amdgcn_wave_barrier();
}

}  // namespace gprx
