// gprx_gemm.h -- the recursion's batched tile GEMMs: unit decomposition, tile_ops .. gemm_unit, and the
// kernels k_gemm_p, k_gemm<PM>, k_gemm_pv.
//
// A part of gprx_kernels.hip, included there once and by no other file (the parts and their order
// are listed at its includes).
#pragma once

namespace gprx {

// z = L^-1 y by forward substitution over the blocks (blk_range), fused into the producers of the
// tiles.  Inside a block every L^-1 tile (ti, tj) (written exactly once, by a diagonal kernel, the
// leaf or LINV21) also writes its 64-row partial  L^-1[ti,tj] Yw[tj]  into
// zp[slot][2 tj + half][ti*64 + r] (half: 32-column halves of the pair-unit GEMM; 64-column
// producers write half 0 and zero half 1).  Left of a block the same rows hold  -L[ti,tj] z[tj],
// written by the TRSM of the split node that owns tile (ti, tj): k_rhs sums them into the block's
// right-hand side Yw, and k_znode sums the block's own partials into z, <= 16 per row.
// 64 x 64 accumulator tile (mma_64x64 layout) of sgn * M[ti,tj] times yv, the lane's 16 elements
// of a 64-vector: loaded here (zp_load4), or spread from the lanes (zl_spread4).  The TRSM tile of
// a split node loads its 64 elements of z one per lane AHEAD of the K loop (gemm_tile): loads and
// stores retire through one in-order counter, so z loaded after the tile's 64 stores waits for all
// of them.  Measured at B = 240, N = 2048, same-box pairs against the build without the epilogue:
// potrf_trsm + 0.09 ms per step with the loads last, + 0.055 just before the stores, + 0.035 ahead
// of the K loop.  LINV21's four z loads stay after its stores, as its z partial's loads always
// were: ahead of the stores or of the K loop trtri_linv21 measured 0.05 ms slower, after them equal.
__device__ __forceinline__ void zp_load4(const double* vec, int tj, double (&yv)[QN][4]) {  // vec: the slot's
  const int lk = (threadIdx.x & 63) >> 4;
  const double* y = vec + tj * TS;
#pragma unroll
  for (int b = 0; b < QN; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) yv[b][q] = y[16 * b + lk + 4 * q];
}
__device__ __forceinline__ void zl_spread4(double zl, double (&yv)[QN][4]) {  // zl: element l of the 64-vector
  const int lk = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int b = 0; b < QN; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) yv[b][q] = __shfl(zl, 16 * b + lk + 4 * q);
}
__device__ __forceinline__ void zp_acc4(const DevBatch& db, int slot, int ti, int tj, const d4 (&acc)[QM][QN],
                                        const double (&yv)[QN][4], double sgn) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  double* z0 = zp_row(db, slot, 2 * tj) + ti * TS;
  double* z1 = zp_row(db, slot, 2 * tj + 1) + ti * TS;
#pragma unroll
  for (int a = 0; a < QM; ++a) {
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < QN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) t = fma(acc[a][b][q], yv[b][q], t);
    t = sum_xor32(sum_xor16(t));
    if (lk == 0) {
      z0[16 * a + lr] = sgn * t;
      z1[16 * a + lr] = 0.0;
    }
  }
}
// alpha = L^-T z across blocks: the LINV21 tile (ti, tj) of a split node, still in the accumulators
// (mma_64x64 layout), writes  L^-1[ti,tj]^T z[ti]  (z of the bottom child is final by then) into
// ap[slot][ti][tj*64 + c]; k_alpha adds the rows ti >= blk_hi to what it streams of Mt inside the
// block.  The 16 lanes' sums by DPP, as the prediction variance's epilogue in gemm_tile.
__device__ __forceinline__ void ap_acc4(const DevBatch& db, int slot, int ti, int tj, const d4 (&acc)[QM][QN]) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const double* z = db.z + (size_t)slot * db.Npad + ti * TS;
  double zv[QM];
#pragma unroll
  for (int a = 0; a < QM; ++a) zv[a] = z[16 * a + lr];
  double* ap = ap_row(db, slot, ti) + tj * TS;
#pragma unroll
  for (int b = 0; b < QN; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double v = 0.0;
#pragma unroll
      for (int a = 0; a < QM; ++a) v = fma(acc[a][b][q], zv[a], v);
      v = row_sum16(v);
      if (lr == 0) ap[16 * b + lk + 4 * q] = v;
    }
}
// Units of the 4-wave workgroups of k_gemm / k_lauum_grad: UR x UC output tiles (UR UC = 4), wave w
// = tile (pr + w / UC, pc + w % UC).  The shape follows the op so that the four waves of a unit
// share one K range where it varies by tile: TRSM (K grows with the column) 4 x 1, TT / LINV21 (K
// set by the row) 1 x 4, SYRK (fixed K; lower triangle) and PREDVAR 2 x 2.
__host__ __device__ inline void unit_shape(int op, int& UR, int& UC) {
  UR = op == OP_TRSM ? 4 : ((op == OP_TT || op == OP_LINV21) ? 1 : 2);
  UC = 4 / UR;
}
// rect R x C: ceil(R/UR) x ceil(C/UC) units; lower triangle of R x R (tri: SYRK, fixed K): four
// consecutive tiles of the row-major lower triangle per unit (no idle wave on the diagonal)
__host__ __device__ inline int quad_units(int R, int C, bool tri, int UR = 2, int UC = 2) {
  if (tri) return (R * (R + 1) / 2 + 3) / 4;
  return ((R + UR - 1) / UR) * ((C + UC - 1) / UC);
}
// Triangular-K ops are folded: a workgroup computes the unit with the longest K range and then
// its mirror along the K-varying dimension (TRSM: columns; TT, LINV21, PREDVAR: rows), so every
// workgroup carries about the same K (measured 58.7 -> 67.4 TF/s on a TRSM-shaped launch,
// scratch/gemm3_bench.hip).
__host__ __device__ inline int op_units(const GemmGeom& g, int nt, int mt) {
  int r0, c0, R, C, UR, UC;
  bool tri;
  op_rect(g, nt, mt, r0, c0, R, C, tri);
  unit_shape(g.op, UR, UC);
  if (tri || g.op == OP_SYRK) return quad_units(R, C, tri, UR, UC);
  const int RU = (R + UR - 1) / UR, CU = (C + UC - 1) / UC;
  return g.op == OP_TRSM ? RU * ((CU + 1) / 2) : ((RU + 1) / 2) * CU;
}
__device__ __forceinline__ void quad_tri(int u, int& rp, int& cp) {
  int r = (int)((sqrtf(8.0f * u + 1.0f) - 1.0f) * 0.5f);
  while ((r + 1) * (r + 2) / 2 <= u) ++r;
  while (r * (r + 1) / 2 > u) --r;
  rp = r;
  cp = u - r * (r + 1) / 2;
}

// ============================================================================================
// Generic batched tile GEMM of the recursion (see GemmOp).  Unit = 4 output tiles (unit_shape;
// a triangular SYRK: 4 consecutive lower tiles); each wave computes one 64 x 64 tile with its own
// K range (triangular operands are skipped at tile granularity).  Waves of tiles outside the rectangle / above the diagonal
// return at once (no workgroup barrier in this kernel).
// ============================================================================================
// One 64 x 64 output tile (ti, tj) of a GemmOp on one wave.
constexpr int TT_S = TS + 2;  // row stride of k_gemm's per-wave transpose buffer (LINV21's Mt store)
constexpr size_t linv21_lds_bytes() { return (size_t)4 * 32 * TT_S * sizeof(double); }  // 4 waves x [32][66]
// operands of tile (ti, tj) of a GemmOp: A and B at the K range's start, B's leading dimension,
// the K range (elements)
struct TileOps {
  const double *A, *B;
  size_t ldb;
  int Kn;
};
__device__ __forceinline__ TileOps tile_ops(const DevBatch& db, int op, const GemmGeom& g, int slot, int ti, int tj) {
  const size_t ld = db.ld, so = (size_t)slot * db.mat;
  int kb, ke;  // K range in tiles
  const double *A, *Bm;
  size_t ldb = ld;
  switch (op) {
    case OP_TRSM: kb = g.o; ke = tj + 1; A = (g.upd ? db.S : db.K) + so; Bm = db.Linv + so; break;
    case OP_SYRK: kb = g.o; ke = g.o + g.h; A = db.Lw + so; Bm = db.Lw + so; break;
    case OP_TT: kb = ti; ke = g.o + g.h; A = db.Mt + so; Bm = db.Lw + so; break;
    case OP_LINV21: kb = g.o + g.h; ke = ti + 1; A = db.Linv + so; Bm = db.Lw + so; break;
    default:
      kb = 0;
      ke = ti + 1;
      A = db.Linv + so;
      Bm = db.KsT + (size_t)slot * db.Npad * db.Mpad;
      ldb = db.Mpad;
      break;
  }
  return TileOps{A + (size_t)kb * TS * ld + ti * TS, Bm + (size_t)kb * TS * ldb + tj * TS, ldb, (ke - kb) * TS};
}
// f0 / pre / nxt / (nti, ntj): the register stage handed from one tile of a wave's folded pair to
// the next (mma_64x64_pm)
template <bool PV, int PM = PLAIN, bool BUF = true>
__device__ __forceinline__ void gemm_tile(const DevBatch& db, const GemmGeom& g, int slot, int ti, int tj, int pass, Frag4& f0,
                                          bool pre, bool nxt, int nti, int ntj) {
  GTS(g, pass, 0);
  const int op = PV ? (int)OP_PREDVAR : g.op;
  const size_t ld = db.ld, so = (size_t)slot * db.mat;
  const TileOps to = tile_ops(db, op, g, slot, ti, tj);
  const size_t ldb = to.ldb;
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  // the output tile's addressing (the SYRK's C and every op's stores): buffer ops over the tile,
  // the lane's byte offset per q in a VGPR, the 16-column block b in an SGPR, the row block a in the
  // offset field: no per-element 64-bit address arithmetic
  const int Lb = (int)ld * (int)sizeof(double);
  const int vl = lk * Lb + lr * (int)sizeof(double);  // + 4 q Lb (formed where used: not live across the K loop)
  d4 acc[QM][QN];
  if (op == OP_SYRK) {  // acc = -C, loaded before the K loop so its latency overlaps the first stage
    const __amdgpu_buffer_rsrc_t cr = buffer_rsrc((g.upd ? db.S : db.K) + so + (size_t)(tj * TS) * ld + ti * TS, 0x7ffffff0);
#pragma unroll
    for (int a = 0; a < QM; ++a)
#pragma unroll
      for (int b = 0; b < QN; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[a][b][q] = neg_f64(buffer_load_f64(cr, vl + 128 * a, (16 * b + 4 * q) * Lb));
  } else {
    acc4_zero(acc);
  }
  const double* Ak = to.A;
  const double* Bk = to.B;
  // a split node's TRSM tile (the REV_B instance): the lane's element of z[tj] (final: the top
  // child returned), in flight under the K loop (see zp_load4)
  const bool split = !PV && g.n > BLK_TILES;
  double zl = 0.0;
  if (PM == REV_B && split && op == OP_TRSM) zl = db.z[(size_t)slot * db.Npad + tj * TS + l];
  if constexpr (PV) {  // prediction (own kernel instance): skip the last test tile's all-padding blocks
    const int nbv = __builtin_amdgcn_readfirstlane((db.M - tj * TS + 15) >> 4);
    if (nbv >= QN) mma_64x64(acc, Ak, ld, Bk, ldb, to.Kn);
    else if (nbv == 3) mma_64x64<3>(acc, Ak, ld, Bk, ldb, to.Kn);
    else if (nbv == 2) mma_64x64<2>(acc, Ak, ld, Bk, ldb, to.Kn);
    else mma_64x64<1>(acc, Ak, ld, Bk, ldb, to.Kn);
  } else {
#ifdef GPRX_STAMPS
    const Stamp st0 = stamp_now();
#endif
    // the operands' triangular tiles (diagonal tiles of Linv / Mt) and SYRK's upper blocks of a
    // diagonal tile are skipped (mma_64x64_m); op and ti == tj are wave-uniform
    const bool tri = (PM == TRI_A_FIRST && op == OP_TT) || (PM == REV_A && op == OP_LINV21) || (PM == REV_B && op == OP_TRSM);
    TileOps tn = to;
    if (nxt) tn = tile_ops(db, op, g, slot, nti, ntj);
    GTS(g, pass, 1);
    mma_64x64_pm<PM, BUF>(acc, f0, Ak, ld, Bk, ldb, to.Kn, tri, pre, nxt, tn.A, tn.B, tn.Kn);
    GTS(g, pass, 2);
#ifdef GPRX_STAMPS
    if ((op == OP_SYRK || op == OP_TT) && g.n == db.nt) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      stamp_store(1, st0, stamp_now());
    }
#endif
  }
  if (PV) {  // OP_PREDVAR runs only in the k_gemm_pv instance
#pragma unroll
    for (int b = 0; b < QN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < QM; ++a) v = fma(acc[a][b][q], acc[a][b][q], v);
        // the 16 lanes' sum by DPP (round 5: was four ds_bpermute exchanges per 32-bit half); the
        // same partners and operand order as the xor-1/2/4/8 tree, so the same sums
        v = row_sum16(v);
        if (lr == 0) db.var_part[((size_t)slot * db.nt + ti) * db.Mpad + tj * TS + 16 * b + lk + 4 * q] = v;
      }
    return;
  }
  double* Cm;
  switch (op) {
    case OP_TRSM: Cm = db.Lw + so; break;
    case OP_SYRK: Cm = db.S + so; break;
    case OP_TT: Cm = db.Lw + so; break;
    default: Cm = db.Linv + so; break;
  }
  // SYRK: C - L L^T = -acc; LINV21: L^-1_21 = -acc.  The sign flips the sign bit (an integer op:
  // an fp64 multiply by -1 takes issue cycles from the MFMA pipe of the SIMD's other wave)
  if (op == OP_SYRK || op == OP_LINV21) {  // wave-uniform
#pragma unroll
    for (int a = 0; a < QM; ++a)
#pragma unroll
      for (int b = 0; b < QN; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[a][b][q] = neg_f64(acc[a][b][q]);
  }
  // wave-uniform: a split node's TRSM hands -L21 z to the bottom child's blocks, its LINV21 forms
  // the alpha partial; inside a block LINV21 writes its z partial as every producer
  double yv[QN][4];
  const __amdgpu_buffer_rsrc_t crw = buffer_rsrc(Cm + (size_t)(tj * TS) * ld + ti * TS, 0x7ffffff0);
#pragma unroll
  for (int a = 0; a < QM; ++a)
#pragma unroll
    for (int b = 0; b < QN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) buffer_store_f64(crw, vl + 128 * a, (16 * b + 4 * q) * Lb, acc[a][b][q]);
  if (op == OP_TRSM && split) {
    if (PM == REV_B) zl_spread4(zl, yv);
    else zp_load4(db.z + (size_t)slot * db.Npad, tj, yv);
    zp_acc4(db, slot, ti, tj, acc, yv, -1.0);
  }
  if (op == OP_LINV21) {
    if (split) {
      ap_acc4(db, slot, ti, tj, acc);
    } else {
      zp_load4(yw_slot(db, slot), tj, yv);
      zp_acc4(db, slot, ti, tj, acc, yv, 1.0);
    }
  }
  if (op != OP_LINV21) GTS(g, pass, 3);
  if (op == OP_LINV21) {  // Mt[tj, ti] = Linv[ti, tj]^T, transposed through LDS 32 rows at a time
    // (round 5: two rounds instead of four 16-row ones, and 16-B reads and stores: every store
    // instruction writes two contiguous 512-B column segments of Mt)
    extern __shared__ __attribute__((aligned(16))) double gsm[];
    // this wave's [32][66] buffer: at row stride 66 the 16 x 4 lanes of a write hit 64 distinct
    // banks per half-wave (stride 65 put lanes with equal lr + lk in one bank); 528-B rows keep the
    // 16-B reads aligned
    double* tb = gsm + (threadIdx.x >> 6) * (32 * TT_S);
    double* Mtt = db.Mt + so + (size_t)(ti * TS) * ld + tj * TS;
    const int hr = l >> 5, c2 = 2 * (l & 31);  // 16-B lane: row parity, column pair
    const int vst = (hr * (int)ld + c2) * (int)sizeof(double);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int aa = 0; aa < 2; ++aa)
#pragma unroll
        for (int b = 0; b < QN; ++b)
#pragma unroll
          for (int q = 0; q < 4; ++q) tb[(16 * aa + lr) * TT_S + 16 * b + lk + 4 * q] = acc[2 * h + aa][b][q];
      __builtin_amdgcn_wave_barrier();
      // all 16 reads in flight before the stores (one LDS round trip per round, not one per row
      // pair); rows 32h + 2 r2 .. + 1: the pair's base in the resource (SGPRs), the lane's row
      // parity and column pair in the VGPR offset (soffset 0: see buffer_store_f64x2)
      double2 v[16];
#pragma unroll
      for (int r2 = 0; r2 < 16; ++r2) v[r2] = *(const double2*)(tb + (2 * r2 + hr) * TT_S + c2);
#pragma unroll
      for (int r2 = 0; r2 < 16; ++r2)
        buffer_store_f64x2(buffer_rsrc(Mtt + (size_t)(32 * h + 2 * r2) * ld, 0x7ffffff0), vst, v[r2].x, v[r2].y);
      __builtin_amdgcn_wave_barrier();
    }
    GTS(g, pass, 3);
  }
}

// The SYRK + TT launch of an 8-tile node (m1 = m2 = 4 tiles): 10 SYRK tiles of K = 4 tiles and 16 TT
// tiles of K = 4 - i (row i), 80 tile-K in all.  The unit decomposition below gives 5 workgroups
// per slot (1200 at B = 240: 2.34 rounds of 512 resident workgroups, i.e. three); this fixed plan
// packs them into 2 workgroups per slot (one round), every wave a list of 3-4 tiles.  Round 6: the
// lists balance issued MFMAs, not tile-K (a diagonal SYRK tile forms 10 of its 16 blocks, a TT
// tile skips 96 of its first K tile's 256 MFMAs): 2112-2240 MFMAs per wave, and 4352 on each SIMD,
// whose two waves are w and w + 4 in k_node8 (scratch/hwid_probe.hip); the round-5 lists had
// 1984-2464 per wave and 4064-4640 per SIMD, and k_node8's SYRK + TT phase ended 45 us apart on a
// slot's waves (scratch/node8_gts.py).  Entry: sel * 16 + 4 i + j, tile (i, j) of the SYRK (sel 0)
// or TT (sel 1) rectangle, each list longest first.
__constant__ int N8_PLAN[8][4] = {{13, 18, 30, -1}, {17, 20, 0, -1},  {8, 10, 24, 28}, {19, 22, 15, -1},
                                   {9, 5, 27, 31},   {14, 21, 26, -1}, {12, 23, 25, -1}, {4, 16, 29, -1}};
__host__ __device__ inline bool n8_plan(const GemmGeom& g1, const GemmGeom& g2) {
  return g1.op == OP_SYRK && g2.op == OP_TT && g1.n == 8 && g1.h == 4;
}
// units per slot of a launch (g2: the appended op; the n = 8 SYRK + TT launch: its fixed plan)
template <bool PV>
__device__ __forceinline__ int gemm_units(const DevBatch& db, const GemmGeom& g1, const GemmGeom& g2, int& T1) {
  const bool plan = !PV && n8_plan(g1, g2);
  T1 = plan ? 2 : op_units(g1, db.nt, db.mt);
  return T1 + ((plan || g2.op == OP_NONE) ? 0 : op_units(g2, db.nt, db.mt));
}
// unit u of a slot on the four waves w = 0..3 that share it
template <bool PV, int PM = PLAIN, bool BUF = true>
__device__ __forceinline__ void gemm_unit(const DevBatch& db, const GemmGeom& g1, const GemmGeom& g2, int slot, int u, int w,
                                          int T1) {
  int r0, c0, R, C, r02, c02, R2, C2;
  bool tri, tri2;
  op_rect(g1, db.nt, db.mt, r0, c0, R, C, tri);
  op_rect(g2, db.nt, db.mt, r02, c02, R2, C2, tri2);
  const bool plan = !PV && n8_plan(g1, g2);
  int pr, pc;
  // the wave's tiles: the plan's list, or the unit (and its folded mirror) of the decomposition
  // below; ONE call site of gemm_tile (its cores are inlined once per kernel instance)
  int np = 1, pr2 = 0, pc2 = 0, sel0 = 0, w8 = 0, wr = 0, wc = 0;
  if (plan) {
    w8 = 4 * u + w;
    np = 4;
  } else {
    if (u >= T1) {
      u -= T1;
      sel0 = 1;
      r0 = r02; c0 = c02; R = R2; C = C2; tri = tri2;
    }
    const int op = (sel0 ? g2 : g1).op;  // block-uniform
    int UR, UC;
    unit_shape(op, UR, UC);
    wr = w / UC;
    wc = w - wr * UC;
    if (tri) {  // lower-triangle tile 4u + w in row-major order
      const int t = 4 * u + w;
      if (t >= R * (R + 1) / 2) return;  // wave-uniform: the last unit's missing tiles
      quad_tri(t, pr, pc);
      wr = wc = 0;
    } else {
      const int RU = (R + UR - 1) / UR, CU = (C + UC - 1) / UC;
      if (op == OP_SYRK) {
        pr = UR * (u / CU);
        pc = UC * (u % CU);
      } else if (op == OP_TRSM) {  // K grows with the column: fold columns
        const int nf = (CU + 1) / 2, pi = u / nf, f = u - pi * nf;
        pr = pr2 = UR * pi;
        pc = UC * (CU - 1 - f);
        pc2 = UC * f;
        np = (CU - 1 - f != f) ? 2 : 1;
      } else {  // fold rows; TT: K shrinks with the row, LINV21 / PREDVAR: K grows with the row
        const int f = u / CU, pj = u - f * CU;
        const int lo = f, hi = RU - 1 - f;
        pr = UR * (op == OP_TT ? lo : hi);
        pr2 = UR * (op == OP_TT ? hi : lo);
        pc = pc2 = UC * pj;
        np = (lo != hi) ? 2 : 1;
      }
    }
  }
  // the register stage handed from tile k to tile k + 1 (mma_64x64_pm), in the SYRK + TT instance:
  // syrk_tt 9.97-10.04 -> 9.84-9.90 ms; TRSM 4.93-4.97 -> 5.03-5.09 and LINV21 unchanged (same-box
  // A/B, scratch/gemm_ab.sh), so those keep the reload
  Frag4 f0;
  bool pre = false;  // f0 holds this tile's first stage
#pragma unroll 1
  for (int k = 0; k < np; ++k) {
    int sel, ti, tj;
    bool nxt = false;  // the next tile of the fold exists on this wave: prefetch its first stage
    int nti = 0, ntj = 0;
    if (plan) {
      const int e = N8_PLAN[w8][k];
      if (e < 0) break;
      sel = e >> 4;
      ti = (sel ? r02 : r0) + ((e >> 2) & 3);
      tj = (sel ? c02 : c0) + (e & 3);
    } else {
      const int ur = k ? pr2 : pr, uc = k ? pc2 : pc;
      if (ur + wr >= R || uc + wc >= C) continue;  // wave-uniform: partial unit
      sel = sel0;
      ti = r0 + ur + wr;
      tj = c0 + uc + wc;
      if (!PV && BUF && PM == TRI_A_FIRST && k + 1 < np && pr2 + wr < R && pc2 + wc < C) {  // TT's folds (see below)
        nxt = true;
        nti = r0 + pr2 + wr;
        ntj = c0 + pc2 + wc;
      }
    }
    // wave-uniform tile indices in SGPRs (the 64 x 64 core needs every VGPR)
    gemm_tile<PV, PM, BUF>(db, sel ? g2 : g1, slot, __builtin_amdgcn_readfirstlane(ti), __builtin_amdgcn_readfirstlane(tj), k, f0,
                           pre, nxt, __builtin_amdgcn_readfirstlane(nti), __builtin_amdgcn_readfirstlane(ntj));
    pre = nxt;
  }
}

template <bool PV, int PM = PLAIN>
__device__ __forceinline__ void gemm_body(const DevBatch& db, const GemmGeom& g1, const GemmGeom& g2) {
  int T1;
  const int T = gemm_units<PV>(db, g1, g2, T1);
  int slot, u;
  if (!map_slot(db, T, slot, u)) return;
  gemm_unit<PV, PM>(db, g1, g2, slot, u, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), T1);
}

// 64 x 32 accumulator half-tile (mma_64x32_s1 layout, columns 32 half ..) of sgn * M[ti,tj]; vec: the slot's Yw or z
__device__ __forceinline__ void zp_acc2(const DevBatch& db, const double* vec, int slot, int ti, int tj, int half,
                                        const d4 (&acc)[WM][WN], double sgn) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  const double* y = vec + tj * TS + 32 * half;
  double yv[WN][4];
#pragma unroll
  for (int b = 0; b < WN; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) yv[b][q] = y[16 * b + lk + 4 * q];
  double* z = zp_row(db, slot, 2 * tj + half) + ti * TS;
#pragma unroll
  for (int a = 0; a < WM; ++a) {
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < WN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) t = fma(acc[a][b][q], yv[b][q], t);
    t = sum_xor32(sum_xor16(t));
    if (lk == 0) z[16 * a + lr] = sgn * t;
  }
}
// ap_acc4 for the half-tile
__device__ __forceinline__ void ap_acc2(const DevBatch& db, int slot, int ti, int tj, int half, const d4 (&acc)[WM][WN],
                                        double sgn) {
  // the lane's indices are formed here, after the K loop: hoisted above it (k_gemm_p runs at 128
  // VGPRs) they would be one more value spilled across it
  int l = threadIdx.x & 63;
  asm volatile("" : "+v"(l));
  const int lr = l & 15, lk = l >> 4;
  const double* z = db.z + (size_t)slot * db.Npad + ti * TS;
  double zv[WM];
#pragma unroll
  for (int a = 0; a < WM; ++a) zv[a] = z[16 * a + lr];
  double* ap = ap_row(db, slot, ti) + tj * TS + 32 * half;
#pragma unroll
  for (int b = 0; b < WN; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double v = 0.0;
#pragma unroll
      for (int a = 0; a < WM; ++a) v = fma(acc[a][b][q], zv[a], v);
      v = row_sum16(v);
      if (lr == 0) ap[16 * b + lk + 4 * q] = sgn * v;
    }
}
// Small recursion nodes: unit = 2 vertically adjacent 64 x 64 tiles, wave = 64 x 32, single-stage
// core at 4 waves/SIMD (more, shorter units than the 2 x 2 form: better for K <= 512).
__device__ __forceinline__ void gemm_tile_pair(const DevBatch& db, const GemmGeom& g, int slot, int ti, int tj, int wc);
// units: tri (SYRK) as pair_unit; TRSM folds column c with C-1-c; TT / LINV21 / PREDVAR fold
// row pair p with P-1-p (the folding of gemm_body, for 2 x 1 units)
__host__ __device__ inline int pair_op_units(const GemmGeom& g, int nt, int mt) {
  int r0, c0, R, C;
  bool tri;
  op_rect(g, nt, mt, r0, c0, R, C, tri);
  if (tri || g.op == OP_SYRK) return pair_units(R, C, tri);
  const int P = (R + 1) / 2;
  return g.op == OP_TRSM ? P * ((C + 1) / 2) : ((P + 1) / 2) * C;
}
__device__ __forceinline__ void gemm_body_pair(const DevBatch& db, const GemmGeom& g1, const GemmGeom& g2) {
  int r0, c0, R, C, r02, c02, R2, C2;
  bool tri, tri2;
  op_rect(g1, db.nt, db.mt, r0, c0, R, C, tri);
  op_rect(g2, db.nt, db.mt, r02, c02, R2, C2, tri2);
  const int T1 = pair_op_units(g1, db.nt, db.mt), T2 = g2.op == OP_NONE ? 0 : pair_op_units(g2, db.nt, db.mt);
  int slot, u, pr, pc;
  if (!map_slot(db, T1 + T2, slot, u)) return;
  const GemmGeom g = u < T1 ? g1 : g2;  // block-uniform
  if (u >= T1) {
    u -= T1;
    r0 = r02; c0 = c02; R = R2; C = C2; tri = tri2;
  }
  const int op = g.op;
  int np = 1, pr2 = 0, pc2 = 0;
  if (tri) {
    pair_unit(u, R, C, tri, pr, pc);
  } else if (op == OP_SYRK) {
    const int P = (R + 1) / 2, pi = u / C;
    pr = 2 * (P - 1 - pi);
    pc = u - pi * C;
  } else if (op == OP_TRSM) {  // K grows with the column: fold columns
    const int nf = (C + 1) / 2, pi = u / nf, f = u - pi * nf;
    pr = pr2 = 2 * pi;
    pc = C - 1 - f;
    pc2 = f;
    np = (pc != pc2) ? 2 : 1;
  } else {  // fold row pairs; TT: K shrinks with the row, LINV21 / PREDVAR: K grows with the row
    const int P = (R + 1) / 2, f = u / C;
    pc = pc2 = u - f * C;
    const int lo = f, hi = P - 1 - f;
    pr = 2 * (op == OP_TT ? lo : hi);
    pr2 = 2 * (op == OP_TT ? hi : lo);
    np = (lo != hi) ? 2 : 1;
  }
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wr = w >> 1, wc = w & 1;
#pragma unroll 1
  for (int pass = 0; pass < np; ++pass) {
    const int ur = pass ? pr2 : pr, uc = pass ? pc2 : pc;
    if (ur + wr >= R) continue;  // wave-uniform: second tile of an odd pair
    gemm_tile_pair(db, g, slot, __builtin_amdgcn_readfirstlane(r0 + ur + wr), __builtin_amdgcn_readfirstlane(c0 + uc), wc);
  }
}
__device__ __forceinline__ void gemm_tile_pair(const DevBatch& db, const GemmGeom& g, int slot, int ti, int tj, int wc) {
  const int op = g.op;
  const size_t ld = db.ld, so = (size_t)slot * db.mat;
  int kb, ke;  // K range in tiles
  const double *A, *Bm;
  size_t ldb = ld;
  switch (op) {
    case OP_TRSM: kb = g.o; ke = tj + 1; A = (g.upd ? db.S : db.K) + so; Bm = db.Linv + so; break;
    case OP_SYRK: kb = g.o; ke = g.o + g.h; A = db.Lw + so; Bm = db.Lw + so; break;
    case OP_TT: kb = ti; ke = g.o + g.h; A = db.Mt + so; Bm = db.Lw + so; break;
    case OP_LINV21: kb = g.o + g.h; ke = ti + 1; A = db.Linv + so; Bm = db.Lw + so; break;
    default:
      kb = 0;
      ke = ti + 1;
      A = db.Linv + so;
      Bm = db.KsT + (size_t)slot * db.Npad * db.Mpad;
      ldb = db.Mpad;
      break;
  }
  d4 acc[WM][WN];
  acc_zero(acc);
  mma_64x32_s1(acc, A + (size_t)kb * TS * ld + ti * TS, ld, Bm + (size_t)kb * TS * ldb + tj * TS + 32 * wc, ldb,
           (ke - kb) * TS);
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
  if (op == OP_PREDVAR) {
#pragma unroll
    for (int b = 0; b < WN; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < WM; ++a) v = fma(acc[a][b][q], acc[a][b][q], v);
        v = row_sum16(v);  // the xor-1/2/4/8 tree's partners and order, by DPP
        if (lr == 0)
          db.var_part[((size_t)slot * db.nt + ti) * db.Mpad + tj * TS + 32 * wc + 16 * b + lk + 4 * q] = v;
      }
    return;
  }
  double* Cm;
  double sgn = 1.0;
  switch (op) {
    case OP_TRSM: Cm = db.Lw + so; break;
    case OP_SYRK: Cm = db.S + so; break;
    case OP_TT: Cm = db.Lw + so; break;
    default: Cm = db.Linv + so; sgn = -1.0; break;
  }
  const size_t co = (size_t)(tj * TS + 32 * wc) * ld + ti * TS;
  double* Ct = Cm + co;
  if (op == OP_SYRK) {  // C (from K, or S once updated) - L L^T into S
    const double* Cs = (g.upd ? db.S : db.K) + so + co;
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
      for (int b = 0; b < WN; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const size_t e = (size_t)(16 * b + lk + 4 * q) * ld + 16 * a + lr;
          Ct[e] = Cs[e] - acc[a][b][q];
        }
  } else {
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
      for (int b = 0; b < WN; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) Ct[(size_t)(16 * b + lk + 4 * q) * ld + 16 * a + lr] = sgn * acc[a][b][q];
  }
  if (op == OP_LINV21) {  // Mt[tj, ti] = Linv[ti, tj]^T (direct: an LDS transpose measured slower here)
    double* Mtt = db.Mt + so + (size_t)(ti * TS) * ld + tj * TS + 32 * wc;
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
      for (int b = 0; b < WN; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) Mtt[(size_t)(16 * a + lr) * ld + 16 * b + lk + 4 * q] = -acc[a][b][q];
  }
  const bool split = g.n > BLK_TILES;  // as gemm_tile, last: nothing else is live; one call site of zp_acc2 (inlined once)
  if (op == OP_LINV21 && split) ap_acc2(db, slot, ti, tj, wc, acc, -1.0);
  else if (op == OP_LINV21 || (op == OP_TRSM && split))
    zp_acc2(db, op == OP_TRSM ? db.z + (size_t)slot * db.Npad : yw_slot(db, slot), slot, ti, tj, wc, acc, -1.0);
}

__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_gemm_p(DevBatch db, GemmGeom g, GemmGeom g2) {
  gemm_body_pair(db, g, g2);
}
// PM: the op whose triangular operand tile the instance peels (TRI_A_FIRST: TT of the SYRK + TT
// launches; REV_B: TRSM; REV_A: LINV21)
template <int PM>
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gemm(DevBatch db, GemmGeom g, GemmGeom g2) {
  gemm_body<false, PM>(db, g, g2);
}
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gemm_pv(DevBatch db, GemmGeom g, GemmGeom g2) {
  gemm_body<true>(db, g, g2);
}

}  // namespace gprx
