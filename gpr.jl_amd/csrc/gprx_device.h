// gprx_device.h -- lane-level pieces of the evaluation kernels: the MFMA wrapper, the block -> (slot,
// unit) mapping, the exp arithmetic with its tables, the DPP / lane-swap row and wave reductions,
// buffer loads and stores, and the z-partial rows.  (The distance forms sqd2 / wacc and the plain
// readlane_d / wave_sum use no device global and live in gprx_internal.h, where gprx_projection.hip
// finds them too.)
//
// A part of gprx_kernels.hip, included there once and by no other file (the parts and their order
// are listed at its includes).
#pragma once

namespace gprx {

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// blockIdx -> (slot, unit).  With B >= 8, slot s runs on the blocks b with b % 8 == s % 8, i.e.
// on one XCD under the dispatcher's round-robin placement (speed only, never correctness), so
// its panels stay in one L2; the grid is padded to 8 * ceil(B/8) * T blocks and surplus blocks
// return at once.  With B < 8 that would leave XCDs idle, so a slot's units are spread over
// all of them (linear mapping).
__host__ __device__ inline int grid_blocks(int B, int T) { return B < 8 ? B * T : 8 * ((B + 7) / 8) * T; }
__device__ __forceinline__ bool map_block(int bid, int B, int T, int& slot, int& unit) {
  if (B < 8) {
    slot = bid / T;
    unit = bid - slot * T;
    return slot < B;
  }
  const int x = bid & 7, q = bid >> 3;
  slot = (q / T) * 8 + x;
  unit = q % T;
  return slot < B;
}

// ... and the slot's evaluation mask: db.active (optional, device) lets the optimiser's rounds skip
// the slots whose optimisers have finished (every workgroup of such a slot returns at once)
__device__ __forceinline__ bool slot_active(const DevBatch& db, int slot) { return !db.active || db.active[slot] != 0; }
__device__ __forceinline__ bool map_slot(const DevBatch& db, int T, int& slot, int& unit) {
  return map_block(blockIdx.x, db.B, T, slot, unit) && slot_active(db, slot);
}

// Units of a tile-pair decomposition.  rect R x C: pairs of rows per column; lower triangle of
// R x R: column c holds rows c..R-1.
__host__ __device__ inline int pair_units(int R, int C, bool tri) {
  if (!tri) return ((R + 1) / 2) * C;
  int u = 0;
  for (int c = 0; c < R; ++c) u += (R - c + 1) / 2;
  return u;
}
__device__ __forceinline__ void pair_unit(int u, int R, int C, bool tri, int& r, int& c) {
  if (!tri) {
    const int P = (R + 1) / 2;
    c = u / P;
    r = 2 * (u - c * P);
    return;
  }
  int cc = 0;
  while (u >= (R - cc + 1) / 2) {
    u -= (R - cc + 1) / 2;
    ++cc;
  }
  c = cc;
  r = cc + 2 * u;
}

// sqrt(p) and 1/sqrt(p) for p > 0 (normal range) by v_rsq_f64 + Newton: two steps on r = p^-1/2,
// then one Heron step on s = p r (about 1 ulp; no library call on the pivot chain)
__device__ __forceinline__ void sqrt_rsqrt(double p, double& s, double& r) {
  r = __builtin_amdgcn_rsq(p);
  r = r * fma(-0.5 * p * r, r, 1.5);
  r = r * fma(-0.5 * p * r, r, 1.5);
  s = p * r;
  s = fma(0.5 * r, fma(-s, s, p), s);
}
// sf2 exp(x) for x <= 0 (the Gram's K and the test cross-covariance): x = (64 m + j) ln2/64 + r
// with |r| <= ln2/128 + 2^-50 (Cody-Waite, r exact by fma), e^r = 1 + q with q a degree-5 Taylor
// polynomial (truncation |r|^6/720 < 4e-17 relative), sf2 2^(j/64) = hi_j + lo_j from a 64-entry
// table the kernel stages in static LDS (sf2 folded in at staging, the product's error by fma;
// the static address makes the lookup two instructions), result hi + (hi q + lo) scaled by 2^m;
// 0 below -745, NaN propagates.  n = rint(x 64/ln2) by the 1.5 2^52 shift: one fma and one add
// for a multiply, a rint and a conversion (the fused product can pick the other neighbour when
// x 64/ln2 lies within an ulp of a half-integer: |r| grows by 2^-50, the accuracy does not
// change).  About 0.51 ulp; the guard is a select, not a branch around the evaluation.
// The coefficients live in a mutable device array that a kernel copies into registers once
// (uniform loads: SGPRs): with literal constants the compiler rematerialises every coefficient
// per exp as two v_mov_b32.
struct ExpK {
  double c[4];         // 1/5!, 1/4!, 1/3!, 1/2
  double k64, hi, lo;  // 64/ln2; ln2/64 split, hi with 32 significant bits (n hi exact, |n| < 2^21)
};
__device__ ExpK g_expk = {{8.333333333333333e-03, 4.1666666666666664e-02, 0.16666666666666666, 0.5},
                          92.33248261689366, 0.01083042469326756, 2.9815858269852933e-12};
__device__ const double g_exp2tab[128] = {  // (hi_j, lo_j): 2^(j/64) = hi_j + lo_j, j = 0..63
    1.0, 0.0, 1.0108892860517005, -1.5234778603368577e-17,
    1.0218971486541166, 5.109225028973444e-17, 1.0330248790212284, 7.600838874027088e-18,
    1.0442737824274138, 8.551889705537965e-17, 1.0556451783605572, 1.759325738772092e-18,
    1.0671404006768237, -7.899853966841582e-17, 1.0787607977571199, -6.656660436056593e-17,
    1.0905077326652577, -3.046782079812471e-17, 1.102382583307841, 5.2660368715706944e-17,
    1.1143867425958924, 1.0410278456845571e-16, 1.1265216186082418, 5.165856758795457e-17,
    1.1387886347566916, 8.912812676025408e-17, 1.1511892299529827, 3.250710218863827e-17,
    1.1637248587775775, 3.8292048369240935e-17, 1.1763969916502812, 5.554203254218079e-17,
    1.189207115002721, 3.982015231465646e-17, 1.202156731452703, 6.644981499252301e-17,
    1.215247359980469, -7.712630692681488e-17, 1.22848053610687, -1.89878163130253e-17,
    1.241857812073484, 4.658027591836937e-17, 1.255380757024691, -6.7113898212968784e-18,
    1.2690509571917332, 2.667932131342186e-18, 1.2828700160787783, 1.713594918243561e-17,
    1.2968395546510096, 2.5382502794888315e-17, 1.3109612115247644, -7.181536135519454e-17,
    1.3252366431597413, -2.8587312100388614e-17, 1.339667524053303, 8.927282594831732e-17,
    1.3542555469368927, 7.70094837980299e-17, 1.3690024229745905, 9.593797919118849e-17,
    1.383909881963832, -6.770511658794786e-17, 1.3989796725383112, -9.614213209051323e-17,
    1.4142135623730951, -9.667293313452913e-17, 1.42961333839197, -1.2031642489053655e-17,
    1.4451808069770467, -3.0237581349939873e-17, 1.460917794180647, -5.600377186075216e-17,
    1.4768261459394993, -3.483994556892796e-17, 1.4929077282912648, 1.4192920154284036e-17,
    1.5091644275934228, -1.016455327754295e-16, 1.5255981507445384, -1.1024941712342561e-16,
    1.5422108254079407, 7.949834809697621e-17, 1.559004400237837, 3.7812070533575275e-17,
    1.5759808451078865, -1.0136916471278304e-17, 1.593142151342267, -1.0094406542311964e-16,
    1.6104903319492543, 2.4707192569797888e-17, 1.6280274218573478, -6.712955084707084e-17,
    1.645755478153965, -1.0125679913674773e-16, 1.6636765803267364, 5.8909926967131e-17,
    1.681792830507429, 8.199010020581497e-17, 1.7001063537185235, -8.0237193703977e-18,
    1.718619298122478, -1.851380418263111e-17, 1.7373338352737062, 3.164389299292957e-17,
    1.7562521603732995, 2.960140695448873e-17, 1.7753764925265212, 6.429731796556572e-17,
    1.7947090750031072, 1.8227458427912087e-17, 1.8142521755003989, -9.969531538920349e-17,
    1.8340080864093424, 3.283107224245627e-17, 1.8539791250833855, 9.761887490727594e-17,
    1.8741676341103, -6.122763413004143e-17, 1.8945759815869656, 3.4034035352165297e-17,
    1.9152065613971474, -1.0619946056195963e-16, 1.9360617934922943, 1.0332385960676326e-16,
    1.9571441241754002, 8.960767791036668e-17, 1.978456026387951, 4.0388753109278167e-17
};
__device__ __forceinline__ double exp_sf(double x, const ExpK& k, const double* tab0) {
  constexpr double SH = 6755399441055744.0;  // 1.5 2^52
  const double t = fma(x, k.k64, SH);
  const double n = t - SH;
  const int ni = (int)__double_as_longlong(t);
  double r = fma(-n, k.hi, x);
  r = fma(-n, k.lo, r);
  double q = k.c[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) q = fma(q, r, k.c[i]);
  q = fma(q, r, 1.0) * r;  // e^r - 1
  const double2 tt = *(const double2*)((const char*)tab0 + ((ni << 4) & 0x3f0));  // entry ni & 63
  const double v = ldexp(tt.x + fma(tt.x, q, tt.y), ni >> 6);
  return x < -745.0 ? 0.0 : v;
}

// v from another lane of the same 16-lane row by a DPP control (two 32-bit DPP moves, no LDS)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
// sum over the 16 lanes of each row, the same value in every lane of the row: quad pairs (quad_perm
// [1,0,3,2], [2,3,0,1]), then quad with quad (row_half_mirror), half-row with half-row (row_mirror)
__device__ __forceinline__ double row_sum16(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  return v;
}
// v + v(lane ^ 16) and v + v(lane ^ 32) by gfx950's lane-swap instructions (VALU, no LDS round
// trip as with ds_bpermute).  A swap of v with itself leaves v and its partner's value in every
// lane, in one order or the other, so the sum of the two results is v + partner exactly (addition
// commutes): the same values as v += __shfl_xor(v, 16 / 32) (scratch/permlane_check.hip).
__device__ __forceinline__ double sum_xor16(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  return __builtin_bit_cast(double, ((long long)hi[0] << 32) | lo[0]) + __builtin_bit_cast(double, ((long long)hi[1] << 32) | lo[1]);
}
__device__ __forceinline__ double sum_xor32(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  return __builtin_bit_cast(double, ((long long)hi[0] << 32) | lo[0]) + __builtin_bit_cast(double, ((long long)hi[1] << 32) | lo[1]);
}

// lane m of each row of 16 lanes, broadcast to the row (DPP row_newbcast, gfx90a+; m folds to a
// constant once the caller's loop is unrolled)
__device__ __forceinline__ double row_bcast16(double v, int m) {
  switch (m & 15) {
    case 0: return dpp_f64<0x150>(v);
    case 1: return dpp_f64<0x151>(v);
    case 2: return dpp_f64<0x152>(v);
    case 3: return dpp_f64<0x153>(v);
    case 4: return dpp_f64<0x154>(v);
    case 5: return dpp_f64<0x155>(v);
    case 6: return dpp_f64<0x156>(v);
    case 7: return dpp_f64<0x157>(v);
    case 8: return dpp_f64<0x158>(v);
    case 9: return dpp_f64<0x159>(v);
    case 10: return dpp_f64<0x15A>(v);
    case 11: return dpp_f64<0x15B>(v);
    case 12: return dpp_f64<0x15C>(v);
    case 13: return dpp_f64<0x15D>(v);
    case 14: return dpp_f64<0x15E>(v);
    default: return dpp_f64<0x15F>(v);
  }
}

// per-tile partials of z = L^-1 y and of the blocks' right-hand sides (see zp_acc4)
__device__ __forceinline__ double* zp_row(const DevBatch& db, int slot, int h) {
  return db.zp + ((size_t)slot * 2 * db.nt + h) * db.Npad;
}
// per-row-tile partials of alpha = L^-T z (see ap_acc4): ap_row(ti)[64 tj + c] for tj left of ti's
// block.  They live in zp's unused triangle, row 2 ti: of zp_row(2 c) the z partials use the
// columns of the row tiles r >= c only, and tj < ti.  No buffer of their own: gprx_batch_bytes and
// the allocation stay what they were.
__device__ __forceinline__ double* ap_row(const DevBatch& db, int slot, int ti) { return zp_row(db, slot, 2 * ti); }
// A block's working right-hand side Yw (k_rhs; DESIGN.md section 4, "Recursion") lives in the alpha
// buffer: alpha is written last, by k_alpha, in stream order after every reader of Yw, and k_rhs
// rewrites Yw before a block reads it, so neither sees the other.
__device__ __forceinline__ double* yw_slot(const DevBatch& db, int slot) { return db.alpha + (size_t)slot * db.Npad; }
// a diagonal tile from an LDS image: row r of X at img[r * rs + c * cs].  The 256-thread
// workgroup splits the 64 columns in 4 quarters through the [256]-double scratch (no serial
// chain); call from every thread of the workgroup (contains barriers).
__device__ __forceinline__ void zp_diag(const DevBatch& db, int slot, int jt, const double* img, int rs, int cs,
                                        double* scr) {
  const double* y = yw_slot(db, slot) + jt * TS;
  const int r = threadIdx.x & 63, qc = threadIdx.x >> 6;
  double t = 0.0;
#pragma unroll
  for (int c = 16 * qc; c < 16 * qc + 16; ++c) t = fma(img[r * rs + c * cs], y[c], t);  // X upper = 0
  __syncthreads();
  scr[qc * TS + r] = t;
  __syncthreads();
  if (qc == 0) {
    zp_row(db, slot, 2 * jt)[jt * TS + r] = ((scr[r] + scr[TS + r]) + scr[2 * TS + r]) + scr[3 * TS + r];
    zp_row(db, slot, 2 * jt + 1)[jt * TS + r] = 0.0;
  }
  __syncthreads();
}

// Buffer resource over [base, base + bytes) (gfx9 word 3: raw, bounds-checked) and a 64-bit load
// at byte offset voff (VGPR) + soff (SGPR): out-of-range reads return 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, bytes, 0x00020000);
}
__device__ __forceinline__ double buffer_load_f64(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
// 8-B store at byte offset voff (VGPR) + soff (SGPR): 64-bit data, no store-data hazard (a VALU
// overwrite of >64-bit store data needs wait states the compiler skips for a register soffset;
// see buffer_store_f64x2)
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void buffer_store_f64(__amdgpu_buffer_rsrc_t r, int voff, int soff, double x) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, x), r, voff, soff, 0);
}
// -x by the sign bit (exact, as a multiply by -1; an integer VALU op)
__device__ __forceinline__ double neg_f64(double x) {
  return __builtin_bit_cast(double, __builtin_bit_cast(unsigned long long, x) ^ 0x8000000000000000ull);
}
// 16-B store at byte offset voff (VGPR).  The SGPR offset field is left 0 on purpose: a MUBUF store
// with a register soffset is exempt from the compiler's store-data hazard check (no wait state
// before a VALU overwrites the data VGPRs), and on gfx950 under memory back-pressure (another
// process on the card) the store then read the NEXT exp's intermediate 1.5*2^52 + n as its data:
// K elements ~6.76e15, a non-PD pivot in a few evaluations in ten (scratch/concurrency.py).  With
// soffset 0 the hazard recognizer inserts the wait states.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void buffer_store_f64x2(__amdgpu_buffer_rsrc_t r, int voff, double x, double y) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, make_double2(x, y)), r, voff, 0, 0);
}

}  // namespace gprx
