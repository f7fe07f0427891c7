// gprx_stamps.h -- the diagnostic builds' in-kernel clocks (-DGPRX_STAMPS, -DGPRX_GSTAMPS=...): device
// globals, writers, and the macros that vanish in the product build; then the two host readers.
//
// A part of gprx_kernels.hip, included there once and by no other file (the parts and their order
// are listed at its includes).
#pragma once

namespace gprx {

// ---- diagnostic build only (-DGPRX_STAMPS, scratch/clock.py): the in-kernel clock of a main loop
// (MI355X_MICROARCH.md 'DVFS give-back' item 6): s_memtime (shader cycles) and s_memrealtime
// (100 MHz) before and after, per wave, into a buffer no other code reads.  Not in the product build.
#ifdef GPRX_STAMPS
constexpr int STAMP_MAX = 1 << 18;  // waves per stamp region
__device__ unsigned long long g_stamps[3][STAMP_MAX][4];
struct Stamp {
  unsigned long long t, r;
};
__device__ __forceinline__ Stamp stamp_now() {
  __builtin_amdgcn_sched_barrier(0);
  Stamp s{__builtin_amdgcn_s_memtime(), __builtin_amdgcn_s_memrealtime()};
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only
  __builtin_amdgcn_sched_barrier(0);
  return s;
}
__device__ __forceinline__ void stamp_store(int region, const Stamp& a, const Stamp& b) {
  const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && i < STAMP_MAX) {
    g_stamps[region][i][0] = a.t;
    g_stamps[region][i][1] = b.t;
    g_stamps[region][i][2] = a.r;
    g_stamps[region][i][3] = b.r;
  }
}
// leaf timeline: s_memrealtime of wave 0 at event ev of leaf o / 4 of this slot (slots < 256)
__device__ __forceinline__ void leaf_ts(int o, int slot, int ev) {
  if (threadIdx.x == 0 && slot < 256) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    (&g_stamps[2][0][0])[((size_t)((o >> 2) & 7) * 256 + slot) * 32 + ev] = t;
  }
}
#define LEAF_TS(ev) leaf_ts(o, slot, ev)
// k_leaf9 timeline (scratch/leaf8_timeline.py): lane 0 of the calling wave stamps event ev of
// leaf o / 4 of this slot
__device__ __forceinline__ void leaf9_ts(int o, int slot, int ev) {
  if ((threadIdx.x & 63) == 0 && slot < 256) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    (&g_stamps[2][0][0])[((size_t)((o >> 2) & 7) * 256 + slot) * 32 + ev] = t;
  }
}
#define L9_TS(ev) leaf9_ts(o, slot, ev)
// the single-wave diagonal routine's internal events (after the leaf stamps in region 2)
__device__ __forceinline__ void diag_ts(int jt, int slot, int ev) {
  if ((threadIdx.x & 63) == 0 && slot < 256) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    (&g_stamps[2][0][0])[65536 + ((((size_t)((jt >> 2) & 7) * 256 + slot) * 4 + (jt & 3)) * 16) + ev] = t;
  }
}
#define D_TS1(ev) diag_ts(jt, slot, ev)
// per-wave item events of the leaf's phase B (after the diagonal routine's events)
__device__ __forceinline__ void wave_ts(int o, int slot, int ev) {
  if ((threadIdx.x & 63) == 0 && slot < 256) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    (&g_stamps[2][0][0])[196608 + ((((size_t)((o >> 2) & 7) * 256 + slot) * 8 + (threadIdx.x >> 6)) * 32) + ev] = t;
  }
}
#define W_TS(ev) wave_ts(o, slot, ev)
// the whole-node kernel (k_node8): thread 0 stamps phase ev of slot's node launch (region
// 0 from entry 2^19: 8 per slot: start, after the top leaf, TRSM, SYRK + TT, the bottom leaf, end,
// then the hardware CU id and XCC id)
__device__ __forceinline__ void node_ts(int slot, int ev) {
  if (threadIdx.x == 0 && slot < 32768) {
    unsigned long long t = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (ev == 6) t = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));
    if (ev == 7) t = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (15 << 11));
    (&g_stamps[0][0][0])[524288 + (size_t)slot * 8 + ev] = t;
  }
}
#define N_TS(ev) node_ts(slot, ev)
#else
#define N_TS(ev)
#define D_TS1(ev)
#define LEAF_TS(ev)
#define L9_TS(ev)
#define W_TS(ev)
#endif
// ---- diagnostic build only (-DGPRX_GSTAMPS=op*100+n, scratch/gemm_timeline.py): per-wave
// s_memrealtime of the GEMM launch of op at node size n: tile entry, core start, core end (loads
// landed), epilogue end (stores landed), for the wave's first two tiles.  Not in the product build.
#ifdef GPRX_GSTAMPS
constexpr int GTS_MAX = 1 << 17;
__device__ unsigned long long g_gts[GTS_MAX][8];
__device__ __forceinline__ void gts(const GemmGeom& g, int pass, int ev) {
  if (GPRX_GSTAMPS == 1208) {  // k_node8's SYRK + TT phase: every wave (8 per block), 4 tiles, 4 events
    if (!((g.op == OP_SYRK || g.op == OP_TT) && g.n == 8) || pass > 3 || blockDim.x != 512) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    const size_t i = (size_t)blockIdx.x * 8 + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && 2 * i + 1 < GTS_MAX) (&g_gts[0][0])[i * 16 + 4 * pass + ev] = t;
    return;
  }
  if (g.op * 100 + g.n != GPRX_GSTAMPS || pass > 1) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long t = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && i < GTS_MAX) g_gts[i][4 * pass + ev] = t;
}
#define GTS(g, pass, ev) gts(g, pass, ev)
// the gradient GEMM (GPRX_GSTAMPS=999): job entry, then per unit u: main loop start, main loop end,
// unit end, at slots 1 + 3u ..; =998: unit 0 only, with its epilogue phases (gts_d)
__device__ __forceinline__ void gts_d(int gu, int ev) {  // =998: unit 0's epilogue phases at slots 4..7
  if (GPRX_GSTAMPS != 998 || gu != 0) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long t = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && i < GTS_MAX) g_gts[i][ev] = t;
}
__device__ __forceinline__ void gts_l(int ev) {
  if (GPRX_GSTAMPS != 999 && !(GPRX_GSTAMPS == 998 && ev < 4)) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long t = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);
  const size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && i < GTS_MAX) g_gts[i][ev] = t;
}
#define GTS_L(ev) gts_l(ev)
#define GTS_D(gu, ev) gts_d(gu, ev)
#else
#define GTS_D(gu, ev)
#define GTS(g, pass, ev)
#define GTS_L(ev)
#endif

}  // namespace gprx

#ifdef GPRX_GSTAMPS
// diagnostic build only: copy (reset = 0) or clear (reset = 1) the GEMM tile timeline
extern "C" int gprx_dbg_gts(unsigned long long* out, long long n, int reset) {
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(gprx::g_gts)) != hipSuccess) return 3;
  const size_t bytes = std::min<size_t>((size_t)n * 8, sizeof(gprx::g_gts));
  if (hipDeviceSynchronize() != hipSuccess) return 3;
  if (reset) return hipMemset(p, 0, sizeof(gprx::g_gts)) == hipSuccess ? 0 : 3;
  return hipMemcpy(out, p, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 3;
}
#endif
#ifdef GPRX_STAMPS
// diagnostic build only: copy (reset = 0) or clear (reset = 1) stamp region `which`
extern "C" int gprx_dbg_stamps(int which, unsigned long long* out, long long n, int reset) {
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(gprx::g_stamps)) != hipSuccess) return 3;
  char* base = (char*)p + (size_t)which * sizeof(gprx::g_stamps[0]);
  const size_t bytes = std::min<size_t>((size_t)n * 8, sizeof(gprx::g_stamps[0]));
  if (hipDeviceSynchronize() != hipSuccess) return 3;
  if (reset) return hipMemset(base, 0, sizeof(gprx::g_stamps[0])) == hipSuccess ? 0 : 3;
  return hipMemcpy(out, base, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 3;
}
#endif
