// gprx_api.hip -- C ABI (include/gprx.h) over the gfx950 kernels: context/stream ownership,
// batch workspaces in HBM, the per-evaluation launch sequence, status mapping, profiling.
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/gprx.h"
#include "gprx_internal.h"

using gprx::DevBatch;
using gprx::TS;

namespace {

struct KStat {
  double ms = 0.0, flops = 0.0, bytes = 0.0;
  int64_t n = 0;
};
struct PendingEv {
  std::string name;
  std::string level;  // optional second key, e.g. "potrf_syrk/n32" (per recursion level)
  hipEvent_t a, b;
  double flops, bytes;
};

}  // namespace

struct gprx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::string err;
  int dist_mode = GPRX_DIST_DIRECT;  // the Gram of GaussianProcesses cov_ij (distij) [ext]
  bool prof = false;
  std::map<std::string, KStat> stats;
  std::vector<hipEvent_t> evpool;
  std::vector<PendingEv> pending;
  // recursion nodes of <= this many tiles run fused in k_leaf; 0 = auto: 4 for batches of >= 32
  // slots (fewer launches), 1 below that (GPRX_OPT_LEAF_TILES)
  int leaf_tiles = 0;
  // recursion nodes of <= this many tiles use the 64 x 32 pair-unit GEMM; 0 = auto (set_geometry:
  // 4 for batches of >= 32 slots, every node below that) (GPRX_OPT_SMALL_N)
  int small_n = 0;
  // replay each batch's launch sequence as a hipGraph (GPRX_OPT_GRAPHS).  Off by default: measured
  // equal to direct launches at B=1..192 (the launches are queued far ahead of the GPU).
  bool use_graphs = false;
  // GPRX_OPT_ACTIVE_DIMS: gprx_batch_set_train looks for the input dimensions that are constant and
  // direct-mode evaluations skip them (DevBatch::da).  last_da: the count the latest evaluation or
  // gprx_batch_set_train of this context ran with (gprx_ctx_kernel_stats "active_dims").
  bool active_dims = true;
  int last_da = 0;
  std::set<gprx_batch*> batches;      // live batches (destroyed with the context)
  void* rbuf = nullptr;               // rollout argument buffer (device), grown on demand
  size_t rcap = 0;
};

struct gprx_batch {
  gprx_ctx* ctx = nullptr;
  DevBatch db{};
  double* h_params = nullptr;  // pinned
  double* h_out = nullptr;     // pinned, B*(d+3)
  double* h_mu = nullptr;      // pinned, B*Mpad
  double* h_var = nullptr;
  int* h_status = nullptr;  // pinned, 2B (status, info)
  int* opt_active = nullptr;  // device, B: the optimiser's per-round evaluation mask (DevBatch::active)
  double* opt_trace = nullptr;  // caller's host buffer for gprx_batch_set_opt_trace (diagnostics)
  int opt_trace_rounds = 0;
  // joint-covariance workspace (gprx_batch_predict_cov / gprx_batch_sample), allocated on first use
  // for the batch's current Mpad and re-allocated when gprx_batch_set_test grows it
  double* cov_vt = nullptr;   // B x [Npad][Mpad]  V^T
  double* cov_sig = nullptr;  // B x Mpad^2        Sigma, compact [M][M] per slot
  double* cov_f = nullptr;    // B x Mpad^2        its factor
  double* cov_z = nullptr;    // B x Mpad^2        Z, up to Mpad vectors per slot a pass
  double* cov_smp = nullptr;  // B x Mpad^2        samples of the pass
  double* cov_jit = nullptr;  // B
  int* cov_st = nullptr;      // B
  double* h_cov = nullptr;    // pinned, B doubles + B ints: jitter and status
  int cov_mpad = 0;           // the Mpad the workspace was sized for (0: none)
  // fold layout of gprx_batch_set_folds (CvArgs in gprx_internal.h): the device table, the ints between
  // two slots' layouts (0: shared), the folds, the largest tile count of a slot; cv_folds = 0: none set
  int* cv_tab = nullptr;
  size_t cv_lstride = 0;
  int cv_folds = 0;
  int cv_njmax = 0;
  bool factored = false;
  bool have_train = false;
  bool have_test = false;
  // the non-constant dimensions gprx_batch_set_train found (every dimension with the option off);
  // as a bit per dimension; db.amask holds what Xc was written for, which is this set in direct
  // mode (sync_active)
  unsigned long long found_mask = 0;
  // captured evaluation graphs, one per (want_grad, want_pred); valid while the key matches
  hipGraphExec_t gexec[4] = {};
  DevBatch gkey[4];
  int gkey_ctx[4][2] = {};
  bool gvalid[4] = {};
};

struct gprx_gp {
  gprx_batch* batch = nullptr;
  int M_cap = 0;
};

namespace {

int set_err(gprx_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}
// A batch call's return code from its per-slot statuses: the first that is not GPRX_OK, with the
// error text "fn: <status string>".
int first_status(gprx_ctx* c, const char* fn, const int* st, int B) {
  for (int s = 0; s < B; ++s)
    if (st[s] != GPRX_OK) return set_err(c, st[s], std::string(fn) + ": " + gprx_status_string(st[s]));
  return GPRX_OK;
}

#define HIPCHK(ctx, expr)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      (void)hipGetLastError(); /* not sticky for the context's next call */                        \
      return set_err((ctx), e_ == hipErrorOutOfMemory ? GPRX_OUT_OF_MEMORY : GPRX_DEVICE_ERROR,     \
                     std::string(#expr) + ": " + hipGetErrorString(e_));                           \
    }                                                                                              \
  } while (0)

hipEvent_t ev_get(gprx_ctx* c) {
  if (!c->evpool.empty()) {
    hipEvent_t e = c->evpool.back();
    c->evpool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

// Launch helper: optional HIP-event bracket per launch, on the context stream.
template <class F>
void timed(gprx_ctx* c, hipStream_t st, const char* name, double flops, double bytes, F&& f, int level = 0) {
  if (!c->prof) {
    f();
    return;
  }
  hipEvent_t a = ev_get(c), b = ev_get(c);
  (void)hipEventRecord(a, st);
  f();
  (void)hipEventRecord(b, st);
  c->pending.push_back({name, level ? std::string(name) + "/n" + std::to_string(level) : std::string(), a, b, flops, bytes});
}

void collect(gprx_ctx* c) {
  for (auto& p : c->pending) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, p.a, p.b);
    for (int k = 0; k < 2; ++k) {
      if (k == 1 && p.level.empty()) break;
      KStat& s = c->stats[k ? p.level : p.name];
      s.ms += ms;
      s.n += 1;
      s.flops += p.flops;
      s.bytes += p.bytes;
    }
    c->evpool.push_back(p.a);
    c->evpool.push_back(p.b);
  }
  c->pending.clear();
}

// The GEMM cores, the Gram and the LINV21 store address their operands through buffer resources of
// 0x7ffffff0 bytes from a tile origin, with 32-bit byte offsets (gprx_kernels.hip buffer_rsrc,
// core_ptr): a K walk spans up to Npad columns of ld = Npad (the factorisation) or Npad rows of
// ld = Mpad (the prediction variance's K*^T).  Beyond that range a load would silently read 0, so
// such sizes are refused (N <= 16320 at M <= Npad).
constexpr size_t BUF_LIMIT = 0x7ffffff0;
size_t pad64(size_t n) { return (n + TS - 1) / TS * TS; }
size_t test_capacity(int M_max) { return std::max<size_t>(pad64(M_max), TS); }  // Mpad: at least one tile
bool sizes_addressable(int N, int M_max) {
  const size_t Npad = pad64(N);
  return Npad * std::max(Npad, test_capacity(M_max)) * sizeof(double) < BUF_LIMIT;
}
bool cov_addressable(int M_max) { return test_capacity(M_max) * test_capacity(M_max) * sizeof(double) < BUF_LIMIT; }

// The dimensions every buffer size follows from (sizes_addressable first): the training side once,
// at creation; the test side whenever the capacity for test points changes.
// The active dimensions of the evaluation kernels and what follows from their count.
unsigned long long all_dims(int d) { return d >= 64 ? ~0ull : (1ull << d) - 1ull; }
void set_active(DevBatch& db, unsigned long long mask) {
  db.amask = mask;
  db.da = __builtin_popcountll(mask);
  db.xs = db.da | 1;
  db.gps = db.da + 2;
}
void set_train_dims(DevBatch& db, int B, int d, int N) {
  db.B = B;
  db.d = d;
  db.N = N;
  db.Npad = (int)pad64(N);
  db.nt = db.Npad / TS;
  db.ntl = db.nt * (db.nt + 1) / 2;
  db.ld = db.Npad;
  db.mat = (size_t)db.Npad * db.Npad;
  db.pst = d + 4;
  // the gradient's units are planned for all d dimensions, whatever the active set: the partition
  // fixes the order in which the partial sums are added, so it must not follow da
  db.nlj = gprx::lauum_plan(db.nt, d, &db.ngu, &db.nimg, nullptr);
  set_active(db, all_dims(d));
}
void set_test_dims(DevBatch& db, int M_max) {
  db.M = 0;
  db.Mpad = (int)test_capacity(M_max);
  db.mt = db.Mpad / TS;
}

// One buffer of a batch: where its pointer lives, elements, element size, device or pinned host
// memory, zero-filled when allocated.  A batch's buffers come in three groups, each listed by one
// function from the batch's dimensions alone (the pointers may be null): allocation, release and
// gprx_batch_bytes / gprx_batch_cov_bytes all read these lists and nothing else.
struct Buf {
  void** p;
  size_t count, size;
  bool pinned, zero;
};
template <class T>
Buf dev(T*& p, size_t count, bool zero = false) {
  return {(void**)&p, count, sizeof(T), false, zero};
}
template <class T>
Buf pin(T*& p, size_t count, size_t size = sizeof(T)) {
  return {(void**)&p, count, size, true, false};
}
using BufList = std::vector<Buf>;

// created with the batch.  Zero padding of X / Y (pad columns never enter a result; kept finite)
// and of the matrices the factorisation writes in part
BufList train_bufs(gprx_batch& b) {
  DevBatch& db = b.db;
  const size_t B = db.B, Np = db.Npad, d = db.d;
  // Xc and grad_part are sized for all d dimensions (an active set uses their front)
  return {dev(db.X, B * Np * d, true), dev(db.Xc, B * Np * (d | 1)), dev(db.Y, B * Np, true), dev(db.K, B * db.mat),
          dev(db.S, B * db.mat, true), dev(db.Lw, B * db.mat, true), dev(db.Linv, B * db.mat, true),
          dev(db.Mt, B * db.mat, true), dev(db.z, B * Np), dev(db.zp, B * 2 * db.nt * Np), dev(db.alpha, B * Np),
          dev(db.params, B * db.pst), dev(db.theta, B * (d + 2)), dev(db.logdet_part, B * db.nt),
          dev(db.grad_part, B * db.ngu * (d + 2)), dev(db.out, B * (d + 3)), dev(db.status, 2 * B) /* status, info */,
          dev(db.lauum_order, 2 * gprx::LU * (size_t)std::max(db.nlj, 0)), dev(b.opt_active, B),
          pin(b.h_params, B * db.pst), pin(b.h_out, B * (d + 3)), pin(b.h_status, 2 * B)};
}
// sized by Mpad, regrown by gprx_batch_set_test
BufList test_bufs(gprx_batch& b) {
  DevBatch& db = b.db;
  const size_t B = db.B, Mp = db.Mpad;
  return {dev(db.Xs, B * Mp * db.d, true), dev(db.KsT, B * db.Npad * Mp), dev(db.mu_part, B * db.nt * Mp),
          dev(db.var_part, B * db.nt * Mp), dev(db.out_mu, B * Mp), dev(db.out_var, B * Mp),
          pin(b.h_mu, B * Mp), pin(b.h_var, B * Mp)};
}
// the joint-covariance workspace, sized by Mpad, allocated on first use (cov_alloc): V^T, Sigma, its
// factor; the Z and sample buffers of a pass; the per-slot jitter and status and their host mirror
BufList cov_bufs(gprx_batch& b) {
  const DevBatch& db = b.db;
  const size_t B = db.B, mm = (size_t)db.Mpad * db.Mpad;
  return {dev(b.cov_vt, B * db.Npad * db.Mpad), dev(b.cov_sig, B * mm), dev(b.cov_f, B * mm), dev(b.cov_z, B * mm),
          dev(b.cov_smp, B * mm), dev(b.cov_jit, B), dev(b.cov_st, B), pin(b.h_cov, B, sizeof(double) + sizeof(int))};
}

void bufs_free(const BufList& l) {
  for (const Buf& u : l) {
    if (*u.p) (void)(u.pinned ? hipHostFree(*u.p) : hipFree(*u.p));
    *u.p = nullptr;
  }
}
// All of a list (its pointers null on entry), or none of it: a failure frees what it got.  An empty
// buffer still gets one element, so that its pointer is valid.
int bufs_alloc(gprx_ctx* c, const BufList& l) {
  for (const Buf& u : l) {
    const size_t bytes = std::max<size_t>(u.count, 1) * u.size;
    hipError_t e = u.pinned ? hipHostMalloc(u.p, bytes) : hipMalloc(u.p, bytes);
    int rc = GPRX_OK;
    if (e != hipSuccess) {
      *u.p = nullptr;
      rc = u.pinned ? set_err(c, GPRX_OUT_OF_MEMORY, "hipHostMalloc failed")
                    : set_err(c, e == hipErrorOutOfMemory ? GPRX_OUT_OF_MEMORY : GPRX_DEVICE_ERROR,
                              std::string("hipMalloc: ") + hipGetErrorString(e));
    } else if (u.zero && hipMemset(*u.p, 0, bytes) != hipSuccess) {
      rc = GPRX_DEVICE_ERROR;
    }
    if (rc) {
      (void)hipGetLastError();  // clear the runtime's sticky error: later calls check hipGetLastError
      bufs_free(l);
      return rc;
    }
  }
  return GPRX_OK;
}
size_t bufs_device_bytes(const BufList& l) {
  size_t n = 0;
  for (const Buf& u : l)
    if (!u.pinned) n += u.count * u.size;
  return n;
}

// The joint-covariance workspace goes with the test buffers it was sized for.
void cov_free(gprx_batch* b) {
  bufs_free(cov_bufs(*b));
  b->cov_mpad = 0;
}
// A batch without test buffers, and saying so: the state after a regrow that failed.  A later
// gprx_batch_set_test allocates afresh; until then there is nothing to predict.
void drop_test(gprx_batch* b) {
  bufs_free(test_bufs(*b));
  cov_free(b);
  b->db.M = b->db.Mpad = b->db.mt = 0;
  b->have_test = false;
}
// The test buffers for M_max points (none held on entry); a failure leaves drop_test's state.
int alloc_test(gprx_batch* b, int M_max) {
  set_test_dims(b->db, M_max);
  const int rc = bufs_alloc(b->ctx, test_bufs(*b));
  if (rc) drop_test(b);
  return rc;
}

int copy_in(gprx_ctx* c, void* dst, const void* src, size_t bytes, int mem) {
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, mem == GPRX_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                           c->stream));
  return GPRX_OK;
}

// Recursive Cholesky + inverse over tile range [o, o+n) (tile units), all slots in lock step.
// upd: the node lies in the trailing block of an ancestor (its tiles were updated into S); the top
// child inherits the parent's flag, the bottom child follows the parent's SYRK.
// The right-hand side goes with it by forward substitution over the blocks (nodes of <= BLK_TILES
// tiles, blk_range).  On entry Yw (yw_slot: the alpha buffer, free until k_alpha) is due to hold,
// for the node's rows, y - L[rows, :64 o] z[:64 o]; on return db.z holds the node's final z.  A
// block forms its Yw from the partials the TRSMs of its split ancestors left in zp (k_rhs), factors
// as before with every L^-1 producer writing its partial of Linv Yw, and sums those into z
// (k_znode); a split node's TRSM writes -L21 z1 for its bottom child, and its LINV21 the alpha
// partial Linv21^T z2 (gemm_tile).
void factor_block(gprx_ctx* c, hipStream_t st, const DevBatch& db, int o, int n, int upd);
void factor_rec(gprx_ctx* c, hipStream_t st, const DevBatch& db, int o, int n, int upd) {
  if (n > gprx::BLK_TILES) {
    factor_block(c, st, db, o, n, upd);  // splits: n exceeds every leaf
    return;
  }
  const double Bd = db.B, rows = n * TS;
  timed(c, st, "alpha", Bd * rows * 2.0 * o, Bd * 8.0 * rows * (2.0 * o + 2.0), [&] { gprx::launch_rhs(db, o, n, st); });
  factor_block(c, st, db, o, n, upd);
  timed(c, st, "alpha", Bd * rows * (n + 1.0), Bd * 8.0 * rows * (n + 2.0), [&] { gprx::launch_znode(db, o, n, st); });
}
void factor_block(gprx_ctx* c, hipStream_t st, const DevBatch& db, int o, int n, int upd) {
  const double T = TS, Bd = db.B;
  const int leaf = c->leaf_tiles > 0 ? c->leaf_tiles : (db.B >= 32 ? 4 : 1);
  if (n > 1 && n <= leaf) {
    const double m = n * T;
    timed(c, st, "leaf", Bd * (m * m * m / 3.0 + m * m * m / 3.0), Bd * 8.0 * 3.0 * m * m,
          [&] { gprx::launch_leaf(db, o, n, upd, st); }, n);
    return;
  }
  if (n == 8 && leaf == 4 && db.B >= 32) {  // the whole node in one launch (k_node8)
    const double m = 4 * T;
    timed(c, st, "node8", Bd * (4.0 * m * m * m / 3.0 + 4.0 * m * m * m), Bd * 8.0 * (16.0 * m * m + 6.5 * m * m),
          [&] { gprx::launch_node8(db, o, upd, st); }, n);
    return;
  }
  if (n == 1) {
    timed(c, st, "diag", Bd * (T * T * T / 3.0 + T * T * T / 3.0), Bd * 8.0 * 3.0 * T * T,
          [&] { gprx::launch_diag(db, o, upd, st); });
    return;
  }
  const int h = n / 2;
  const double m1 = h * T, m2 = (n - h) * T;
  const auto child = n > gprx::BLK_TILES ? factor_rec : factor_block;  // inside a block: no further blocks
  child(c, st, db, o, h, upd);
  gprx::GemmGeom g{gprx::OP_TRSM, o, h, n, upd};
  const double f_trsm = Bd * m2 * m1 * m1, f_syrk = Bd * m2 * m2 * m1, f_tt = Bd * m2 * m1 * m1,
               f_linv = Bd * m1 * m2 * m2;
  const double b_trsm = Bd * 8.0 * (2.0 * m2 * m1 + m1 * m1 / 2.0), b_syrk = Bd * 8.0 * (m2 * m1 + m2 * m2),
               b_tt = Bd * 8.0 * (2.0 * m2 * m1 + m1 * m1 / 2.0), b_linv = Bd * 8.0 * (3.0 * m2 * m1 + m2 * m2 / 2.0);
  timed(c, st, "potrf_trsm", f_trsm, b_trsm, [&] { gprx::launch_gemm(db, g, st); }, n);
  gprx::GemmGeom gs{gprx::OP_SYRK, o, h, n, upd}, gt{gprx::OP_TT, o, h, n, upd};
  // T^T = L11^-T L21^T needs only rec(A11) and the TRSM: it runs in the SYRK's launch
  timed(c, st, "syrk_tt", f_syrk + f_tt, b_syrk + b_tt, [&] { gprx::launch_gemm(db, gs, st, gt); }, n);
  child(c, st, db, o + h, n - h, 1);
  g.op = gprx::OP_LINV21;
  timed(c, st, "trtri_linv21", f_linv, b_linv, [&] { gprx::launch_gemm(db, g, st); }, n);
}

void predict_cross(gprx_ctx* c, hipStream_t st, const DevBatch& db) {
  const double N = db.N, M = db.M, d = db.d, B = db.B;
  timed(c, st, "pred_cross", B * 3.0 * N * M * d, B * 8.0 * (N * db.Mpad + (N + M) * d),
        [&] { gprx::launch_pred_cross(db, st); });
}
void predict_var(gprx_ctx* c, hipStream_t st, const DevBatch& db) {
  if (!db.want_var) return;
  const double N = db.N, M = db.M, B = db.B;
  gprx::GemmGeom g{gprx::OP_PREDVAR, 0, 0, 0};
  timed(c, st, "pred_var", B * N * N * M, B * 8.0 * (N * N / 2 + N * db.Mpad), [&] { gprx::launch_gemm(db, g, st); });
}
void predict_mean_final(gprx_ctx* c, hipStream_t st, const DevBatch& db) {
  const double B = db.B;
  timed(c, st, "pred_final", B * 2.0 * db.nt * db.Mpad, B * 16.0 * db.nt * db.Mpad,
        [&] { gprx::launch_pred_final(db, st); });
}
void predict_group(gprx_ctx* c, hipStream_t st, const DevBatch& db) {
  predict_cross(c, st, db);
  predict_var(c, st, db);
  predict_mean_final(c, st, db);
}

// Whole evaluation of a batch (or a slot range of it) on stream `st`.
void eval_group(gprx_ctx* c, hipStream_t st, const DevBatch& db, bool want_grad, bool want_pred) {
  const double Bd = db.B, Np = db.Npad, d = db.d;
  timed(c, st, "gram", Bd * 3.0 * db.N * (double)db.N * d / 2.0, Bd * 8.0 * (Np * Np / 2.0 + Np * d),
        [&] { gprx::launch_gram(db, st); });
  factor_rec(c, st, db, 0, db.nt, 0);
  // k_alpha streams Mt's upper triangle inside each block and adds the ap rows below it
  double tri = 0.0, apn = 0.0;  // elements per slot
  for (int i = 0, lo, hi; i < db.nt; ++i) {
    gprx::blk_range(db.nt, i, lo, hi);
    tri += (double)TS * TS * (hi - i);
    apn += (double)TS * (db.nt - hi);
  }
  timed(c, st, "alpha", Bd * (2.0 * tri + apn), Bd * 8.0 * (tri + apn + 2.0 * Np), [&] { gprx::launch_alpha(db, st); });
  if (want_grad)
    timed(c, st, "lauum_grad", Bd * (Np * Np * Np / 3.0 + Np * Np * d + 4.0 * Np * Np),
          Bd * 8.0 * (Np * Np + Np * (db.xs + 2.0)),  // minimum: Mt upper, Kf lower, Xc, alpha once
          [&] { gprx::launch_lauum_grad(db, st); });
  timed(c, st, "finalize", Bd * 2.0 * db.N, Bd * 16.0 * db.N, [&] { gprx::launch_finalize(db, want_grad ? 1 : 0, st); });
  if (want_pred) predict_group(c, st, db);
}

// One evaluation as a replayed hipGraph: ~40-50 dependent launches per evaluation become one
// graph launch (captured on first use; re-captured when the batch geometry, the test set or a
// kernel variant changes).  Used when profiling is off and the batch is one slot group.
int run_graph(gprx_batch* b, bool want_grad, bool want_pred) {
  gprx_ctx* c = b->ctx;
  const DevBatch& db = b->db;
  const int gi = (want_grad ? 1 : 0) + (want_pred ? 2 : 0);
  const bool same = b->gvalid[gi] && memcmp(&b->gkey[gi], &db, sizeof(DevBatch)) == 0 &&
                    b->gkey_ctx[gi][0] == c->leaf_tiles && b->gkey_ctx[gi][1] == c->small_n;
  if (!same) {
    if (b->gvalid[gi]) (void)hipGraphExecDestroy(b->gexec[gi]);
    b->gvalid[gi] = false;
    hipGraph_t graph = nullptr;
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    eval_group(c, c->stream, db, want_grad, want_pred);
    const hipError_t le = hipGetLastError();
    const hipError_t ce = hipStreamEndCapture(c->stream, &graph);
    if (le != hipSuccess || ce != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      return set_err(c, GPRX_DEVICE_ERROR, std::string("graph capture: ") + hipGetErrorString(le != hipSuccess ? le : ce));
    }
    const hipError_t ie = hipGraphInstantiate(&b->gexec[gi], graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    HIPCHK(c, ie);
    memcpy(&b->gkey[gi], &db, sizeof(DevBatch));
    b->gkey_ctx[gi][0] = c->leaf_tiles;
    b->gkey_ctx[gi][1] = c->small_n;
    b->gvalid[gi] = true;
  }
  HIPCHK(c, hipGraphLaunch(b->gexec[gi], c->stream));
  return GPRX_OK;
}

// One evaluation on the context stream: direct launches, or the captured graph when enabled.
// factor = false: prediction only, from the last factorisation.
int run_eval(gprx_batch* b, bool want_grad, bool want_pred, bool factor) {
  gprx_ctx* c = b->ctx;
  if (factor && c->use_graphs && !c->prof) return run_graph(b, want_grad, want_pred);
  if (factor) eval_group(c, c->stream, b->db, want_grad, want_pred);
  else if (want_pred) predict_group(c, c->stream, b->db);
  HIPCHK(c, hipGetLastError());
  return GPRX_OK;
}

// Before an evaluation: Xc and the active list follow the context's distance mode.  Direct mode
// takes the list gprx_batch_set_train found; expanded mode keeps every dimension (a^2 + b^2 - 2ab of
// a constant is no exact zero).  A change re-centres Xc on the stream and drops the captured graphs,
// which hold DevBatch by value.
int sync_active(gprx_batch* b) {
  gprx_ctx* c = b->ctx;
  DevBatch& db = b->db;
  const unsigned long long mask = c->dist_mode == GPRX_DIST_DIRECT ? b->found_mask : all_dims(db.d);
  c->last_da = __builtin_popcountll(mask);
  if (mask == db.amask) return GPRX_OK;
  set_active(db, mask);
  for (int i = 0; i < 4; ++i) {
    if (b->gvalid[i]) (void)hipGraphExecDestroy(b->gexec[i]);
    b->gvalid[i] = false;
  }
  gprx::launch_center(db, c->stream);
  HIPCHK(c, hipGetLastError());
  return GPRX_OK;
}

// Per-call settings of an evaluation: the context's distance mode, whether a predictive variance
// is wanted, and the launch geometry from the context options and the batch size.
void set_geometry(const gprx_ctx* c, DevBatch& db, bool want_var) {
  db.dist_mode = c->dist_mode;
  db.want_var = want_var;
  db.small_n = c->small_n > 0 ? c->small_n : (db.B >= 32 ? 4 : 64);  // small batches: more, smaller units
}

// ---- one-call workspaces: a block carved into 16-byte aligned pieces, and its owner --------------
// take<T>(n) reserves n Ts and returns their byte offset; size is the block's size so far.  at<T>
// is the piece's address once the block exists.
struct Layout {
  size_t size = 0;
  template <class T>
  size_t take(size_t n) {
    const size_t o = size;
    size = (o + n * sizeof(T) + 15) / 16 * 16;
    return o;
  }
};
template <class T>
T* at(char* base, size_t offset) {
  return (T*)(base + offset);
}
struct DevFree {
  void operator()(char* p) const { (void)hipFree(p); }
};
struct PinFree {
  void operator()(char* p) const { (void)hipHostFree(p); }
};
using DevBlock = std::unique_ptr<char, DevFree>;
using PinBlock = std::unique_ptr<char, PinFree>;
DevBlock dev_block(size_t bytes) {  // null on failure
  char* p = nullptr;
  if (hipMalloc((void**)&p, bytes) != hipSuccess) (void)hipGetLastError(), p = nullptr;
  return DevBlock(p);
}
PinBlock pin_block(size_t bytes) {
  char* p = nullptr;
  if (hipHostMalloc((void**)&p, bytes) != hipSuccess) (void)hipGetLastError(), p = nullptr;
  return PinBlock(p);
}

}  // namespace

extern "C" {

int gprx_abi_version(void) { return GPRX_ABI_VERSION; }

int gprx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

const char* gprx_status_string(int s) {
  switch (s) {
    case GPRX_OK: return "ok";
    case GPRX_NOT_POSITIVE_DEFINITE: return "not positive definite";
    case GPRX_INVALID_ARGUMENT: return "invalid argument";
    case GPRX_DEVICE_ERROR: return "device error";
    case GPRX_OUT_OF_MEMORY: return "out of memory";
    case GPRX_NOT_READY: return "not ready";
  }
  return "unknown";
}

int gprx_ctx_create(int device, gprx_ctx** out) {
  if (!out) return GPRX_INVALID_ARGUMENT;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GPRX_DEVICE_ERROR;
  if (device < 0 || device >= n) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = new gprx_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return GPRX_DEVICE_ERROR;
  }
  {  // kernel attributes of this device, once, before any context on it can launch
    static std::mutex m;
    static std::map<int, std::unique_ptr<std::once_flag>> once;
    std::once_flag* f;
    {
      std::lock_guard<std::mutex> g(m);
      auto& p = once[device];
      if (!p) p.reset(new std::once_flag());
      f = p.get();
    }
    std::call_once(*f, [] { gprx::set_kernel_attributes(); });
  }
  *out = c;
  return GPRX_OK;
}

void gprx_ctx_destroy(gprx_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  while (!c->batches.empty()) gprx_batch_destroy(*c->batches.begin());  // handles become invalid
  for (auto& p : c->pending) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  for (auto e : c->evpool) (void)hipEventDestroy(e);
  if (c->rbuf) (void)hipFree(c->rbuf);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* gprx_ctx_last_error(const gprx_ctx* c) { return c ? c->err.c_str() : "null context"; }

int gprx_ctx_set_dist_mode(gprx_ctx* c, int mode) {
  if (!c || (mode != GPRX_DIST_EXPANDED && mode != GPRX_DIST_DIRECT)) return GPRX_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(c->mu);
  c->dist_mode = mode;
  return GPRX_OK;
}

int gprx_ctx_device(const gprx_ctx* c) { return c ? c->device : -1; }

int gprx_ctx_set_option(gprx_ctx* c, int option, int value) {
  if (!c) return GPRX_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(c->mu);
  switch (option) {
    case GPRX_OPT_LEAF_TILES:
      if (value < 0 || value > 8) return set_err(c, GPRX_INVALID_ARGUMENT, "leaf tiles: 0 (auto) .. 8");
      c->leaf_tiles = value;
      return GPRX_OK;
    case GPRX_OPT_SMALL_N:
      if (value < 0) return set_err(c, GPRX_INVALID_ARGUMENT, "small_n: >= 0 (0 = auto)");
      c->small_n = value;
      return GPRX_OK;
    case GPRX_OPT_GRAPHS:
      c->use_graphs = value != 0;
      return GPRX_OK;
    case GPRX_OPT_ACTIVE_DIMS:
      c->active_dims = value != 0;
      return GPRX_OK;
  }
  return set_err(c, GPRX_INVALID_ARGUMENT, "unknown option");
}

int gprx_ctx_set_profiling(gprx_ctx* c, int enable) {
  if (!c) return GPRX_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(c->mu);
  c->prof = enable != 0;
  return GPRX_OK;
}

int gprx_ctx_kernel_stats(gprx_ctx* c, const char* kernel, double* total_ms, int64_t* launches, double* algo_flops,
                          double* algo_bytes) {
  if (!c || !kernel) return GPRX_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->stats.find(kernel);
  KStat s = it == c->stats.end() ? KStat() : it->second;
  if (!strcmp(kernel, "active_dims")) s.n = c->last_da;  // no kernel: the active dimension count, as launches
  if (total_ms) *total_ms = s.ms;
  if (launches) *launches = s.n;
  if (algo_flops) *algo_flops = s.flops;
  if (algo_bytes) *algo_bytes = s.bytes;
  return GPRX_OK;
}

int gprx_ctx_reset_stats(gprx_ctx* c) {
  if (!c) return GPRX_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(c->mu);
  c->stats.clear();
  return GPRX_OK;
}

static void batch_free(gprx_batch* b);

int gprx_batch_create(gprx_ctx* c, int B, int d, int N, int M_max, gprx_batch** out) {
  if (!c || !out) return GPRX_INVALID_ARGUMENT;
  *out = nullptr;
  if (B < 1 || d < 1 || d > gprx::DMAX || N < 1 || M_max < 0)
    return set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_create: need B>=1, 1<=d<=64, N>=1, M_max>=0");
  if (!sizes_addressable(N, M_max))
    return set_err(c, GPRX_INVALID_ARGUMENT,
                   "gprx_batch_create: Npad * max(Npad, Mpad) * 8 must stay below the 2 GiB buffer range (N <= 16320)");
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  gprx_batch* b = new gprx_batch();
  b->ctx = c;
  c->batches.insert(b);
  DevBatch& db = b->db;
  set_train_dims(db, B, d, N);
  int rc = GPRX_OK;
  auto fail = [&](int r) {  // under c->mu: unlink here, free without re-locking
    c->batches.erase(b);
    batch_free(b);
    return r;
  };
  if (db.nlj < 1) return fail(set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_create: lauum plan failed"));
  if ((rc = bufs_alloc(c, train_bufs(*b)))) return fail(rc);
  db.info = db.status + B;
  {
    std::vector<int> ord(2 * gprx::LU * (size_t)db.nlj);
    int nu, ni;
    gprx::lauum_plan(db.nt, d, &nu, &ni, ord.data());
    if (hipMemcpy(db.lauum_order, ord.data(), ord.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
      return fail(GPRX_DEVICE_ERROR);
  }
  if ((rc = alloc_test(b, M_max))) return fail(rc);
  *out = b;
  return GPRX_OK;
}

// Frees a batch that is no longer in its context's set (the caller holds no lock, or the creating
// call's own lock: gprx_batch_create's failure path).
static void batch_free(gprx_batch* b) {
  if (b->ctx) (void)hipSetDevice(b->ctx->device);
  if (b->ctx) (void)hipStreamSynchronize(b->ctx->stream);
  for (int i = 0; i < 4; ++i)
    if (b->gvalid[i]) (void)hipGraphExecDestroy(b->gexec[i]);
  bufs_free(train_bufs(*b));
  drop_test(b);
  if (b->cv_tab) (void)hipFree(b->cv_tab);
  delete b;
}

void gprx_batch_destroy(gprx_batch* b) {
  if (!b) return;
  if (b->ctx) {
    std::lock_guard<std::mutex> g(b->ctx->mu);
    b->ctx->batches.erase(b);
  }
  batch_free(b);
}

int gprx_batch_dims(const gprx_batch* b, int* B, int* d, int* N, int* M_max) {
  if (!b) return GPRX_INVALID_ARGUMENT;
  if (B) *B = b->db.B;
  if (d) *d = b->db.d;
  if (N) *N = b->db.N;
  if (M_max) *M_max = b->db.Mpad;
  return GPRX_OK;
}

int gprx_batch_bytes(int B, int d, int N, int M_max, uint64_t* bytes) {
  if (bytes) *bytes = 0;
  if (!bytes || B < 1 || d < 1 || d > gprx::DMAX || N < 1 || M_max < 0) return GPRX_INVALID_ARGUMENT;
  if (!sizes_addressable(N, M_max)) return GPRX_INVALID_ARGUMENT;
  gprx_batch b;  // dimensions only: what gprx_batch_create would allocate for them
  set_train_dims(b.db, B, d, N);
  set_test_dims(b.db, M_max);
  *bytes = bufs_device_bytes(train_bufs(b)) + bufs_device_bytes(test_bufs(b));
  return GPRX_OK;
}

int gprx_ctx_mem_info(gprx_ctx* c, uint64_t* free_bytes, uint64_t* total_bytes) {
  if (!c) return GPRX_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  size_t f = 0, t = 0;
  HIPCHK(c, hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return GPRX_OK;
}

int gprx_batch_set_train(gprx_batch* b, const double* X, int64_t xs, const double* Y, int64_t ys, int mem) {
  if (!b || !X || !Y || xs < 0 || ys < 0) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  DevBatch& db = b->db;
  int rc;
  for (int s = 0; s < db.B; ++s) {
    // X slot: d x N contiguous (column t = CState t) -> d x Npad (tail zero)
    if ((rc = copy_in(c, db.X + (size_t)s * db.Npad * db.d, X + (size_t)s * xs, (size_t)db.N * db.d * sizeof(double), mem)))
      return rc;
    if ((rc = copy_in(c, db.Y + (size_t)s * db.Npad, Y + (size_t)s * ys, (size_t)db.N * sizeof(double), mem))) return rc;
  }
  // which dimensions are one constant in every slot: flags by slot and dimension, through grad_part
  // (scratch of an evaluation) and the pinned h_out, read back under the synchronisation the copies
  // need anyway
  const int B = db.B, d = db.d;
  int* h_flags = (int*)b->h_out;  // B x d ints <= B x (d + 3) doubles
  if (c->active_dims) {
    gprx::launch_const_flags(db, (int*)db.grad_part, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_flags, db.grad_part, (size_t)B * d * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  b->found_mask = 0;
  for (int p = 0; p < d; ++p) {
    bool varies = !c->active_dims;
    for (int s = 0; s < B && !varies; ++s) varies = h_flags[(size_t)s * d + p] != 0;
    if (varies) b->found_mask |= 1ull << p;
  }
  if (!b->found_mask) b->found_mask = 1;  // all constant: keep dimension 0
  db.amask = 0;  // X changed: Xc is rewritten whatever the set
  if ((rc = sync_active(b))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  b->have_train = true;
  b->factored = false;
  return GPRX_OK;
}

int gprx_batch_set_test(gprx_batch* b, const double* Xs, int M, int64_t xss, int mem) {
  if (!b || (!Xs && M > 0) || M < 0 || xss < 0) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  DevBatch& db = b->db;
  if (M > db.Mpad || !db.Xs) {  // grow the capacity (or allocate afresh after a failed regrow)
    if (!sizes_addressable(db.N, M))
      return set_err(c, GPRX_INVALID_ARGUMENT, "test points: Npad * max(Npad, Mpad) * 8 exceeds the 2 GiB buffer range");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bufs_free(test_bufs(*b));
    int rc = alloc_test(b, M);
    if (rc) return rc;  // no test buffers, no test points, no covariance workspace (drop_test)
  }
  HIPCHK(c, hipMemsetAsync(db.Xs, 0, (size_t)db.B * db.Mpad * db.d * sizeof(double), c->stream));
  int rc;
  for (int s = 0; s < db.B && M > 0; ++s)
    if ((rc = copy_in(c, db.Xs + (size_t)s * db.Mpad * db.d, Xs + (size_t)s * xss, (size_t)M * db.d * sizeof(double), mem)))
      return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db.M = M;
  b->have_test = M > 0;
  return GPRX_OK;
}

// Page-locked host memory (hipHostMalloc / registered, e.g. torch's pinned tensors): the device
// writes it by DMA, so the predictive outputs can go straight into the caller's buffer (one
// pitched copy) instead of through the batch's staging buffer and a host copy per slot.
static bool pinned_host(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: not known to the runtime
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
// queue the copy of a [B][Mpad] device output to the caller's [B][M] buffer when it is pinned;
// returns whether it did (else the caller stages it)
static bool out_direct(gprx_ctx* c, double* dst, const double* src, const DevBatch& db) {
  if (!pinned_host(dst)) return false;
  return hipMemcpy2DAsync(dst, (size_t)db.M * sizeof(double), src, (size_t)db.Mpad * sizeof(double), (size_t)db.M * sizeof(double),
                          db.B, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
}

// The predictive outputs of a batch on their way to the caller (NULL: not wanted).  pred_out_queue
// queues the copies on the context stream, straight into a pinned caller buffer or else into the
// batch's staging buffers, and reports which went direct; pred_out_unpack, after the stream has been
// synchronised, copies the staged ones out slot by slot.
struct PredDirect {
  bool mu = false, var = false;
};
static int pred_out_queue(gprx_batch* b, double* mu, double* var, PredDirect* pd) {
  gprx_ctx* c = b->ctx;
  const DevBatch& db = b->db;
  const size_t bytes = (size_t)db.B * db.Mpad * sizeof(double);
  pd->mu = mu && out_direct(c, mu, db.out_mu, db);
  pd->var = var && out_direct(c, var, db.out_var, db);
  if (mu && !pd->mu) HIPCHK(c, hipMemcpyAsync(b->h_mu, db.out_mu, bytes, hipMemcpyDeviceToHost, c->stream));
  if (var && !pd->var) HIPCHK(c, hipMemcpyAsync(b->h_var, db.out_var, bytes, hipMemcpyDeviceToHost, c->stream));
  return GPRX_OK;
}
static void pred_out_unpack(const gprx_batch* b, double* mu, double* var, PredDirect pd) {
  const DevBatch& db = b->db;
  for (int s = 0; s < db.B; ++s) {
    if (mu && !pd.mu) memcpy(mu + (size_t)s * db.M, b->h_mu + (size_t)s * db.Mpad, db.M * sizeof(double));
    if (var && !pd.var) memcpy(var + (size_t)s * db.M, b->h_var + (size_t)s * db.Mpad, db.M * sizeof(double));
  }
}

static int batch_predict_locked(gprx_batch* b, double* mu, double* var) {
  gprx_ctx* c = b->ctx;
  DevBatch& db = b->db;
  if (!b->factored) return set_err(c, GPRX_NOT_READY, "predict before a successful factorisation");
  if (!b->have_test || db.M == 0) return GPRX_OK;
  db.want_var = var != nullptr;
  int rc = run_eval(b, false, true, false);
  if (rc) return rc;
  PredDirect pd;
  if ((rc = pred_out_queue(b, mu, var, &pd))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  pred_out_unpack(b, mu, var, pd);
  return GPRX_OK;
}

int gprx_batch_run(gprx_batch* b, const double* theta, unsigned flags, double* mll, double* grad, double* mu,
                   double* var, int* status, int* info) {
  if (!b || !theta) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (!b->have_train) return set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_run before gprx_batch_set_train");
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  DevBatch& db = b->db;
  {
    int rc = sync_active(b);
    if (rc) return rc;
  }
  set_geometry(c, db, var != nullptr);
  const int d = db.d, B = db.B, np = d + 2;
  // hyper-parameters -> kernel parameters on the device (derive_params: SEArd / GPE's
  // il2 = exp(-2 log ell), sf2 = exp(2 log sf), noise = exp(2 logNoise) + eps()); h_params is the
  // pinned staging buffer (pst >= d + 2 doubles per slot)
  memcpy(b->h_params, theta, (size_t)B * np * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(db.theta, b->h_params, (size_t)B * np * sizeof(double), hipMemcpyHostToDevice, c->stream));
  gprx::launch_params(db, c->stream);
  HIPCHK(c, hipGetLastError());
  const bool want_grad = (flags & GPRX_WANT_GRAD) != 0;
  const bool want_pred = (flags & GPRX_WANT_PREDICT) != 0 && b->have_test && db.M > 0;
  {
    int rc = run_eval(b, want_grad, want_pred, true);
    if (rc) return rc;
  }
  HIPCHK(c, hipMemcpyAsync(b->h_out, db.out, (size_t)B * (d + 3) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(b->h_status, db.status, 2 * (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  PredDirect pd;
  if (want_pred) {
    int rc = pred_out_queue(b, mu, var, &pd);
    if (rc) return rc;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  for (int s = 0; s < B; ++s) {
    if (status) status[s] = b->h_status[s];
    if (info) info[s] = b->h_status[B + s];
    const double* o = b->h_out + (size_t)s * (d + 3);
    if (mll) mll[s] = o[0];
    if (grad && want_grad) memcpy(grad + (size_t)s * np, o + 1, np * sizeof(double));
  }
  if (want_pred) pred_out_unpack(b, mu, var, pd);
  b->factored = true;
  return first_status(c, "gprx_batch_run", b->h_status, B);
}

int gprx_batch_alpha(gprx_batch* b, double* alpha) {
  if (!b || !alpha) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (!b->factored) return set_err(c, GPRX_NOT_READY, "alpha before a successful factorisation");
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  const DevBatch& db = b->db;
  HIPCHK(c, hipMemcpy2DAsync(alpha, (size_t)db.N * sizeof(double), db.alpha, (size_t)db.Npad * sizeof(double),
                             (size_t)db.N * sizeof(double), db.B, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // h_status holds the per-slot status of the evaluation that factorised the batch (gprx_batch_run
  // or the optimiser's refit): a slot that failed there has no alpha
  for (int s = 0; s < db.B; ++s)
    if (b->h_status[s] != GPRX_OK)
      for (int t = 0; t < db.N; ++t) alpha[(size_t)s * db.N + t] = NAN;
  return GPRX_OK;
}

int gprx_batch_predict(gprx_batch* b, double* mu, double* var) {
  if (!b) return GPRX_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> g(b->ctx->mu);
  if (hipSetDevice(b->ctx->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  return batch_predict_locked(b, mu, var);
}

// ---- joint predictive covariance and posterior samples (gprx_predcov.h) -------------------------
// The workspace for the batch's current Mpad; a failure frees what it got and leaves the batch
// without one.
static int cov_alloc(gprx_batch* b) {
  gprx_ctx* c = b->ctx;
  if (b->cov_mpad == b->db.Mpad) return GPRX_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  cov_free(b);
  const int rc = bufs_alloc(c, cov_bufs(*b));
  if (rc) return rc;
  b->cov_mpad = b->db.Mpad;
  return GPRX_OK;
}

// mu (copied to the caller when non-NULL) and Sigma on the device, from the last factorisation:
// the prediction's own cross-covariance and mean launches, then pred_whiten and pred_cov
static int cov_compute(gprx_batch* b, double* mu) {
  gprx_ctx* c = b->ctx;
  DevBatch& db = b->db;
  if (!b->factored) return set_err(c, GPRX_NOT_READY, "joint covariance before a successful factorisation");
  if (!b->have_test || db.M == 0) return set_err(c, GPRX_NOT_READY, "joint covariance without test points (gprx_batch_set_test)");
  if (!cov_addressable(db.Mpad))
    return set_err(c, GPRX_INVALID_ARGUMENT, "joint covariance: Mpad^2 * 8 exceeds the 2 GiB buffer range");
  int rc = cov_alloc(b);
  if (rc) return rc;
  if ((rc = batch_predict_locked(b, mu, nullptr))) return rc;
  const double N = db.N, M = db.M, B = db.B;
  timed(c, c->stream, "pred_whiten", B * N * N * M, B * 8.0 * (N * N / 2 + 2.0 * N * db.Mpad),
        [&] { gprx::launch_pred_whiten(db, b->cov_vt, c->stream); });
  timed(c, c->stream, "pred_cov", B * N * M * M, B * 8.0 * (N * db.Mpad + M * M + 2.0 * M * db.d),
        [&] { gprx::launch_pred_cov(db, b->cov_vt, b->cov_sig, c->stream); });
  HIPCHK(c, hipGetLastError());
  return GPRX_OK;
}
static void nan_fill(double* p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = NAN;
}

int gprx_batch_cov_bytes(int B, int N, int M_max, uint64_t* bytes) {
  if (bytes) *bytes = 0;
  if (!bytes || B < 1 || N < 1 || M_max < 0) return GPRX_INVALID_ARGUMENT;
  if (!sizes_addressable(N, M_max) || !cov_addressable(M_max)) return GPRX_INVALID_ARGUMENT;
  gprx_batch b;  // dimensions only: what cov_alloc would allocate for them
  set_train_dims(b.db, B, 1, N);  // d does not enter the workspace's sizes
  set_test_dims(b.db, M_max);
  *bytes = bufs_device_bytes(cov_bufs(b));
  return GPRX_OK;
}

int gprx_batch_predict_cov(gprx_batch* b, double* mu, double* cov) {
  if (!b || !cov) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  int rc = cov_compute(b, mu);
  if (rc) return rc;
  const DevBatch& db = b->db;
  const size_t M = db.M;
  // Sigma is compact on the device ([M][M] per slot, slots M M apart): one copy
  HIPCHK(c, hipMemcpyAsync(cov, b->cov_sig, (size_t)db.B * M * M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  for (int s = 0; s < db.B; ++s)  // h_status: the evaluation that factorised the batch (gprx_batch_alpha)
    if (b->h_status[s] != GPRX_OK) {
      nan_fill(cov + (size_t)s * M * M, M * M);
      if (mu) nan_fill(mu + (size_t)s * M, M);
    }
  return GPRX_OK;
}

int gprx_batch_sample(gprx_batch* b, const double* Z, int S, int64_t zss, double* samples, double* jitter, int* status) {
  if (!b || !Z || !samples || S < 1 || zss < 0) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  const DevBatch& db = b->db;
  if (b->factored && b->have_test && db.M > 1024)
    return set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_sample: M > 1024 test points");
  int rc = cov_compute(b, nullptr);
  if (rc) return rc;
  const size_t M = db.M, B = db.B, mm = (size_t)db.Mpad * db.Mpad;
  timed(c, c->stream, "cov_chol", (double)B * M * M * M / 3.0, (double)B * 8.0 * 2.0 * M * M,
        [&] { gprx::launch_cov_chol(db, b->cov_sig, b->cov_f, mm, b->cov_jit, b->cov_st, c->stream); });
  HIPCHK(c, hipGetLastError());
  // Z and the samples pass through device buffers of Mpad vectors per slot: S beyond that in passes
  for (int s0 = 0; s0 < S; s0 += db.Mpad) {
    const size_t sc = std::min<size_t>(db.Mpad, S - s0), w = sc * M * sizeof(double);
    if (zss == 0)
      HIPCHK(c, hipMemcpyAsync(b->cov_z, Z + (size_t)s0 * M, w, hipMemcpyHostToDevice, c->stream));
    else
      HIPCHK(c, hipMemcpy2DAsync(b->cov_z, mm * sizeof(double), Z + (size_t)s0 * M, (size_t)zss * sizeof(double), w, B,
                                 hipMemcpyHostToDevice, c->stream));
    timed(c, c->stream, "cov_sample", (double)B * sc * M * M, (double)B * 8.0 * (M * M / 2.0 + 2.0 * sc * M), [&] {
      gprx::launch_cov_sample(db, b->cov_f, mm, b->cov_z, zss == 0 ? 0 : mm, b->cov_smp, mm, (int)sc, b->cov_st, c->stream);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy2DAsync(samples + (size_t)s0 * M, (size_t)S * M * sizeof(double), b->cov_smp, mm * sizeof(double), w, B,
                               hipMemcpyDeviceToHost, c->stream));
  }
  double* hj = b->h_cov;
  int* hs = (int*)(b->h_cov + B);
  HIPCHK(c, hipMemcpyAsync(hj, b->cov_jit, B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hs, b->cov_st, B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  for (size_t s = 0; s < B; ++s) {
    // a slot whose evaluation failed: NaN rows (the kernels wrote them), not a failure of this call
    const bool dead = b->h_status[s] != GPRX_OK;
    if (dead) nan_fill(samples + s * S * M, (size_t)S * M);
    if (jitter) jitter[s] = dead ? NAN : hj[s];
    if (status) status[s] = dead ? b->h_status[s] : hs[s];
    if (dead) hs[s] = GPRX_OK;
  }
  return first_status(c, "gprx_batch_sample", hs, (int)B);
}

// ---- device hyper-parameter optimisation (gprx_lbfgs.hip) ---------------------------------------
static_assert(GPRX_STOP_ITERATIONS == gprx::LB_STOP_ITERATIONS && GPRX_STOP_G_TOL == gprx::LB_STOP_G_TOL &&
                  GPRX_STOP_X_TOL == gprx::LB_STOP_X_TOL && GPRX_STOP_F_TOL == gprx::LB_STOP_F_TOL &&
                  GPRX_STOP_LINESEARCH == gprx::LB_STOP_LINESEARCH && GPRX_STOP_MAX_EVALS == gprx::LB_STOP_MAX_EVALS &&
                  GPRX_STOP_TIME_LIMIT == gprx::LB_STOP_TIME_LIMIT &&
                  GPRX_STOP_NAN_GRADIENT == gprx::LB_STOP_NAN_GRADIENT,
              "stop codes");

void gprx_opt_defaults(gprx_opt_options* o) {
  if (!o) return;
  o->m = 10;
  o->iterations = 1000;
  o->max_evals = -1;
  o->ls_iterations = 1000;
  o->scaleinvH0 = 1;
  o->refit = 1;
  o->successive_f_tol = 1;
  o->g_abstol = 1e-8;
  o->time_limit = NAN;  // Optim: no limit
  o->alphaguess = 1.0;
  o->c_1 = 1e-4;
  o->rho_hi = 0.5;
  o->rho_lo = 0.1;
}

// The leave-one-out launches (defined with gprx_batch_loo_grad below), which the optimiser's rounds
// share with it: the workspace's pieces in the context scratch and the six launches.
static int ctx_scratch(gprx_ctx* c, size_t need, char** base);
struct LooWs {
  double *kinv, *mu, *var, *lp, *beta, *bp, *gp, *out, *logp;
};
static size_t loo_ws_bytes(const DevBatch& db);
static LooWs loo_ws_at(char* base, const DevBatch& db);
static void loo_grad_launches(gprx_ctx* c, const DevBatch& db, const LooWs& w);

// gprx_batch_optimize and gprx_batch_optimize_obj.  objective GPRX_OBJ_LOO: a round is the evaluation
// without the marginal-likelihood gradient (gram .. finalize) followed by the six leave-one-out
// launches, all under the round's mask, and k_lbfgs reads the slot's answer from the leave-one-out
// result rows ([logp, grad(d+2)], db.out's layout) through a DevBatch copy whose out points at them.
static int batch_optimize(gprx_batch* b, int objective, const double* theta0, const gprx_opt_options* opt, double* theta_out,
                          double* minimum, int* iterations, int* f_calls, int* g_calls, int* stopped, int* rounds) {
  if (!b || !theta0 || (objective != GPRX_OBJ_MLL && objective != GPRX_OBJ_LOO)) return GPRX_INVALID_ARGUMENT;
  const bool loo = objective == GPRX_OBJ_LOO;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (!b->have_train) return set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_optimize before gprx_batch_set_train");
  gprx_opt_options o;
  gprx_opt_defaults(&o);
  if (opt) o = *opt;
  if (o.m < 1 || o.m > 64 || o.iterations < 0 || o.ls_iterations < 0 || o.successive_f_tol < 0 || !(o.c_1 > 0.0) || !(o.rho_lo > 0.0) ||
      !(o.rho_hi > 0.0) || !std::isfinite(o.alphaguess) || std::isnan(o.g_abstol))
    return set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_optimize: bad options");
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  DevBatch& db = b->db;
  {
    int rc = sync_active(b);
    if (rc) return rc;
  }
  set_geometry(c, db, false);
  const int B = db.B, n = db.d + 2;
  gprx::LbArgs a{};
  a.n = n;
  a.m = o.m;
  a.max_evals = o.max_evals;
  a.iterations = o.iterations;
  a.ls_iterations = o.ls_iterations;
  a.scaleinvH0 = o.scaleinvH0 ? 1 : 0;
  a.successive_f_tol = o.successive_f_tol;
  a.g_abstol = o.g_abstol;
  a.alphaguess = o.alphaguess;
  a.c_1 = o.c_1;
  a.rho_hi = o.rho_hi;
  a.rho_lo = o.rho_lo;
  // one device block: state, start points, flags, results; one pinned host mirror of the flags
  // and results
  const size_t rd = (size_t)B * (n + 1);
  Layout dl, hl;
  const size_t o_ws = dl.take<double>((size_t)B * gprx::lb_ws_doubles(n, o.m)), o_th0 = dl.take<double>((size_t)B * n),
               o_res = dl.take<double>(rd), o_iws = dl.take<int>((size_t)B * gprx::LB_NI), o_ri = dl.take<int>((size_t)B * 4);
  const size_t oh_res = hl.take<double>(rd), oh_act = hl.take<int>(B), oh_ri = hl.take<int>((size_t)B * 4);
  DevBlock dbuf = dev_block(dl.size);
  if (!dbuf) return set_err(c, GPRX_OUT_OF_MEMORY, "gprx_batch_optimize: workspace");
  PinBlock hbuf = pin_block(hl.size);
  if (!hbuf) return set_err(c, GPRX_OUT_OF_MEMORY, "gprx_batch_optimize: host buffer");
  a.ws = at<double>(dbuf.get(), o_ws);
  double* th0d = at<double>(dbuf.get(), o_th0);
  a.theta0 = th0d;
  a.result = at<double>(dbuf.get(), o_res);
  a.iws = at<int>(dbuf.get(), o_iws);
  // the optimisers' activity flags double as the evaluation mask of the rounds (finished slots are
  // skipped by every kernel); a per-batch buffer, so the captured round graph is reused across calls
  a.active = b->opt_active;
  a.result_i = at<int>(dbuf.get(), o_ri);
  double* h_res = at<double>(hbuf.get(), oh_res);
  int* h_act = at<int>(hbuf.get(), oh_act);
  int* h_ri = at<int>(hbuf.get(), oh_ri);
  // theta, L and the factorisation flags are overwritten from here on: the batch holds no valid
  // factorisation until the refit below has succeeded for every slot
  b->factored = false;
  struct Unmask {  // every exit path evaluates all slots again
    DevBatch& db;
    ~Unmask() { db.active = nullptr; }
  } um{db};
  // evaluation trace (gprx_batch_set_opt_trace): per round the evaluated theta and the answer of
  // every slot, staged in pinned memory (copied under the round's own synchronisation)
  const int trr = b->opt_trace ? b->opt_trace_rounds : 0;
  const size_t trs = (size_t)B * (2 * n + 1);  // staged doubles per round: theta(n), out(n + 1)
  std::vector<int> tr_act((size_t)trr * B, 0);
  PinBlock trbuf = trr > 0 ? pin_block((size_t)trr * trs * sizeof(double)) : PinBlock();
  if (trr > 0 && !trbuf) return set_err(c, GPRX_OUT_OF_MEMORY, "gprx_batch_optimize: trace buffer");
  double* h_tr = (double*)trbuf.get();
  // the leave-one-out workspace, sized once: ctx_scratch may free and reallocate, so no round calls it
  LooWs lw{};
  if (loo) {
    char* base = nullptr;
    int rc = ctx_scratch(c, loo_ws_bytes(db), &base);
    if (rc) return rc;
    lw = loo_ws_at(base, db);
  }
  HIPCHK(c, hipMemcpyAsync(th0d, theta0, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  gprx::launch_lbfgs(a, db, 1, c->stream);
  db.active = a.active;
  DevBatch dba = db;  // what k_lbfgs reads its answers from: the evaluation's rows, or the leave-one-out rows
  if (loo) dba.out = lw.out;
  const auto t0 = std::chrono::steady_clock::now();
  int nr = 0;
  for (;;) {
    HIPCHK(c, hipMemcpyAsync(h_act, a.active, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int act = 0;
    for (int s = 0; s < B; ++s) act += h_act[s] != 0;
    if (!act) break;
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    a.time_up = (o.time_limit >= 0.0 && el > o.time_limit) ? 1 : 0;  // false for NaN
    int rc = run_eval(b, !loo, false, true);
    if (rc) return rc;
    if (loo) loo_grad_launches(c, db, lw);
    collect(c);
    if (nr < trr) {
      double* h = h_tr + (size_t)nr * trs;
      memcpy(&tr_act[(size_t)nr * B], h_act, (size_t)B * sizeof(int));
      HIPCHK(c, hipMemcpyAsync(h, db.theta, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(h + (size_t)B * n, dba.out, (size_t)B * (n + 1) * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
    }
    gprx::launch_lbfgs(a, dba, 0, c->stream);
    HIPCHK(c, hipGetLastError());
    ++nr;
  }
  HIPCHK(c, hipMemcpyAsync(h_res, a.result, rd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h_ri, a.result_i, (size_t)B * 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  db.active = nullptr;
  if (o.refit) {  // optimize!: set_params!(gp, minimizer); update_target!(gp)
    gprx::launch_lbfgs_final(a, db, c->stream);
    int rc = run_eval(b, true, false, true);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(b->h_out, db.out, (size_t)B * (db.d + 3) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(b->h_status, db.status, 2 * (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  if (trr > 0) {  // [active, theta(n), mll, dmll(n)] per slot and round (logp, dlogp for GPRX_OBJ_LOO); NaN beyond the last round
    const size_t w = 2 * (size_t)n + 2;
    for (int r = 0; r < trr; ++r)
      for (int s = 0; s < B; ++s) {
        double* t = b->opt_trace + ((size_t)r * B + s) * w;
        if (r >= nr) {
          for (size_t q = 0; q < w; ++q) t[q] = NAN;
          continue;
        }
        const double* h = h_tr + (size_t)r * trs;
        t[0] = tr_act[(size_t)r * B + s] ? 1.0 : 0.0;
        memcpy(t + 1, h + (size_t)s * n, n * sizeof(double));
        memcpy(t + 1 + n, h + (size_t)B * n + (size_t)s * (n + 1), (n + 1) * sizeof(double));
      }
  }
  for (int s = 0; s < B; ++s) {
    const double* r = h_res + (size_t)s * (n + 1);
    if (theta_out) memcpy(theta_out + (size_t)s * n, r, n * sizeof(double));
    if (minimum) minimum[s] = r[n];
    const int* ri = h_ri + (size_t)s * 4;
    if (iterations) iterations[s] = ri[0];
    if (f_calls) f_calls[s] = ri[1];
    if (g_calls) g_calls[s] = ri[2];
    if (stopped) stopped[s] = ri[3];
  }
  if (rounds) *rounds = nr;
  if (!o.refit) return GPRX_OK;
  // the refit's per-slot status, as gprx_batch_run reports it: a minimiser that is not finite
  // (status 2) or not positive definite (status 1) is an error of update_target!, and the batch is
  // then not left factorised
  int first = GPRX_OK, bad = -1;
  for (int s = 0; s < B && first == GPRX_OK; ++s)
    if (b->h_status[s] != GPRX_OK) first = b->h_status[s], bad = s;
  if (first != GPRX_OK)
    return set_err(c, first, "gprx_batch_optimize: refit at the minimiser of slot " + std::to_string(bad) + ": " +
                                 gprx_status_string(first));
  b->factored = true;
  return GPRX_OK;
}

int gprx_batch_optimize(gprx_batch* b, const double* theta0, const gprx_opt_options* opt, double* theta_out,
                        double* minimum, int* iterations, int* f_calls, int* g_calls, int* stopped, int* rounds) {
  return batch_optimize(b, GPRX_OBJ_MLL, theta0, opt, theta_out, minimum, iterations, f_calls, g_calls, stopped, rounds);
}

int gprx_batch_optimize_obj(gprx_batch* b, int objective, const double* theta0, const gprx_opt_options* opt,
                            double* theta_out, double* minimum, int* iterations, int* f_calls, int* g_calls, int* stopped,
                            int* rounds) {
  return batch_optimize(b, objective, theta0, opt, theta_out, minimum, iterations, f_calls, g_calls, stopped, rounds);
}

int gprx_batch_set_opt_trace(gprx_batch* b, double* trace, int max_rounds, int64_t capacity) {
  if (!b || max_rounds < 0 || (max_rounds > 0 && !trace)) return GPRX_INVALID_ARGUMENT;
  const int64_t need = (int64_t)max_rounds * b->db.B * (2 * (int64_t)(b->db.d + 2) + 2);
  if (max_rounds > 0 && capacity < need)
    return set_err(b->ctx, GPRX_INVALID_ARGUMENT,
                   "gprx_batch_set_opt_trace: capacity " + std::to_string(capacity) + " < max_rounds * B * (2(d+2)+2) = " +
                       std::to_string(need) + " doubles");
  std::lock_guard<std::mutex> g(b->ctx->mu);
  b->opt_trace = max_rounds > 0 ? trace : nullptr;
  b->opt_trace_rounds = max_rounds;
  return GPRX_OK;
}

// ---- single GP ---------------------------------------------------------------------------------
int gprx_gp_create(gprx_ctx* c, const double* X, int d, int N, const double* y, gprx_gp** out) {
  if (!c || !X || !y || !out) return GPRX_INVALID_ARGUMENT;
  *out = nullptr;
  gprx_batch* b = nullptr;
  int rc = gprx_batch_create(c, 1, d, N, 0, &b);
  if (rc) return rc;
  rc = gprx_batch_set_train(b, X, 0, y, 0, GPRX_MEM_HOST);
  if (rc) {
    gprx_batch_destroy(b);
    return rc;
  }
  gprx_gp* gp = new gprx_gp();
  gp->batch = b;
  *out = gp;
  return GPRX_OK;
}

void gprx_gp_destroy(gprx_gp* gp) {
  if (!gp) return;
  gprx_batch_destroy(gp->batch);
  delete gp;
}

int gprx_gp_lml(gprx_gp* gp, const double* theta, double* mll) {
  if (!gp) return GPRX_INVALID_ARGUMENT;
  return gprx_batch_run(gp->batch, theta, 0u, mll, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int gprx_gp_lml_grad(gprx_gp* gp, const double* theta, double* mll, double* grad) {
  if (!gp) return GPRX_INVALID_ARGUMENT;
  return gprx_batch_run(gp->batch, theta, GPRX_WANT_GRAD, mll, grad, nullptr, nullptr, nullptr, nullptr);
}

int gprx_gp_predict(gprx_gp* gp, const double* Xs, int M, double* mu, double* var) {
  if (!gp || M < 0) return GPRX_INVALID_ARGUMENT;
  if (M == 0) return GPRX_OK;
  int rc = gprx_batch_set_test(gp->batch, Xs, M, 0, GPRX_MEM_HOST);
  if (rc) return rc;
  return gprx_batch_predict(gp->batch, mu, var);
}

int gprx_gp_predict_cov(gprx_gp* gp, const double* Xs, int M, double* mu, double* cov) {
  if (!gp || !Xs || M < 1 || !cov) return GPRX_INVALID_ARGUMENT;
  int rc = gprx_batch_set_test(gp->batch, Xs, M, 0, GPRX_MEM_HOST);
  if (rc) return rc;
  return gprx_batch_predict_cov(gp->batch, mu, cov);
}

int gprx_gp_sample(gprx_gp* gp, const double* Xs, int M, const double* Z, int S, double* samples, double* jitter) {
  if (!gp || !Xs || M < 1 || !Z || !samples || S < 1) return GPRX_INVALID_ARGUMENT;
  int rc = gprx_batch_set_test(gp->batch, Xs, M, 0, GPRX_MEM_HOST);
  if (rc) return rc;
  return gprx_batch_sample(gp->batch, Z, S, 0, samples, jitter, nullptr);
}

// ---- physics calls: common parts ----------------------------------------------------------------
// device scratch of a context for the physics calls: [args | in | out], grown on demand
static int ctx_scratch(gprx_ctx* c, size_t need, char** base) {
  if (need > c->rcap) {
    if (c->rbuf) HIPCHK(c, hipFree(c->rbuf));
    c->rbuf = nullptr;
    c->rcap = 0;
    HIPCHK(c, hipMalloc(&c->rbuf, need));
    c->rcap = need;
  }
  *base = (char*)c->rbuf;
  return GPRX_OK;
}

// ---- leave-one-out predictions (gprx_loo.h) ------------------------------------------------------
// Workspace in the context scratch: kinv, mu, var, lp (B x Npad each), logp (B).  Not part of the
// captured evaluation graphs: two launches (loo_launches) straight on the context stream.
static void loo_launches(gprx_ctx* c, const DevBatch& db, double* kinv, double* mu, double* var, double* lp, double* logp) {
  const double B = db.B, N = db.N, tri = N * (N + 1.0) / 2.0;
  timed(c, c->stream, "loo_diag", B * 2.0 * tri, B * 8.0 * (tri + N), [&] { gprx::launch_loo_diag(db, kinv, c->stream); });
  timed(c, c->stream, "loo_final", B * 10.0 * N, B * 8.0 * 6.0 * N,
        [&] { gprx::launch_loo_final(db, kinv, mu, var, lp, logp, c->stream); });
}
int gprx_batch_loo(gprx_batch* b, double* mu, double* var, double* logp_i, double* logp, int* status) {
  if (!b) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (!b->factored) return set_err(c, GPRX_NOT_READY, "leave-one-out before a successful factorisation");
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  const DevBatch& db = b->db;
  const size_t rows = (size_t)db.B * db.Npad;
  char* base = nullptr;
  int rc = ctx_scratch(c, (4 * rows + db.B) * sizeof(double), &base);
  if (rc) return rc;
  double* kinv = (double*)base;
  double *d_mu = kinv + rows, *d_var = d_mu + rows, *d_lp = d_var + rows, *d_logp = d_lp + rows;
  loo_launches(c, db, kinv, d_mu, d_var, d_lp, d_logp);
  HIPCHK(c, hipGetLastError());
  const size_t w = (size_t)db.N * sizeof(double), p = (size_t)db.Npad * sizeof(double);
  if (mu) HIPCHK(c, hipMemcpy2DAsync(mu, w, d_mu, p, w, db.B, hipMemcpyDeviceToHost, c->stream));
  if (var) HIPCHK(c, hipMemcpy2DAsync(var, w, d_var, p, w, db.B, hipMemcpyDeviceToHost, c->stream));
  if (logp_i) HIPCHK(c, hipMemcpy2DAsync(logp_i, w, d_lp, p, w, db.B, hipMemcpyDeviceToHost, c->stream));
  if (logp) HIPCHK(c, hipMemcpyAsync(logp, d_logp, (size_t)db.B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  // h_status: the evaluation that factorised the batch (gprx_batch_alpha); k_loo_final wrote the
  // NaN rows of a failed slot from the same status on the device
  if (status) memcpy(status, b->h_status, (size_t)db.B * sizeof(int));
  return first_status(c, "gprx_batch_loo", b->h_status, db.B);
}

int gprx_gp_loo(gprx_gp* gp, double* mu, double* var, double* logp) {
  if (!gp) return GPRX_INVALID_ARGUMENT;
  return gprx_batch_loo(gp->batch, mu, var, nullptr, logp, nullptr);
}

// ---- gradient of the leave-one-out log predictive probability (gprx_loograd.h) ---------------------
// Workspace in the context scratch: gprx_batch_loo's (kinv, mu, var, lp, logp), beta (B x Npad), the
// beta partials (B x nt x Npad), the unit partials (B x ngu x gps) and the result rows (B x (d + 3)).
// P = K^-1 diag(sqrt c) goes to Lw, which only the factorisation reads and every evaluation rewrites.
// Not part of the captured evaluation graphs: six launches straight on the context stream.
static size_t loo_ws_bytes(const DevBatch& db) {
  const size_t rows = (size_t)db.B * db.Npad;
  return (5 * rows + db.B + rows * db.nt + (size_t)db.B * db.ngu * db.gps + (size_t)db.B * (db.d + 3)) * sizeof(double);
}
static LooWs loo_ws_at(char* base, const DevBatch& db) {
  const size_t rows = (size_t)db.B * db.Npad;
  const size_t n_bp = rows * db.nt, n_gp = (size_t)db.B * db.ngu * db.gps, n_out = (size_t)db.B * (db.d + 3);
  LooWs w;
  w.kinv = (double*)base;
  w.mu = w.kinv + rows, w.var = w.mu + rows, w.lp = w.var + rows, w.beta = w.lp + rows;
  w.bp = w.beta + rows, w.gp = w.bp + n_bp, w.out = w.gp + n_gp, w.logp = w.out + n_out;
  return w;
}
// the six launches on the context stream, for the slots of db's evaluation mask (all of them without
// one); the caller checks hipGetLastError
static void loo_grad_launches(gprx_ctx* c, const DevBatch& db, const LooWs& w) {
  const int d = db.d;
  const double B = db.B, Np = db.Npad;
  loo_launches(c, db, w.kinv, w.mu, w.var, w.lp, w.logp);
  timed(c, c->stream, "loo_kinv", B * (Np * Np * Np / 3.0 + 4.0 * Np * Np), B * 8.0 * (1.5 * Np * Np + 2.0 * db.nt * Np),
        [&] { gprx::launch_loo_kinv(db, w.kinv, w.bp, c->stream); });
  timed(c, c->stream, "loo_beta", B * db.nt * Np, B * 8.0 * (db.nt + 1.0) * Np, [&] { gprx::launch_loo_beta(db, w.bp, w.beta, c->stream); });
  timed(c, c->stream, "loo_grad", B * (Np * Np * Np + Np * Np * db.da + 6.0 * Np * Np),
        B * 8.0 * (1.5 * Np * Np + Np * db.da), [&] { gprx::launch_loo_grad(db, w.beta, w.gp, c->stream); });
  timed(c, c->stream, "loo_grad_final", B * (double)db.ngu * db.gps, B * 8.0 * ((double)db.ngu * db.gps + d + 3),
        [&] { gprx::launch_loo_grad_final(db, w.gp, w.logp, w.out, c->stream); });
}

int gprx_batch_loo_grad(gprx_batch* b, double* logp, double* grad, int* status) {
  if (!b) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (!b->factored) return set_err(c, GPRX_NOT_READY, "leave-one-out gradient before a successful factorisation");
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  const DevBatch& db = b->db;
  const int d = db.d;
  char* base = nullptr;
  int rc = ctx_scratch(c, loo_ws_bytes(db), &base);
  if (rc) return rc;
  const LooWs lw = loo_ws_at(base, db);
  double* d_out = lw.out;
  loo_grad_launches(c, db, lw);
  HIPCHK(c, hipGetLastError());
  const size_t ro = (size_t)(d + 3) * sizeof(double);
  if (logp) HIPCHK(c, hipMemcpy2DAsync(logp, sizeof(double), d_out, ro, sizeof(double), db.B, hipMemcpyDeviceToHost, c->stream));
  if (grad)
    HIPCHK(c, hipMemcpy2DAsync(grad, (size_t)(d + 2) * sizeof(double), d_out + 1, ro, (size_t)(d + 2) * sizeof(double), db.B,
                               hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  // h_status: the evaluation that factorised the batch; k_loo_grad_final wrote the NaN rows of a
  // failed slot from the same status on the device
  if (status) memcpy(status, b->h_status, (size_t)db.B * sizeof(int));
  return first_status(c, "gprx_batch_loo_grad", b->h_status, db.B);
}

int gprx_gp_loo_grad(gprx_gp* gp, double* logp, double* grad) {
  if (!gp) return GPRX_INVALID_ARGUMENT;
  return gprx_batch_loo_grad(gp->batch, logp, grad, nullptr);
}

// ---- k-fold cross-validation (gprx_cvfold.h) ------------------------------------------------------
// The layout table of CvArgs, built on the host for every layout (one, or one per slot) and uploaded
// once.  It belongs to the batch and is not part of gprx_batch_bytes.
int gprx_batch_set_folds(gprx_batch* b, const int* fold_of, size_t slot_stride, int nfolds) {
  if (!b || !fold_of) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  const DevBatch& db = b->db;
  const int N = db.N, Npad = db.Npad, nt = db.nt, F = nfolds;
  if (F < 1) return set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_set_folds: nfolds < 1");
  if (slot_stride != 0 && slot_stride != (size_t)N)
    return set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_set_folds: slot_stride must be 0 (shared) or N");
  const int S = slot_stride ? db.B : 1;
  // pass 1: fold sizes and starts, the packed order, the tile rows' first columns
  std::vector<std::vector<int>> perm(S), fstart(S), rowlo(S);
  int njmax = 0;
  for (int s = 0; s < S; ++s) {
    const int* fo = fold_of + (size_t)s * slot_stride;
    std::vector<int> cnt(F, 0);
    for (int i = 0; i < N; ++i) {
      if (fo[i] < 0 || fo[i] >= F) return set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_set_folds: fold id out of range");
      ++cnt[fo[i]];
    }
    fstart[s].assign(F + 1, 0);
    for (int f = 0; f < F; ++f) {
      if (cnt[f] > GPRX_CVFOLD_MAX)
        return set_err(c, GPRX_INVALID_ARGUMENT, "gprx_batch_set_folds: a fold of more than GPRX_CVFOLD_MAX points");
      fstart[s][f + 1] = fstart[s][f] + cnt[f];
    }
    perm[s].assign(Npad, -1);
    std::vector<int> at(fstart[s].begin(), fstart[s].end() - 1);
    for (int i = 0; i < N; ++i) perm[s][at[fo[i]]++] = i;  // ascending i within a fold: a stable sort
    rowlo[s].assign(nt, nt);
    for (int f = 0; f < F; ++f) {
      if (!cnt[f]) continue;
      const int t0 = fstart[s][f] / gprx::TS, t1 = (fstart[s][f + 1] - 1) / gprx::TS;
      for (int t = t0; t <= t1; ++t) rowlo[s][t] = std::min(rowlo[s][t], t0);
    }
    int nj = 0;
    for (int t = 0; t < nt; ++t) nj += t - rowlo[s][t] + 1;  // every tile row holds a point: rowlo <= t
    njmax = std::max(njmax, nj);
  }
  // pass 2: the tables, one after the other
  const size_t ls = gprx::cv_tab_ints(Npad, nt, F, njmax);
  std::vector<int> tab(ls * S);
  for (int s = 0; s < S; ++s) {
    int* p = tab.data() + ls * s;
    std::copy(perm[s].begin(), perm[s].end(), p);
    p += Npad;
    std::copy(fstart[s].begin(), fstart[s].end(), p);
    p += F + 1;
    p[0] = 0;
    for (int f = 0; f < F; ++f) {
      const int m = fstart[s][f + 1] - fstart[s][f];
      p[f + 1] = p[f] + m * m;  // <= N^2 < 2^31 (sizes_addressable)
    }
    p += F + 1;
    std::copy(rowlo[s].begin(), rowlo[s].end(), p);
    p += nt;
    int* jobs = p + (nt + 1) + nt;
    std::fill(jobs, jobs + 2 * (size_t)njmax, -1);
    int nj = 0;
    for (int t = 0; t < nt; ++t) {
      p[t] = nj;
      for (int u = rowlo[s][t]; u <= t; ++u, ++nj) jobs[2 * nj] = t, jobs[2 * nj + 1] = u;
    }
    p[nt] = nj;
    p += nt + 1;
    for (int t = 0; t < nt; ++t) {
      int lo = N - 1;
      for (int r = t * gprx::TS; r < (t + 1) * gprx::TS && r < N; ++r) lo = std::min(lo, perm[s][r]);
      p[t] = lo / gprx::TS * gprx::TS;
    }
  }
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  // the new table first: a failed allocation (GPRX_OUT_OF_MEMORY) or upload leaves the batch's folds as they were
  int* nt_tab = nullptr;
  HIPCHK(c, hipMalloc(&nt_tab, tab.size() * sizeof(int)));
  if (hipMemcpy(nt_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(nt_tab);
    return set_err(c, GPRX_DEVICE_ERROR, "gprx_batch_set_folds: upload failed");
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));  // no launch still reads the old table
  if (b->cv_tab) (void)hipFree(b->cv_tab);
  b->cv_tab = nt_tab;
  b->cv_lstride = S > 1 ? ls : 0;
  b->cv_folds = F;
  b->cv_njmax = njmax;
  return GPRX_OK;
}

// Workspace in the context scratch: the tiles (B x njmax x 4096), r, pvar, mu, var (B x Npad each),
// logp_fold (B x F), logp (B), then the ints: the folds' statuses (B x F) and the slots' (B).  Not part
// of the captured evaluation graphs: four launches straight on the context stream.
int gprx_batch_cvfold(gprx_batch* b, double* mu, double* var, double* logp_fold, double* logp, int* status) {
  if (!b) return GPRX_INVALID_ARGUMENT;
  gprx_ctx* c = b->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if (!b->factored) return set_err(c, GPRX_NOT_READY, "cross-validation before a successful factorisation");
  if (!b->cv_folds) return set_err(c, GPRX_NOT_READY, "cross-validation before gprx_batch_set_folds");
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  const DevBatch& db = b->db;
  const int F = b->cv_folds, nB = db.B;
  const size_t rows = (size_t)nB * db.Npad, nfl = (size_t)nB * F, ntl = (size_t)nB * b->cv_njmax * gprx::TS * gprx::TS;
  char* base = nullptr;
  int rc = ctx_scratch(c, (ntl + 4 * rows + nfl + nB) * sizeof(double) + (nfl + nB) * sizeof(int), &base);
  if (rc) return rc;
  gprx::CvArgs a;
  a.tab = b->cv_tab, a.lstride = b->cv_lstride, a.F = F, a.njmax = b->cv_njmax;
  a.tiles = (double*)base;
  a.r = a.tiles + ntl, a.pvar = a.r + rows, a.mu = a.pvar + rows, a.var = a.mu + rows;
  a.lpf = a.var + rows, a.logp = a.lpf + nfl;
  a.fst = (int*)(a.logp + nB), a.st = a.fst + nfl;
  const double B = nB, N = db.N, Np = db.Npad;
  double tiles = 0.0, m2 = 0.0, m3 = 0.0;  // of the layout the statistics are estimated for: an even split
  {
    const double m = N / F;
    tiles = b->cv_njmax, m2 = F * m * m, m3 = F * m * m * m;
  }
  timed(c, c->stream, "cv_pack", 0.0, B * 8.0 * 1.5 * Np * Np, [&] { gprx::launch_cv_pack(db, a, c->stream); });
  timed(c, c->stream, "cv_kinv", B * tiles * 2.0 * 64.0 * 64.0 * Np / 2.0, B * 8.0 * tiles * (64.0 * Np + 4096.0),
        [&] { gprx::launch_cv_kinv(db, a, c->stream); });
  timed(c, c->stream, "cv_fold", B * m3, B * 8.0 * 3.0 * m2, [&] { gprx::launch_cv_fold(db, a, c->stream); });
  timed(c, c->stream, "cv_final", B * (2.0 * N + F), B * 8.0 * (5.0 * N + F), [&] { gprx::launch_cv_final(db, a, c->stream); });
  HIPCHK(c, hipGetLastError());
  const size_t w = (size_t)db.N * sizeof(double), p = (size_t)db.Npad * sizeof(double);
  std::vector<int> hst(nB);
  if (mu) HIPCHK(c, hipMemcpy2DAsync(mu, w, a.mu, p, w, nB, hipMemcpyDeviceToHost, c->stream));
  if (var) HIPCHK(c, hipMemcpy2DAsync(var, w, a.var, p, w, nB, hipMemcpyDeviceToHost, c->stream));
  if (logp_fold) HIPCHK(c, hipMemcpyAsync(logp_fold, a.lpf, nfl * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (logp) HIPCHK(c, hipMemcpyAsync(logp, a.logp, (size_t)nB * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hst.data(), a.st, (size_t)nB * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  if (status) memcpy(status, hst.data(), (size_t)nB * sizeof(int));
  return first_status(c, "gprx_batch_cvfold", hst.data(), nB);
}

int gprx_gp_set_folds(gprx_gp* gp, const int* fold_of, int nfolds) {
  if (!gp) return GPRX_INVALID_ARGUMENT;
  return gprx_batch_set_folds(gp->batch, fold_of, 0, nfolds);
}

int gprx_gp_cvfold(gprx_gp* gp, double* mu, double* var, double* logp_fold, double* logp) {
  if (!gp) return GPRX_INVALID_ARGUMENT;
  return gprx_batch_cvfold(gp->batch, mu, var, logp_fold, logp, nullptr);
}

// The ngroups x G GPs of a rollout (entry point fn), gathered from batch slots of this context that
// have input dimension d (dwhat: how the message names it), are factorised and passed their last
// evaluation; the trajectories' groups range-checked.  *np: the training points a trajectory step
// visits, summed over the trajectories (the launch's flop and byte estimates).
static int rollout_gps(gprx_ctx* c, const std::string& fn, int ngroups, int G, gprx_batch* const* batches, const int* slots,
                       int d, const std::string& dwhat, int T, const int* traj_group, std::vector<gprx::RolloutGP>& gps,
                       double* np) {
  gps.resize((size_t)ngroups * G);
  for (size_t k = 0; k < gps.size(); ++k) {
    gprx_batch* b = batches[k];
    const int s = slots[k];
    if (!b || b->ctx != c || s < 0 || s >= b->db.B)
      return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": GP " + std::to_string(k) + " is not a slot of a batch of this context");
    if (b->db.d != d)
      return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": input dimension " + std::to_string(b->db.d) + " != " + dwhat);
    if (!b->factored) return set_err(c, GPRX_NOT_READY, fn + ": batch not factorised (run it first)");
    if (b->h_status[s] != 0) return set_err(c, b->h_status[s], fn + ": slot " + std::to_string(s) + " failed its last evaluation");
    const DevBatch& db = b->db;
    gps[k] = gprx::RolloutGP{db.X + (size_t)s * db.Npad * db.d, db.alpha + (size_t)s * db.Npad, db.params + (size_t)s * db.pst, db.N, 0};
  }
  *np = 0.0;
  for (int t = 0; t < T; ++t) {
    if (traj_group[t] < 0 || traj_group[t] >= ngroups) return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": trajectory group out of range");
    for (int g = 0; g < G; ++g) *np += gps[(size_t)traj_group[t] * G + g].N;
  }
  return GPRX_OK;
}

// ---- maximal-coordinate physics -----------------------------------------------------------------
// The experiment mechanisms' joints (examples/utils/data/simulations.jl; oracle/projection_oracle.py
// mechanism()): sub-joints in the order of the equality constraints and their rows.
static bool build_mech(int mech, gprx::MechDev& M) {
  M = gprx::MechDev{};
  struct Sj {
    int kind, rows, a, b;
    double pa[3], pb[3], axis[3];
  };
  std::vector<Sj> js;
  const double O[3] = {0, 0, 0}, EX[3] = {1, 0, 0}, EY[3] = {0, 1, 0};
  auto add = [&](int kind, int rows, int a, int b, const double* pa, const double* pb, const double* ax) {
    Sj j{kind, rows, a, b, {pa[0], pa[1], pa[2]}, {pb[0], pb[1], pb[2]}, {ax[0], ax[1], ax[2]}};
    js.push_back(j);
  };
  auto rev = [&](int a, int b, const double* ax, const double* pa, const double* pb) {
    add(0, 3, a, b, pa, pb, ax);  // Translational3
    add(1, 2, a, b, pa, pb, ax);  // Rotational2 (free about the axis)
  };
  const double h1[3] = {0, 0, 0.5}, h1m[3] = {0, 0, -0.5}, hcp[3] = {0, 0, 0.25};
  switch (mech) {
    case GPRX_MECH_P1: M.nb = 1; rev(0, 1, EX, O, h1); break;
    case GPRX_MECH_P2: M.nb = 2; rev(0, 1, EX, O, h1); rev(1, 2, EX, h1m, h1); break;
    case GPRX_MECH_CP:
      M.nb = 2;
      add(0, 2, 0, 1, O, O, EY);  // Prismatic: Translational2 (free along y) + Rotational3
      add(1, 3, 0, 1, O, O, EY);
      rev(1, 2, EX, O, hcp);
      break;
    case GPRX_MECH_FB:
      M.nb = 4;
      rev(0, 1, EX, O, h1);
      rev(1, 2, EX, h1m, h1);
      add(0, 2, 1, 3, h1, h1, EX);  // Cylindrical: Translational2 + Rotational2
      add(1, 2, 1, 3, h1, h1, EX);
      rev(3, 4, EX, h1m, h1);
      rev(2, 4, EX, h1m, h1m);
      break;
    default: return false;
  }
  // bodies as examples/utils/data/simulations.jl builds them (gprx/vi.py MECHANISMS): m = 1, J = I m
  // l^2 / 12 for the unit links, the cart-pole's pole l = 0.5 (I / 48) and its cart a 0.2 x 0.3 x 0.1
  // box, diag(y^2 + z^2, x^2 + z^2, x^2 + y^2) m / 12
  for (int b = 0; b < M.nb; ++b) {
    M.m[b] = 1.0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) M.J[b][r][c] = r == c ? 1.0 / 12.0 : 0.0;
  }
  if (mech == GPRX_MECH_CP) {
    const double x = 0.2, y = 0.3, z = 0.1;
    M.J[0][0][0] = (y * y + z * z) * 1.0 / 12.0;
    M.J[0][1][1] = (x * x + z * z) * 1.0 / 12.0;
    M.J[0][2][2] = (x * x + y * y) * 1.0 / 12.0;
    for (int r = 0; r < 3; ++r) M.J[1][r][r] = 1.0 / 48.0;
  }
  int row = 0;
  M.nsub = (int)js.size();
  for (int k = 0; k < M.nsub; ++k) {
    gprx::SubJoint& S = M.sub[k];
    const Sj& j = js[k];
    S.kind = j.kind;
    S.a = j.a;
    S.b = j.b;
    S.rows = j.rows;
    S.row0 = row;
    row += j.rows;
    for (int i = 0; i < 3; ++i) {
      S.pa[i] = j.pa[i];
      S.pb[i] = j.pb[i];
    }
    if (j.rows == 3) {
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) S.C[r][c] = r == c ? 1.0 : 0.0;
    } else {  // two orthonormal rows normal to the axis (oracle normal_rows)
      const double* a = j.axis;
      const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
      const double u[3] = {a[0] / na, a[1] / na, a[2] / na};
      const double t[3] = {std::fabs(u[2]) < 0.9 ? 0.0 : 1.0, 0.0, std::fabs(u[2]) < 0.9 ? 1.0 : 0.0};
      double v1[3] = {u[1] * t[2] - u[2] * t[1], u[2] * t[0] - u[0] * t[2], u[0] * t[1] - u[1] * t[0]};
      const double n1 = std::sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]);
      for (double& x : v1) x /= n1;
      const double v2[3] = {u[1] * v1[2] - u[2] * v1[1], u[2] * v1[0] - u[0] * v1[2], u[0] * v1[1] - u[1] * v1[0]};
      for (int c = 0; c < 3; ++c) {
        S.C[0][c] = v1[c];
        S.C[1][c] = v2[c];
        S.C[2][c] = 0.0;
      }
    }
  }
  M.nd = row;
  return 6 * M.nb + M.nd <= gprx::PJ_MAXN;
}

}  // extern "C"

namespace {

// gprx_projectv and gprx_vi_step (name, without the prefix): per trajectory a CState of 13 nb
// doubles and, when in2_w > 0, a second input of in2_w nb doubles go in; out_w nb doubles, the
// Newton iterations and a status come out, the latter two only where the caller wants them.  Args
// is the launcher's argument struct; `extra` sets the fields the two do not share.
template <class Args, class Extra>
int newton_call(gprx_ctx* c, const char* name, int mech, double dt, int T, const double* cstates, const double* in2, int in2_w,
                double regularizer, int newton_iter, double eps, double* out, int out_w, int* iterations, int* status,
                void (*launch)(const Args&, hipStream_t), Extra extra) {
  if (!c) return GPRX_INVALID_ARGUMENT;
  const std::string fn = std::string("gprx_") + name;
  Args a{};
  if (!build_mech(mech, a.mech) || T < 0 || newton_iter < 0 || !(dt > 0.0) || !std::isfinite(regularizer) || !(eps >= 0.0))
    return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": bad mechanism / T / newton_iter / dt / regularizer / eps");
  if (T == 0) return GPRX_OK;
  if (!cstates || (in2_w > 0 && !in2) || !out) return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": null argument");
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  const size_t nb = a.mech.nb, n_cs = (size_t)T * 13 * nb, n_in2 = (size_t)T * in2_w * nb, n_out = (size_t)T * out_w * nb;
  Layout l;
  const size_t o_cs = l.take<double>(n_cs), o_in2 = l.take<double>(n_in2), o_out = l.take<double>(n_out),
               o_it = l.take<int>(T), o_st = l.take<int>(T);
  char* base;
  int rc = ctx_scratch(c, l.size, &base);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(base + o_cs, cstates, n_cs * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (in2_w > 0) HIPCHK(c, hipMemcpyAsync(base + o_in2, in2, n_in2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  a.dt = dt;
  a.reg = regularizer;
  a.eps = eps;
  a.iters = newton_iter;
  a.T = T;
  a.cs = at<double>(base, o_cs);
  a.out = at<double>(base, o_out);
  a.iters_out = at<int>(base, o_it);
  a.status = at<int>(base, o_st);
  extra(a, at<double>(base, o_in2));
  timed(c, c->stream, name, 0.0, (double)T * 8.0 * (13 + in2_w + out_w) * nb, [&] { launch(a, c->stream); });
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, base + o_out, n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (iterations) HIPCHK(c, hipMemcpyAsync(iterations, base + o_it, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (status) HIPCHK(c, hipMemcpyAsync(status, base + o_st, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  return GPRX_OK;
}

// What the rollout calls share around their launch: one device buffer [gps | group | start | out |
// the per-trajectory outputs `extra`, in their order] with its three uploads, and after the launch
// the copies back -- out, then every extra output the caller wants -- with the synchronise.
struct RolloutIo {
  struct Extra {
    void* host;   // where the caller wants the T values, or null
    size_t elem;  // bytes per trajectory
    size_t off;
  };
  char* base = nullptr;
  size_t o_gps = 0, o_grp = 0, o_st = 0, o_out = 0, sw = 0;  // sw: bytes of start and of out
  std::vector<Extra> extra;
  template <class T>
  T* dev(size_t k) const {
    return at<T>(base, extra[k].off);
  }
};
template <class Args>
int rollout_upload(gprx_ctx* c, RolloutIo& io, const std::vector<gprx::RolloutGP>& gps, int T, const int* traj_group,
                   const double* start, Args& a) {
  Layout l;
  io.o_gps = l.take<gprx::RolloutGP>(gps.size());
  io.o_grp = l.take<int>(T);
  io.o_st = l.take<char>(io.sw);
  io.o_out = l.take<char>(io.sw);
  for (RolloutIo::Extra& e : io.extra) e.off = l.take<char>((size_t)T * e.elem);
  int rc = ctx_scratch(c, l.size, &io.base);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(io.base + io.o_gps, gps.data(), gps.size() * sizeof(gprx::RolloutGP), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(io.base + io.o_grp, traj_group, (size_t)T * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(io.base + io.o_st, start, io.sw, hipMemcpyHostToDevice, c->stream));
  a.gps = at<gprx::RolloutGP>(io.base, io.o_gps);
  a.group = at<int>(io.base, io.o_grp);
  a.start = at<double>(io.base, io.o_st);
  a.out = at<double>(io.base, io.o_out);
  return GPRX_OK;
}
int rollout_download(gprx_ctx* c, const RolloutIo& io, int T, double* final_state) {
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(final_state, io.base + io.o_out, io.sw, hipMemcpyDeviceToHost, c->stream));
  for (const RolloutIo::Extra& e : io.extra)
    if (e.host) HIPCHK(c, hipMemcpyAsync(e.host, io.base + e.off, (size_t)T * e.elem, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  return GPRX_OK;
}

// What the recorded entry points (gprx_rollout_*_rec) add to their one-launch counterparts: the
// records wanted, the launch bound and where the records go.  A null RecReq is the one-launch call.
struct RecReq {
  int R;
  const int* rec;
  int steps_per_launch;
  double* traj;
};
// last (or null): the largest index wanted, 1 at least
int rec_check(gprx_ctx* c, const std::string& fn, const RecReq& q, int steps, int T, int* last = nullptr) {
  if (q.R > 0 && (!q.rec || !q.traj)) return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": null argument");
  int hi = 1;
  for (int t = 0; t < T; ++t)
    for (int r = 0; r < q.R; ++r) {
      const int j = q.rec[(size_t)t * q.R + r];
      if (j < 1 || j > steps + 1 || (r > 0 && j < q.rec[(size_t)t * q.R + r - 1]))
        return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": rec must be non-decreasing per trajectory, in [1, steps + 1]");
      hi = j > hi ? j : hi;
    }
  if (last) *last = hi;
  return GPRX_OK;
}
// The device buffers of a recorded call follow the one-launch call's in its RolloutIo (the records
// come back with the outputs); `row` doubles per record.
constexpr size_t REC_EXTRAS = 5;
void rec_extras(RolloutIo& io, const RecReq& q, size_t row) {
  io.extra.push_back({q.traj, (size_t)q.R * row * sizeof(double), 0});
  io.extra.push_back({nullptr, (size_t)q.R * sizeof(int), 0});                        // rec
  io.extra.push_back({nullptr, sizeof(int), 0});                                      // cursor
  io.extra.push_back({nullptr, (size_t)gprx::ROLLOUT_CARRY * sizeof(double), 0});     // carry
  io.extra.push_back({nullptr, 2 * sizeof(int), 0});                                  // icarry
}
int rec_upload(gprx_ctx* c, const RolloutIo& io, const RecReq& q, int T, gprx::RolloutRec& rr) {
  const size_t k = io.extra.size() - REC_EXTRAS;
  rr.R = q.R;
  rr.traj = q.R ? io.dev<double>(k) : nullptr;
  rr.rec = q.R ? io.dev<int>(k + 1) : nullptr;
  rr.cursor = io.dev<int>(k + 2);
  rr.carry = io.dev<double>(k + 3);
  rr.icarry = io.dev<int>(k + 4);
  if (q.R) HIPCHK(c, hipMemcpyAsync(io.base + io.extra[k + 1].off, q.rec, (size_t)T * q.R * sizeof(int), hipMemcpyHostToDevice, c->stream));
  return GPRX_OK;
}
// The default steps per launch of a recorded rollout keeps a launch near 0.2 s, as gprx_simulate's,
// at the largest shapes the project rolls out: the four-bar, N = 512 (G = 12 maximal; usesin minimal).
// A step of T trajectories takes lat + T traj seconds there -- the line through the two measurements on
// an MI355X, T = 100 (the step chain's latency: the workgroups run side by side) and T = 3200 (several
// rounds of resident workgroups) -- so the default falls with T (DESIGN.md section 4 has the figures).
struct RecStepTime {
  double lat, traj;  // seconds
};
constexpr RecStepTime REC_MAX{3.29e-3, 2.56e-6}, REC_MAX_MD{5.33e-3, 4.15e-6},  // 3.55 / 11.5 ms and 5.75 / 18.6 ms per step
    REC_MIN{3.5e-6, 8.5e-9}, REC_MIN_MD{0.62e-3, 2.71e-6};                       // 0.0043 / 0.031 ms and 0.89 / 9.29 ms
int rec_default_spl(const RecStepTime& s, int T) {
  const double n = 0.2 / (s.lat + s.traj * T);
  return n < 1.0 ? 1 : (n > 1e6 ? 1000000 : (int)n);
}
// steps [0, steps) in launches of at most spl steps (one launch when steps = 0: record 1 and the outputs)
template <class Args, class Launch>
int rec_launches(gprx_ctx* c, const char* stat, Args& a, int spl, double flops_step, double bytes_step, Launch launch) {
  a.rr.step0 = 0;
  do {
    a.rr.nsteps = a.steps - a.rr.step0 < spl ? a.steps - a.rr.step0 : spl;
    timed(c, c->stream, stat, flops_step * a.rr.nsteps, bytes_step * a.rr.nsteps, [&] { launch(a, c->dist_mode, c->stream); });
    HIPCHK(c, hipGetLastError());
    a.rr.step0 += a.rr.nsteps;
  } while (a.rr.step0 < a.steps);
  return GPRX_OK;
}

}  // namespace

extern "C" {

int gprx_projectv(gprx_ctx* c, int mech, double dt, int T, const double* cstates, const double* vw_pred,
                  double regularizer, int newton_iter, double eps, double* vw_out, int* iterations, int* status) {
  return newton_call<gprx::ProjArgs>(c, "projectv", mech, dt, T, cstates, vw_pred, 6, regularizer, newton_iter, eps, vw_out, 6,
                                     iterations, status, gprx::launch_project,
                                     [](gprx::ProjArgs& a, const double* vw) { a.vw = vw; });
}

int gprx_vi_step(gprx_ctx* c, int mech, double dt, int T, const double* cstates, double regularizer, int newton_iter,
                 double eps, double* out, int* iterations, int* status) {
  return newton_call<gprx::ViArgs>(c, "vi_step", mech, dt, T, cstates, nullptr, 0, regularizer, newton_iter, eps, out, 13,
                                   iterations, status, gprx::launch_vi_step,
                                   [](gprx::ViArgs& a, const double*) { a.grav = 9.81; });  // |mechanism.g| (simulations.jl; gprx/vi.py GRAV)
}

// simulate!(mechanism, steps dt, control!, record = true) of the datasets (examples/utils/data/
// simulations.jl:7-213; examples/parallel/dataframes.jl:58-93 reads the storage at the sampled
// indices) for T trajectories: k_simulate in launches of at most steps_per_launch steps, so that no
// launch runs for seconds; the device buffer [cs | mass | inertia | damp | rec | out | cursor |
// status] carries state, record cursor and status from one launch to the next.
int gprx_simulate(gprx_ctx* c, int mech, double dt, int steps, int T, const double* start, const double* mass,
                  const double* inertia, const double* damp, double vi_regularizer, int newton_iter, double eps, int R,
                  const int* rec, int steps_per_launch, double* out, int* status) {
  if (!c) return GPRX_INVALID_ARGUMENT;
  const std::string fn = "gprx_simulate";
  gprx::SimArgs a{};
  if (!build_mech(mech, a.mech) || steps < 0 || T < 0 || R < 1 || newton_iter < 0 || steps_per_launch < 0 || !(dt > 0.0) ||
      !std::isfinite(vi_regularizer) || !(eps >= 0.0))
    return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": bad mechanism / steps / T / R / newton_iter / steps_per_launch / dt / regularizer / eps");
  if (T == 0) return GPRX_OK;
  if (!start || !rec || !out) return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": null argument");
  int last = 1;  // the largest index wanted: no trajectory steps past it
  if (int rc = rec_check(c, fn, RecReq{R, rec, steps_per_launch, out}, steps, T, &last)) return rc;
  // The default bounds a launch whose every step runs all newton_iter = 100 iterations (a solve whose twist
  // does not settle; a stagnated one ends sooner, k_simulate): a four-bar step then takes 12 ms with 200
  // trajectories in flight (measured), 16 of them 0.19 s.  One wave per trajectory: beyond about
  // 1024 trajectories the waves no longer run side by side and a launch grows with T, so the default shrinks.
  const int spl = steps_per_launch > 0 ? steps_per_launch : (T <= 16 * 1024 ? 16 / ((T + 1023) / 1024) : 1);
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  const size_t nb = a.mech.nb, n_cs = (size_t)T * 13 * nb, n_rec = (size_t)T * R, n_out = n_rec * 13 * nb;
  Layout l;
  const size_t o_cs = l.take<double>(n_cs), o_m = l.take<double>(mass ? T * nb : 0), o_J = l.take<double>(inertia ? T * nb * 9 : 0),
               o_c = l.take<double>(damp ? T * nb * 6 : 0), o_rec = l.take<int>(n_rec), o_out = l.take<double>(n_out),
               o_cur = l.take<int>(T), o_st = l.take<int>(T);
  char* base;
  int rc = ctx_scratch(c, l.size, &base);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(base + o_cs, start, n_cs * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (mass) HIPCHK(c, hipMemcpyAsync(base + o_m, mass, T * nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (inertia) HIPCHK(c, hipMemcpyAsync(base + o_J, inertia, T * nb * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (damp) HIPCHK(c, hipMemcpyAsync(base + o_c, damp, T * nb * 6 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(base + o_rec, rec, n_rec * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(base + o_cur, 0, (size_t)T * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(base + o_st, 0, (size_t)T * sizeof(int), c->stream));
  a.dt = dt;
  a.reg = vi_regularizer;
  a.eps = eps;
  a.grav = 9.81;  // |mechanism.g| (simulations.jl:10, :110; gprx/vi.py GRAV)
  a.iters = newton_iter;
  a.T = T;
  a.R = R;
  a.mass = mass ? at<double>(base, o_m) : nullptr;
  a.inertia = inertia ? at<double>(base, o_J) : nullptr;
  a.damp = damp ? at<double>(base, o_c) : nullptr;
  a.rec = at<int>(base, o_rec);
  a.cs = at<double>(base, o_cs);
  a.cursor = at<int>(base, o_cur);
  a.status = at<int>(base, o_st);
  a.out = at<double>(base, o_out);
  const int total = last - 1;  // steps any trajectory takes
  a.step0 = 0;
  do {  // at least one launch: index 1 is recorded without a step
    a.nsteps = total - a.step0 < spl ? total - a.step0 : spl;
    timed(c, c->stream, "simulate", 0.0, 0.0, [&] { gprx::launch_simulate(a, c->stream); });
    HIPCHK(c, hipGetLastError());
    a.step0 += a.nsteps;
  } while (a.step0 < total);
  HIPCHK(c, hipMemcpyAsync(out, base + o_out, n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (status) HIPCHK(c, hipMemcpyAsync(status, base + o_st, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect(c);
  return GPRX_OK;
}

// ---- rollout in minimal coordinates ------------------------------------------------------------
// gprx_rollout_min (vi_regularizer null: MeanZero GPs, k_rollout<., RolloutArgs>) and
// gprx_rollout_min_md (predictdynamicsmin with MeanDynamics GPs, examples/utils/predictdynamics.jl:
// 30-102 with src/mDynamics.jl:41-55: the physics mean per step, k_rollout<., RolloutMinMdArgs>): one
// validation, scratch layout and launch.  With rq (gprx_rollout_min_rec, gprx_rollout_min_md_rec) the
// same call keeps the records rq names and runs as launches of at most rq->steps_per_launch steps of
// the recording instantiations, the records, cursor and carried state further entries of the scratch.
static int rollout_min_call(gprx_ctx* c, const std::string& fn, const char* stat, int mech, int usesin, double dt, int steps,
                            const double* vi_regularizer, int ngroups, gprx_batch* const* batches, const int* slots, int T,
                            const int* traj_group, const double* start, double* final_state, int* status, int* vi_status,
                            const RecReq* rq = nullptr) {
  if (!c) return GPRX_INVALID_ARGUMENT;
  gprx::RolloutMinMdRecArgs a{};  // every form's arguments: each launcher takes the part it knows
  // The MeanZero form accepts any finite dt, as it always has (dt only scales the updates); the
  // physics step of the MeanDynamics form needs dt > 0, as gprx_vi_step does.
  if (!build_mech(mech, a.mech) || steps < 0 || ngroups < 1 || T < 0 || !std::isfinite(dt) ||
      (vi_regularizer && (!(dt > 0.0) || !std::isfinite(*vi_regularizer))))
    return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": bad mechanism / steps / groups / dt" + (vi_regularizer ? " / regularizer" : ""));
  if (rq && (rq->R < 0 || rq->steps_per_launch < 0)) return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": bad R / steps_per_launch");
  if (T == 0) return GPRX_OK;
  if (!batches || !slots || !traj_group || !start || !final_state) return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": null argument");
  if (rq)
    if (int rc = rec_check(c, fn, *rq, steps, T)) return rc;
  // coordinates (q, qdot) per mechanism: P1 theta; P2 theta1, theta2 (relative); CP x, theta;
  // FB theta1, theta3 -- the angle coordinates get (sin, cos) features when usesin
  const int nc = mech == GPRX_MECH_P1 ? 1 : 2;
  const int ang0 = mech == GPRX_MECH_CP ? 0 : 1, ang1 = nc > 1 ? 1 : 0;
  const int dobs = (usesin && ang0 ? 3 : 2) + (nc > 1 ? (usesin && ang1 ? 3 : 2) : 0);
  std::lock_guard<std::mutex> g(c->mu);
  std::vector<gprx::RolloutGP> gps;
  double np = 0.0;
  int rc = rollout_gps(c, fn, ngroups, nc, batches, slots, dobs, std::to_string(dobs) + " for this mechanism / usesin", T,
                       traj_group, gps, &np);
  if (rc) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  RolloutIo io;
  io.sw = (size_t)T * 2 * nc * sizeof(double);
  io.extra = {{status, sizeof(int), 0}, {vi_status, sizeof(int), 0}};
  if (rq) rec_extras(io, *rq, 2 * (size_t)nc);
  if ((rc = rollout_upload(c, io, gps, T, traj_group, start, a))) return rc;
  a.T = T;
  a.nc = nc;
  a.d = dobs;
  a.steps = steps;
  a.usesin = usesin ? 1 : 0;
  a.ang0 = ang0;
  a.ang1 = ang1;
  a.dt = dt;
  a.mech_id = mech;
  // link lengths of the experiment mechanisms (examples/utils/simulations.jl; gprx/rollout.py LENGTHS)
  a.len[0] = mech == GPRX_MECH_CP ? 0.5 : 1.0;
  a.len[1] = 1.0;
  a.status = io.dev<int>(0);
  if (vi_regularizer)  // newton! as gprx_vi_step's callers run it (gprx/projection.py vi_step)
    a.vi = gprx::RolloutViArgs{*vi_regularizer, 1e-10, 9.81, 100, vi_status ? io.dev<int>(1) : nullptr};
  const double flops = np * (3.0 * dobs + 24.0), bytes = np * (dobs + 1) * 8.0;  // per step
  if (!rq) {
    timed(c, c->stream, stat, flops * steps, bytes * steps, [&] {
      if (vi_regularizer) gprx::launch_rollout_min_md(a, c->dist_mode, c->stream);
      else gprx::launch_rollout(a, c->dist_mode, c->stream);
    });
    return rollout_download(c, io, T, final_state);
  }
  if ((rc = rec_upload(c, io, *rq, T, a.rr))) return rc;
  const int spl = rq->steps_per_launch > 0 ? rq->steps_per_launch : rec_default_spl(vi_regularizer ? REC_MIN_MD : REC_MIN, T);
  if (vi_regularizer) {
    rc = rec_launches(c, stat, a, spl, flops, bytes, gprx::launch_rollout_min_md_rec);
  } else {
    gprx::RolloutRecArgs z{};
    static_cast<gprx::RolloutArgs&>(z) = a;
    z.rr = a.rr;
    rc = rec_launches(c, stat, z, spl, flops, bytes, gprx::launch_rollout_rec);
  }
  return rc ? rc : rollout_download(c, io, T, final_state);
}

int gprx_rollout_min(gprx_ctx* c, int mech, int usesin, double dt, int steps, int ngroups,
                     gprx_batch* const* batches, const int* slots, int T, const int* traj_group,
                     const double* start, double* final_state) {
  return rollout_min_call(c, "gprx_rollout_min", "rollout", mech, usesin, dt, steps, nullptr, ngroups, batches, slots, T,
                          traj_group, start, final_state, nullptr, nullptr);
}

int gprx_rollout_min_md(gprx_ctx* c, int mech, int usesin, double dt, int steps, double vi_regularizer, int ngroups,
                        gprx_batch* const* batches, const int* slots, int T, const int* traj_group, const double* start,
                        double* final_state, int* status, int* vi_status) {
  return rollout_min_call(c, "gprx_rollout_min_md", "rollout_min_md", mech, usesin, dt, steps, &vi_regularizer, ngroups, batches,
                          slots, T, traj_group, start, final_state, status, vi_status);
}

// ---- rollout in maximal coordinates ------------------------------------------------------------
// gprx_rollout_max (vi_regularizer null: MeanZero GPs, k_rollout_max) and gprx_rollout_max_md (the
// physics mean per step, k_rollout_max<., RolloutMaxMdArgs>): one validation, scratch layout and launch;
// with rq the recorded forms (gprx_rollout_max_rec, gprx_rollout_max_md_rec), as rollout_min_call
static int rollout_max_call(gprx_ctx* c, const std::string& fn, const char* stat, int mech, double dt, int steps, double regularizer,
                            const double* vi_regularizer, int ngroups, gprx_batch* const* batches, const int* slots, int G,
                            const int* vw_idx1, int T, const int* traj_group, const double* start, double* final_state,
                            double* proj_err, int* status, int* vi_status, const RecReq* rq = nullptr) {
  if (!c) return GPRX_INVALID_ARGUMENT;
  gprx::MechDev M;
  if (!build_mech(mech, M) || steps < 0 || ngroups < 1 || T < 0 || G < 1 || G > gprx::PJ_MAXG || !(dt > 0.0) ||
      !std::isfinite(regularizer) || (vi_regularizer && !std::isfinite(*vi_regularizer)))
    return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": bad mechanism / steps / groups / G / dt / regularizer");
  if (rq && (rq->R < 0 || rq->steps_per_launch < 0)) return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": bad R / steps_per_launch");
  if (T == 0) return GPRX_OK;
  if (!batches || !slots || !vw_idx1 || !traj_group || !start || !final_state)
    return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": null argument");
  if (rq)
    if (int rc = rec_check(c, fn, *rq, steps, T)) return rc;
  const int d = 13 * M.nb;
  gprx::RolloutMaxMdRecArgs a{};  // every form's arguments: each launcher takes the part it knows
  for (int g = 0; g < G; ++g) {
    const int k = (vw_idx1[g] - 1) % 13;
    if (vw_idx1[g] < 1 || vw_idx1[g] > d || k < 7)
      return set_err(c, GPRX_INVALID_ARGUMENT, fn + ": vw index " + std::to_string(vw_idx1[g]) +
                                                   " is not a velocity / angular-velocity slot of the CState");
    a.vw[g] = vw_idx1[g] - 1;
  }
  std::lock_guard<std::mutex> lk(c->mu);
  std::vector<gprx::RolloutGP> gps;
  double np = 0.0;
  int rc = rollout_gps(c, fn, ngroups, G, batches, slots, d, "13 nbodies", T, traj_group, gps, &np);
  if (rc) return rc;
  if (hipSetDevice(c->device) != hipSuccess) return GPRX_DEVICE_ERROR;
  RolloutIo io;
  io.sw = (size_t)T * d * sizeof(double);
  io.extra = {{proj_err, sizeof(double), 0}, {status, sizeof(int), 0}, {vi_status, sizeof(int), 0}};
  if (rq) rec_extras(io, *rq, (size_t)d);
  if ((rc = rollout_upload(c, io, gps, T, traj_group, start, a))) return rc;
  a.mech = M;
  a.dt = dt;
  a.reg = regularizer;
  a.eps = 1e-10;  // projectv! defaults (implicitProjection.jl:80)
  a.iters = 100;
  a.steps = steps;
  a.T = T;
  a.G = G;
  a.d = d;
  a.perr = io.dev<double>(0);
  a.status = io.dev<int>(1);
  if (vi_regularizer)  // newton! as gprx_vi_step's callers run it (gprx/projection.py vi_step)
    a.vi = gprx::RolloutViArgs{*vi_regularizer, 1e-10, 9.81, 100, vi_status ? io.dev<int>(2) : nullptr};
  const double flops = np * (3.0 * d + 24.0), bytes = np * (d + 1) * 8.0;  // per step
  if (!rq) {
    timed(c, c->stream, stat, flops * steps, bytes * steps, [&] {
      if (vi_regularizer) gprx::launch_rollout_max_md(a, c->dist_mode, c->stream);
      else gprx::launch_rollout_max(a, c->dist_mode, c->stream);
    });
    return rollout_download(c, io, T, final_state);
  }
  if ((rc = rec_upload(c, io, *rq, T, a.rr))) return rc;
  const int spl = rq->steps_per_launch > 0 ? rq->steps_per_launch : rec_default_spl(vi_regularizer ? REC_MAX_MD : REC_MAX, T);
  if (vi_regularizer) {
    rc = rec_launches(c, stat, a, spl, flops, bytes, gprx::launch_rollout_max_md_rec);
  } else {
    gprx::RolloutMaxRecArgs z{};
    static_cast<gprx::RolloutMaxArgs&>(z) = a;
    z.rr = a.rr;
    rc = rec_launches(c, stat, z, spl, flops, bytes, gprx::launch_rollout_max_rec);
  }
  return rc ? rc : rollout_download(c, io, T, final_state);
}

int gprx_rollout_max(gprx_ctx* c, int mech, double dt, int steps, double regularizer, int ngroups,
                     gprx_batch* const* batches, const int* slots, int G, const int* vw_idx1, int T,
                     const int* traj_group, const double* start, double* final_state, double* proj_err, int* status) {
  return rollout_max_call(c, "gprx_rollout_max", "rollout_max", mech, dt, steps, regularizer, nullptr, ngroups, batches, slots, G,
                          vw_idx1, T, traj_group, start, final_state, proj_err, status, nullptr);
}

int gprx_rollout_max_md(gprx_ctx* c, int mech, double dt, int steps, double regularizer, double vi_regularizer, int ngroups,
                        gprx_batch* const* batches, const int* slots, int G, const int* vw_idx1, int T,
                        const int* traj_group, const double* start, double* final_state, double* proj_err, int* status,
                        int* vi_status) {
  return rollout_max_call(c, "gprx_rollout_max_md", "rollout_max_md", mech, dt, steps, regularizer, &vi_regularizer, ngroups,
                          batches, slots, G, vw_idx1, T, traj_group, start, final_state, proj_err, status, vi_status);
}

// ---- the recorded rollouts: the same calls in launches of at most steps_per_launch steps --------
int gprx_rollout_min_rec(gprx_ctx* c, int mech, int usesin, double dt, int steps, int ngroups, gprx_batch* const* batches,
                         const int* slots, int T, const int* traj_group, const double* start, double* final_state, int R,
                         const int* rec, int steps_per_launch, double* traj) {
  const RecReq q{R, rec, steps_per_launch, traj};
  return rollout_min_call(c, "gprx_rollout_min_rec", "rollout_rec", mech, usesin, dt, steps, nullptr, ngroups, batches, slots, T,
                          traj_group, start, final_state, nullptr, nullptr, &q);
}

int gprx_rollout_min_md_rec(gprx_ctx* c, int mech, int usesin, double dt, int steps, double vi_regularizer, int ngroups,
                            gprx_batch* const* batches, const int* slots, int T, const int* traj_group, const double* start,
                            double* final_state, int* status, int* vi_status, int R, const int* rec, int steps_per_launch,
                            double* traj) {
  const RecReq q{R, rec, steps_per_launch, traj};
  return rollout_min_call(c, "gprx_rollout_min_md_rec", "rollout_min_md_rec", mech, usesin, dt, steps, &vi_regularizer, ngroups,
                          batches, slots, T, traj_group, start, final_state, status, vi_status, &q);
}

int gprx_rollout_max_rec(gprx_ctx* c, int mech, double dt, int steps, double regularizer, int ngroups, gprx_batch* const* batches,
                         const int* slots, int G, const int* vw_idx1, int T, const int* traj_group, const double* start,
                         double* final_state, double* proj_err, int* status, int R, const int* rec, int steps_per_launch,
                         double* traj) {
  const RecReq q{R, rec, steps_per_launch, traj};
  return rollout_max_call(c, "gprx_rollout_max_rec", "rollout_max_rec", mech, dt, steps, regularizer, nullptr, ngroups, batches,
                          slots, G, vw_idx1, T, traj_group, start, final_state, proj_err, status, nullptr, &q);
}

int gprx_rollout_max_md_rec(gprx_ctx* c, int mech, double dt, int steps, double regularizer, double vi_regularizer, int ngroups,
                            gprx_batch* const* batches, const int* slots, int G, const int* vw_idx1, int T,
                            const int* traj_group, const double* start, double* final_state, double* proj_err, int* status,
                            int* vi_status, int R, const int* rec, int steps_per_launch, double* traj) {
  const RecReq q{R, rec, steps_per_launch, traj};
  return rollout_max_call(c, "gprx_rollout_max_md_rec", "rollout_max_md_rec", mech, dt, steps, regularizer, &vi_regularizer,
                          ngroups, batches, slots, G, vw_idx1, T, traj_group, start, final_state, proj_err, status, vi_status, &q);
}

gprx_batch* gprx_gp_batch(gprx_gp* gp) { return gp ? gp->batch : nullptr; }

// ---- host CState helpers -----------------------------------------------------------------------
int gprx_cstate_pack(int nb, const double* xc, const double* q, const double* vc, const double* wc, double* out) {
  if (nb < 1 || !xc || !q || !vc || !wc || !out) return GPRX_INVALID_ARGUMENT;
  for (int b = 0; b < nb; ++b) {
    double* o = out + 13 * b;
    for (int k = 0; k < 3; ++k) o[k] = xc[3 * b + k];
    for (int k = 0; k < 4; ++k) o[3 + k] = q[4 * b + k];
    for (int k = 0; k < 3; ++k) o[7 + k] = vc[3 * b + k];
    for (int k = 0; k < 3; ++k) o[10 + k] = wc[3 * b + k];
  }
  return GPRX_OK;
}

int gprx_select_outputs(const double* Xc, int d, int N, const int* idx1, int G, double* Y) {
  if (!Xc || !idx1 || !Y || d < 1 || N < 0 || G < 0) return GPRX_INVALID_ARGUMENT;
  for (int k = 0; k < G; ++k)
    if (idx1[k] < 1 || idx1[k] > d) return GPRX_INVALID_ARGUMENT;
  for (int k = 0; k < G; ++k)
    for (int t = 0; t < N; ++t) Y[(size_t)k * N + t] = Xc[(size_t)t * d + (idx1[k] - 1)];
  return GPRX_OK;
}

}  // extern "C"
