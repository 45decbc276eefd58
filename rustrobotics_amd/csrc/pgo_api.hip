// pgo_api.hip -- librr_pgo.so: C ABI (include/rr_pgo.h) over the HIP engine.
//
// Host side of the hot path, mirroring the reference's PoseGraph
// (src/mapping/pose_graph_optimization.rs:214-373): create = parse + upload +
// one-off symbolic analysis; optimize = the GN / LM loop with every kernel of an
// iteration replayed from one hipGraph on the handle's own stream; the host
// reads two scalars (chi2, |dx|) per iteration.
#include <mutex>
#include <queue>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/rr_pgo.h"
#include "host_graph.h"
#include "kernels.hip.h"
#include "flow.hip.h"
#include "lds_flow.hip.h"
#include "selinv.hip.h"
#include "chordal.hip.h"
#include "treesolve.hip.h"
#include "symbolic.h"
#include "host_threads.h"

#ifndef RRPGO_UPD_DEPTH
#define RRPGO_UPD_DEPTH 1   // k-chunks of the trailing update requested ahead of the MFMAs
#endif
namespace rrpgo {


struct ApiError : std::runtime_error {
  int code;
  ApiError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

static thread_local std::string g_last_error;

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      throw ApiError(RR_PGO_ENODEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)

// One handle makes ~45 device buffers, and hipMalloc / hipFree cost 50-100 us each (the frees also
// synchronise): a caller that builds a graph, runs ten iterations and drops it -- the reference's own
// criterion bench -- would spend more time there than iterating.  Buffers are carved out of a few large
// chunks owned by the engine instead; a DevBuf only calls hipMalloc itself when no arena is active.
// Chunks of dropped handles are kept per device and handed to the next handle (hipFree synchronises the device and costs
// ~0.1 ms per chunk: "drop" was 0.4 - 0.5 ms of the 7 ms closure the reference's bench times, benches/graph_slam.rs:9-10, a
// loop of new + optimize(10) + drop).  Only small chunks, and only a bounded total: the arenas of the large graphs are freed.
// Nothing reads memory it has not written (scripts/gpu_soak.py rebuilds handles on poisoned memory), so a recycled chunk needs no clearing.
struct ChunkPool {
  struct Idle { int dev; char *base; size_t cap; };
  std::mutex mu;
  std::vector<Idle> idle;
  size_t idle_bytes = 0;
  static constexpr size_t kMaxChunk = 64u << 20, kMaxIdle = 256u << 20;
  char *take(size_t min_bytes, size_t *cap) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    size_t best = idle.size();
    for (size_t i = 0; i < idle.size(); i++)
      if (idle[i].dev == dev && idle[i].cap >= min_bytes && idle[i].cap <= 4 * min_bytes + (1u << 20) && (best == idle.size() || idle[i].cap < idle[best].cap)) best = i;
    if (best == idle.size()) return nullptr;
    char *p = idle[best].base;
    *cap = idle[best].cap;
    idle_bytes -= idle[best].cap;
    idle.erase(idle.begin() + (long)best);
    return p;
  }
  void trim() {
    std::lock_guard<std::mutex> lk(mu);
    for (Idle &c : idle) (void)hipFree(c.base);
    idle.clear();
    idle_bytes = 0;
  }
  void put(int dev, char *base, size_t cap) {   // dev: the device the chunk was allocated on (the caller's current device may be another by now)
    if (cap <= kMaxChunk && dev >= 0) {
      std::lock_guard<std::mutex> lk(mu);
      if (idle_bytes + cap <= kMaxIdle) { idle.push_back(Idle{dev, base, cap}); idle_bytes += cap; return; }
    }
    (void)hipFree(base);
  }
};
static ChunkPool &chunk_pool() { static ChunkPool *p = new ChunkPool; return *p; }   // leaked on purpose, like the stream pool

struct DeviceArena {
  struct Chunk { char *base; size_t cap, used; int dev; };
  std::vector<Chunk> chunks;
  size_t next_chunk = 8u << 20;
  DeviceArena() = default;
  DeviceArena(const DeviceArena &) = delete;
  DeviceArena &operator=(const DeviceArena &) = delete;
  bool stream_failed = false;   // the engine's stream could not be synchronised when it was given back (a device fault, a launch that
                                // never drained): work may still be touching the chunks -- they are freed (hipFree waits for the
                                // device), not handed to the next handle
  // (the engine's stream was synchronised when it went back to its pool: declared after the arena, destroyed before it)
  ~DeviceArena() {
    for (Chunk &c : chunks) {
      if (stream_failed) (void)hipFree(c.base);
      else chunk_pool().put(c.dev, c.base, c.cap);
    }
  }
  void reserve(size_t bytes) { next_chunk = std::max(next_chunk, bytes); }
  void *take(size_t bytes) {
    for (Chunk &c : chunks) {
      const size_t off = (c.used + 255) & ~(size_t)255;
      if (off + bytes <= c.cap) { c.used = off + bytes; return c.base + off; }
    }
    Chunk c{nullptr, std::max(next_chunk, bytes + 256), 0, -1};
    if (hipGetDevice(&c.dev) != hipSuccess) c.dev = -1;
    if (char *p = chunk_pool().take(c.cap, &c.cap)) c.base = p;
    else HIPCHK(hipMalloc((void **)&c.base, c.cap));
    next_chunk = std::max<size_t>(8u << 20, c.cap / 4);
    c.used = bytes;
    chunks.push_back(c);
    return c.base;
  }
};
static thread_local DeviceArena *t_arena = nullptr;   // set while an engine allocates
struct ArenaScope {   // every DevBuf::alloc of the scope draws from `a` (null: a buffer of its own, freed when it grows and with the handle)
  DeviceArena *const prev = t_arena;
  explicit ArenaScope(DeviceArena *a) { t_arena = a; }
  ArenaScope(const ArenaScope &) = delete;
  ArenaScope &operator=(const ArenaScope &) = delete;
  ~ArenaScope() { t_arena = prev; }
};

// hipStreamCreate costs ~2 ms (a hardware queue) and hipStreamDestroy about as much: more than the ten
// Gauss-Newton iterations of the reference's bench on intel.g2o.  Streams of destroyed handles are kept
// per device and handed to the next handle (idle: they were synchronised before being returned).
struct StreamPool {
  std::mutex mu;
  std::vector<std::pair<int, hipStream_t>> idle;
  hipStream_t get() {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < idle.size(); i++)
        if (idle[i].first == dev) { hipStream_t s = idle[i].second; idle.erase(idle.begin() + (long)i); return s; }
    }
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
  }
  bool put(hipStream_t s) {   // false: the stream could not be synchronised (it is destroyed, not pooled)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { (void)hipStreamDestroy(s); return false; }
    std::lock_guard<std::mutex> lk(mu);
    if (idle.size() < 16) idle.emplace_back(dev, s);
    else (void)hipStreamDestroy(s);
    return true;
  }
  void trim() {
    std::lock_guard<std::mutex> lk(mu);
    for (auto &p : idle) (void)hipStreamDestroy(p.second);
    idle.clear();
  }
};
static StreamPool &stream_pool() { static StreamPool *p = new StreamPool; return *p; }   // leaked on purpose: outlives the runtime's teardown order

// RAII holders: an Engine constructor that throws (hipMalloc failure, RR_PGO_EUNSUPPORTED) still releases these
struct PooledStream {
  hipStream_t s = nullptr;
  PooledStream() = default;
  PooledStream(const PooledStream &) = delete;
  PooledStream &operator=(const PooledStream &) = delete;
  bool *failed = nullptr;   // the arena's flag (DeviceArena::stream_failed)
  ~PooledStream() { if (s && !stream_pool().put(s) && failed) *failed = true; }
  void acquire() { if (!s) s = stream_pool().get(); }
  operator hipStream_t() const { return s; }
};
struct EventHolder {
  hipEvent_t e = nullptr;
  EventHolder() = default;
  EventHolder(const EventHolder &) = delete;
  EventHolder &operator=(const EventHolder &) = delete;
  ~EventHolder() { if (e) (void)hipEventDestroy(e); }
  void create(unsigned flags) { if (!e) HIPCHK(hipEventCreateWithFlags(&e, flags)); }
  operator hipEvent_t() const { return e; }
};
template <typename U> struct PinnedBuf {
  U *p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  // coherent (fine-grained): a kernel's system-scope stores are visible to the polling host while the kernel runs
  void alloc(size_t n, bool coherent = true) {
    if (p) { (void)hipHostFree(p); p = nullptr; }
    HIPCHK(hipHostMalloc((void **)&p, n * sizeof(U), coherent ? (hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) : hipHostMallocDefault));
  }
  U &operator[](size_t i) const { return p[i]; }
  operator U *() const { return p; }
};

template <typename U> struct DevBuf {
  U *p = nullptr;
  size_t n = 0;
  bool owned = false;   // false: lives in the engine's arena
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p && owned) (void)hipFree(p); }
  void alloc(size_t count) {
    if (p && owned) (void)hipFree(p);
    p = nullptr;
    n = count;
    if (!count) return;
    if (t_arena) { p = (U *)t_arena->take(count * sizeof(U)); owned = false; }
    else { HIPCHK(hipMalloc((void **)&p, count * sizeof(U))); owned = true; }
  }
  void upload(const std::vector<U> &v) {
    alloc(v.size());
    if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice));
  }
  void zero() { if (n) HIPCHK(hipMemset(p, 0, n * sizeof(U))); }
};

static double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// one step of rr_pgo_extend's initial guess as the host plans it: node dst from node src and a measurement (graph packing)
struct HostGuessStep { int32_t src, dst, op; double m[7]; };

// the prior list of a handle (rr_pgo_set_priors) as the caller gave it, checked: rr_pgo_extend carries it to the grown handle
struct PriorSet {
  std::vector<int32_t> node;
  std::vector<double> meas, info;   // packed in prior order by the node's kind, as edge measurements and information are
  std::vector<uint8_t> robust;      // per prior
  int keep_anchor = 1;
  int n() const { return (int)node.size(); }
};

// What a handle has been told since it was created, as its setters normalised it.  rr_pgo_extend and rr_pgo_remove_edges
// build a new engine and carry this record to it: carry_settings is the ONE place that enumerates the fields, so a new
// field is carried by adding it there.  (The engine's device copies and derived host tables are not settings.)
struct HandleSettings {
  // robust kernel (rr_pgo_set_robust_kernel / rr_pgo_set_robust_tls): ROBUST_* of kernels.hip.h; delta is 1 under ROBUST_NONE;
  // mu is ROBUST_TLS's continuation parameter, 0 under every other kind; the per-edge mask (empty: every edge)
  int robust_kind = ROBUST_NONE;
  double robust_delta = 1.0, robust_mu = 0.0;
  std::vector<uint8_t> robust_mask;
  PriorSet priors;                  // rr_pgo_set_priors: the caller's list (keep_anchor is 1 while it is empty)
  std::vector<int32_t> fixed;       // rr_pgo_set_fixed: the distinct nodes in ascending order
  int fixed_keep_anchor = 1;        // (1 while the set is empty)
  bool query_big = false;           // rr_pgo_set_query_big_fronts: fronts beyond LDS go to the k_tree_*_big kernels
  bool marg_big = false;            // rr_pgo_set_marginals_big_fronts: ... and to the k_selinv_big_* kernels
};

// an edge mask of the ABI in the record's form: one byte per edge, 0 or 1; null: empty (every edge)
static std::vector<uint8_t> mask_bytes(const int32_t *mask, int n_edges) {
  std::vector<uint8_t> m(mask ? (size_t)n_edges : 0);
  for (size_t k = 0; k < m.size(); k++) m[k] = mask[k] != 0 ? 1 : 0;
  return m;
}

struct EngineBase {
  enum Query { Q_MARGINALS, Q_COVARIANCES, Q_GATE, Q_GATE_JOINT, Q_CROSS, Q_CHECK, N_QUERY };   // the factor queries, in the order of their ABI functions
  virtual ~EngineBase() = default;
  virtual void chi2(double *out) = 0;
  virtual void linearize_solve(double lambda, int lm, double *dx_out) = 0;
  virtual void update(const double *dx, double sign) = 0;
  virtual void optimize(int solver, int iters, double *errors, int *n_errors, double *norms) = 0;
  virtual void get_state(double *out) = 0;
  virtual void set_state(const double *st) = 0;
  virtual void assemble(double lambda, int lm, std::vector<double> &hvals, std::vector<double> &b) = 0;
  virtual void iterate_async(int iters) = 0;
  virtual void sync() = 0;
  virtual void profile(int iters, double *ms, int64_t *launches) = 0;
  virtual hipStream_t stream() = 0;
  virtual void read_stamps(std::vector<unsigned long long> &out) = 0;
  virtual void mark_flow_fronts(std::vector<char> &in_flow) = 0;   // fronts whose level runs as k_big_flow
  virtual int schur_tile() const = 0;                              // tile edge of k_big_schur, 0 = no Schur split
  virtual void solve_form(int32_t *kform, double *k_bytes, double *k_flops) const = 0;   // rr_pgo_solve_form
  virtual int flow_trace(int level, std::vector<int32_t> &tasks, std::vector<unsigned long long> &stamps, int *nf, double *est_us) = 0;
  // sharded runs
  virtual void exchange_buffer(int which, void **ptr, int64_t *n, int32_t *esize) = 0;
  virtual void set_exchange_buffer(int which, void *ptr, int64_t n) = 0;
  virtual void stage(int stage, double lambda, int lm) = 0;
  virtual void read_last_scalars(double *chi, double *norm) = 0;
  virtual void debug_withhold(int mode) = 0;   // failure injection for the dataflow launches (rr_pgo_debug_withhold)
  virtual const HandleSettings &settings() const = 0;   // what the setters below have left: read by the ABI's getters and by the carry
  // rr_pgo_set_robust_kernel / rr_pgo_set_robust_tls (arguments checked; mu: ROBUST_TLS alone; mask: in the record's form)
  virtual void set_robust(int kind, double delta, double mu, std::vector<uint8_t> mask) = 0;
  virtual void set_robust_mu(double mu) = 0;                                   // rr_pgo_set_robust_mu (arguments checked)
  // rr_pgo_optimize_gnc (arguments checked) / rr_pgo_gnc_times
  virtual void optimize_gnc(int solver, const rr_pgo_gnc_options &opt, const int32_t *mask, rr_pgo_gnc_result *res, double *stage_mu, double *stage_cost) = 0;
  virtual void gnc_times(double *ms) const = 0;
  virtual void edge_errors(double *s_out, double *w_out) = 0;                  // rr_pgo_edge_errors
  virtual void refuse_priors(const char *who) const = 0;                       // EUNSUPPORTED where priors cannot be held
  virtual void set_priors(const PriorSet &ps) = 0;                             // rr_pgo_set_priors (arguments checked)
  virtual void prior_errors(double *s_out, double *w_out) = 0;                 // rr_pgo_prior_errors
  virtual void refuse_fixed(const char *who) const = 0;                        // EUNSUPPORTED where fixed nodes cannot be held
  virtual void set_fixed(const std::vector<int32_t> &nodes, int keep_anchor) = 0;   // rr_pgo_set_fixed (distinct, ascending, checked)
  virtual void initialize(int method) = 0;                       // rr_pgo_initialize / rr_pgo_initialize_times
  virtual void initialize_times(double *ms) const = 0;
  // rr_pgo_marginals (arguments checked; off: [nq + 1] offsets of the blocks in out) / rr_pgo_marginals_times
  virtual void marginals(int nq, const int32_t *na, const int32_t *nb, const int64_t *off, double *out) = 0;
  // rr_pgo_covariances (arguments checked; off as for marginals) / rr_pgo_covariances_times
  virtual void covariances(int nq, const int32_t *na, const int32_t *nb, const int64_t *off, double *out) = 0;
  // rr_pgo_gate_edges (arguments checked; cand: kind, nodes, measurement, Omega and Omega^-1 filled in; soff: [n + 1] offsets
  // of the innovation covariances in innov; chi2 and innov may be null) / rr_pgo_gate_times
  virtual void gate_edges(int n, const int32_t *from, const int32_t *to, const int64_t *soff, std::vector<GateCand> &cand,
                          double *d2, double *chi2, double *innov) = 0;
  // rr_pgo_check_edges (arguments checked; cand: the queried edges' records as for gate_edges, pad = the mask bit; soff: [n + 1]
  // offsets of the residual covariances in resid; red, chi2 and resid may be null) / rr_pgo_check_edges_times
  virtual void check_edges(int n, const int32_t *from, const int32_t *to, const int64_t *soff, std::vector<GateCand> &cand,
                           double *d2, double *red, double *chi2, double *resid) = 0;
  virtual void refuse_factor_query(const char *who) const = 0;   // what every factor query refuses, before its arguments are read
  virtual void set_query_big_fronts(int on) = 0;                  // rr_pgo_set_query_big_fronts
  virtual void set_marginals_big_fronts(int on) = 0;              // rr_pgo_set_marginals_big_fronts
  // rr_pgo_gate_joint (arguments checked; set s is the records [set_ptr[s], set_ptr[s + 1]) of from / to / cand, the sets
  // expanded one after the other; dim: D_s; ioff: [n_sets + 1] offsets of the sets' S in innov; prefix and innov may be null) /
  // rr_pgo_gate_joint_times
  virtual void gate_joint(int n_sets, const int32_t *set_ptr, const int32_t *from, const int32_t *to, const int32_t *dim,
                          const int64_t *ioff, std::vector<GateCand> &cand, double *d2, double *prefix, double *innov) = 0;
  // rr_pgo_cross_covariances (arguments checked; row_node null: every node; roff / coff: [n + 1] first scalar of every row /
  // column node in out, R x C row-major) / rr_pgo_cross_covariances_times
  virtual void cross_covariances(int n_row, const int32_t *row_node, int n_col, const int32_t *col_node, const int64_t *roff,
                                 const int64_t *coff, double *out) = 0;
  // the six rr_pgo_*_times: the three phases of the last call of query `which`, in ms
  virtual void last_query_times(Query which, double *ms) const = 0;
  // rr_pgo_extend (arguments checked).  The state buffer is in node order, so a grown graph's buffer starts with the old one.
  virtual const void *pose_dev() const = 0;
  virtual size_t pose_node_bytes() const = 0;   // bytes of one node in the state buffer
  // initial values of the nodes n_old .. n_total - 1: the old state and the steps' results in a staging buffer of this engine
  // (guess_dev), made on its stream; new_state_out: the new nodes in rr_pgo_get_state's packing; *ms: HIP-event time
  virtual void guess_nodes(const std::vector<HostGuessStep> &steps, const std::vector<int32_t> &tree_ptr, int n_old, int n_total,
                           bool is3d, const int32_t *new_kind, double *new_state_out, double *ms) = 0;
  virtual const void *guess_dev() const = 0;
  // the first n_nodes nodes of the state from src (device memory of the same arithmetic type), on this engine's stream; waits
  virtual void adopt_state(const void *src, size_t n_nodes, double *ms) = 0;
  int n_launches_per_iter = 0;
  // rr_pgo_launch_counts: iterations put on the stream as plain launches / as replays of the captured hipGraph / as items of
  // the device-side loop, and instantiations of that graph.  Host-side, counted where the launches are enqueued.
  int64_t launch_counts[4] = {0, 0, 0, 0};
};

constexpr int HIST = 4096;  // ring of (chi2, |dx|) pairs written by k_finalize

__global__ void k_finalize_slot(const double *chi_partial, int n_chi, const double *norm_partial,
                                int n_norm, double *hist, int *counter, int advance) {
  __shared__ double red[4];
  double c = 0.0, n = 0.0;
  for (int i = threadIdx.x; i < n_chi; i += 256) c += chi_partial[i];
  for (int i = threadIdx.x; i < n_norm; i += 256) n += norm_partial[i];
  double ct = block_sum<double, 256>(c, red);
  double nt = block_sum<double, 256>(n, red);
  if (threadIdx.x == 0) {
    int slot = *counter % HIST;
    if (n_chi > 0) hist[2 * slot] = ct;
    if (n_norm > 0) hist[2 * slot + 1] = sqrt(nt);
    if (advance) *counter = *counter + 1;
  }
}

// sharded runs: this rank's partial sums (chi2, |dx|^2) for the caller's sum all-reduce; `which` bit 0 = chi2, bit 1 = |dx|^2
__global__ void k_finalize_partial(const double *chi_partial, int n_chi, const double *norm_partial, int n_norm, double *scal) {
  __shared__ double red[4];
  double c = 0.0, n = 0.0;
  for (int i = threadIdx.x; i < n_chi; i += 256) c += chi_partial[i];
  for (int i = threadIdx.x; i < n_norm; i += 256) n += norm_partial[i];
  double ct = block_sum<double, 256>(c, red);
  double nt = block_sum<double, 256>(n, red);
  if (threadIdx.x == 0) {
    if (n_chi > 0) scal[0] = ct;
    scal[1] = n_norm > 0 ? nt : 0.0;
  }
}

// T: type of H, b, L, x (factor + solve).  S: type of the state, the measurements and the
// linearisation arithmetic (S == T, or S = double with T = float: "mixed" mode).
template <typename T, typename S = T> class Engine final : public EngineBase {
  using V4 = typename VecT<S>::V4;
  using V2 = typename VecT<S>::V2;
  // pack_state / unpack_state (host_graph.h) in S: one V4, for SE(3) two; return the scalars read / written
  static int pack_v4(int kind, const double *s, V4 *v) {
    double p[8];
    const int n = pack_state(kind, s, p);
    v[0] = V4{(S)p[0], (S)p[1], (S)p[2], (S)p[3]};
    if (kind == NODE_SE3 || kind == NODE_XYZ) v[1] = V4{(S)p[4], (S)p[5], (S)p[6], (S)p[7]};   // (XYZ: zeros)
    return n;
  }
  static int unpack_v4(int kind, const V4 *v, double *s) {
    double p[8] = {(double)v[0].x, (double)v[0].y, (double)v[0].z, (double)v[0].w};
    if (kind == NODE_SE3) { p[4] = (double)v[1].x; p[5] = (double)v[1].y; p[6] = (double)v[1].z; p[7] = (double)v[1].w; }
    return unpack_state(kind, p, s);
  }
  const HostGraph &g_;
  const Symbolic &sym_;
  DeviceArena arena_;   // declared before every DevBuf: destroyed after them
  PooledStream stream_;
  hipGraphExec_t gn_exec_ = nullptr;
  // graph data
  DevBuf<V4> pose_;
  DevBuf<EdgeRec<S>> e_rec_;   // SE(2): every edge's from / to / slot / measurement / information as one record
  DevBuf<int2> e_idx_;         // SE(3): from, to;
  DevBuf<V4> e_meas_;          //        the measurement, a pair per edge;
  DevBuf<int64_t> e_slot_;     //        (offset into hvals << 1) | transposed
  DevBuf<int64_t> diag_off_;
  DevBuf<int32_t> inc_ptr_, node_offset_, node_pcol_;
  DevBuf<int2> inc_list_;
  DevBuf<uint8_t> node_dim_;
  DevBuf<S> e_info3_;   // SE(3): 21 information entries per edge
  bool is3d_ = false;
  bool has_lm_ = false;   // a 3-D graph with XYZ landmarks: the LM kernels (k_linearize_lm, k_update_lm) run
  bool has_br_ = false;   // a 2-D graph with bearing-only / range-only edges: the BR kernels (k_linearize_br, k_edge_errors_br) run
  // sharding over ranks
  int rank_ = 0, world_ = 1;
  bool sharded_ = false;            // driven by rr_pgo_stage (world_size > 1, or opt.sharded with one rank)
  int64_t xch_n_ = 0;               // elements of exchange buffer 0: world * chunk
  DevBuf<int32_t> node_list_;       // nodes this rank linearises and updates: own + shared (null: all)
  DevBuf<uint8_t> norm_counts_;     // per node: this rank adds its |dx|^2 to the partial sum (and prior / lambda to its diagonal)
  DevBuf<int64_t> shared_src_;      // scalars of the shared nodes' diagonal blocks and rhs (k_pack_shared / k_sum_shared)
  int n_shared_ = 0;
  int n_list_ = 0;
  DevBuf<double> scal_own_;         // exchange buffer 1: partial (chi2, |dx|^2) unless the caller binds one
  double *scal_ = nullptr;
  hipGraphExec_t stage_exec_[2] = {nullptr, nullptr};
  DevBuf<T> xch_own_;               // exchange buffer 0 (boundary update matrices) unless the caller binds one
  T *xch_ = nullptr, *x_ptr_ = nullptr;
  int solve_threads_max_ = 512;     // RR_PGO_SOLVE_THREADS=<n>: cap of the back-substitution workgroup size
  static constexpr int factor_threads_max_ = 1024;   // 16-wave workgroups for steps whose fronts exceed 128 rows (8 waves: intel 4134 against 4318 it/s, r04)
  struct UpdMap { int64_t offset; int n_tiles; };   // slice of upd_map_buf_: a tile list of k_big_update or k_big_schur
  static constexpr int schur_tile_ = 64;        // k_big_schur's tile edge (128 x 128 tiles, k_big_schur<T, 4>: measured 13 % slower, r03)
  bool schur_split_ = true;                     // RR_PGO_SCHUR_SPLIT=0: every super-panel's update reaches through the Schur complement (r02)
  DevBuf<int32_t> upd_map_buf_;
  static constexpr bool xcd_remap_ = true;   // k_big_update / k_big_schur: one contiguous eighth of the tile list per XCD (dispatch order: FETCH_SIZE 96 against 37 MB per launch, r02)
  int sp_solve_min_nc_ = 256;       // back substitution: levels whose widest pivot block has at least this many columns run k_big_solve_sp (RR_PGO_SP_SOLVE_MIN)
  static constexpr bool gather_update_ = true;   // big fronts: k_big_build builds the pivot columns only, a front's first trailing update gathers its tiles from the children
  // k_big_flow (flow.hip.h): levels of at most flow_max_nf_ big fronts run as ONE launch of ticket-ordered tile tasks
  struct FlowLevel {
    DevBuf<FlowRec> tasks;     // every task with a copy of its front's records (one 128-byte load per task)
    int n_tasks = 0;
    bool schur_split = false;  // the level's Schur complements are a k_big_schur launch behind the flow launch
    std::vector<FlowTask> host_tasks;   // diagnostic builds: the sorted list, for rr_pgo_debug_flow_trace
    DevBuf<unsigned long long> trace;   // diagnostic builds only
    int64_t ticket_word = 0;   // index of the level's ticket in flow_flags_
    int wfill_begin = 0, wfill_end = 0;   // the level's entries in flow_wfill_
    double est_us = 0;         // critical path of the cost model that orders the tasks
  };
  std::vector<SnMeta> host_task_meta_;   // host copy of task_meta_ (one record per task = per front of a big level)
  std::vector<SnMeta> host_sn_meta_;     // host copy of sn_meta_
  DevBuf<int64_t> flow_wfill_;      // per four W blocks of a front of a flow level: offset and count of scalars in winv (k_flow_reset marks them)
  DevBuf<unsigned> flow_flags_;     // tickets + completion flags of every flow level, zeroed at the start of a factorisation
  int flow_max_nf_ = 1 << 20;       // RR_PGO_FLOW=<n> (0: never): levels of at most n fronts ...
  int flow_max_tasks_ = 1 << 20;    // RR_PGO_FLOW_TASKS=<n>: ... and of at most n tasks run as ONE k_big_flow launch: by default every level.
                                    // History on the 1M-edge lattice (r03): with tickets in the order of earliest starts only the levels of 1
                                    // and 2 fronts gained; with the list schedule and the Schur complements left to k_big_schur the levels up
                                    // to 64 fronts; with W polled in place and no tile on the chain every level does (limits 64 / 128 / 256 /
                                    // none: 4.57 / 4.54 / 4.53 / 4.52 ms) -- the launch sequence (k_big_panel32 + k_big_update) remains as the
                                    // parity alternative (RR_PGO_FLOW=0)
  // cross-level form of k_big_flow (flow.hip.h, XL): graphs of a few dozen fronts beyond LDS (sphere2500: 46 in six levels) run ALL
  // their levels as ONE launch -- BUILD tasks in place of k_big_build, Schur complements as UPDATE tasks, parent waits for child by counter
  bool xl_ = false;                 // RR_PGO_FLOW_XL=0: one build + one flow launch per level (the r03 / r04 form; bit-identical)
  int xl_max_fronts_ = 256;         // RR_PGO_FLOW_XL=<n>: graphs of at most n fronts beyond LDS
  int xl_level_tasks_ = 1 << 20;    // RR_PGO_FLOW_XL_TASKS=<n>: ... none of whose levels has more than n tasks in that form
  bool xl_refused_ = false;         // a level went over the task limit under the cross-level plan: planned again level by level
  DevBuf<FlowRec> xl_recs_;
  std::vector<FlowRec> xl_host_;
  DevBuf<int2> xl_child_done_;
  DevBuf<unsigned long long> xl_trace_;   // diagnostic builds only
  int64_t xl_ticket_word_ = 0;
  static constexpr bool fused_assembly_ = true;   // H entries and rhs of the fronts beyond LDS by k_big_build's own waves when its launch is a single round of workgroups (else a k_big_assemble launch)
  static constexpr bool flow_deep_ = true;   // fast mode: panel steps of blocks 0 and 1 look back over the previous super-panel (see build_flow_levels)
  bool flow_exact_ = false;         // RR_PGO_FLOW_EXACT=1: bit-identical to the launch sequence (tile (0, 0) forms the next super-panel's first block)
  struct SolveFlowLevel { DevBuf<SolveFlowFront> fronts; DevBuf<SolveFlowTask> tasks; int n_tasks = 0; int64_t ticket_word = 0; };
  // What one step of sym_.steps launches, built once by the constructor: every launch function reads it, and
  // n_launches_per_iter is a sum over it (factor_launches / solve_launches)
  enum { L11_FLOW, L11_SP, L11_MID };   // back substitution of a big level's pivot blocks: k_big_solve_flow | k_big_solve_sp per super-panel | k_solve_mid
  struct StepPlan {
    int kind = STEP_TASKS, nf = 0, task_begin = 0;   // nf: tasks of an LDS step, fronts of a big level
    int max_nc = 1, maxM = 0, max_nr = 1;            // the level's widest pivot block, tallest front, most rows below a pivot block
    bool has_rows = false;                           // some front has rows below its pivot block
    // an LDS step: k_factor_tasks / k_solve_tasks, step 0 of the dataflow schedule k_factor_flow / k_solve_flow
    size_t factor_lds = 0;                           // bytes
    int factor_threads = 0, solve_threads = 0;       // workgroup sizes after the caps
    int solve_lds = 0;                               // scalars of LDS of the step's back substitution (every kind of step)
    // factorisation of a big level
    int build_gx = 0, asm_gx = 0;                    // k_big_build's grid x; k_big_assemble's, 0: assembly fused into the build
    bool any_dup = false, has_root = false;          // k_big_assemble_dup runs; the level holds the gauge root
    std::vector<int> panel_gx;                       // k_big_panel32's grid x per 32-column block (launch sequence only)
    std::vector<UpdMap> upd;                         // k_big_update's tile list per super-panel (launch sequence only)
    UpdMap schur{0, 0};                              // k_big_schur's tile list (none: no split on this level)
    std::unique_ptr<FlowLevel> flow;                 // null: launch sequence
    // back substitution of a big level
    int cb = 0, R = 1;                               // k_big_gemv_partial's column blocks and row slices (launched if has_rows)
    int l11 = L11_MID, l11_gx = 0, n_sp = 0;         // the L11 form, its grid x, super-panels of the widest pivot block
    std::unique_ptr<SolveFlowLevel> solve_flow;      // L11_FLOW: k_big_solve_flow's tasks and counters
    bool in_solve_flow = false;                      // the level's back substitution runs as tasks of k_solve_flow, not as launches
  };
  std::vector<StepPlan> plan_;
  bool solve_flow_on_ = true;       // RR_PGO_SOLVE_FLOW=0: one k_big_solve_sp launch per 128 columns
  int flow_schur_min_ = 512;        // RR_PGO_FLOW_SCHUR_MIN=<n>: flow levels with at least n Schur tiles leave them to k_big_schur
  int flow_grid_ = 0;               // persistent workgroups of a flow launch (RR_PGO_FLOW_GRID; default CUs x RRPGO_FLOW_WAVES)
  // k_factor_flow / k_solve_flow (lds_flow.hip.h): every front in LDS, the factorisation and the back substitution ONE launch each
  bool lds_flow_ = false;
  DevBuf<int32_t> child_dep_, parent_dep_;
  DevBuf<int32_t> child_due_;   // per child_meta entry: the block of the parent's panel at which the child is added (Symbolic::child_due)
  std::vector<int32_t> host_child_dep_;
  DevBuf<unsigned> dep_flags_;      // [0, S) factor flags, [S, 2 S) solve flags, then the two tickets on lines of their own, then a word nobody sets
  DevBuf<LdsFlowTask> lds_ftasks_, lds_stasks_;
  int lds_n_tasks_ = 0, lds_flow_cus_ = 256;
  std::vector<LdsFlowTask> host_stasks_;   // k_solve_flow's tickets: [per narrow level of fronts beyond LDS, top level first: GEMV units, L11 tasks] + the LDS tasks
  int lds_n_stasks_ = 0;
  unsigned long long wait_ticks_ = 200000000ull;   // bound of one in-launch wait: 2 s of the 100 MHz wall clock (RR_PGO_FLOW_TIMEOUT_MS)
  // failure injection (rr_pgo_debug_withhold): what was changed, to put it back
  int withheld_child_ = -1, withheld_parent_ = -1, withheld_level_ = -1, withheld_task_ = -1;
  int32_t withheld_parent_val_ = -1;
  FlowRec withheld_rec_{};
  static constexpr int kDeadFlagWords = 4096;   // flag words behind the live ones that no consumer ever looks at
  // gauge transfer (single-precision factor, Gauss-Newton; kernels.hip.h "gauge transfer")
  bool gauge_ok_ = false;            // the root front is a big front with an SE2 pivot node
  bool stage_gauge_ = false;         // sharded handle: the gauge stage 0 linearised in -- written by stage 0 alone, read by stage 1 alone
  int gauge_root_ = -1;              // supernode that takes the rank-3 term
  DevBuf<int32_t> gauge_col_node_;
  DevBuf<T> gauge_v_;
  double gauge_ox_ = 0, gauge_oy_ = 0, gauge_mu_t_ = 0, gauge_mu_r_ = 0;
  DevBuf<int64_t> pack_list_;       // (front, exchange offset) of the in-place boundary fronts this rank owns
  int n_pack_ = 0, pack_max_nu_ = 0;
  // numeric
  DevBuf<T> hvals_, b_, x_, dx_ref_, lvals_, uvals_, winv_, xnew_, gemv_part_;
  // K form of the back substitution (kernels.hip.h, kform_front): [K^T; c^T] of the LDS fronts, laid out like lvals up to the
  // last LDS panel.  On for the handles whose LDS fronts qualify for the dataflow launches (Symbolic::flow_eligible, one rank,
  // not sharded) -- in the level schedule of such a handle too (RR_PGO_LDS_FLOW=0: the same bits); RR_PGO_SOLVE_KFORM=0: the
  // chain form (read at creation)
  DevBuf<T> kvals_;
  bool kform_ = false;
  double kform_bytes_ = 0, kform_flops_ = 0;   // one factorisation's K steps: panel rows read + X written, 2 per multiply-add
  // queries over the factor (rr_pgo_marginals, rr_pgo_covariances, rr_pgo_gate_edges, rr_pgo_gate_joint): the tree tables and the events are made
  // by the first such call
  static constexpr bool f64_ = std::is_same<T, double>::value && std::is_same<S, double>::value;
  std::vector<int32_t> front_depth_, col_front_;   // depth of a front (a root: 0); permuted scalar column -> front
  EventHolder query_ev_[4];
  // the last call of each query (EngineBase::Query): linearise + factor | selected inverse or tree solve | the query's own
  // kernel (gather; products + gather; gate kernel + copy; joint kernel + copy; gather + copy)
  double query_ms_[N_QUERY][3] = {};
  // marginal covariances (selinv.hip.h; rr_pgo_marginals): everything made on the first call
  DevBuf<T> svals_;                  // the selected inverse, a front's image laid out like its factor image (less the rhs row)
  DevBuf<SelMeta> sel_meta_;
  DevBuf<int32_t> sel_order_;        // fronts by tree level, root level first
  std::vector<int32_t> sel_level_ptr_;   // ranges of sel_order_
  std::vector<int64_t> sel_soff_;
  size_t sel_lds_ = 0;
  bool sel_ready_ = false;
  // fronts beyond LDS in the selected inverse (rr_pgo_set_marginals_big_fronts): per level the LDS fronts
  // come first in sel_order_, and the tiles of the others' kernels follow each other, launch by launch, in sel_tile_
  std::vector<int32_t> sel_big_ptr_;     // per level: its first front beyond LDS in sel_order_
  std::vector<int32_t> sel_tile_ptr_;    // ranges of sel_tile_: k_selinv_big_z, _y, _zz; then per level: k_selinv_big_rp, _pp
  DevBuf<SelBig> sel_big_;
  DevBuf<SelTile> sel_tile_;
  DevBuf<T> sel_work_;                   // Z and Y of every front beyond LDS
  // covariances of arbitrary pairs (treesolve.hip.h; rr_pgo_covariances): the per-front records are made on the first call,
  // in the arena; the plan of a call and its workspace live in buffers of their own that only grow
  DevBuf<TsMeta> ts_meta_;
  size_t ts_lds_ = 0;
  size_t ts_ws_bytes_ = TS_WS_BYTES;   // bound of Z + U of one pass (RR_PGO_TS_WS_BYTES=<n>, read at creation)
  bool ts_ready_ = false;
  bool ts_trace_ = false;              // RR_PGO_QUERY_TRACE=1, read at creation: every pass of a tree query describes its plan on stderr
  DevBuf<TsTask> ts_tasks_;
  DevBuf<TsSlab> ts_slab_, cross_slab_;   // slabs of the fronts beyond LDS, by level: rows below (forward), pivot rows (backward)
  DevBuf<int32_t> ts_child_, ts_unit_, ts_czrow_;
  DevBuf<CovQuery> ts_query_;
  DevBuf<T> ts_z_, ts_u_;
  DevBuf<double> ts_out_;
  // the gate of candidate edges (rr_pgo_gate_edges): the covariance plan and workspace above, plus its own records
  DevBuf<GateCand> gate_cand_;
  // joint compatibility of sets of candidates (rr_pgo_gate_joint): gate_cand_ holds the sets' records one after the other;
  // per set its record, the pivot columns of its fronts and the Z rows of its candidates' nodes there
  DevBuf<JointSet> joint_set_;
  DevBuf<int32_t> joint_fnc_, joint_fz_;
  // Sigma[rows, cols] (rr_pgo_cross_covariances): the covariance plan of the column nodes and its workspace above, plus the
  // backward-active fronts by level, their rows in V, the rows and columns of out in V, and V itself
  DevBuf<int32_t> cross_order_, cross_fvrow_, cross_rsrc_;
  DevBuf<int64_t> cross_csrc_;
  DevBuf<T> ts_v_;
  static constexpr int kGemvSlices = 16;   // row slices of the multi-workgroup L21^T x product
  DevBuf<double> chi_partial_, norm_partial_, hist_;
  DevBuf<int> counter_, err_, blocks_done_;
  DevBuf<unsigned long long> stamps_;  // diagnostic builds only
  // symbolic tables
  DevBuf<int32_t> task_ptr_, task_sn_, fasm_src_, fasm_dst_, fasm_colptr_, fdup_src_, fdup_dst_, scat_, rel_, perm_, sn_rows_;
  DevBuf<SnMeta> sn_meta_, task_meta_;
  DevBuf<ChildMeta> child_meta_;
  PinnedBuf<double> host_pair_;      // pinned: chi2, |dx|, and (as an int in slot 2) the device error flag; behind them (32-byte
                                     // aligned) the OPT_RING slots rr_pgo_optimize's device-side loop publishes its iterations in
  PinnedBuf<V4> state_stage_;        // rr_pgo_set_state's staging buffer (made on first use) and the event behind its last copy
  EventHolder state_stage_ev_;
  std::vector<double> state_in_;     // ... and the state that call was given
  DevBuf<V4> pose_saved_;            // ... and its device-side copy
  OptSlot *opt_ring_ = nullptr;      // = host_pair_ + 4: host-coherent, written by the device, polled by optimize_pipelined
  DevBuf<OptCtrl> opt_ctrl_;         // the loop state of the running rr_pgo_optimize call (kernels.hip.h, OptCtrl)
  bool stop_dirty_ = false;          // the stop word err_[1] may be set: cleared before the next launch outside a pipelined rr_pgo_optimize call
  bool sync_optimize_ = false;       // RR_PGO_SYNC_OPTIMIZE=1: rr_pgo_optimize with one host round trip per iteration (the r01 - r05
                                     // form, bit-identical: the parity alternative; always with the edge-parallel linearisation)
  int n_lin_blocks_ = 0, n_upd_blocks_ = 0;
  bool no_graph_ = false, force_graph_ = false;   // RR_PGO_NO_GRAPH=1 / RR_PGO_FORCE_GRAPH=1 (read when the handle is created): plain launches / replays of the captured hipGraph everywhere
  bool edge_lin_ = false;           // RR_PGO_EDGE_LINEARIZE=1: k_linearize_edges (one thread per edge, atomics) instead of the pull form
  bool edge_lin_wave_ = false;      // RR_PGO_EDGE_LINEARIZE=2: k_linearize_wave_edges (one WAVEFRONT per edge, operands staged in LDS, LDS-reduced scatter-add)
  bool edge_lin_env_ = false, edge_lin_wave_env_ = false;   // what the knob asked for (a robust kernel runs the pull form)
  int lin_blocks_pull_ = 0, lin_blocks_edge_ = 0;            // n_lin_blocks_ of the pull form / of the edge-parallel form
  HandleSettings settings_;          // everything the setters were told (the robust kernel, the priors, the fixed nodes, the big-front switches)
  // rr_pgo_optimize_gnc: k_edge_errors' (s, w) and k_tls_scan's partials on the device, the scan's four numbers in host-coherent
  // memory, the time of the last call's scans / stages / closing iterations
  DevBuf<double> gnc_sw_, gnc_partial_;
  DevBuf<int> gnc_done_;
  PinnedBuf<double> gnc_host_;
  double gnc_ms_[3] = {0, 0, 0};
  DevBuf<uint8_t> robust_mask_;      // the robust kernel's per-edge mask on the device (none: every edge)
  // priors (rr_pgo_set_priors): the device form of settings_.priors -- CSR by node, records in CSR order (a node's priors
  // in the call's order).  The buffers live in the arena and only grow (DevBuf::n is their capacity).
  std::vector<int32_t> prior_order_;   // CSR position -> index in the call
  DevBuf<int32_t> prior_ptr_, prior_node_;
  DevBuf<EdgeRec<S>> prior_rec_;       // SE(2)
  DevBuf<V4> prior_meas_;              // SE(3)
  DevBuf<S> prior_info3_;              // SE(3)
  DevBuf<uint8_t> prior_robust_;
  // fixed nodes (rr_pgo_set_fixed): settings_.fixed as one byte per node, on the host and on the device (arena;
  // allocated by the first non-empty set).  While the set is empty k_linearize and k_update get a null pointer.
  std::vector<uint8_t> fixed_host_;    // [n_nodes] while the set is non-empty (the queries' plans read it)
  DevBuf<uint8_t> fixed_;
  // rr_pgo_initialize (chordal.hip.h): the projected rotations per node, the exported solution of the first rotation stage
  // (3-D), the events around the stages and the last call's times; buffers and events are made by the first call
  DevBuf<S> chordal_rot_;
  DevBuf<T> chordal_sol_;
  EventHolder chordal_ev_[4];
  double chordal_ms_[3] = {0, 0, 0};
  DevBuf<V4> guess_stage_;           // rr_pgo_extend's initial guess: the old state and the new nodes behind it (made by that call)
  int host_counter_ = 0;             // mirrors the device slot counter

 public:
  Engine(const HostGraph &g, const Symbolic &sym, int rank, int world, bool sharded)
      : g_(g), sym_(sym), rank_(rank), world_(world), sharded_(sharded || world > 1) {
    ArenaScope scope(&arena_);
    const bool ctimes = getenv("RR_PGO_ANALYZE_TIMES") != nullptr;   // wall time of the phases of this constructor on stderr
    double ct0 = now_ms();
    auto cmark = [&](const char *what) {
      if (!ctimes) return;
      const double t = now_ms();
      std::fprintf(stderr, "engine:  %-12s %8.3f ms\n", what, t - ct0);
      ct0 = t;
    };
    // the factor storage dominates: one chunk sized for it and the value arrays, tables follow in 8 MB chunks
    arena_.reserve((size_t)(sym.l_elems + sym.u_elems + sym.n_hvals + 8 * (int64_t)g.dim + sym.xch_elems) * sizeof(T) + (4u << 20));
    stream_.failed = &arena_.stream_failed;
    stream_.acquire();
    cmark("stream");
    host_pair_.alloc(4 + OPT_RING * sizeof(OptSlot) / sizeof(double));
    opt_ring_ = reinterpret_cast<OptSlot *>(host_pair_.p + 4);
    cmark("pinned");
    const int N = g.n_nodes(), E = g.n_edges();
    // ---- graph arrays
    is3d_ = g.has_se3;
    has_lm_ = g.has_xyz;
    if (has_lm_ && sharded_)
      throw ApiError(RR_PGO_EUNSUPPORTED, "sharded handle on a graph with XYZ landmarks (the ranks' exchange of SE(3) fronts is not taught the 3-scalar nodes)");
    has_br_ = g.has_br;
    if (has_br_ && sharded_)
      throw ApiError(RR_PGO_EUNSUPPORTED, "sharded handle on a graph with bearing-only or range-only edges (the ranks' linearisation is not taught them)");
    if (has_br_ && getenv("RR_PGO_EDGE_LINEARIZE") != nullptr)
      throw ApiError(RR_PGO_EUNSUPPORTED, "RR_PGO_EDGE_LINEARIZE on a graph with bearing-only or range-only edges (the edge-parallel linearisation forms are not taught them)");
    std::vector<uint8_t> ndim(N);
    for (int i = 0; i < N; i++) ndim[i] = (uint8_t)node_dim(g.node_kind[i]);
    node_dim_.upload(ndim);
    auto edge_slot = [&](int k) { return (int64_t)((sym.blk_off[sym.edge_slot[k]] << 1) | (sym.edge_transposed[k] ? 1 : 0)); };
    {   // states and edges in their device form (the host copies end with the block): one V4 per node, SE(3) a pair; an SE(2)
      // edge is one record, an SE(3) edge an entry of four arrays.
      // The loops are split by dimension and the 2-D ones name their two kinds, so that each compiles to its own forms alone.
      const size_t per = is3d_ ? 2 : 1;
      std::vector<V4> pose(per * (size_t)N);
      if (is3d_ && has_lm_) for (int i = 0; i < N; i++) pack_v4(g.node_kind[i] == NODE_XYZ ? NODE_XYZ : NODE_SE3, &g.node_state[g.node_state_off[i]], &pose[2 * (size_t)i]);
      else if (is3d_) for (int i = 0; i < N; i++) pack_v4(NODE_SE3, &g.node_state[g.node_state_off[i]], &pose[2 * (size_t)i]);
      else for (int i = 0; i < N; i++) pack_v4(g.node_kind[i] == NODE_SE2 ? NODE_SE2 : NODE_XY, &g.node_state[g.node_state_off[i]], &pose[i]);
      pose_.upload(pose);
      if (!is3d_) {
        std::vector<EdgeRec<S>> erec(E);
        for (int k = 0; k < E; k++) {
          EdgeRec<S> &r = erec[k];
          r.from = g.edge_from[k];
          r.to = g.edge_to[k];
          r.slot = edge_slot(k);
          const double *w = &g.edge_info[g.edge_info_off[k]];
          if (g.edge_kind[k] == EDGE_SE2) {
            pack_v4(EDGE_SE2, &g.edge_meas[g.edge_meas_off[k]], &r.meas);
            r.info_a = V4{(S)w[0], (S)w[1], (S)w[2], (S)w[3]};
            r.info_b = V2{(S)w[4], (S)w[5]};
          } else if (has_br_ && edge_is_br(g.edge_kind[k])) {
            // one scalar: the measurement with its kind in lane 3 (pack_meas), omega as W[0][0] of the zero-padded information
            double pm[8];
            pack_meas(g.edge_kind[k], &g.edge_meas[g.edge_meas_off[k]], pm);
            r.meas = V4{(S)pm[0], (S)pm[1], (S)pm[2], (S)pm[3]};
            r.info_a = V4{(S)w[0], (S)0, (S)0, (S)0};
            r.info_b = V2{(S)0, (S)0};
          } else {
            pack_v4(EDGE_SE2_XY, &g.edge_meas[g.edge_meas_off[k]], &r.meas);
            r.info_a = V4{(S)w[0], (S)w[1], (S)0, (S)w[2]};
            r.info_b = V2{(S)0, (S)0};
          }
        }
        e_rec_.upload(erec);
      } else {
        std::vector<int2> eidx(E);
        std::vector<int64_t> eslot(E);
        std::vector<V4> emeas(2 * (size_t)E);
        std::vector<S> einfo(21 * (size_t)E);
        for (int k = 0; k < E; k++) {
          eidx[k] = int2{g.edge_from[k], g.edge_to[k]};
          eslot[k] = edge_slot(k);
          // (an SE3_XYZ edge: the point and a zero V4; its 6 information values in the upper-left 3 x 3 of the 21)
          pack_v4(g.edge_kind[k] == EDGE_SE3_XYZ ? EDGE_SE3_XYZ : EDGE_SE3, &g.edge_meas[g.edge_meas_off[k]], &emeas[2 * (size_t)k]);
          pack_info_3d<S>(g.edge_kind[k], &g.edge_info[g.edge_info_off[k]], &einfo[21 * (size_t)k]);
        }
        e_idx_.upload(eidx);
        e_slot_.upload(eslot);
        e_meas_.upload(emeas);
        e_info3_.upload(einfo);
      }
    }
    std::vector<int2> inc(sym.inc_list.size());
    if (E >= (1 << 27)) throw ApiError(RR_PGO_EUNSUPPORTED, "more than 2^27 edges");
    for (size_t q = 0; q < inc.size(); q++) {
      int k = sym.inc_list[q] >> 1, role = sym.inc_list[q] & 1;
      // Sharded runs: an edge's contributions to diagonal blocks, right-hand side and chi2 are computed by ONE
      // rank, its owner = the rank of its from-node, else of its to-node, else (both shared) rank 0 -- only
      // the owner is sure to hold current poses of both endpoints.  The off-diagonal block of an edge between
      // two shared nodes is needed (and computable) on every rank.
      const int pf = world_ > 1 ? sym.node_part[g.edge_from[k]] : 0, pt = world_ > 1 ? sym.node_part[g.edge_to[k]] : 0;
      const int owns = (pf >= 0 ? pf : pt >= 0 ? pt : 0) == rank_ ? 1 : 0;
      const int offd = role == 0 && (owns || (pf < 0 && pt < 0)) ? 1 : 0;
      inc[q] = int2{(k << 4) | (offd << 3) | (owns << 2) | ((g.edge_kind[k] == EDGE_SE2_XY || g.edge_kind[k] == EDGE_SE3_XYZ || edge_is_br(g.edge_kind[k]) ? 1 : 0) << 1) | role,
                    role ? g.edge_from[k] : g.edge_to[k]};
    }
    inc_ptr_.upload(sym.inc_ptr);
    inc_list_.upload(inc);
    node_offset_.upload(g.node_offset);
    node_pcol_.upload(sym.node_pcol);
    diag_off_.upload(sym.diag_off);
    cmark("graph arrays");
    // ---- numeric buffers
    hvals_.alloc((size_t)sym.n_hvals);
    hvals_.zero();
    b_.alloc((size_t)g.dim);
    x_.alloc((size_t)g.dim);
    dx_ref_.alloc((size_t)g.dim);
    b_.zero(); x_.zero(); dx_ref_.zero();
    x_ptr_ = x_.p;
    n_list_ = N;
    if (sharded_) {
      xch_n_ = std::max<int64_t>(sym.xch_elems, 64 * (int64_t)world_);
      xch_own_.alloc((size_t)xch_n_ + 4);
      xch_own_.zero();
      xch_ = xch_own_.p;
      scal_own_.alloc(2);
      scal_own_.zero();
      scal_ = scal_own_.p;
    }
    if (world_ > 1) {
      std::vector<int32_t> nl;
      std::vector<uint8_t> nc(N);
      std::vector<int64_t> sh;   // the shared nodes' diagonal blocks (offset in hvals) and rhs entries (~offset in b)
      for (int i = 0; i < N; i++) {
        const int pt = sym.node_part[i];
        if (pt == rank_ || pt < 0) nl.push_back(i);
        nc[i] = (pt == rank_ || (pt < 0 && rank_ == 0)) ? 1 : 0;
        if (pt < 0) {
          const int d = node_dim(g.node_kind[i]);
          for (int t = 0; t < d * d; t++) sh.push_back(sym.diag_off[i] + t);
          for (int t = 0; t < d; t++) sh.push_back(~(int64_t)(g.node_offset[i] + t));
        }
      }
      n_list_ = (int)nl.size();
      node_list_.upload(nl);
      norm_counts_.upload(nc);
      n_shared_ = (int)sh.size();
      if (sym.xch_shared_off + n_shared_ > sym.xch_chunk) throw ApiError(RR_PGO_EINVAL, "internal: exchange chunk too small");
      shared_src_.upload(sh);
      std::vector<int64_t> pl;
      for (int f = 0; f < sym.S; f++)
        if (sym.sn_xch_off[f] >= 0 && sym.sn_big[f] && sym.sn_owner[f] == rank_) {
          pl.push_back(f);
          pl.push_back(sym.sn_xch_off[f]);
          pack_max_nu_ = std::max(pack_max_nu_, sym.sn_nrows[f] + 1);
        }
      n_pack_ = (int)pl.size() / 2;
      pack_list_.upload(pl);
    }
    setup_gauge();
    lvals_.alloc((size_t)sym.l_elems + 4);
    uvals_.alloc((size_t)sym.u_elems + 4);
    lvals_.zero(); uvals_.zero();
    {
      bool any_big = false;
      for (const Step &st : sym.steps) any_big = any_big || st.kind != STEP_TASKS;
      gemv_part_.alloc(any_big ? (size_t)kGemvSlices * g.dim : 4);
    }
    if (const char *e = getenv("RR_PGO_SOLVE_THREADS")) solve_threads_max_ = std::atoi(e);
    if (const char *e = getenv("RR_PGO_SP_SOLVE_MIN")) sp_solve_min_nc_ = std::atoi(e);
    if (const char *e = getenv("RR_PGO_SCHUR_SPLIT")) schur_split_ = std::atoi(e) != 0;
    no_graph_ = getenv("RR_PGO_NO_GRAPH") != nullptr;
    force_graph_ = getenv("RR_PGO_FORCE_GRAPH") != nullptr && !no_graph_;
    if (const char *e = getenv("RR_PGO_FLOW")) flow_max_nf_ = std::atoi(e);
    if (const char *e = getenv("RR_PGO_FLOW_EXACT")) flow_exact_ = std::atoi(e) != 0;
    if (const char *e = getenv("RR_PGO_FLOW_TASKS")) flow_max_tasks_ = std::atoi(e);
    if (const char *e = getenv("RR_PGO_SOLVE_FLOW")) solve_flow_on_ = std::atoi(e) != 0;
    if (const char *e = getenv("RR_PGO_FLOW_SCHUR_MIN")) flow_schur_min_ = std::atoi(e);
    if (const char *e = getenv("RR_PGO_TS_WS_BYTES"))
      if (const long long v = std::atoll(e); v > 0) ts_ws_bytes_ = (size_t)v;
    if (const char *e = getenv("RR_PGO_QUERY_TRACE")) ts_trace_ = std::atoi(e) != 0;
    n_lin_blocks_ = (int)(((int64_t)n_list_ * LIN_GROUP + LIN_THREADS - 1) / LIN_THREADS);
    lin_blocks_pull_ = n_lin_blocks_;
    edge_lin_ = getenv("RR_PGO_EDGE_LINEARIZE") != nullptr && !is3d_ && !sharded_ && g_.n_edges() > 0;
    edge_lin_wave_ = edge_lin_ && std::atoi(getenv("RR_PGO_EDGE_LINEARIZE")) == 2;
    if (edge_lin_) n_lin_blocks_ = std::max(1, (g_.n_edges() + (edge_lin_wave_ ? WE_EDGES : LIN_THREADS) - 1) / (edge_lin_wave_ ? WE_EDGES : LIN_THREADS));
    edge_lin_env_ = edge_lin_;
    edge_lin_wave_env_ = edge_lin_wave_;
    lin_blocks_edge_ = n_lin_blocks_;
    n_upd_blocks_ = (n_list_ + UPD_THREADS - 1) / UPD_THREADS;
    chi_partial_.alloc((size_t)(edge_lin_ ? std::max(lin_blocks_pull_, lin_blocks_edge_) : n_lin_blocks_));   // (a robust kernel switches to the pull form)
    norm_partial_.alloc((size_t)n_upd_blocks_);
    hist_.alloc(2 * HIST);
    hist_.zero();
    counter_.alloc(1);
    counter_.zero();
    err_.alloc(2);   // [0] sticky error flag, [1] stop word of the running rr_pgo_optimize call (kernels.hip.h, OptCtrl)
    err_.zero();
    opt_ctrl_.alloc(1);
    opt_ctrl_.zero();
    sync_optimize_ = getenv("RR_PGO_SYNC_OPTIMIZE") != nullptr;
    blocks_done_.alloc(2);   // [0] k_update's last-workgroup counter, [1] k_linearize's
    blocks_done_.zero();
    cmark("numeric");
    // ---- symbolic tables
    task_ptr_.upload(sym.task_ptr);
    task_sn_.upload(sym.task_sn);
    {
      std::vector<SnMeta> meta(sym.S);
      std::vector<ChildMeta> cm(sym.child_list.size());
      int64_t wblk_total = 0;
      for (int f = 0; f < sym.S; f++) {
        SnMeta &m = meta[f];
        m.nc = sym.sn_ncols[f];
        m.nr = sym.sn_nrows[f];
        m.col0 = sym.sn_col0[f];
        m.uld = sym.sn_uld[f];
        m.asm_begin = (int32_t)sym.fasm_ptr[f];
        m.asm_count = (int32_t)(sym.fasm_ptr[f + 1] - sym.fasm_ptr[f]);
        m.dup_begin = (int32_t)sym.fdup_ptr[f];
        m.dup_count = (int32_t)(sym.fdup_ptr[f + 1] - sym.fdup_ptr[f]);
        m.child_begin = sym.child_ptr[f];
        m.child_count = sym.child_ptr[f + 1] - sym.child_ptr[f];
        if (sym.sn_rows_ptr[f] > 0x7fffffffLL) throw ApiError(RR_PGO_EUNSUPPORTED, "row structure exceeds 32-bit indexing");
        m.rows_ptr = (int32_t)sym.sn_rows_ptr[f];
        m.wblk = (int32_t)wblk_total;
        // 16 x 16 blocks per 16 columns; the 32-column block kernels of the big fronts keep 32 x 32 per 32 columns
        wblk_total += sym.sn_big[f] ? 4 * ((sym.sn_ncols[f] + 31) / 32) : (sym.sn_ncols[f] + 15) / 16;
        m.loff = sym.sn_loff[f];
        m.uoff = sym.sn_uoff[f];
        if (sym.sn_xch_off[f] >= 0 && !sym.sn_big[f]) {   // LDS boundary front: writes straight into the exchange buffer
          m.uld = -1;
          m.uoff = sym.sn_xch_off[f];
        }
      }
      for (size_t q = 0; q < cm.size(); q++) {
        const int c = sym.child_list[q];
        cm[q].uoff = sym.sn_uoff[c];
        cm[q].scat_ptr = sym.scat_ptr[c];
        cm[q].rel_ptr = sym.rel_ptr[c];
        cm[q].ncu = sym.sn_nrows[c] + 1;
        cm[q].uld = sym.sn_uld[c];
        if (sym.sn_xch_off[c] >= 0) {   // boundary child: every rank reads it from the (all-reduced) exchange buffer
          cm[q].uld = -1;
          cm[q].uoff = sym.sn_xch_off[c];
        }
      }
      sn_meta_.upload(meta);
      host_sn_meta_ = meta;
      {
        std::vector<SnMeta> tm(sym.task_ptr.size() - 1);
        for (size_t t = 0; t + 1 < sym.task_ptr.size(); t++) tm[t] = meta[sym.task_sn[sym.task_ptr[t]]];
        task_meta_.upload(tm);
        host_task_meta_ = tm;
        // k_big_panel32 / k_big_update / k_big_flow address a front with 32-bit BYTE offsets from its base
        for (const Step &st : sym.steps)
          if (st.kind == STEP_BIG)
            for (int t = st.task_begin; t < st.task_end; t++) {
              const int sn = sym.task_sn[sym.task_ptr[t]];
              const int64_t Mf = sym.sn_ncols[sn] + sym.sn_nrows[sn] + 1;
              if (Mf * Mf * (int64_t)sizeof(T) >= (1LL << 32))
                throw ApiError(RR_PGO_EUNSUPPORTED, "a front of more than 4 GiB exceeds the 32-bit addressing of the big-front kernels");
            }
      }
      if (wblk_total > 0x7fffff00LL) throw ApiError(RR_PGO_EUNSUPPORTED, "too many diagonal blocks");
      winv_.alloc((size_t)wblk_total * 256 + 4);
      winv_.zero();
      kform_ = sym.flow_eligible && !sharded_ && world_ <= 1;
      if (const char *e = getenv("RR_PGO_SOLVE_KFORM")) kform_ = kform_ && std::atoi(e) != 0;
      if (kform_) {
        int64_t kend = 0;
        for (int f = 0; f < sym.S; f++)
          if (!sym.sn_big[f] && sym.sn_nrows[f] > 0) {
            const double nc = sym.sn_ncols[f], nu = sym.sn_nrows[f] + 1;
            kend = std::max<int64_t>(kend, sym.sn_loff[f] + (int64_t)(nc + nu) * sym.sn_ncols[f]);
            kform_bytes_ += (nc * (nc + 1) / 2 + 2 * nu * nc) * sizeof(T);   // L11, then B read and X written once each
            kform_flops_ += nu * nc * nc;                                    // X = B L11^-1: nu nc^2 / 2 multiply-adds
          }
        kvals_.alloc((size_t)kend + 4);
        kvals_.zero();
      }
      {
        bool any_big = false;
        for (const Step &st : sym.steps) any_big = any_big || st.kind == STEP_BIG;
        xnew_.alloc(any_big ? (size_t)wblk_total * 256 + 4 : 4);   // the chain waves' X blocks of the flow fronts (laid out like winv; flow.hip.h)
        xnew_.zero();
      }
      child_meta_.upload(cm);
      if (sizeof(T) != 8)   // the fp32 kernels add every child before the panel (kernels.hip.h, process_front)
        for (int32_t d : sym.child_due)
          if (d != 0) throw ApiError(RR_PGO_EUNSUPPORTED, "internal: a due block in a handle with an fp32 factor");
      child_due_.upload(sym.child_due);
      if (const char *e = getenv("RR_PGO_FLOW_TIMEOUT_MS")) wait_ticks_ = (unsigned long long)std::max(1.0, std::atof(e) * 1e5);
      if (sym.lds_flow) {
        // dataflow launches of the LDS fronts: who waits for whom (a dependency inside one task needs no flag), and
        // one 128-byte record per ticket
        if (sharded_ || world_ > 1) throw ApiError(RR_PGO_EUNSUPPORTED, "internal: dataflow schedule on a sharded handle");
        lds_flow_ = true;
        // (the dataflow step is step 0: every LDS front; fronts beyond LDS follow level by level as STEP_BIG steps)
        if (sym.steps.empty() || sym.steps[0].kind != STEP_TASKS || sym.steps[0].task_begin != 0)
          throw ApiError(RR_PGO_EUNSUPPORTED, "internal: the dataflow step must come first");
        for (size_t si = 1; si < sym.steps.size(); si++)
          if (sym.steps[si].kind != STEP_BIG) throw ApiError(RR_PGO_EUNSUPPORTED, "internal: a second LDS step behind the dataflow step");
        const int nt = sym.steps[0].task_end;
        std::vector<int32_t> task_of(sym.S, -1);
        for (size_t t = 0; t + 1 < sym.task_ptr.size(); t++)
          for (int q = sym.task_ptr[t]; q < sym.task_ptr[t + 1]; q++) task_of[sym.task_sn[q]] = (int)t;
        host_child_dep_.assign(cm.size(), -1);
        std::vector<int32_t> pdep(sym.S, -1);
        for (int f = 0; f < sym.S; f++) {
          for (int q = sym.child_ptr[f]; q < sym.child_ptr[f + 1]; q++) {
            const int c = sym.child_list[q];
            if (task_of[c] != task_of[f]) host_child_dep_[q] = c;
            else if (c > f) throw ApiError(RR_PGO_EUNSUPPORTED, "internal: child after its parent in one task");
          }
          const int pf = sym.sn_parent[f];
          if (pf >= 0 && !sym.sn_big[pf] && task_of[pf] != task_of[f]) pdep[f] = sym.S + pf;   // (a parent beyond LDS was solved by an earlier launch)
        }
        child_dep_.upload(host_child_dep_);
        parent_dep_.upload(pdep);
        dep_flags_.alloc((size_t)2 * sym.S + 128);
        dep_flags_.zero();
        std::vector<LdsFlowTask> ft(nt), stk(nt);
        for (int t = 0; t < nt; t++) {
          LdsFlowTask r{};
          r.sn_begin = sym.task_ptr[t];
          r.sn_end = sym.task_ptr[t + 1];
          r.sn = sym.task_sn[r.sn_begin];
          r.m = meta[r.sn];
          ft[t] = r;
        }
        if ((int)sym.solve_order.size() != nt) throw ApiError(RR_PGO_EUNSUPPORTED, "internal: solve order of the dataflow schedule");
        for (int k = 0; k < nt; k++) {
          LdsFlowTask r = ft[sym.solve_order[k]];
          r.sn = sym.task_sn[r.sn_end - 1];
          r.m = meta[r.sn];
          stk[k] = r;
        }
        lds_ftasks_.upload(ft);
        host_stasks_ = std::move(stk);   // uploaded by plan_mid_solve_tasks (fronts beyond LDS may join the list)
        lds_n_tasks_ = nt;
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        (void)hipDeviceGetAttribute(&lds_flow_cus_, hipDeviceAttributeMultiprocessorCount, dev);
        lds_flow_cus_ = std::max(lds_flow_cus_, 1);
        if (const char *e = getenv("RR_PGO_LDS_FLOW_GRID")) lds_flow_cus_ = std::max(1, std::atoi(e));   // workgroups of the two dataflow launches (experiments)
      }
    }
    cmark("front tables");
    plan_shapes();
    build_flow_levels();   // (after the front records: every flow task carries a copy of its front's)
    build_update_maps();
    cmark("flow levels");
    fasm_src_.upload(sym.fasm_src);
    fasm_dst_.upload(sym.fasm_dst);
    fasm_colptr_.upload(sym.fasm_colptr);
    fdup_src_.upload(sym.fdup_src);
    fdup_dst_.upload(sym.fdup_dst);
    scat_.upload(sym.scat);
    rel_.upload(sym.rel);
    perm_.upload(sym.perm);
    sn_rows_.upload(sym.sn_rows);
    for (size_t si = 0; si < sym.steps.size(); si++) {
      const Step &st = sym.steps[si];
      int need = 0;
      if (st.kind == STEP_MID) throw ApiError(RR_PGO_EUNSUPPORTED, "internal: the panel-in-LDS step class has no kernel (SymbolicOptions::panel_budget_elems must be 0)");
      if (st.kind == STEP_TASKS) {
        for (int t = st.task_begin; t < st.task_end; t++)
          for (int q = sym.task_ptr[t]; q < sym.task_ptr[t + 1]; q++) {
            int s = sym.task_sn[q], nc = sym.sn_ncols[s], nr = sym.sn_nrows[s];
            if (nc > 256) throw ApiError(RR_PGO_EUNSUPPORTED, "internal: LDS-path supernode wider than 256 columns");
            // x[rows] and t, padded as solve_front lays them out; k_solve_flow adds an LDS image of L11 where it fits
            const int ncp = (nc + 15) / 16 * 16, base = ((nr + 15) & ~15) + ncp + 2;
            const int cap = (int)((size_t)kMaxLds / sizeof(T));
            const bool image = sym.lds_flow && si == 0;
            need = std::max(need, image && base + ncp * (ncp + 1) <= cap ? base + ncp * (ncp + 1) : base + ncp / 16 * (2 * 16 * 17));
          }
      } else {
        for (int t = st.task_begin; t < st.task_end; t++) {
          int s = sym.task_sn[sym.task_ptr[t]];
          need = std::max(need, sym.sn_ncols[s] + sym.sn_nrows[s] + 64 * 65 + 4);
        }
      }
      if ((size_t)need * sizeof(T) > (size_t)kMaxLds) throw ApiError(RR_PGO_EUNSUPPORTED, "front too large for the back-substitution scratch");
      plan_[si].solve_lds = need;
    }
#ifdef RRPGO_STAMPS
    stamps_.alloc((size_t)sym.S * 12 + 400000);   // per-front phase stamps | launch trace
    stamps_.zero();
#endif
    plan_mid_solve_tasks();
    plan_launches();
    cmark("index tables");
    configure_kernels();
    cmark("kernel attrs");
    // linearise and update, every step's launches; the cross-level form factors all the big levels in one launch
    n_launches_per_iter = 2 + (xl_ ? 1 : 0);
    for (const StepPlan &p : plan_) n_launches_per_iter += (xl_ && p.kind == STEP_BIG ? 0 : factor_launches(p)) + solve_launches(p);
  }

  ~Engine() override { drop_graphs(); }   // streams, events and the pinned buffer release themselves

  hipStream_t stream() override { return stream_; }

 private:
  // ---- k_big_flow, host side: the task list of every level that runs as a dataflow launch.
  // Tasks and their dependencies are those flow.hip.h waits for; the list is sorted by the earliest start time a
  // task can have under a simple cost model with unlimited workgroups (us; the constants are the r02 in-kernel marks).
  // A dependency always FINISHES (so also starts) before its dependant starts, hence the sorted list is a topological
  // order -- all the ticket scheme needs -- and roughly the order in which tasks become ready.
  void build_flow_levels() {
    for (StepPlan &p : plan_) { p.flow.reset(); p.solve_flow.reset(); }
    constexpr double kDiag = 4.0, kPre = 2.5, kNewest = 1.5, kX = 1.5, kLook = 4.5, kTile = 8.0, kTail = 4.5, kHop = 0.7;
    int64_t words = 0;
    int dev = 0, cus = 256;
    HIPCHK(hipGetDevice(&dev));
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    flow_grid_ = std::max(cus, 1) * (sizeof(T) == 4 ? RRPGO_FLOW_WAVES : 1);
    if (const char *e = getenv("RR_PGO_FLOW_GRID")) flow_grid_ = std::max(1, std::atoi(e));
    {
      // the cross-level form: every front beyond LDS sits above the LDS fronts (the dataflow schedule's condition), few of them,
      // none with parallel-edge blocks (k_big_assemble_dup has no task form), no gauge term on the root, default flow limits
      if (const char *e = getenv("RR_PGO_FLOW_XL")) xl_max_fronts_ = std::atoi(e);
      int n_big = 0;
      bool dup = false;
      for (const Step &st : sym_.steps)
        if (st.kind == STEP_BIG)
          for (int t = st.task_begin; t < st.task_end; t++) {
            const int sn = sym_.task_sn[sym_.task_ptr[t]];
            n_big++;
            dup = dup || sym_.fdup_ptr[sn + 1] > sym_.fdup_ptr[sn];
          }
      xl_ = lds_flow_ && !sharded_ && world_ == 1 && gather_update_ && fused_assembly_ && !gauge_ok_ && !dup && n_big > 0 && n_big <= xl_max_fronts_ &&
            flow_max_nf_ >= (1 << 20) && flow_max_tasks_ >= (1 << 20) && !xl_refused_;
      if (const char *e = getenv("RR_PGO_FLOW_XL_TASKS")) xl_level_tasks_ = std::atoi(e);
    }
    // first W block of every supernode in winv (as the SnMeta table lays them out), for the marks k_flow_reset writes
    std::vector<int64_t> sn_wblk(sym_.S + 1, 0);
    for (int f = 0; f < sym_.S; f++)
      sn_wblk[f + 1] = sn_wblk[f] + (sym_.sn_big[f] ? 4 * ((sym_.sn_ncols[f] + 31) / 32) : (sym_.sn_ncols[f] + 15) / 16);
    std::vector<int64_t> wfill;
    std::vector<std::vector<FlowTask>> all_tasks(sym_.steps.size());
    std::vector<std::vector<FlowFront>> all_fronts(sym_.steps.size());
    for (size_t si = 0; si < sym_.steps.size(); si++) {
      const Step &st = sym_.steps[si];
      const int nf = st.task_end - st.task_begin;
      if (st.kind != STEP_BIG || nf > flow_max_nf_ || flow_max_nf_ <= 0) continue;
      auto lvl = std::make_unique<FlowLevel>();
      lvl->ticket_word = words;
      // The Schur complements of the level's fronts: as UPDATE tiles of this launch (one per super-panel), or left to ONE
      // k_big_schur launch behind it (K = nc, six workgroups per CU, MfmaUtil 52 - 55 % on the lattice's levels of 4 ... 32
      // fronts).  In the launch they cost twice the workgroup time, but at the top of the tree the launch is
      // bound by its chain and most workgroups idle: the tiles stay in when the list schedule says they fit into 60 % of
      // that idle time (lattice: the level of 2 fronts, -60 us; the level of 4 fronts would lose 70 us)
      int64_t schur_tiles = 0;
      double schur_in_flow_us = 0;   // workgroup time of the Schur tiles as UPDATE tasks
      for (int z = 0; z < nf; z++) {
        const int sn = sym_.task_sn[sym_.task_ptr[st.task_begin + z]];
        const int nc = sym_.sn_ncols[sn], M = nc + sym_.sn_nrows[sn] + 1, o = big_schur_origin(nc, schur_tile_);
        if (o < M) {
          const int64_t nt = (M - o + 63) / 64;
          schur_tiles += nt * (nt + 1) / 2;
          schur_in_flow_us += (double)(nt * (nt + 1) / 2) * ((nc + BIG_SUPER - 1) / BIG_SUPER) * kTile;
        }
      }
      lvl->schur_split = schur_split_ && schur_tiles >= flow_schur_min_;
      if (xl_) lvl->schur_split = false;   // one launch: the Schur complements are UPDATE tasks
      std::vector<FlowTask> tasks;
      std::vector<FlowFront> fronts(nf);
      double level_end = 0, busy_us = 0;
      bool too_many = false;
      auto plan = [&]() {
      tasks.clear();
      level_end = busy_us = 0;
      // The level's tasks in their natural order (front by front, step by step), each with the flags it waits for and the
      // flags it sets. The ticket order is then the START order of a list schedule of this DAG on the launch's workgroups
      // (priority: longest remaining path), so that a workgroup drawing the next ticket finds what the schedule would
      // have given it: the next chain step of a front ahead of the bulk of the previous super-panel's far tiles.
      struct Gen {
        FlowTask t;
        int need0, need1, prod0, prod1;
        int wflag;             // the W flag a PANEL task waits for after its pre-work, or -1
        float pre, newest;     // PANEL: work on the older blocks / on the newest block, both before W is needed
        float dur;             // W there (or start) -> workgroup free
        float blevel;
      };
      struct Need { int flag, cls; };          // cls 0: needed at the start; 1: the newest block's X (after `pre`)
      struct Prod { int flag; float off; };    // set `off` after W arrived (or after the start)
      std::vector<Gen> gen;
      std::vector<Need> need;
      std::vector<Prod> prod;
      constexpr int TS = 64;           // edge of a trailing-update tile (k_big_flow<T, 2>)
      words = lvl->ticket_word + 32;   // the ticket on a 128-byte line of its own
      const int64_t flag0 = words;
      for (int z = 0; z < nf; z++) {
        const int sn = sym_.task_sn[sym_.task_ptr[st.task_begin + z]];
        const int nc = sym_.sn_ncols[sn], M = nc + sym_.sn_nrows[sn] + 1;
        const int nblk = (nc + BIG_NB - 1) / BIG_NB, nsp = (nc + BIG_SUPER - 1) / BIG_SUPER;
        const int pstride = (M + 31) / 32 + 1;
        const int ntmax = (M + TS - 1) / TS + 1, ustride = ntmax * (ntmax + 1) / 2;
        FlowFront &ff = fronts[z];
        ff.wf = (int32_t)words; words += nblk + 1;
        ff.pf = (int32_t)words; ff.pstride = pstride; words += (int64_t)nblk * pstride;
        ff.uf = (int32_t)words; ff.ustride = ustride; words += (int64_t)nsp * ustride;
        ff.bf = -1; ff.nbuild = 0; ff.done = -1;
        if (xl_) {   // build counter + "built" flag, and the counter of finished UPDATE tasks, on a line of their own
          words = (words + 31) & ~(int64_t)31;
          ff.bf = (int32_t)words; ff.done = (int32_t)words + 2; words += 3;
          ff.nbuild = (big_built_cols(nc, M) + FLOW_BUILD_COLS - 1) / FLOW_BUILD_COLS;
        }
        words = (words + 31) & ~(int64_t)31;
        if (words > 0x7fffff00LL) throw ApiError(RR_PGO_EUNSUPPORTED, "too many flow flags");
        const int wf = (int)(ff.wf - flag0), pf = (int)(ff.pf - flag0), uf = (int)(ff.uf - flag0);
        auto tri = [](int bx, int by) { return bx * (bx + 1) / 2 + by; };
        auto open_task = [&](FlowTask t) {
          gen.push_back(Gen{t, (int)need.size(), 0, (int)prod.size(), 0, -1, 0.f, 0.f, 0.f, 0.f});
        };
        auto close_task = [&]() { gen.back().need1 = (int)need.size(); gen.back().prod1 = (int)prod.size(); };
        open_task(FlowTask{(FLOW_DIAG0 << 24) | z, 0, 0, 0});
        prod.push_back(Prod{wf + 0, (float)kDiag});
        gen.back().dur = (float)kDiag;
        close_task();
        const int o_schur = lvl->schur_split ? std::min(big_schur_origin(nc, schur_tile_), M) : M;   // UPDATE tiles start left of it
        // fast mode: the first two blocks of a super-panel look back over the previous super-panel too, and that one's
        // update skips these 64 columns (its tile column 0) -- the chain does not wait for a tile at a super-panel's end
        auto deep = [&](int spx) { return flow_deep_ && !flow_exact_ && spx > 0 && spx * BIG_SUPER + 64 <= nc; };
        for (int sp = 0; sp < nsp; sp++) {
          const int K0 = sp * BIG_SUPER, ke = std::min(K0 + BIG_SUPER, nc);
          // the tiles under rows [r0, r1] x columns [c0, c1] of the update whose tile grid starts at column Ko (the update
          // before a left-looking range that starts there); tiles right of the Schur origin are not this launch's
          auto prev_tiles = [&](int Ko, int r0, int r1, int c0, int c1, int cls) {
            if (Ko <= 0) return;
            const int spo = Ko / BIG_SUPER - 1;
            for (int bx = (r0 - Ko) / TS; bx <= (std::min(r1, M - 1) - Ko) / TS; bx++)
              for (int by = (c0 - Ko) / TS; by <= std::min((std::min(c1, M - 1) - Ko) / TS, bx); by++)
                if (Ko + TS * by < o_schur && !(by == 0 && deep(spo + 1))) need.push_back(Need{uf + spo * ustride + tri(bx, by), cls});
          };
          for (int kb = K0; kb < ke; kb += BIG_NB) {
            const int blk = kb / BIG_NB, qb = (kb - K0) / BIG_NB, nb = std::min(BIG_NB, nc - kb), kn = kb + BIG_NB;
            const int Ks = deep(sp) && qb < 2 ? K0 - BIG_SUPER : K0;   // first column of the step's left-looking range
            const int q = (kb - Ks) / BIG_NB;
            const int skip = deep(sp) && qb == 1 ? BIG_SUPER / BIG_NB : 0;   // the NEXT diagonal block's range starts that many blocks later
            const int nrb = (M - (kb + nb) + 31) / 32;
            for (int g0 = 0; g0 < nrb; g0 += FLOW_GROUP) {
              open_task(FlowTask{(FLOW_PANEL << 24) | z, kb, g0, Ks | (skip << 24)});
              Gen &g = gen.back();
              g.wflag = wf + blk;
              g.pre = (float)(q > 1 ? kPre * (q - 1) * 0.5 : 0.5);
              g.newest = (float)(q > 0 ? kNewest : 0.0);
              g.dur = (float)kX;
              for (int w = 0; w < FLOW_GROUP && g0 + w < nrb; w++) {
                const int rb = g0 + w, R0 = kb + nb + 32 * rb;
                const bool look = rb == 0 && kn < (flow_exact_ ? ke : nc);
                // a wave starts with everything that needs neither W nor the newest block (the older blocks and the C
                // tiles), then the newest block's term, then W, then X; the look wave goes on with the next block
                for (int j = 1; j <= q; j++) {
                  const int r0p = kb - 32 * j + 32;
                  need.push_back(Need{pf + (blk - j) * pstride + (j - 1), j == 1});
                  for (int rbp = (R0 - r0p) / 32; rbp <= (std::min(R0 + 31, M - 1) - r0p) / 32; rbp++)
                    need.push_back(Need{pf + (blk - j) * pstride + rbp, j == 1});
                }
                prev_tiles(Ks, R0, R0 + 31, kb, kb + nb - 1, 0);
                if (look) prev_tiles(Ks + BIG_NB * skip, kn, kn + 31, kn, kn + 31, 0);
                prod.push_back(Prod{pf + blk * pstride + rb, (float)kX});   // X is published before the look wave goes on
                if (look) { prod.push_back(Prod{wf + blk + 1, (float)(kX + kLook)}); g.dur = (float)(kX + kLook); }
              }
              close_task();
            }
          }
          // trailing update of the super-panel: tiles of rows / columns >= ke
          const int t0 = ke;
          const int nt = (M - t0 + TS - 1) / TS;
          for (int by = deep(sp + 1) ? 1 : 0; by < nt; by++)       // column-major: the next super-panel's own columns first
            for (int bx = by; bx < nt; bx++) {
              const int I0 = t0 + TS * bx, J0 = t0 + TS * by;
              if (J0 >= o_schur) continue;       // the Schur complement: one k_big_schur launch behind the flow launch
              open_task(FlowTask{(FLOW_UPDATE << 24) | z, K0, bx, by});
              for (int kb = K0; kb < ke; kb += BIG_NB) {
                const int nbq = std::min(BIG_NB, nc - kb), r0 = kb + nbq;
                for (int strip = 0; strip < 2; strip++) {
                  const int lo = strip ? J0 : I0, hi = std::min(lo + TS - 1, M - 1);
                  for (int rb = (lo - r0) / 32; rb <= (hi - r0) / 32; rb++) need.push_back(Need{pf + (kb / BIG_NB) * pstride + rb, 0});
                }
              }
              prev_tiles(K0, I0, I0 + TS - 1, J0, J0 + TS - 1, 0);
              prod.push_back(Prod{uf + sp * ustride + tri(bx, by), (float)kTile});
              gen.back().dur = (float)kTile;
              if (flow_exact_ && bx == 0 && by == 0 && t0 < nc) {
                prod.push_back(Prod{wf + t0 / BIG_NB, (float)(kTile + kTail)});
                gen.back().dur = (float)(kTile + kTail);
              }
              close_task();
            }
        }
      }
      const int n_gen = (int)gen.size();
      if (n_gen > (xl_ ? std::min(flow_max_tasks_, xl_level_tasks_) : flow_max_tasks_)) { too_many = true; return; }
      const int n_flags = (int)(words - flag0);
      // who sets a flag, who waits for it
      std::vector<int> producer(n_flags, -1), cons_ptr(n_flags + 1, 0), cons;
      for (int i = 0; i < n_gen; i++)
        for (int k = gen[i].prod0; k < gen[i].prod1; k++) producer[prod[k].flag] = i;
      auto for_each_need = [&](int i, auto &&fn) {   // (flag, lead): lead = how long after the task's start the flag is needed
        const Gen &g = gen[i];
        for (int k = g.need0; k < g.need1; k++) fn(need[k].flag, need[k].cls ? g.pre : 0.f);
        if (g.wflag >= 0) fn(g.wflag, g.pre + g.newest);
      };
      for (int i = 0; i < n_gen; i++) for_each_need(i, [&](int f, float) { cons_ptr[f + 1]++; });
      for (int f = 0; f < n_flags; f++) cons_ptr[f + 1] += cons_ptr[f];
      cons.resize(cons_ptr[n_flags]);
      {
        std::vector<int> fill(cons_ptr.begin(), cons_ptr.end() - 1);
        for (int i = 0; i < n_gen; i++) for_each_need(i, [&](int f, float) { cons[fill[f]++] = i; });
      }
      // longest remaining path of every task (its consumers come later in the natural order)
      {
        std::vector<float> after(n_flags, 0.f);   // per flag: the longest path that starts when it is set
        for (int i = n_gen - 1; i >= 0; i--) {
          Gen &g = gen[i];
          const float lead = g.pre + g.newest;
          float bl = lead + g.dur;
          for (int k = g.prod0; k < g.prod1; k++) bl = std::max(bl, lead + prod[k].off + after[prod[k].flag]);
          g.blevel = bl;
          for_each_need(i, [&](int f, float ld) { after[f] = std::max(after[f], (float)kHop + bl - ld); });
        }
      }
      // the list schedule
      tasks.reserve(n_gen);
      {
        // half the launch's workgroups: the model's tiles are cheaper than loaded ones, and a chain step drawn a little
        // early only waits, while one drawn late stalls its front (measured: 128 ... 256 slots equal, 512 1 % slower)
        int P = std::max(1, flow_grid_ / 2);
        std::vector<float> ftime(n_flags, 0.f);
        std::vector<int> pending(n_gen, 0);
        for (int i = 0; i < n_gen; i++) for_each_need(i, [&](int f, float) { if (producer[f] >= 0) pending[i]++; });
        using Fut = std::pair<float, int>;                 // (earliest useful start, task)
        std::priority_queue<Fut, std::vector<Fut>, std::greater<Fut>> future;
        auto less_urgent = [&](int x, int y) { return gen[x].blevel != gen[y].blevel ? gen[x].blevel < gen[y].blevel : x > y; };
        std::priority_queue<int, std::vector<int>, decltype(less_urgent)> ready(less_urgent);
        std::priority_queue<float, std::vector<float>, std::greater<float>> slots;
        for (int k = 0; k < P; k++) slots.push(0.f);
        auto becomes_known = [&](int i) {
          float r = 0.f;
          for_each_need(i, [&](int f, float ld) { if (producer[f] >= 0) r = std::max(r, ftime[f] + (float)kHop - ld); });
          future.push(Fut{r, i});
        };
        for (int i = 0; i < n_gen; i++) if (pending[i] == 0) becomes_known(i);
        float now = 0.f;
        for (int done = 0; done < n_gen; done++) {
          now = std::max(now, slots.top());
          while (!future.empty() && future.top().first <= now) { ready.push(future.top().second); future.pop(); }
          if (ready.empty()) {
            if (future.empty()) throw ApiError(RR_PGO_EUNSUPPORTED, "flow task graph is not schedulable");
            now = future.top().first;
            while (!future.empty() && future.top().first <= now) { ready.push(future.top().second); future.pop(); }
          }
          const int i = ready.top();
          ready.pop();
          slots.pop();
          const Gen &g = gen[i];
          float t_new = 0.f, t_w = 0.f;
          for (int k = g.need0; k < g.need1; k++)
            if (need[k].cls && producer[need[k].flag] >= 0) t_new = std::max(t_new, ftime[need[k].flag] + (float)kHop);
          if (g.wflag >= 0 && producer[g.wflag] >= 0) t_w = ftime[g.wflag] + (float)kHop;
          const float go = std::max(std::max(now + g.pre, t_new) + g.newest, t_w);
          slots.push(go + g.dur);
          level_end = std::max(level_end, (double)(go + g.dur));
          busy_us += g.pre + g.newest + g.dur;
          tasks.push_back(g.t);
          for (int k = g.prod0; k < g.prod1; k++) {
            const int f = prod[k].flag;
            ftime[f] = go + prod[k].off;
            for (int c = cons_ptr[f]; c < cons_ptr[f + 1]; c++)
              if (--pending[cons[c]] == 0) becomes_known(cons[c]);
          }
        }
      }
      };   // plan
      plan();
      if (!too_many && !xl_ && lvl->schur_split && busy_us + schur_in_flow_us <= 0.6 * flow_grid_ * level_end) {
        lvl->schur_split = false;
        plan();
        if (too_many) { too_many = false; lvl->schur_split = true; plan(); }
      }
      if (too_many) { words = lvl->ticket_word; continue; }   // throughput-bound level: launch sequence (its flag words are given back)
      if (xl_) {
        // BUILD tasks ahead of the level's other tasks, chunk by chunk over all fronts (every front's first columns first)
        std::vector<FlowTask> bt;
        int max_nb = 0;
        for (int z = 0; z < nf; z++) max_nb = std::max(max_nb, fronts[z].nbuild);
        for (int k = 0; k < max_nb; k++)
          for (int z = 0; z < nf; z++)
            if (k < fronts[z].nbuild) bt.push_back(FlowTask{(FLOW_BUILD << 24) | z, k * FLOW_BUILD_COLS, 0, 0});
        bt.insert(bt.end(), tasks.begin(), tasks.end());
        tasks.swap(bt);
      }
      lvl->n_tasks = (int)tasks.size();
      lvl->est_us = level_end;
      lvl->wfill_begin = (int)(wfill.size() / 2);
      for (int z = 0; z < nf; z++) {
        const int sn = sym_.task_sn[sym_.task_ptr[st.task_begin + z]];
        const int64_t w0 = sn_wblk[sn] * 256, wn = (int64_t)((sym_.sn_ncols[sn] + BIG_NB - 1) / BIG_NB) * 1024;
        for (int64_t o = 0; o < wn; o += 4096) { wfill.push_back(w0 + o); wfill.push_back(std::min<int64_t>(4096, wn - o)); }   // one workgroup of k_flow_reset each
      }
      lvl->wfill_end = (int)(wfill.size() / 2);
      all_tasks[si] = std::move(tasks);
      all_fronts[si] = std::move(fronts);
      plan_[si].flow = std::move(lvl);
    }
    if (xl_) {
      // the cross-level form needs a task list for EVERY level of fronts beyond LDS (with all Schur tiles as UPDATE tasks a
      // level has several times the tasks of its per-level plan): a level that went over the limit takes the whole graph back to
      // one build + one flow launch per level, planned afresh with the per-level Schur split -- never a refused handle
      bool complete = true;
      for (size_t si = 0; si < sym_.steps.size(); si++) complete = complete && (sym_.steps[si].kind != STEP_BIG || plan_[si].flow);
      if (!complete) {
        xl_refused_ = true;
        build_flow_levels();
        return;
      }
    }
    // k_big_solve_flow (back substitution of wide pivot blocks as one launch per level): a ticket and counters per front in
    // the same zeroed block, and the level's task list: by step, the chain tasks first, then the folds, the groups nearest
    // to the current super-panel first (the next chain step waits for those)
    std::vector<std::vector<SolveFlowFront>> all_sf(sym_.steps.size());
    std::vector<std::vector<SolveFlowTask>> all_st(sym_.steps.size());
    if (solve_flow_on_)
      for (size_t si = 0; si < sym_.steps.size(); si++) {
        const Step &st = sym_.steps[si];
        if (st.kind != STEP_BIG) continue;
        const int nf = st.task_end - st.task_begin, max_nc = plan_[si].max_nc;
        if (max_nc < sp_solve_min_nc_) continue;
        plan_[si].solve_flow = std::make_unique<SolveFlowLevel>();
        plan_[si].solve_flow->ticket_word = words;
        words += 32;
        const int max_S = (max_nc + BIG_SUPER - 1) / BIG_SUPER;
        for (int z = 0; z < nf; z++) {
          const int nc = sym_.sn_ncols[sym_.task_sn[sym_.task_ptr[st.task_begin + z]]];
          all_sf[si].push_back(SolveFlowFront{(int32_t)words, (int32_t)(words + 1)});
          words += 1 + (nc + 63) / 64;
          words = (words + 31) & ~(int64_t)31;
        }
        for (int ell = 0; ell < max_S; ell++) {
          for (int z = 0; z < nf; z++) {
            const int nc = sym_.sn_ncols[sym_.task_sn[sym_.task_ptr[st.task_begin + z]]];
            if (ell < (nc + BIG_SUPER - 1) / BIG_SUPER) all_st[si].push_back(SolveFlowTask{z, ell, -1});
          }
          for (int z = 0; z < nf; z++) {
            const int nc = sym_.sn_ncols[sym_.task_sn[sym_.task_ptr[st.task_begin + z]]];
            const int n_sp = (nc + BIG_SUPER - 1) / BIG_SUPER;
            if (ell >= n_sp) continue;
            const int K0 = BIG_SUPER * (n_sp - 1 - ell);
            for (int g = (K0 + 63) / 64 - 1; g >= 0; g--) all_st[si].push_back(SolveFlowTask{z, ell, g});   // columns [64 g, ...) left of K0
          }
        }
        plan_[si].solve_flow->n_tasks = (int)all_st[si].size();
      }
    if (words == 0) return;
    wfill.resize(wfill.size() + 2, 0);   // never empty
    flow_wfill_.upload(wfill);
    flow_flags_.alloc((size_t)words + kDeadFlagWords);
    flow_flags_.zero();
    for (size_t si = 0; si < sym_.steps.size(); si++)
      if (plan_[si].solve_flow) {
        plan_[si].solve_flow->fronts.upload(all_sf[si]);
        plan_[si].solve_flow->tasks.upload(all_st[si]);
      }
    for (size_t si = 0; si < sym_.steps.size(); si++)
      if (plan_[si].flow) {
        {
          const Step &st = sym_.steps[si];
          std::vector<FlowRec> recs(all_tasks[si].size());
          for (size_t i = 0; i < recs.size(); i++) {
            const int slot = all_tasks[si][i].kind_front & 0xffffff;
            recs[i].t = all_tasks[si][i];
            recs[i].ff = all_fronts[si][slot];
            recs[i].m = host_task_meta_[st.task_begin + slot];
            std::memset(recs[i].pad, 0, sizeof(recs[i].pad));
          }
          plan_[si].flow->tasks.upload(recs);
        }
#ifdef RRPGO_FLOW_TRACE
        plan_[si].flow->host_tasks = all_tasks[si];
        plan_[si].flow->trace.alloc(all_tasks[si].size() * 16);
        plan_[si].flow->trace.zero();
#endif
      }
    if (xl_) {
      // the cross-level list: every level's records, level after level (children have smaller tickets than their parents), and
      // per child_meta entry where the child's `done` counter lives and how many UPDATE tasks it counts
      std::vector<int32_t> sn_done(sym_.S, -1), sn_nupd(sym_.S, 0);
      for (size_t si = 0; si < sym_.steps.size(); si++) {
        if (!plan_[si].flow) { if (sym_.steps[si].kind == STEP_BIG) xl_ = false; continue; }
        const Step &st = sym_.steps[si];
        for (const FlowTask &t : all_tasks[si]) {
          const int slot = t.kind_front & 0xffffff, sn = sym_.task_sn[sym_.task_ptr[st.task_begin + slot]];
          sn_done[sn] = all_fronts[si][slot].done;
          if ((t.kind_front >> 24) == FLOW_UPDATE) sn_nupd[sn]++;
        }
      }
      if (!xl_) throw ApiError(RR_PGO_EUNSUPPORTED, "internal: a level of fronts beyond LDS without a dataflow task list in the cross-level form");
      std::vector<int2> cd(sym_.child_list.size(), int2{-1, 0});
      for (size_t q = 0; q < cd.size(); q++) {
        const int c = sym_.child_list[q];
        if (sn_done[c] >= 0) cd[q] = int2{sn_done[c], sn_nupd[c]};
      }
      xl_child_done_.upload(cd);
      bool first = true;
      for (size_t si = 0; si < sym_.steps.size(); si++) {
        if (!plan_[si].flow) continue;
        if (first) { xl_ticket_word_ = plan_[si].flow->ticket_word; first = false; }
        const Step &st = sym_.steps[si];
        for (const FlowTask &t : all_tasks[si]) {
          const int slot = t.kind_front & 0xffffff;
          FlowRec r{};
          r.t = t;
          r.ff = all_fronts[si][slot];
          r.m = host_task_meta_[st.task_begin + slot];
          xl_host_.push_back(r);
        }
      }
      xl_recs_.upload(xl_host_);
#ifdef RRPGO_FLOW_TRACE
      xl_trace_.alloc(xl_host_.size() * 16);
      xl_trace_.zero();
#endif
    }
  }
  // k_big_update's and k_big_schur's grids: per level of the launch sequence the list of real tiles, front after front
  // -- per super-panel the tiles left of the Schur origin (schur_split_: the Schur complement is ONE pass of k_big_schur
  // at the end of the level; else every tile right of the super-panel), and the Schur tiles themselves
  void build_update_maps() {
    std::vector<int32_t> buf;
    for (size_t si = 0; si < sym_.steps.size(); si++) {
      const Step &st = sym_.steps[si];
      if (st.kind != STEP_BIG) continue;
      const bool flow_level = (bool)plan_[si].flow;   // its per-super-panel tiles are UPDATE tasks; only the Schur pass is a launch
      const int nf = st.task_end - st.task_begin;
      if (nf > 0xffff) throw ApiError(RR_PGO_EUNSUPPORTED, "more than 65535 big fronts in one level");
      const int max_nc = plan_[si].max_nc;
      auto tri_ok = [](int nt) { if (nt * (nt + 1) / 2 > 0xffff) throw ApiError(RR_PGO_EUNSUPPORTED, "a front of more than 65535 update tiles"); };
      for (int K0 = 0; K0 < max_nc && !flow_level; K0 += BIG_SUPER) {
        UpdMap um{(int64_t)buf.size(), 0};
        for (int z = 0; z < nf; z++) {
          const int sn = sym_.task_sn[sym_.task_ptr[st.task_begin + z]];
          const int nc = sym_.sn_ncols[sn], M = nc + sym_.sn_nrows[sn] + 1;
          if (K0 >= nc) continue;
          const int t0 = std::min(K0 + BIG_SUPER, nc), nt = (M - t0 + 63) / 64;
          tri_ok(nt);
          const int o = schur_split_ ? std::min(big_schur_origin(nc, schur_tile_), M) : M;   // tiles whose first column is left of it
          for (int bx = 0; bx < nt; bx++)
            for (int by = 0; by <= bx; by++)
              if (t0 + 64 * by < o) buf.push_back((z << 16) | (bx * (bx + 1) / 2 + by));
        }
        um.n_tiles = (int)((int64_t)buf.size() - um.offset);
        plan_[si].upd.push_back(um);
      }
      if (flow_level ? plan_[si].flow->schur_split : schur_split_) {
        UpdMap um{(int64_t)buf.size(), 0};
        for (int z = 0; z < nf; z++) {
          const int sn = sym_.task_sn[sym_.task_ptr[st.task_begin + z]];
          const int nc = sym_.sn_ncols[sn], M = nc + sym_.sn_nrows[sn] + 1;
          const int o = big_schur_origin(nc, schur_tile_);
          if (o >= M) continue;
          const int nt = (M - o + schur_tile_ - 1) / schur_tile_;
          tri_ok(nt);
          for (int t = 0; t < nt * (nt + 1) / 2; t++) buf.push_back((z << 16) | t);
        }
        um.n_tiles = (int)((int64_t)buf.size() - um.offset);
        plan_[si].schur = um;
      }
    }
    if (!buf.empty()) upd_map_buf_.upload(buf);
  }
  bool any_flow(size_t from, size_t to) const {   // a factorisation range that must zero the flag block first
    for (size_t si = from; si < to && si < plan_.size(); si++) if (plan_[si].flow) return true;
    for (const StepPlan &p : plan_) if (p.solve_flow) return true;   // the back substitution of ANY level may use its counters afterwards
    return false;
  }
  FlowArgs<T> flow_args() {
    FlowArgs<T> fa;
    fa.flags = flow_flags_.p;
    fa.gather = gather_update_ ? 1 : 0;
    fa.exact = flow_exact_ ? 1 : 0;
    fa.child_meta = child_meta_.p;
    fa.scat = scat_.p;
    fa.lvals = lvals_.p;
    fa.uvals = uvals_.p;
    fa.xch = xch_;
    fa.winv = winv_.p;
    fa.xnew = xnew_.p;
    fa.err = err_.p;
    fa.wait_ticks = wait_ticks_;
    fa.trace = nullptr;
    fa.child_done = xl_child_done_.p;
    fa.fasm_colptr = fasm_colptr_.p;
    fa.fasm_dst = fasm_dst_.p;
    fa.fasm_src = fasm_src_.p;
    fa.perm = perm_.p;
    fa.hvals = hvals_.p;
    fa.b = b_.p;
    return fa;
  }
  void launch_flow(const FlowLevel &lvl) {
    FlowArgs<T> fa = flow_args();
    fa.tasks = lvl.tasks.p;
    fa.ticket = flow_flags_.p + lvl.ticket_word;
    fa.n_tasks = lvl.n_tasks;
    fa.schur_tile = lvl.schur_split ? schur_tile_ : 0;
    fa.trace = lvl.trace.p;
    hipLaunchKernelGGL((k_big_flow<T, 2>), dim3((unsigned)std::min(lvl.n_tasks, flow_grid_)), dim3(256), 0, stream_, fa);
    check_launch("k_big_flow");
  }
  // every level of fronts beyond LDS as ONE launch (the cross-level form: BUILD tasks, Schur complements inside, counters between levels)
  void launch_flow_xl() {
    FlowArgs<T> fa = flow_args();
    fa.tasks = xl_recs_.p;
    fa.ticket = flow_flags_.p + xl_ticket_word_;
    fa.n_tasks = (int)xl_host_.size();
    fa.schur_tile = 0;
    fa.trace = xl_trace_.p;
    hipLaunchKernelGGL((k_big_flow<T, 2, true>), dim3((unsigned)std::min(fa.n_tasks, flow_grid_)), dim3(256), 0, stream_, fa);
    check_launch("k_big_flow (cross-level)");
  }

  // Gauge transfer applies to a single-precision factor (T = float) of an SE(2) graph whose root front is
  // one of the big in-place fronts; RR_PGO_GAUGE=0 keeps the reference's anchor prior (comparison runs).
  void setup_gauge() {
    if (sizeof(T) != 4 || is3d_ || g_.anchor_node < 0 || sym_.S == 0) return;
    if (const char *e = getenv("RR_PGO_GAUGE")) if (std::atoi(e) == 0) return;
    const int root = sym_.S - 1;
    if (!sym_.sn_big[root] || !sym_.sn_huge[root] || sym_.sn_nrows[root] != 0) return;
    std::vector<int32_t> cn;
    double sx = 0, sy = 0, ext = 0;
    int n_se2 = 0, n_nodes = 0;
    for (int p = sym_.sn_first_pos[root]; p < sym_.sn_first_pos[root] + sym_.sn_npos[root]; p++) {
      const int node = sym_.order[p];
      const double *st = &g_.node_state[g_.node_state_off[node]];
      sx += st[0]; sy += st[1]; n_nodes++;
      n_se2 += g_.node_kind[node] == NODE_SE2;
      for (int t = 0; t < node_dim(g_.node_kind[node]); t++) cn.push_back((node << 2) | t);
    }
    if (n_se2 == 0 || (int)cn.size() != sym_.sn_ncols[root]) return;
    gauge_ox_ = sx / n_nodes; gauge_oy_ = sy / n_nodes;
    for (int p = sym_.sn_first_pos[root]; p < sym_.sn_first_pos[root] + sym_.sn_npos[root]; p++) {
      const double *st = &g_.node_state[g_.node_state_off[sym_.order[p]]];
      ext = std::max(ext, std::max(std::fabs(st[0] - gauge_ox_), std::fabs(st[1] - gauge_oy_)));
    }
    // entries of the added term stay at the scale of the information matrices: mu * max|v|^2 = w
    double w = 0;
    for (int k = 0; k < g_.n_edges(); k++) {
      const double *wi = &g_.edge_info[g_.edge_info_off[k]];
      w = std::max(w, std::fabs(wi[0]));
    }
    gauge_mu_t_ = w;
    gauge_mu_r_ = w / std::max(1.0, ext * ext);
    gauge_root_ = root;
    gauge_col_node_.upload(cn);
    gauge_v_.alloc(3 * cn.size());
    gauge_ok_ = true;
  }
  void launch_gauge_term() {
    GaugeArgs<T, S> ga;
    ga.pose = pose_.p;
    ga.col_node = gauge_col_node_.p;
    ga.nc = sym_.sn_ncols[gauge_root_];
    ga.M = ga.nc + sym_.sn_nrows[gauge_root_] + 1;
    ga.F = lvals_.p + sym_.sn_loff[gauge_root_];
    ga.v = gauge_v_.p;
    ga.ox = (S)gauge_ox_; ga.oy = (S)gauge_oy_;
    ga.mu_t = (T)gauge_mu_t_; ga.mu_r = (T)gauge_mu_r_;
    ga.err = err_.p;
    hipLaunchKernelGGL((k_gauge_vectors<T, S>), dim3((ga.nc + 255) / 256), dim3(256), 0, stream_, ga);
    hipLaunchKernelGGL((k_big_gauge<T, S>), dim3(ga.nc), dim3(256), 0, stream_, ga);
    check_launch("k_big_gauge");
  }

  static constexpr int kMaxLds = 160 * 1024 - 9216;   // the kernels also hold static __shared__ scratch (W16_SCR: a W slot + identity, tickets)

  template <int TH> void set_lds_attr() {
    HIPCHK(hipFuncSetAttribute((const void *)k_factor_tasks<T, TH>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
    HIPCHK(hipFuncSetAttribute((const void *)k_solve_tasks<T, TH>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
  }
  // ---- the plan of every step.  First what depends on the fronts alone (build_flow_levels, build_update_maps and
  // plan_mid_solve_tasks read it and add their tables), then plan_launches: what follows from those tables too.
  void plan_shapes() {
    plan_.clear();
    plan_.resize(sym_.steps.size());
    for (size_t si = 0; si < plan_.size(); si++) {
      const Step &st = sym_.steps[si];
      StepPlan &p = plan_[si];
      p.kind = st.kind;
      p.nf = st.task_end - st.task_begin;
      p.task_begin = st.task_begin;
      if (st.kind == STEP_TASKS) {
        // Workgroup size of an LDS-front step: the symbolic phase sizes it for the latency of ONE task (a 16-wave workgroup per
        // front of > 128 rows).  Smaller workgroups for levels of thousands of tasks were measured slower (r02, lattice, 5244
        // tasks: 690 us with 1024 threads, 873 with 512, 1045 with 256).
        p.factor_lds = (size_t)st.max_lds_elems * sizeof(T);
        p.factor_threads = std::min(st.threads, factor_threads_max_);
        p.solve_threads = std::min(st.threads, solve_threads_max_);
        continue;
      }
      auto front = [&](int z) { return sym_.task_sn[sym_.task_ptr[st.task_begin + z]]; };
      int64_t max_asm = 0;
      for (int z = 0; z < p.nf; z++) {
        const int s = front(z), nc = sym_.sn_ncols[s], nr = sym_.sn_nrows[s];
        p.max_nc = std::max(p.max_nc, nc);
        p.maxM = std::max(p.maxM, nc + nr + 1);
        p.max_nr = std::max(p.max_nr, nr);
        p.has_rows = p.has_rows || nr > 0;
        max_asm = std::max<int64_t>(max_asm, std::max<int64_t>(sym_.fasm_ptr[s + 1] - sym_.fasm_ptr[s], nc));
        p.any_dup = p.any_dup || sym_.fdup_ptr[s + 1] > sym_.fdup_ptr[s];
        p.has_root = p.has_root || (gauge_ok_ && s == gauge_root_);
      }
      // one pass writes every entry of the level's fronts once: the sum of the children's contributions (gathered
      // through inverse maps), zeros elsewhere; the H entries and the rhs are added on top -- by the building waves
      // themselves when the launch is a single round of workgroups (three dependent loads per column at the end of every
      // workgroup: cheaper than a launch there, dearer on the levels of hundreds of fronts -- lattice 4.62 against 4.68 ms
      // with every level fused, sphere2500 +1 % fused), else by a k_big_assemble launch
      p.build_gx = std::min(std::max(((gather_update_ ? std::min(p.maxM, ((p.max_nc + 127) / 128) * 128) : p.maxM) + 3) / 4, 1), 8192);
      const bool fused = fused_assembly_ && (int64_t)p.build_gx * p.nf <= 2048;
      p.asm_gx = fused ? 0 : (int)std::min<int64_t>((max_asm + 255) / 256, 2048);
      // row slices of a level's k_big_gemv_partial launch: enough workgroups to fill the chip, but never thinner than 128 rows
      // (every slice is a partial sum the solve has to fetch and add per column)
      p.cb = (p.max_nc + 63) / 64;
      p.R = std::max(1, std::min(std::min(kGemvSlices, (p.max_nr + 127) / 128), (768 + p.nf * p.cb - 1) / (p.nf * p.cb)));
      p.n_sp = (p.max_nc + BIG_SUPER - 1) / BIG_SUPER;
    }
  }
  void plan_launches() {
    for (StepPlan &p : plan_) {
      if (p.kind != STEP_BIG) continue;
      // the launch sequence (a flow level's panel chain and trailing updates are tasks of its one launch): a k_big_panel32
      // launch per 32 columns, over the rows of the fronts still active there
      for (int kb = 0; kb < p.max_nc && !p.flow; kb += BIG_NB) {
        int rows = 0;   // max over fronts still active at column kb of (M - kb)
        for (int z = 0; z < p.nf; z++) {
          const int s = sym_.task_sn[sym_.task_ptr[p.task_begin + z]];
          if (sym_.sn_ncols[s] > kb) rows = std::max(rows, sym_.sn_ncols[s] + sym_.sn_nrows[s] + 1 - kb);
        }
        p.panel_gx.push_back((std::max(rows - 1, 1) + 31) / 32);
      }
      // L11: per 128-column super-panel over the chip (wide pivot blocks; as one launch of ticketed tasks where the level has
      // the list), or one workgroup per front
      p.l11 = p.max_nc < sp_solve_min_nc_ ? L11_MID : p.solve_flow ? L11_FLOW : L11_SP;
      p.l11_gx = p.l11 == L11_MID  ? p.nf
                 : p.l11 == L11_SP ? 1 + (p.max_nc + 63) / 64
                                   : std::min(p.solve_flow->n_tasks, std::max(flow_grid_ / (sizeof(T) == 4 ? RRPGO_FLOW_WAVES : 1), 1));
    }
  }
  // launches of one factorisation / one back substitution of a step (the two gauge launches counted whether or not they run)
  static int factor_launches(const StepPlan &p) {
    if (p.kind != STEP_BIG) return 1;
    int n = 1 + (p.asm_gx > 0) + p.any_dup + 2 * p.has_root + (p.flow ? 1 : 0) + (int)p.panel_gx.size() + (p.schur.n_tiles > 0);
    for (const UpdMap &um : p.upd) n += um.n_tiles > 0;
    return n;
  }
  static int solve_launches(const StepPlan &p) {
    if (p.in_solve_flow) return 0;
    if (p.kind != STEP_BIG) return 1;
    return p.has_rows + (p.l11 == L11_SP ? p.n_sp : 1);
  }
  // the instantiation of a kernel family for a workgroup size: the first of the family's sizes that holds it, else the last
  template <int TH, int... More, typename F> static void for_threads(int threads, F &&f) {
    if constexpr (sizeof...(More) == 0) f(std::integral_constant<int, TH>{});
    else if (threads <= TH) f(std::integral_constant<int, TH>{});
    else for_threads<More...>(threads, f);
  }
  // Graphs on the dataflow schedule with fronts beyond LDS (sphere2500: 46, six levels): the levels whose pivot blocks are
  // narrower than RR_PGO_SP_SOLVE_MIN columns -- all but the top one or two -- are back-substituted as TASKS of k_solve_flow
  // (lds_flow.hip.h: GEMV units + one L11 task per front) instead of a k_big_gemv_partial + k_solve_mid launch pair per level.
  // The wide top levels stay launches in front of k_solve_flow.  RR_PGO_SOLVE_MID_FLOW=0: every level as launches (the
  // r03 - r05 form; the same sums in the same order: bit-identical).
  void plan_mid_solve_tasks() {
    if (!lds_flow_) return;
    bool on = true;
    if (const char *e = getenv("RR_PGO_SOLVE_MID_FLOW")) on = std::atoi(e) != 0;
    int top = (int)sym_.steps.size() - 1;
    while (on && top >= 1 && plan_[top].max_nc >= sp_solve_min_nc_) top--;   // the wide top levels
    std::vector<LdsFlowTask> mid;
    int need = 1024;   // a GEMV unit's x[rows] chunk
    for (int i = top; on && i >= 1; i--) {
      const Step &st = sym_.steps[i];
      if (plan_[i].max_nc >= sp_solve_min_nc_) { on = false; break; }   // a wide level under a narrow one: keep every level a launch
      const int R = plan_[i].R;
      for (int pass = 1; pass <= 2; pass++)   // the level's GEMV units first, then its L11 tasks
        for (int t = st.task_begin; t < st.task_end; t++) {
          LdsFlowTask r{};
          r.sn_begin = sym_.task_ptr[t];
          r.sn_end = r.sn_begin + 1;
          r.sn = sym_.task_sn[r.sn_begin];
          r.m = host_sn_meta_[r.sn];
          r.kind = pass;
          r.slices = R;
          const int nc = sym_.sn_ncols[r.sn], nr = sym_.sn_nrows[r.sn];
          const int units = nr > 0 ? (nc + 63) / 64 * R : 0;
          if (pass == 2) {
            r.n_units = units;
            mid.push_back(r);
            need = std::max(need, ((nc + 3) & ~3) + 2 * 32 * 33 + 64);
          } else {
            for (int u = 0; u < units; u++) { r.bx = u / R; r.by = u % R; mid.push_back(r); }
          }
        }
    }
    if (on && !mid.empty() && (size_t)need * sizeof(T) <= (size_t)kMaxLds) {
      for (int i = top; i >= 1; i--) plan_[i].in_solve_flow = true;
      plan_[0].solve_lds = std::max(plan_[0].solve_lds, need);
      mid.insert(mid.end(), host_stasks_.begin(), host_stasks_.end());
      host_stasks_.swap(mid);
    }
    lds_n_stasks_ = (int)host_stasks_.size();
    lds_stasks_.upload(host_stasks_);
  }

  void configure_kernels() {
    // opt in to > 64 KiB of dynamic LDS
    set_lds_attr<64>();
    set_lds_attr<128>();
    set_lds_attr<256>();
    set_lds_attr<512>();
    HIPCHK(hipFuncSetAttribute((const void *)k_factor_tasks<T, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
    HIPCHK(hipFuncSetAttribute((const void *)k_solve_mid<T, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
    HIPCHK(hipFuncSetAttribute((const void *)k_factor_flow<T, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
    HIPCHK(hipFuncSetAttribute((const void *)k_factor_flow<T, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
    HIPCHK(hipFuncSetAttribute((const void *)k_factor_flow<T, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
    HIPCHK(hipFuncSetAttribute((const void *)k_solve_flow<T, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
    HIPCHK(hipFuncSetAttribute((const void *)k_solve_flow<T, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
  }

  // ---- what a launch is told by whoever enqueues it.  One linearisation: chi2 only, or the system too; gauge: without the anchor prior --
  // the enqueuer hands the SAME value to the factorisation (the root front takes the gauge term) and to the update of the solved step
  struct Lin { int write_system; bool gauge; int lm; double lambda; };
  // Gauss-Newton with a single-precision factor: no anchor prior, the root front carries the gauge term
  // (not with priors: the gauge term assumes that H without the anchor term is singular along the SE(2) gauge)
  // (nor with fixed nodes, rr_pgo_set_fixed: their identity rows are no part of that singular system)
  bool gauge_rule(int lm, bool reference_prior = false) const { return gauge_ok_ && !lm && !reference_prior && settings_.priors.n() == 0 && settings_.fixed.empty(); }
  static Lin lin_chi2() { return Lin{0, false, 0, 0.0}; }
  Lin lin_system(double lambda, int lm) const { return Lin{1, gauge_rule(lm), lm, lambda}; }
  Lin lin_reference_system(double lambda, int lm) const { return Lin{1, gauge_rule(lm, true), lm, lambda}; }   // rr_pgo_assemble: always the anchor prior
  // ... and what one inside a pipelined rr_pgo_optimize call carries on top (absent: a launch outside such a call).  reset: the call's
  // first launch, it resets the loop state (lambda to lambda0); publish: LinArgs::publish; lambda_dev: lambda from the loop state
  struct OptLin { bool reset; double lambda0; int publish; bool lambda_dev; };
  // a solved step: exported in reference order, the state untouched | applied | + the reduction in k_update's last workgroup | + a pipelined call's decisions
  enum StepUse { STEP_EXPORT, STEP_APPLY, STEP_APPLY_REDUCE, STEP_APPLY_REDUCE_OPT };
  LinArgs<T, S> lin_args(const Lin &m, const OptLin *opt) const {
    LinArgs<T, S> a;
    a.n_nodes = n_list_;
    a.node_list = node_list_.p;
    a.pose = pose_.p;
    a.e_rec = e_rec_.p;
    a.e_idx = e_idx_.p;
    a.e_meas = e_meas_.p;
    a.e_info = e_info3_.p;
    a.e_slot = e_slot_.p;
    a.inc_ptr = inc_ptr_.p;
    a.inc_list = inc_list_.p;
    a.node_dim = (is3d_ && !has_lm_) ? nullptr : node_dim_.p;
    a.node_offset = node_offset_.p;
    a.diag_off = diag_off_.p;
    a.hvals = hvals_.p;
    a.b = b_.p;
    a.chi2_partial = chi_partial_.p;
    a.anchor = ((m.write_system && m.gauge) || !settings_.priors.keep_anchor || !settings_.fixed_keep_anchor) ? -1 : g_.anchor_node;
    a.lambda = m.lm ? (S)m.lambda : (S)0;
    a.write_system = m.write_system;
    a.adds_diag = norm_counts_.p;
    a.zero_words = lds_flow_ ? dep_flags_.p : nullptr;
    a.n_zero_words = lds_flow_ ? 2 * sym_.S + 64 : 0;
    a.fill_words = lds_flow_ ? reinterpret_cast<unsigned *>(x_ptr_) : nullptr;
    a.n_fill_words = lds_flow_ ? (int)((size_t)g_.dim * sizeof(T) / 4) : 0;
    a.ctrl = opt ? opt_ctrl_.p : nullptr;
    a.err = err_.p;
    a.lambda_from_ctrl = (opt && opt->lambda_dev) ? 1 : 0;
    a.reset_ctrl = (opt && opt->reset) ? 1 : 0;
    a.reset_lambda = opt ? opt->lambda0 : 0.01;
    a.reset_tolerance = 1e-4;   // :253
    a.publish = opt ? opt->publish : 0;
    a.ring_host = opt_ring_;
    a.blocks_done = blocks_done_.p + 1;
    robust_fields(a);
    prior_fields(a);
    a.fixed = settings_.fixed.empty() ? nullptr : fixed_.p;   // (every instantiation reads it)
    return a;
  }
  void robust_fields(LinArgs<T, S> &a) const {
    a.robust_delta = (S)settings_.robust_delta;
    a.robust_delta2 = (S)(settings_.robust_delta * settings_.robust_delta);
    a.robust_mask = robust_mask_.n ? robust_mask_.p : nullptr;
    const TlsParams p = tls_params();
    a.tls_lo = (S)p.lo; a.tls_hi = (S)p.hi; a.tls_cs = (S)p.cs; a.tls_mu = (S)p.mu;
  }
  // ROBUST_TLS: what the host precomputes from (delta, mu) for every kernel that reads the weight (zeros under the other kinds)
  struct TlsParams { double lo, hi, cs, mu; };
  TlsParams tls_params() const {
    if (settings_.robust_kind != ROBUST_TLS) return TlsParams{0.0, 0.0, 0.0, 0.0};
    const double c2 = settings_.robust_delta * settings_.robust_delta, mu = settings_.robust_mu;
    return TlsParams{mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2, settings_.robust_delta * std::sqrt(mu * (mu + 1.0)), mu};
  }
  void prior_fields(LinArgs<T, S> &a) const {   // (read by the PR instantiations alone: launch_pull)
    a.prior_ptr = prior_ptr_.p;
    a.prior_rec = prior_rec_.p;
    a.prior_meas = prior_meas_.p;
    a.prior_info = prior_info3_.p;
    a.prior_robust = prior_robust_.p;
  }

  FactorArgs<T> factor_args(int task_begin) {
    FactorArgs<T> a;
    a.task_ptr = task_ptr_.p;
    a.task_sn = task_sn_.p;
    a.task_begin = task_begin;
    a.sn_meta = sn_meta_.p;
    a.task_meta = task_meta_.p;
    a.child_meta = child_meta_.p;
    a.fasm_src = fasm_src_.p;
    a.fasm_dst = fasm_dst_.p;
    a.fasm_colptr = fasm_colptr_.p;
    a.fdup_src = fdup_src_.p;
    a.fdup_dst = fdup_dst_.p;
    a.scat = scat_.p;
    a.rel = rel_.p;
    a.perm = perm_.p;
    a.sn_rows = sn_rows_.p;
    a.hvals = hvals_.p;
    a.b = b_.p;
    a.lvals = lvals_.p;
    a.uvals = uvals_.p;
    a.xch = xch_;
    a.x = x_ptr_;
    a.winv = winv_.p;
    a.err = err_.p;
    a.stamps = stamps_.p;
#if defined(RRPGO_TRACE) && defined(RRPGO_STAMPS)
    a.trace = stamps_.p ? stamps_.p + (size_t)sym_.S * 12 : nullptr;
#else
    a.trace = nullptr;
#endif
    a.child_dep = child_dep_.p;
    a.child_due = child_due_.p;
    a.parent_dep = parent_dep_.p;
    a.dep_flags = dep_flags_.p;
    a.parent_dep_self = sym_.S;
    a.wait_ticks = wait_ticks_;
    a.solve_lds = 0;
    a.kvals = kform_ ? kvals_.p : nullptr;
    return a;
  }

  // Optional per-launch event timing (rr_pgo_profile).
  struct Prof {
    bool on = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double ms[RR_PGO_NUM_KCLASS] = {0};
    int64_t n[RR_PGO_NUM_KCLASS] = {0};
  } prof_;
  void pbegin() { if (prof_.on) HIPCHK(hipEventRecord(prof_.e0, stream_)); }
  void pend(int k, int launches = 1) {   // launches: kernels in the timed segment
    if (!prof_.on) return;
    HIPCHK(hipEventRecord(prof_.e1, stream_));
    HIPCHK(hipEventSynchronize(prof_.e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, prof_.e0, prof_.e1));
    prof_.ms[k] += ms;
    prof_.n[k] += launches;
  }

  // a launch with an invalid configuration fails silently unless asked
  void check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw ApiError(RR_PGO_ENODEVICE, std::string("kernel launch failed (") + what + "): " + hipGetErrorString(e));
  }

  // a pipelined rr_pgo_optimize call may have left its stop word set: every path outside such a call starts here -- the plain launches
  // in launch_linearize, the replays in ensure_gn_graph (before the capture: a captured graph must hold no memset node)
  void clear_stop_word() {
    if (stop_dirty_) {
      HIPCHK(hipMemsetAsync(err_.p + 1, 0, sizeof(int), stream_));
      stop_dirty_ = false;
    }
  }

  void launch_linearize(const Lin &m, const OptLin *opt = nullptr) {
    if (!opt) clear_stop_word();
    pbegin();
    const LinArgs<T, S> la = lin_args(m, opt);
    if (!is3d_ && edge_lin_) {
      // the edge-parallel form (experiment knob RR_PGO_EDGE_LINEARIZE): clear + prior, one thread per edge, mirror
      const unsigned nb = (unsigned)((g_.n_nodes() + 255) / 256);
      if (lds_flow_) {
        hipLaunchKernelGGL(k_fill_words, dim3(4), dim3(256), 0, stream_, dep_flags_.p, 2 * sym_.S + 64, 0u);
        hipLaunchKernelGGL(k_fill_words, dim3(16), dim3(256), 0, stream_, reinterpret_cast<unsigned *>(x_ptr_), (int)((size_t)g_.dim * sizeof(T) / 4), X_PENDING_WORD);
      }
      if (m.write_system) hipLaunchKernelGGL((k_lin_init<T, S>), dim3(nb), dim3(256), 0, stream_, la);
      if (edge_lin_wave_) hipLaunchKernelGGL((k_linearize_wave_edges<T, S>), dim3(n_lin_blocks_), dim3(256), 0, stream_, la, g_.n_edges());
      else hipLaunchKernelGGL((k_linearize_edges<T, S>), dim3(n_lin_blocks_), dim3(LIN_THREADS), 0, stream_, la, g_.n_edges());
      if (m.write_system) hipLaunchKernelGGL((k_lin_finish<T, S>), dim3(nb), dim3(256), 0, stream_, la);
    } else {
      if (settings_.robust_kind == ROBUST_HUBER) launch_pull<ROBUST_HUBER>(la);
      else if (settings_.robust_kind == ROBUST_CAUCHY) launch_pull<ROBUST_CAUCHY>(la);
      else if (settings_.robust_kind == ROBUST_TLS) launch_pull<ROBUST_TLS>(la);
      else launch_pull<ROBUST_NONE>(la);
    }
    check_launch("k_linearize");
    pend(RR_PGO_K_LINEARIZE);
  }
  template <int RK> void launch_pull(const LinArgs<T, S> &la) {   // the pull form of either dimension under robust kernel RK
    if (has_lm_) {   // a 3-D graph with XYZ landmarks: the LM instantiations (a pure SE(3) handle launches the kernels it always did)
      if (settings_.priors.n() > 0) hipLaunchKernelGGL((k_linearize_lm<T, S, RK, true>), dim3(n_lin_blocks_), dim3(LIN_THREADS), 0, stream_, la);
      else hipLaunchKernelGGL((k_linearize_lm<T, S, RK, false>), dim3(n_lin_blocks_), dim3(LIN_THREADS), 0, stream_, la);
      return;
    }
    if (has_br_) {   // a 2-D graph with bearing-only / range-only edges: the BR instantiations (every other 2-D handle launches the kernels it always did)
      if (settings_.priors.n() > 0) hipLaunchKernelGGL((k_linearize_br<T, S, RK, true>), dim3(n_lin_blocks_), dim3(LIN_THREADS), 0, stream_, la);
      else hipLaunchKernelGGL((k_linearize_br<T, S, RK, false>), dim3(n_lin_blocks_), dim3(LIN_THREADS), 0, stream_, la);
      return;
    }
    if (settings_.priors.n() > 0) {   // (a handle without priors launches the kernels it always did)
      if (is3d_) hipLaunchKernelGGL((k_linearize<T, S, RK, 6, true>), dim3(n_lin_blocks_), dim3(LIN_THREADS), 0, stream_, la);
      else hipLaunchKernelGGL((k_linearize<T, S, RK, 3, true>), dim3(n_lin_blocks_), dim3(LIN_THREADS), 0, stream_, la);
      return;
    }
    if (is3d_) hipLaunchKernelGGL((k_linearize<T, S, RK, 6>), dim3(n_lin_blocks_), dim3(LIN_THREADS), 0, stream_, la);
    else hipLaunchKernelGGL((k_linearize<T, S, RK, 3>), dim3(n_lin_blocks_), dim3(LIN_THREADS), 0, stream_, la);
  }

  void launch_factor_range(size_t from, size_t to, bool gauge) {
    // tickets and completion flags of the flow levels (one small kernel per factorisation; flow.hip.h, k_flow_reset)
    if (any_flow(from, to)) {
      // ... and the "not there yet" marks of the W blocks of the range's flow fronts
      int e0 = 0, e1 = 0;
      for (size_t si = from; si < to && si < plan_.size(); si++)
        if (const FlowLevel *l = plan_[si].flow.get()) { if (e1 == 0) e0 = l->wfill_begin; e1 = l->wfill_end; }
      const int flag_wgs = (int)std::min<int64_t>(((int64_t)flow_flags_.n + 255) / 256, 256);
      hipLaunchKernelGGL(k_flow_reset<T>, dim3((unsigned)(flag_wgs + std::max(e1 - e0, 0))), dim3(256), 0, stream_, flow_flags_.p, (int64_t)flow_flags_.n, flag_wgs,
                         winv_.p, flow_wfill_.p + 2 * e0, xnew_.p, (const int *)err_.p);
      check_launch("k_flow_reset");
    }
    if (lds_flow_ && from == 0 && to > 0) {
      // every front in LDS: their whole factorisation as ONE launch of ticket-ordered tasks (lds_flow.hip.h)
      const StepPlan &p = plan_[0];
      pbegin();
      const FactorArgs<T> a = factor_args(0);
      const int grid = std::min(lds_n_tasks_, lds_flow_cus_);
      unsigned *ticket = dep_flags_.p + 2 * sym_.S;
      for_threads<256, 512, 1024>(p.factor_threads, [&](auto th) {
        hipLaunchKernelGGL((k_factor_flow<T, th()>), dim3(grid), dim3(th()), p.factor_lds, stream_, a, (const LdsFlowTask *)lds_ftasks_.p, lds_n_tasks_, ticket);
      });
      check_launch("k_factor_flow");
      pend(RR_PGO_K_FACTOR);
      from = 1;
    }
    if (xl_ && from == 1 && to == plan_.size()) {
      pbegin();
      launch_flow_xl();
      pend(RR_PGO_K_BIG_FLOW);
      return;
    }
    for (size_t si = from; si < to; si++) {
      const StepPlan &p = plan_[si];
      pbegin();
      if (p.kind == STEP_TASKS) {
        const FactorArgs<T> a = factor_args(p.task_begin);
        for_threads<64, 128, 256, 512, 1024>(p.factor_threads, [&](auto th) {
          hipLaunchKernelGGL((k_factor_tasks<T, th()>), dim3(p.nf), dim3(th()), p.factor_lds, stream_, a);
        });
        pend(RR_PGO_K_FACTOR);
      } else {
        launch_big_level(p, gauge);
        pend(RR_PGO_K_BIGFRONT);
      }
    }
  }

  // The fronts beyond LDS of one level, batched (grid y / z = front): ONE gather pass builds the pivot columns from
  // the children (k_big_build) and adds the H entries and the right-hand side (k_big_assemble); then either the whole
  // level as one dataflow launch (k_big_flow: levels of few fronts and few tasks), or per 128-column super-panel four
  // left-looking k_big_panel32 launches and one K = 128 trailing update (k_big_update; the first one of a front gathers
  // its tiles from the children, its tile (0, 0) factors and inverts the next super-panel's first diagonal block).
  // (The r01 / r02 alternatives -- right-looking K = 32 steps, whole super-panels per chain step, the two-stream far
  // update, zero + extend-add assembly, the one-workgroup panel class -- were measured slower and removed in r03:
  // profiles/EXPERIMENTS.md.)  Every launch here has its term in factor_launches.
  void launch_big_level(const StepPlan &p, bool gauge) {
    const FactorArgs<T> a = factor_args(p.task_begin);
    hipLaunchKernelGGL(k_big_build<T>, dim3((unsigned)p.build_gx, p.nf), dim3(256), 0, stream_, a, gather_update_ ? 1 : 0, p.asm_gx > 0 ? 0 : 1);
    check_launch("k_big_build");
    if (p.asm_gx > 0) {
      hipLaunchKernelGGL(k_big_assemble<T>, dim3((unsigned)p.asm_gx, p.nf), dim3(256), 0, stream_, a, 1);
      check_launch("k_big_assemble");
    }
    if (p.any_dup) hipLaunchKernelGGL(k_big_assemble_dup<T>, dim3(1, p.nf), dim3(64), 0, stream_, a);
    if (p.has_root && gauge) launch_gauge_term();
    pend(RR_PGO_K_BIGFRONT);   // closes the build / assemble segment
    if (p.flow) {
      // the whole panel chain and every trailing update of the level: ONE launch of ticket-ordered tasks
      pbegin();
      launch_flow(*p.flow);
      pend(RR_PGO_K_BIG_FLOW);
    }
    for (size_t sp = 0; sp < p.upd.size(); sp++) {   // the super-panels of the launch sequence (a flow level has none)
      // left-looking inside the super-panel: ONE launch per 32 columns (update from the columns K0..kb, multiply by the
      // inverse diagonal block, next diagonal block).  The level's first block is factored and inverted inside its own
      // row launch (by every workgroup); the first block of a later super-panel comes out of the previous trailing update.
      const int K0 = (int)sp * BIG_SUPER, k_end = std::min(K0 + BIG_SUPER, p.max_nc);
      pbegin();
      for (int kb = K0; kb < k_end; kb += BIG_NB) {
        hipLaunchKernelGGL(k_big_panel32<T>, dim3(p.panel_gx[kb / BIG_NB], p.nf), dim3(64), 0, stream_, a, kb, K0, kb == 0 ? 1 : 0);
        check_launch("k_big_panel32");
      }
      pend(RR_PGO_K_BIG_PANEL, (k_end - K0 + BIG_NB - 1) / BIG_NB);
      // everything right of the super-panel, Schur complement included: the level's real 64 x 64 tiles as a
      // one-dimensional grid (StepPlan::upd: front slot and tile of every grid index)
      const UpdMap &um = p.upd[sp];
      if (um.n_tiles == 0) continue;   // schur_split_: a level of single-super-panel fronts has no per-super-panel update at all
      pbegin();
      hipLaunchKernelGGL((k_big_update<T, 2, RRPGO_UPD_DEPTH>), dim3((unsigned)um.n_tiles), dim3(256), 0, stream_, a, K0,
                         (gather_update_ && K0 == 0) ? 1 : 0, (const int32_t *)upd_map_buf_.p + um.offset, um.n_tiles, xcd_remap_ ? 1 : 0,
                         schur_split_ ? schur_tile_ : 0);
      check_launch("k_big_update");
      pend(RR_PGO_K_BIG_UPDATE);
    }
    if (p.schur.n_tiles > 0) {
      // the Schur complements of the level's fronts: ONE pass over all pivot columns (K = nc), each tile written once
      // (no map: no split on this level, or no Schur complement at all)
      pbegin();
      hipLaunchKernelGGL((k_big_schur<T, 2>), dim3((unsigned)p.schur.n_tiles), dim3(256), 0, stream_, a, gather_update_ ? 1 : 0,
                         (const int32_t *)upd_map_buf_.p + p.schur.offset, p.schur.n_tiles, xcd_remap_ ? 1 : 0);
      check_launch("k_big_schur");
      pend(RR_PGO_K_BIG_UPDATE);
    }
    pbegin();   // re-arm: the caller closes the level with pend(BIGFRONT)
  }

  void launch_solve() {
    launch_solve_steps(lds_flow_ ? 1 : 0);   // the fronts beyond LDS (and, in the level schedule, everything), top down
    if (lds_flow_) {
      const StepPlan &p = plan_[0];
      pbegin();
      FactorArgs<T> a = factor_args(0);
      a.solve_lds = p.solve_lds;
      const int grid = std::min(lds_n_stasks_, lds_flow_cus_ * (p.solve_threads <= 256 ? 4 : 2));
      unsigned *ticket = dep_flags_.p + 2 * sym_.S + 32;
      for_threads<256, 512>(p.solve_threads, [&](auto th) {
        hipLaunchKernelGGL((k_solve_flow<T, th()>), dim3(grid), dim3(th()), (size_t)p.solve_lds * sizeof(T), stream_, a, (const LdsFlowTask *)lds_stasks_.p, lds_n_stasks_,
                           ticket, gemv_part_.p, (int64_t)g_.dim);
      });
      check_launch("k_solve_flow");
      pend(RR_PGO_K_SOLVE);
    }
  }
  // Every launch here has its term in solve_launches.
  void launch_solve_steps(int first_step) {
    for (int i = (int)plan_.size() - 1; i >= first_step; i--) {   // shared top fronts first, then this rank's subtrees
      const StepPlan &p = plan_[(size_t)i];
      if (p.in_solve_flow) continue;   // its fronts are tasks of k_solve_flow
      const size_t lds = (size_t)p.solve_lds * sizeof(T);
      pbegin();
      FactorArgs<T> a = factor_args(p.task_begin);
      if (p.kind == STEP_TASKS) {
        a.solve_lds = p.solve_lds;
        for_threads<64, 128, 256, 512>(p.solve_threads, [&](auto th) {
          hipLaunchKernelGGL((k_solve_tasks<T, th()>), dim3(p.nf), dim3(th()), lds, stream_, a);
        });
        pend(RR_PGO_K_SOLVE);
        continue;
      }
      // t = y1 - L21^T x[rows] over the whole chip, then L11 in the level's form (plan_launches)
      if (p.has_rows) {   // (a level of root fronts -- no rows below the pivot block -- has no L21^T x to form: the solves read no partial sums)
        hipLaunchKernelGGL(k_big_gemv_partial<T>, dim3(p.cb, p.R, p.nf), dim3(256), 0, stream_, a, gemv_part_.p, (int64_t)g_.dim, p.R);
        check_launch("k_big_gemv_partial");
      }
      if (p.l11 == L11_FLOW) {
        // wide pivot blocks, the whole level's chain steps and folds as ONE launch of ticketed tasks (flow.hip.h)
        const SolveFlowLevel &sl = *p.solve_flow;
        hipLaunchKernelGGL(k_big_solve_flow<T>, dim3((unsigned)p.l11_gx), dim3(1024), 0, stream_, a, (const T *)gemv_part_.p, (int64_t)g_.dim, p.R,
                           flow_flags_.p, (const SolveFlowFront *)sl.fronts.p, (const SolveFlowTask *)sl.tasks.p, sl.n_tasks,
                           flow_flags_.p + sl.ticket_word);
        check_launch("k_big_solve_flow");
        pend(RR_PGO_K_BIG_SOLVE, 2);
      } else if (p.l11 == L11_SP) {
        // wide pivot blocks: one launch per 128-column super-panel, L11 read by the whole chip
        for (int ell = 0; ell < p.n_sp; ell++) {
          hipLaunchKernelGGL(k_big_solve_sp<T>, dim3(p.l11_gx, p.nf), dim3(1024), 0, stream_, a, ell, (const T *)gemv_part_.p, (int64_t)g_.dim, p.R);
          check_launch("k_big_solve_sp");
        }
        pend(RR_PGO_K_BIG_SOLVE, 1 + p.n_sp);
      } else {
        hipLaunchKernelGGL((k_solve_mid<T, 1024>), dim3(p.nf), dim3(1024), lds, stream_, a, 1, (const T *)gemv_part_.p, (int64_t)g_.dim, p.R);
        pend(RR_PGO_K_BIG_SOLVE, 2);
      }
    }
  }

  // k_update: launch_step  the solved step -> reference order (dx_ref_) and, unless STEP_EXPORT, onto the state; gauge: Lin::gauge of its system
  //           launch_dx    sign * dx_ref_ onto the state: a caller's step, Levenberg-Marquardt's undo (never the anchor gauge); gate: only where that device word says so
  void launch_step(bool gauge, StepUse use) {
    FinArgs fin{};
    if (use >= STEP_APPLY_REDUCE) {
      fin.enabled = 1; fin.chi_partial = chi_partial_.p; fin.n_chi = n_lin_blocks_; fin.hist = hist_.p; fin.counter = counter_.p;
      fin.advance = 1; fin.ring = HIST; fin.blocks_done = blocks_done_.p;
      if (use == STEP_APPLY_REDUCE_OPT) { fin.ctrl = opt_ctrl_.p; fin.ring_host = opt_ring_; fin.err = err_.p; }
    }
    launch_update(nullptr, 1.0, gauge, use == STEP_EXPORT, nullptr, fin);
  }
  void launch_dx(double sign, const int *gate = nullptr) { launch_update(dx_ref_.p, sign, false, false, gate, FinArgs{}); }
  void launch_update(const T *dx_ref_in, double sign, bool gauge, bool export_only, const int *gate, const FinArgs &fin) {
    pbegin();
    UpdArgs<T, S> u;
    u.n_nodes = n_list_;
    u.node_list = node_list_.p;
    u.norm_counts = norm_counts_.p;
    u.pose = pose_.p;
    u.node_dim = (is3d_ && !has_lm_) ? nullptr : node_dim_.p;
    u.node_pcol = node_pcol_.p;
    u.node_offset = node_offset_.p;
    u.x = x_ptr_;
    u.dx_ref_in = dx_ref_in;
    u.dx_ref_out = dx_ref_in ? nullptr : dx_ref_.p;
    u.sign = (S)sign;
    u.norm_partial = norm_partial_.p;
    u.gauge_anchor = (!is3d_ && !dx_ref_in && gauge) ? g_.anchor_node : -1;
    u.export_only = export_only ? 1 : 0;
    u.err = dx_ref_in ? nullptr : err_.p;
    u.gate = gate;
    u.fixed = settings_.fixed.empty() ? nullptr : fixed_.p;
    u.fin = fin;
    if (has_lm_) hipLaunchKernelGGL((k_update_lm<T, S>), dim3(n_upd_blocks_), dim3(UPD_THREADS), 0, stream_, u);
    else if (is3d_) hipLaunchKernelGGL((k_update<T, S, 6>), dim3(n_upd_blocks_), dim3(UPD_THREADS), 0, stream_, u);
    else hipLaunchKernelGGL((k_update<T, S, 3>), dim3(n_upd_blocks_), dim3(UPD_THREADS), 0, stream_, u);
    check_launch("k_update");
    pend(RR_PGO_K_UPDATE);
  }

  enum Partials { CHI2_PARTIALS, NORM_PARTIALS };
  void launch_finalize(Partials which) {   // the sum of the chi2 or of the |dx|^2 partials -> the current slot
    pbegin();
    hipLaunchKernelGGL(k_finalize_slot, dim3(1), dim3(256), 0, stream_, chi_partial_.p, which == CHI2_PARTIALS ? n_lin_blocks_ : 0,
                       norm_partial_.p, which == NORM_PARTIALS ? n_upd_blocks_ : 0, hist_.p, counter_.p, 0);
    pend(RR_PGO_K_REDUCE);
  }

  // linearise and factor (what the factor queries need), and the back substitution behind them: the system of `m`, in its gauge
  void enqueue_factor(const Lin &m, const OptLin *opt = nullptr) { launch_linearize(m, opt); launch_factor_range(0, sym_.steps.size(), m.gauge); }
  void enqueue_solve(const Lin &m, const OptLin *opt = nullptr) { enqueue_factor(m, opt); launch_solve(); }
  // one Gauss-Newton iteration: chi2(state) -> slot.chi, |dx| -> slot.norm, slot++
  void enqueue_gn_iteration(const OptLin *opt = nullptr) {
    const Lin m = lin_system(0.0, 0);
    enqueue_solve(m, opt);
    launch_step(m.gauge, opt ? STEP_APPLY_REDUCE_OPT : STEP_APPLY_REDUCE);   // + the reduction of the chi2 / |dx|^2 partials in its last workgroup
  }

  // what `body` puts on the stream, as an executable hipGraph
  template <typename F> hipGraphExec_t capture(F &&body) {
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    try {
      body();
    } catch (...) {
      // a failed launch must not leave the (pooled) stream in capture mode
      (void)hipStreamEndCapture(stream_, &graph);
      if (graph) (void)hipGraphDestroy(graph);
      throw;
    }
    HIPCHK(hipStreamEndCapture(stream_, &graph));
    hipGraphExec_t exec = nullptr;
    const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) throw ApiError(RR_PGO_ENODEVICE, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
    return exec;
  }
  // the captured graphs hold kernels, pointers and arguments of the time of their capture
  void drop_stage_graphs() {
    for (hipGraphExec_t &e : stage_exec_) if (e) { (void)hipGraphExecDestroy(e); e = nullptr; }
  }
  void drop_graphs() {
    if (gn_exec_) { (void)hipGraphExecDestroy(gn_exec_); gn_exec_ = nullptr; }
    drop_stage_graphs();
  }
  void ensure_gn_graph() {
    clear_stop_word();   // before the capture and before every replay: the graph holds no memset, and its replays pass no launch_linearize
    if (gn_exec_) return;
    gn_exec_ = capture([&] { enqueue_gn_iteration(); });
    launch_counts[3]++;
  }

  // One host round trip per iteration: the two scalars and the device error flag come back in
  // two async copies behind a single stream synchronisation.
  void read_slot(int slot, double *chi, double *norm) {
    int *eflag = reinterpret_cast<int *>(host_pair_.p + 2);
    HIPCHK(hipMemcpyAsync(host_pair_.p, hist_.p + 2 * (slot % HIST), 2 * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(eflag, err_.p, sizeof(int), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    if (chi) *chi = host_pair_[0];
    if (norm) *norm = host_pair_[1];
    throw_on_flag(*eflag);
  }

  void throw_on_flag(int e) {
    if (!e) return;
    HIPCHK(hipMemsetAsync(err_.p, 0, sizeof(int), stream_));
    // (a launch that drains after a timed-out hand-off computes on tiles that are not there: whatever else it flags is noise)
    if (e & DEVERR_FLOW_TIMEOUT)
      throw ApiError(RR_PGO_ETIMEOUT, "a hand-off between workgroups of one launch timed out; the step was not applied");
    if (e & DEVERR_NOT_SPD) throw ApiError(RR_PGO_ENOTSPD, "normal matrix is not positive definite (non-positive pivot)");
    throw ApiError(RR_PGO_ENODEVICE, "device-side error flag " + std::to_string(e));
  }

  void check_device_error() {
    int *eflag = reinterpret_cast<int *>(host_pair_.p + 2);
    HIPCHK(hipMemcpyAsync(eflag, err_.p, sizeof(int), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    throw_on_flag(*eflag);
  }

  void reset_counter() {
    HIPCHK(hipMemsetAsync(counter_.p, 0, sizeof(int), stream_));
    host_counter_ = 0;
  }

  double chi2_now() {
    reset_counter();
    launch_linearize(lin_chi2());
    launch_finalize(CHI2_PARTIALS);
    double c = 0;
    read_slot(0, &c, nullptr);
    return c;
  }

 public:
  // On a handle that holds ONE RANK's share of a graph (world_size > 1) these three would return rank-partial
  // results (chi2 of the edges this rank owns, partial diagonal blocks of the shared nodes, an update of this
  // rank's nodes only): refused -- rr_pgo_stage(h, 2) + the sum all-reduce of exchange buffer 1 is the chi2 of a
  // sharded graph, rr_pgo_stage(h, 0 / 1) its iteration.
  void refuse_rank_partial(const char *what) const {
    if (world_ > 1)
      throw ApiError(RR_PGO_EUNSUPPORTED, std::string(what) + " on one rank of a sharded graph would be rank-partial: use rr_pgo_stage + the two collectives");
  }
  void chi2(double *out) override { refuse_rank_partial("rr_pgo_chi2"); *out = chi2_now(); }

  void linearize_solve(double lambda, int lm, double *dx_out) override {
    if (sharded_) throw ApiError(RR_PGO_EUNSUPPORTED, "sharded handle: drive it with rr_pgo_stage + the two collectives");
    const Lin m = lin_system(lambda, lm);
    enqueue_solve(m);
    launch_step(m.gauge, STEP_EXPORT);   // permuted solution -> reference order (and the anchor gauge), state untouched
    std::vector<T> tmp((size_t)g_.dim);
    HIPCHK(hipMemcpyAsync(tmp.data(), dx_ref_.p, tmp.size() * sizeof(T), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    check_device_error();
    for (int i = 0; i < g_.dim; i++) dx_out[i] = (double)tmp[i];
  }

  void update(const double *dx, double sign) override {
    refuse_rank_partial("rr_pgo_update");
    std::vector<T> tmp((size_t)g_.dim);
    for (int i = 0; i < g_.dim; i++) tmp[i] = (T)dx[i];
    HIPCHK(hipMemcpyAsync(dx_ref_.p, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice, stream_));
    launch_dx(sign);
    HIPCHK(hipStreamSynchronize(stream_));
  }

  // optimize(), pose_graph_optimization.rs:247-303
  void optimize(int solver, int iters, double *errors, int *n_errors, double *norms) override {
    if (sharded_) throw ApiError(RR_PGO_EUNSUPPORTED, "sharded handle: drive it with rr_pgo_stage + the two collectives");
    // (an iteration of dozens of launches -- the 1M-edge lattice: 67, 4.4 ms -- gains nothing from the loop on the device: a host
    // round trip is 0.5 % of its iteration, and the item behind the stop would be dozens of empty launches.  Built and measured, r06:
    // 4.55 against 4.50 ms per iteration through optimize(), also with only the next linearisation enqueued ahead.)
    if (!edge_lin_ && !sync_optimize_ && !prof_.on && n_launches_per_iter < 48) {
      optimize_pipelined(solver, iters, errors, n_errors, norms);
      return;
    }
    const double tolerance = 1e-4;  // :253
    int ne = 0;
    if (solver == RR_PGO_GAUSS_NEWTON) {
      // chi2 of the state BEFORE an update comes out of that iteration's own
      // linearisation pass, so errors[i] is known once iteration i has run and
      // one chi2-only pass after the loop supplies the last entry.
      // an iteration of a handful of launches (the dataflow form of the small graphs: four) is enqueued as it is; capturing
      // and instantiating a hipGraph costs more than ten such iterations save (the closure the reference's bench times,
      // benches/graph_slam.rs:9-10, is ONE new() + optimize(10)).  Graphs of dozens of launches replay a captured graph.
      // (optimize() reads two scalars back after every iteration, so the enqueueing is not hidden behind the device as it is
      // in iterate_async: dozens of launches stay one graph launch here.)  RR_PGO_FORCE_GRAPH=1: always the graph.
      const bool eager = (no_graph_ || n_launches_per_iter <= 8) && !gn_exec_ && !force_graph_;
      if (!eager) ensure_gn_graph();
      reset_counter();
      for (int i = 0; i < iters; i++) {
        if (eager) enqueue_gn_iteration();
        else HIPCHK(hipGraphLaunch(gn_exec_, stream_));
        launch_counts[eager ? 0 : 1]++;
        double chi, nrm;
        read_slot(i, &chi, &nrm);
        errors[ne++] = chi;
        if (norms) norms[i] = nrm;
        if (nrm < tolerance) break;  // :298-300
      }
      errors[ne++] = chi2_now();
    } else {
      double lambda = 0.01;  // :254
      double last_error = chi2_now();
      errors[ne++] = last_error;
      for (int i = 0; i < iters; i++) {
        reset_counter();
        launch_counts[0]++;
        const Lin m = lin_system(lambda, 1);
        enqueue_solve(m);
        launch_step(m.gauge, STEP_APPLY);
        launch_finalize(NORM_PARTIALS);
        launch_linearize(lin_chi2());
        launch_finalize(CHI2_PARTIALS);
        double error, nrm;
        read_slot(0, &error, &nrm);
        if (last_error < error) {  // :276-281
          launch_dx(-1.0);
          lambda *= 2.0;
        } else {
          lambda /= 2.0;
        }
        last_error = error;  // :284
        if (norms) norms[i] = nrm;
        errors[ne++] = error;
        if (nrm < tolerance) break;
      }
      HIPCHK(hipStreamSynchronize(stream_));
    }
    *n_errors = ne;
  }

  // ---- rr_pgo_optimize without a host round trip per iteration (on the small graphs an iteration is a few launches of
  // 0.1 - 0.6 ms altogether, and a stream synchronisation + two copies per iteration were ~25 us of idle device; handles of
  // fewer than 48 launches per iteration).
  // The loop of :247-303 is cut into ITEMS, each a fixed sequence of launches whose last kernel publishes (chi2, |dx|, flags)
  // in the host-coherent ring and -- on the device -- takes the decisions the reference takes on the host: the stop rule
  // (:298-300, the stop word err[1]: every later launch of the call is empty or leaves the state alone), Levenberg-
  // Marquardt's accept / reject and lambda (:275-282), the end of the call after a failed factorisation (:271).
  //   Gauss-Newton          item k < n: iteration k (k_linearize ... k_update; chi2 of the state BEFORE the step and |dx|);
  //                         item n: chi2 of the final state.  After a stop in iteration k, item k + 1 IS that chi2 (its
  //                         linearisation runs, the rest is skipped): the errors are the reference's list, shifted by one
  //   Levenberg-Marquardt   item 0: the initial error (:255); item k: iteration k - 1 = step, chi2, decision, gated undo
  // The host keeps ONE item queued behind the one that is running (enqueueing an item takes a fraction of its run time), polls
  // the ring, and stops enqueueing when it sees the stop: optimize(100) that stops after 6 iterations pays one skipped item.
  // the running call, owned by optimize_pipelined; reset_due: no launch of it has been enqueued yet, the first one resets the loop state
  struct OptCall { bool lm; double lambda0; bool reset_due; };
  void enqueue_opt_item(OptCall &call, long k, int iters) {
    const bool reset = std::exchange(call.reset_due, false);   // for the item's first launch; every linearisation is also told what it publishes and where its lambda comes from
    OptItemArgs oi{};
    oi.chi_partial = chi_partial_.p; oi.norm_partial = norm_partial_.p; oi.n_chi = n_lin_blocks_; oi.n_norm = 0; oi.mode = 0;
    oi.ctrl = opt_ctrl_.p; oi.ring = opt_ring_; oi.err = err_.p;
    launch_counts[2]++;
    if (!call.lm) {
      // an iteration: its linearisation publishes only when the stop word is set (then the rest of the item is empty
      // launches); the item behind the last iteration: chi2 only, published by the linearisation's last workgroup
      const OptLin o{reset, call.lambda0, k < iters ? 1 : 2, false};
      if (k < iters) enqueue_gn_iteration(&o);
      else launch_linearize(lin_chi2(), &o);
      return;
    }
    if (k > 0) {
      // (as Gauss-Newton's: behind the stop this linearisation publishes the skipped item, every launch behind it returns at its stop word)
      const Lin m = lin_system(0.0, 1);
      const OptLin o{reset, call.lambda0, 1, true};   // lambda: OptCtrl::lambda
      enqueue_solve(m, &o);
      launch_step(m.gauge, STEP_APPLY);
      oi.n_norm = n_upd_blocks_; oi.mode = 1;
    }
    const OptLin chi_only{k == 0 && reset, call.lambda0, 0, false};   // (k_opt_item publishes)
    launch_linearize(lin_chi2(), &chi_only);
    hipLaunchKernelGGL(k_opt_item, dim3(1), dim3(256), 0, stream_, oi);
    check_launch("k_opt_item");
    if (k > 0) launch_dx(-1.0, &opt_ctrl_.p->reject);   // :277, when the device decided so
  }
  // the slot of item `idx` (0-based); false: the stream went idle or failed without publishing it
  bool wait_opt_slot(long idx, OptSlot *out) {
    volatile OptSlot *s = opt_ring_ + idx % OPT_RING;
    const unsigned long long want = (unsigned long long)idx + 1;
    double t_query = now_ms();
    for (unsigned spins = 0;; spins++) {
      if (__atomic_load_n(const_cast<unsigned long long *>(&s->seq), __ATOMIC_ACQUIRE) == want) break;
      __builtin_ia32_pause();
      if ((spins & 1023u) == 1023u && now_ms() - t_query > 1.0) {
        // every wait inside a launch is bounded, so the stream always drains: an idle stream without the slot is a lost launch
        const hipError_t q = hipStreamQuery(stream_);
        if (q == hipSuccess) {
          if (__atomic_load_n(const_cast<unsigned long long *>(&s->seq), __ATOMIC_ACQUIRE) == want) break;
          return false;
        }
        if (q != hipErrorNotReady) throw ApiError(RR_PGO_ENODEVICE, std::string("hipStreamQuery: ") + hipGetErrorString(q));
        t_query = now_ms();
      }
    }
    out->chi2 = s->chi2; out->norm = s->norm; out->flags = s->flags; out->seq = want;
    return true;
  }
  void optimize_pipelined(int solver, int iters, double *errors, int *n_errors, double *norms) {
    const bool lm = solver != RR_PGO_GAUSS_NEWTON;
    const long total = (long)iters + 1;
    for (int i = 0; i < OPT_RING; i++) opt_ring_[i].seq = 0ull;   // (nothing of an earlier call is in flight: every call consumes what it enqueued)
    struct Scope {   // whatever happens, the launches behind this call know about the stop word
      Engine *e;
      bool done = false;
      ~Scope() {
        e->stop_dirty_ = true;
        // left by an exception (a failed launch, a lost item): what is still enqueued must not publish into the next call's ring
        if (!done) (void)hipStreamSynchronize(e->stream_);
      }
    } scope{this};
    OptCall call{lm, 0.01, true};   // :254
    // TWO whole items in the queue: the device never waits for the host.  The item behind the stop is its linearisation (which
    // publishes the final chi2: the call returns on that) and a handful of launches that read the stop word and nothing else
    //  -- they are still on the stream when the call returns, and whatever is enqueued next runs behind them
    long enq = 0, seen = 0;   // items enqueued / consumed
    int ne = 0, dev_err = 0;
    bool stop_seen = false;
    while (true) {
      while (enq < total && enq < seen + 2 && !stop_seen) enqueue_opt_item(call, enq++, iters);
      if (seen >= enq) break;
      OptSlot sl;
      if (!wait_opt_slot(seen, &sl)) {
        HIPCHK(hipStreamSynchronize(stream_));
        check_device_error();
        throw ApiError(RR_PGO_ENODEVICE, "internal: an item of rr_pgo_optimize was never published");
      }
      const long k = seen++;
      const int e = sl.flags >> OPT_ERR_SHIFT;
      if (e) { dev_err = e; stop_seen = true; continue; }
      if (!lm) {
        if (k == iters || (sl.flags & OPT_SKIPPED)) { if (!dev_err) errors[ne++] = sl.chi2; continue; }   // chi2 of the final state
        errors[ne++] = sl.chi2;
        if (norms) norms[k] = sl.norm;
      } else {
        if (sl.flags & OPT_SKIPPED) continue;
        errors[ne++] = sl.chi2;
        if (k > 0 && norms) norms[k - 1] = sl.norm;
      }
      if (sl.flags & OPT_STOP) stop_seen = true;
    }
    scope.done = true;   // every item that was enqueued has been consumed
    if (dev_err) throw_on_flag(dev_err);
    *n_errors = ne;
  }

  void get_state(double *out) override {
    const int N = g_.n_nodes();
    std::vector<V4> pose(pose_.n);
    HIPCHK(hipMemcpyAsync(pose.data(), pose_.p, pose.size() * sizeof(V4), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    const size_t per = is3d_ ? 2 : 1;
    for (int i = 0; i < N; i++) out += unpack_v4(g_.node_kind[i], &pose[per * i], out);
  }

  // (the poses go through a pinned staging buffer into a device-side copy, from there into the state, and the call does not
  // wait for either copy; the state of the previous call is remembered, so setting the SAME state again -- restarting a run,
  // what the benchmark does between two optimize() calls -- costs the host a comparison and one small launch instead of the
  // conversion loop (a cosine and a sine per pose) and a host-to-device copy)
  void restore_saved_state() { copy_words16(pose_saved_.p, pose_.p, pose_.n * sizeof(V4)); }
  void set_state(const double *st) override {
    const int N = g_.n_nodes();
    const size_t n_in = g_.node_state.size();
    if (state_stage_.p && state_in_.size() == n_in && std::memcmp(state_in_.data(), st, n_in * sizeof(double)) == 0) {
      restore_saved_state();
      return;
    }
    if (!state_stage_.p) {
      state_stage_.alloc(pose_.n, false);
      state_stage_ev_.create(hipEventDisableTiming);
      pose_saved_.alloc(pose_.n);
    } else {
      HIPCHK(hipEventSynchronize(state_stage_ev_));   // the previous copy out of the buffer has been made
    }
    state_in_.assign(st, st + n_in);
    V4 *pose = state_stage_.p;
    if (is3d_ && has_lm_) for (int i = 0; i < N; i++) st += pack_v4(g_.node_kind[i] == NODE_XYZ ? NODE_XYZ : NODE_SE3, st, pose + 2 * (size_t)i);
    else if (is3d_) for (int i = 0; i < N; i++) st += pack_v4(NODE_SE3, st, pose + 2 * (size_t)i);   // (split as in the constructor)
    else for (int i = 0; i < N; i++) st += pack_v4(g_.node_kind[i] == NODE_SE2 ? NODE_SE2 : NODE_XY, st, pose + i);
    HIPCHK(hipMemcpyAsync(pose_saved_.p, pose, pose_.n * sizeof(V4), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipEventRecord(state_stage_ev_, stream_));
    restore_saved_state();
  }

  // ---- rr_pgo_extend
  const void *pose_dev() const override { return pose_.p; }
  size_t pose_node_bytes() const override { return (is3d_ ? 2 : 1) * sizeof(V4); }
  const void *guess_dev() const override { return guess_stage_.p; }
  // HIP-event time, in ms, of what `work` puts on the stream; waits for it
  template <typename F> double timed_ms(F &&work) {
    EventHolder ev0, ev1;
    ev0.create(hipEventDefault);
    ev1.create(hipEventDefault);
    HIPCHK(hipEventRecord(ev0, stream_));
    work();
    HIPCHK(hipEventRecord(ev1, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, ev0, ev1));
    return t;
  }
  void copy_words16(const void *src, void *dst, size_t bytes) {
    const int64_t n16 = (int64_t)(bytes / 16);
    if (n16 == 0) return;
    hipLaunchKernelGGL(k_copy_words16, dim3((unsigned)std::min<int64_t>((n16 + 255) / 256, 1024)), dim3(256), 0, stream_,
                       reinterpret_cast<const uint4 *>(src), reinterpret_cast<uint4 *>(dst), n16);
    check_launch("k_copy_words16");
  }
  void guess_nodes(const std::vector<HostGuessStep> &steps, const std::vector<int32_t> &tree_ptr, int n_old, int n_total, bool is3d,
                   const int32_t *new_kind, double *out, double *ms) override {
    const size_t per = is3d ? 2 : 1;
    if (n_old > 0 && is3d != is3d_) throw ApiError(RR_PGO_EINVAL, "internal: 2-D / 3-D form of the guess");
    std::vector<GuessStep<S>> ds(steps.size());
    for (size_t k = 0; k < steps.size(); k++) {
      const HostGuessStep &h = steps[k];
      if (h.src < 0 || h.src >= n_total || h.dst < n_old || h.dst >= n_total) throw ApiError(RR_PGO_EINVAL, "internal: guess step out of range");
      GuessStep<S> &d = ds[k];
      d.src = h.src; d.dst = h.dst; d.op = h.op; d.pad = 0;
      V4 m[2] = {};
      pack_v4(h.op == GUESS_XY ? EDGE_SE2_XY : h.op == GUESS_XYZ ? EDGE_SE3_XYZ : h.op == GUESS_SE3 || h.op == GUESS_SE3_INV ? EDGE_SE3 : EDGE_SE2, h.m, m);
      d.m0 = m[0];
      d.m1 = m[1];
    }
    const int n_trees = (int)tree_ptr.size() - 1;
    DevBuf<GuessStep<S>> dsteps;   // (no arena outside the constructor: buffers of their own, freed on return)
    DevBuf<int32_t> dtree;
    guess_stage_.alloc(per * (size_t)n_total);
    HIPCHK(hipMemsetAsync(guess_stage_.p, 0, guess_stage_.n * sizeof(V4), stream_));
    dsteps.alloc(ds.size());
    dtree.alloc(tree_ptr.size());
    HIPCHK(hipMemcpyAsync(dsteps.p, ds.data(), ds.size() * sizeof(GuessStep<S>), hipMemcpyHostToDevice, stream_));
    HIPCHK(hipMemcpyAsync(dtree.p, tree_ptr.data(), tree_ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    *ms = timed_ms([&] {
      copy_words16(pose_.p, guess_stage_.p, per * (size_t)n_old * sizeof(V4));
      hipLaunchKernelGGL((k_guess_nodes<S>), dim3((unsigned)((n_trees + 63) / 64)), dim3(64), 0, stream_, guess_stage_.p, n_total, is3d ? 1 : 0,
                         dsteps.p, dtree.p, n_trees);
      check_launch("k_guess_nodes");
    });
    std::vector<V4> pose(per * (size_t)(n_total - n_old));
    HIPCHK(hipMemcpyAsync(pose.data(), guess_stage_.p + per * (size_t)n_old, pose.size() * sizeof(V4), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    for (int i = 0; i < n_total - n_old; i++) out += unpack_v4(new_kind[i], &pose[per * i], out);
  }
  void adopt_state(const void *src, size_t n_nodes, double *ms) override {
    if (n_nodes > (size_t)g_.n_nodes()) throw ApiError(RR_PGO_EINVAL, "internal: more nodes adopted than the graph has");
    *ms = timed_ms([&] { copy_words16(src, pose_.p, n_nodes * pose_node_bytes()); });
  }
  const HandleSettings &settings() const override { return settings_; }

  void assemble(double lambda, int lm, std::vector<double> &hv, std::vector<double> &b) override {
    refuse_rank_partial("rr_pgo_assemble");
    launch_linearize(lin_reference_system(lambda, lm));   // always the reference's system (anchor prior), whatever the factor's gauge
    std::vector<T> th((size_t)sym_.n_hvals), tb((size_t)g_.dim);
    HIPCHK(hipMemcpyAsync(th.data(), hvals_.p, th.size() * sizeof(T), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(tb.data(), b_.p, tb.size() * sizeof(T), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    hv.assign(th.begin(), th.end());
    b.assign(tb.begin(), tb.end());
  }

  void iterate_async(int iters) override {
    if (sharded_) throw ApiError(RR_PGO_EUNSUPPORTED, "sharded handle: drive it with rr_pgo_stage + the two collectives");
    // RR_PGO_NO_GRAPH=1: plain launches (rocprofv3 --kernel-trace crashes on replays of graphs
    // with thousands of nodes; profiling runs of the large workloads use this switch)
    // plain launches queue back to back while consecutive graph launches leave the GPU idle for ~8 us each (rocprofv3
    // --kernel-trace, scripts/kernel_gaps.py), and the host stays far ahead of the device even at 67 launches per iteration
    // (the 1M-edge lattice: ~0.2 ms of enqueueing against 4.4 ms of kernels).  Measured: intel + 2 %, sphere2500 + 0.8 %,
    // lattice + 0.7 %.  RR_PGO_FORCE_GRAPH=1: replays of the captured hipGraph (r01 - r03's form).
    if (no_graph_ || !force_graph_) {
      for (int i = 0; i < iters; i++) { enqueue_gn_iteration(); launch_counts[0]++; }
      return;
    }
    ensure_gn_graph();
    for (int i = 0; i < iters; i++) { HIPCHK(hipGraphLaunch(gn_exec_, stream_)); launch_counts[1]++; }
  }

  void sync() override {
    HIPCHK(hipStreamSynchronize(stream_));
    check_device_error();
  }

  int schur_tile() const override { return schur_split_ ? schur_tile_ : 0; }
  void solve_form(int32_t *kform, double *k_bytes, double *k_flops) const override {
    *kform = kform_ ? 1 : 0;
    if (k_bytes) *k_bytes = kform_bytes_;
    if (k_flops) *k_flops = kform_flops_;
  }
  void mark_flow_fronts(std::vector<char> &in_flow) override {
    for (size_t si = 0; si < plan_.size(); si++)
      if (plan_[si].flow)
        for (int t = sym_.steps[si].task_begin; t < sym_.steps[si].task_end; t++)
          in_flow[sym_.task_sn[sym_.task_ptr[t]]] = plan_[si].flow->schur_split ? 1 : 2;   // 2: its Schur tiles are UPDATE tasks too
  }
  // diagnostic builds: the task list and the stamps of the `level`-th flow level (-1: no such level)
  int flow_trace(int level, std::vector<int32_t> &tasks, std::vector<unsigned long long> &stamps, int *nf, double *est_us) override {
    if (xl_) {
      // the cross-level list as "level 0": the front slot of every task replaced by its SUPERNODE (slots repeat from level to level)
      if (level != 0) return -1;
      tasks.resize(xl_host_.size() * 4);
      size_t i = 0;
      for (size_t si = 0; si < plan_.size(); si++) {
        if (!plan_[si].flow) continue;
        const Step &st = sym_.steps[si];
        for (int k2 = 0; k2 < plan_[si].flow->n_tasks; k2++, i++) {
          const FlowTask &t = xl_host_[i].t;
          const int sn = sym_.task_sn[sym_.task_ptr[st.task_begin + (t.kind_front & 0xffffff)]];
          tasks[4 * i] = (t.kind_front & ~0xffffff) | sn;
          tasks[4 * i + 1] = t.p0; tasks[4 * i + 2] = t.p1; tasks[4 * i + 3] = t.p2;
        }
      }
      stamps.resize(xl_trace_.n);
      if (xl_trace_.n) HIPCHK(hipMemcpy(stamps.data(), xl_trace_.p, xl_trace_.n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      *nf = sym_.S;
      *est_us = 0;
      return (int)xl_host_.size();
    }
    int k = 0;
    for (size_t si = 0; si < plan_.size(); si++) {
      if (!plan_[si].flow) continue;
      if (k++ != level) continue;
      FlowLevel &l = *plan_[si].flow;
      tasks.resize(l.host_tasks.size() * 4);
      if (!l.host_tasks.empty()) std::memcpy(tasks.data(), l.host_tasks.data(), l.host_tasks.size() * sizeof(FlowTask));
      stamps.resize(l.trace.n);
      if (l.trace.n) HIPCHK(hipMemcpy(stamps.data(), l.trace.p, l.trace.n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      *nf = sym_.steps[si].task_end - sym_.steps[si].task_begin;
      *est_us = l.est_us;
      return l.n_tasks;
    }
    return -1;
  }

  void read_stamps(std::vector<unsigned long long> &out) override {
    out.resize(stamps_.n);
    if (stamps_.n) HIPCHK(hipMemcpy(out.data(), stamps_.p, stamps_.n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }

  // ---- sharded execution: one GN iteration = stage 0, all-gather of exchange buffer 0, stage 1, sum all-reduce
  // of exchange buffer 1 (two doubles).  Both collectives are the caller's (RCCL), issued on this stream.
  void exchange_buffer(int which, void **ptr, int64_t *n, int32_t *esize) override {
    if (!sharded_) throw ApiError(RR_PGO_EINVAL, "handle is not sharded");
    if (which == 0) { *ptr = xch_; *n = xch_n_; *esize = (int32_t)sizeof(T); }
    else if (which == 1) { *ptr = scal_; *n = 2; *esize = (int32_t)sizeof(double); }
    else throw ApiError(RR_PGO_EINVAL, "exchange buffer index must be 0 or 1");
  }
  void set_exchange_buffer(int which, void *ptr, int64_t n) override {
    if (!sharded_) throw ApiError(RR_PGO_EINVAL, "handle is not sharded");
    drop_stage_graphs();   // captured pointers
    if (which == 0 && n >= xch_n_) xch_ = (T *)ptr;
    else if (which == 1 && n >= 2) scal_ = (double *)ptr;
    else throw ApiError(RR_PGO_EINVAL, "exchange buffer index / size mismatch");
  }
  void enqueue_stage(int stg, double lambda, int lm, bool gauge) {   // gauge: Lin::gauge of the pair's system (stage 2: unused)
    const size_t n_local = world_ > 1 ? (size_t)sym_.n_local_steps : sym_.steps.size();
    if (stg == 0) {
      // linearise this rank's nodes (own + shared top separators), factor its own subtrees, publish the
      // boundary fronts' update matrices in this rank's chunk of buffer 0
      launch_linearize(Lin{1, gauge, lm, lambda});
      if (n_shared_ > 0)   // this rank's partial sums of the shared nodes' diagonal blocks and rhs, behind its update matrices
        hipLaunchKernelGGL(k_pack_shared<T>, dim3((n_shared_ + 255) / 256), dim3(256), 0, stream_, shared_src_.p, n_shared_,
                           (const T *)hvals_.p, (const T *)b_.p, xch_ + (int64_t)rank_ * sym_.xch_chunk + sym_.xch_shared_off);
      launch_factor_range(0, n_local, gauge);
      if (n_pack_ > 0) {
        hipLaunchKernelGGL(k_pack_boundary<T>, dim3(std::min(pack_max_nu_, 1024), n_pack_), dim3(256), 0, stream_,
                           factor_args(0), pack_list_.p);
        check_launch("k_pack_boundary");
      }
      if (world_ > 1)   // this rank's error flag travels with its chunk (the group must agree on ENOTSPD)
        hipLaunchKernelGGL(k_pack_err<T>, dim3(1), dim3(64), 0, stream_, (const int *)err_.p,
                           xch_ + (int64_t)rank_ * sym_.xch_chunk + sym_.xch_flag_off);
    } else if (stg == 1) {
      // after the all-gather: the shared top fronts (every rank, identical), the back substitution of the top
      // and of this rank's subtrees, the update of this rank's nodes, its partial chi2 / |dx|^2
      if (n_shared_ > 0)   // the shared nodes' diagonal blocks and rhs: the P partial sums, added in rank order
        hipLaunchKernelGGL(k_sum_shared<T>, dim3((n_shared_ + 255) / 256), dim3(256), 0, stream_, shared_src_.p, n_shared_, hvals_.p, b_.p,
                           (const T *)xch_, sym_.xch_chunk, sym_.xch_shared_off, world_);
      if (world_ > 1)
        hipLaunchKernelGGL(k_merge_err<T>, dim3(1), dim3(64), 0, stream_, err_.p, (const T *)xch_, sym_.xch_chunk, sym_.xch_flag_off, world_);
      launch_factor_range(n_local, sym_.steps.size(), gauge);
      launch_solve();
      launch_step(gauge, STEP_APPLY);
      hipLaunchKernelGGL(k_finalize_partial, dim3(1), dim3(256), 0, stream_, chi_partial_.p, n_lin_blocks_, norm_partial_.p,
                         n_upd_blocks_, scal_);
    } else {
      // chi2 of the current state only (the last entry of optimize()'s error list): partial sum -> buffer 1
      launch_linearize(lin_chi2());
      hipLaunchKernelGGL(k_finalize_partial, dim3(1), dim3(256), 0, stream_, chi_partial_.p, n_lin_blocks_, norm_partial_.p, 0, scal_);
    }
    check_launch("stage");
  }
  void stage(int stg, double lambda, int lm) override {
    if (!sharded_) throw ApiError(RR_PGO_EINVAL, "handle is not sharded");
    if (stg < 0 || stg > 2) throw ApiError(RR_PGO_EINVAL, "stage must be 0, 1 or 2");
    // stage 1 factors the top fronts in the gauge stage 0 linearised in, whatever lm it is given; the captured graphs hold the
    // Gauss-Newton gauge, so a stage 1 behind a Levenberg-Marquardt stage 0 that differs in it is plain launches
    if (stg == 0) stage_gauge_ = gauge_rule(lm);
    if (stg == 2 || lm || no_graph_ || stage_gauge_ != gauge_rule(0)) { enqueue_stage(stg, lambda, lm, stage_gauge_); return; }
    if (!stage_exec_[stg])   // Gauss-Newton stages replay a captured graph like the unsharded iteration
      stage_exec_[stg] = capture([&] { enqueue_stage(stg, 0.0, 0, gauge_rule(0)); });
    HIPCHK(hipGraphLaunch(stage_exec_[stg], stream_));
  }
  // (chi2, |dx|) of the last stage-1 / stage-2 call, valid once the caller has all-reduced buffer 1
  void read_last_scalars(double *chi, double *norm) override {
    if (!sharded_) throw ApiError(RR_PGO_EINVAL, "handle is not sharded");
    int *eflag = reinterpret_cast<int *>(host_pair_.p + 2);
    HIPCHK(hipMemcpyAsync(host_pair_.p, scal_, 2 * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipMemcpyAsync(eflag, err_.p, sizeof(int), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    *chi = host_pair_[0];
    *norm = std::sqrt(host_pair_[1]);
    throw_on_flag(*eflag);
  }

  // ---- robust kernels (include/rr_pgo.h, rr_pgo_set_robust_kernel)
  void set_robust(int kind, double delta, double mu, std::vector<uint8_t> m) override {   // m: empty, or 0 / 1 per edge
    if (kind == ROBUST_NONE) m.clear();
    if (!m.empty() && m.size() != (size_t)g_.n_edges()) throw ApiError(RR_PGO_EINVAL, "internal: robust mask of another graph");
    HIPCHK(hipStreamSynchronize(stream_));   // launches already enqueued read the old mask
    robust_mask_.upload(m);                  // (empty: freed, every edge)
    settings_.robust_mask = std::move(m);
    settings_.robust_kind = kind;
    settings_.robust_delta = kind != ROBUST_NONE ? delta : 1.0;
    settings_.robust_mu = kind == ROBUST_TLS ? mu : 0.0;
    // the captured graphs hold the old kernel and its arguments
    drop_graphs();
    // the edge-parallel experiment forms have no robust instantiation: the pull form runs while a kernel is set
    edge_lin_ = edge_lin_env_ && kind == ROBUST_NONE;
    edge_lin_wave_ = edge_lin_wave_env_ && kind == ROBUST_NONE;
    n_lin_blocks_ = edge_lin_ ? lin_blocks_edge_ : lin_blocks_pull_;
  }
  // mu alone (rr_pgo_set_robust_mu): a kernel argument of every later launch.  The captured graphs hold the old value: dropped
  // (behind whatever replay is still on the stream), so the next iteration captures anew.  No mask upload, no allocation.
  void set_robust_mu(double mu) override {
    if (settings_.robust_kind != ROBUST_TLS) throw ApiError(RR_PGO_EINVAL, "rr_pgo_set_robust_mu: the handle's robust kernel is not RR_PGO_ROBUST_TLS");
    bool captured = gn_exec_ != nullptr;
    for (hipGraphExec_t e : stage_exec_) captured = captured || e != nullptr;
    if (captured) {
      HIPCHK(hipStreamSynchronize(stream_));
      drop_graphs();
    }
    settings_.robust_mu = mu;
  }
  // ---- graduated non-convexity on truncated least squares (include/rr_pgo.h, rr_pgo_optimize_gnc)
  // One scan: the k_edge_errors family into device memory, k_tls_scan over it, ONE synchronisation, four numbers read.
  struct TlsScan { double r2_max, rho; int frac, rej; };
  TlsScan tls_scan() {
    const int E = g_.n_edges(), nb = (E + 255) / 256;
    launch_edge_errors(gnc_sw_.p, gnc_sw_.p + E);
    TlsScanArgs<S> a;
    a.n_edges = E;
    a.s = gnc_sw_.p;
    a.w = gnc_sw_.p + E;
    a.mask = robust_mask_.n ? robust_mask_.p : nullptr;
    const TlsParams p = tls_params();
    a.delta2 = (S)(settings_.robust_delta * settings_.robust_delta);
    a.tls_lo = (S)p.lo; a.tls_hi = (S)p.hi; a.tls_cs = (S)p.cs; a.tls_mu = (S)p.mu;
    a.partial = gnc_partial_.p;
    a.blocks_done = gnc_done_.p;
    a.out = gnc_host_.p;
    hipLaunchKernelGGL((k_tls_scan<S>), dim3((unsigned)nb), dim3(256), 0, stream_, a);
    check_launch("k_tls_scan");
    HIPCHK(hipStreamSynchronize(stream_));
    return TlsScan{gnc_host_[0], gnc_host_[3], (int)gnc_host_[1], (int)gnc_host_[2]};
  }
  // the loop of the header, statement by statement; the iterations go through optimize(), the path of rr_pgo_optimize
  void optimize_gnc(int solver, const rr_pgo_gnc_options &o, const int32_t *mask, rr_pgo_gnc_result *res, double *stage_mu,
                    double *stage_cost) override {
    if (sharded_ || world_ > 1) throw ApiError(RR_PGO_EUNSUPPORTED, "rr_pgo_optimize_gnc on a sharded handle");
    const int E = g_.n_edges();
    if (E == 0) throw ApiError(RR_PGO_EINVAL, "rr_pgo_optimize_gnc: the graph has no edge");
    const size_t nb = ((size_t)E + 255) / 256;
    if (gnc_sw_.n < 2 * (size_t)E) gnc_sw_.alloc(2 * (size_t)E);
    if (gnc_partial_.n < 4 * nb) gnc_partial_.alloc(4 * nb);
    if (!gnc_done_.p) { gnc_done_.alloc(1); gnc_done_.zero(); }
    if (!gnc_host_.p) gnc_host_.alloc(4);
    *res = rr_pgo_gnc_result{};
    double ms[3] = {0, 0, 0};
    TlsScan sc{};
    auto scan = [&] { ms[0] += timed_ms([&] { sc = tls_scan(); }); };
    std::vector<double> errors((size_t)std::max(o.inner_iterations, o.final_iterations) + 2);
    int ne = 0;
    const double c2 = o.delta * o.delta;
    set_robust(ROBUST_TLS, o.delta, 1.0, mask_bytes(mask, g_.n_edges()));   // (the mask goes up once; the stages change mu alone)
    scan();
    res->r2_max = sc.r2_max;
    res->mu0 = 2.0 * sc.r2_max > c2 ? c2 / (2.0 * sc.r2_max - c2) : 1.0;
    double mu = res->mu0;
    for (int t = 0;; t++) {
      set_robust_mu(mu);
      res->mu_last = mu;
      ms[1] += timed_ms([&] { optimize(solver, o.inner_iterations, errors.data(), &ne, nullptr); });
      scan();
      if (stage_mu) stage_mu[t] = mu;
      if (stage_cost) stage_cost[t] = sc.rho;
      res->n_stages = t + 1;
      if (sc.frac == 0) { res->converged = 1; break; }
      if (t + 1 == o.max_stages) break;
      mu *= o.mu_factor;
    }
    if (o.final_iterations > 0) {
      ms[2] += timed_ms([&] { optimize(solver, o.final_iterations, errors.data(), &ne, nullptr); });
      res->final_iterations_run = ne - 1;
      scan();
    }
    res->n_rejected = sc.rej;
    res->n_fractional = sc.frac;
    res->cost_last = sc.rho;
    for (int k = 0; k < 3; k++) gnc_ms_[k] = ms[k];
  }
  void gnc_times(double *ms) const override { for (int k = 0; k < 3; k++) ms[k] = gnc_ms_[k]; }
  void edge_errors(double *s_out, double *w_out) override {
    if (sharded_) throw ApiError(RR_PGO_EUNSUPPORTED, "rr_pgo_edge_errors on a sharded handle");
    const int E = g_.n_edges();
    if (E == 0) return;
    DevBuf<double> out;
    out.alloc(2 * (size_t)E);
    launch_edge_errors(out.p, out.p + E);
    std::vector<double> host(2 * (size_t)E);
    HIPCHK(hipMemcpyAsync(host.data(), out.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    std::memcpy(s_out, host.data(), E * sizeof(double));
    if (w_out) std::memcpy(w_out, host.data() + E, E * sizeof(double));
  }
  // (s, w) of every edge into device memory: rr_pgo_edge_errors, and the scan of rr_pgo_optimize_gnc
  void launch_edge_errors(double *s_dev, double *w_dev) {
    const int E = g_.n_edges();
    EdgeErrArgs<S> a;
    a.n_edges = E;
    a.is3d = is3d_ ? (has_lm_ ? 2 : 1) : 0;
    a.kind = settings_.robust_kind;
    a.e_rec = e_rec_.p;
    a.pose = pose_.p;
    a.e_idx = e_idx_.p;
    a.e_meas = e_meas_.p;
    a.e_info = e_info3_.p;
    a.node_dim = node_dim_.p;
    a.delta = (S)settings_.robust_delta;
    a.delta2 = (S)(settings_.robust_delta * settings_.robust_delta);
    a.mask = robust_mask_.n ? robust_mask_.p : nullptr;
    a.s_out = s_dev;
    a.w_out = w_dev;
    const TlsParams p = tls_params();
    a.tls_lo = (S)p.lo; a.tls_hi = (S)p.hi; a.tls_cs = (S)p.cs; a.tls_mu = (S)p.mu;
    if (has_lm_) hipLaunchKernelGGL((k_edge_errors<S, true>), dim3((E + 255) / 256), dim3(256), 0, stream_, a);
    else if (has_br_) hipLaunchKernelGGL((k_edge_errors_br<S>), dim3((E + 255) / 256), dim3(256), 0, stream_, a);
    else hipLaunchKernelGGL((k_edge_errors<S>), dim3((E + 255) / 256), dim3(256), 0, stream_, a);
    check_launch("k_edge_errors");
  }

  // ---- priors (include/rr_pgo.h, rr_pgo_set_priors)
  void refuse_priors(const char *who) const override {
    const std::string w = who;
    if (sharded_ || world_ > 1) throw ApiError(RR_PGO_EUNSUPPORTED, w + ": sharded handle (the ranks' node lists and diagonal ownership are not taught the priors)");
    if (edge_lin_env_) throw ApiError(RR_PGO_EUNSUPPORTED, w + ": handle created under RR_PGO_EDGE_LINEARIZE (the edge-parallel linearisation forms are not taught the priors)");
  }
  template <typename U> void upload_grow(DevBuf<U> &buf, const std::vector<U> &v) {
    if (v.size() > buf.n) {
      ArenaScope scope(&arena_);
      buf.alloc(v.size());
    }
    if (!v.empty()) HIPCHK(hipMemcpy(buf.p, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice));
  }
  void set_priors(const PriorSet &ps) override {
    refuse_priors("rr_pgo_set_priors");
    const int P = ps.n(), N = g_.n_nodes();
    // CSR by node; a node's priors keep the call's order (they are summed in it)
    std::vector<int32_t> ptr((size_t)N + 1, 0), order((size_t)P), pnode((size_t)P);
    for (int p = 0; p < P; p++) ptr[(size_t)ps.node[p] + 1]++;
    for (int i = 0; i < N; i++) ptr[(size_t)i + 1] += ptr[i];
    std::vector<int64_t> moff((size_t)P + 1, 0), ioff((size_t)P + 1, 0);
    for (int p = 0; p < P; p++) {
      const int ek = prior_edge_kind(g_.node_kind[ps.node[p]]);
      moff[(size_t)p + 1] = moff[p] + edge_meas_len(ek);
      ioff[(size_t)p + 1] = ioff[p] + edge_info_len(ek);
    }
    {
      std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
      for (int p = 0; p < P; p++) order[(size_t)fill[ps.node[p]]++] = p;
    }
    std::vector<EdgeRec<S>> rec(is3d_ ? 0 : (size_t)P);
    std::vector<V4> meas(is3d_ ? 2 * (size_t)P : 0);
    std::vector<S> info(is3d_ ? 21 * (size_t)P : 0);
    std::vector<uint8_t> rob((size_t)P);
    for (int c = 0; c < P; c++) {
      const int p = order[c], node = ps.node[p];
      const double *m = &ps.meas[(size_t)moff[p]], *w = &ps.info[(size_t)ioff[p]];
      pnode[c] = node;
      rob[c] = ps.robust[p];
      if (is3d_) {
        const int ek = prior_edge_kind(g_.node_kind[node]);   // SE3, or SE3_XYZ on a landmark
        pack_v4(ek, m, &meas[2 * (size_t)c]);
        pack_info_3d<S>(ek, w, &info[21 * (size_t)c]);
        continue;
      }
      EdgeRec<S> &r = rec[c];   // (slot stays 0: a prior has no off-diagonal block)
      r.from = -1;
      r.to = node;
      if (g_.node_kind[node] == NODE_SE2) {
        pack_v4(EDGE_SE2, m, &r.meas);
        r.info_a = V4{(S)w[0], (S)w[1], (S)w[2], (S)w[3]};
        r.info_b = V2{(S)w[4], (S)w[5]};
      } else {
        pack_v4(EDGE_SE2_XY, m, &r.meas);
        r.info_a = V4{(S)w[0], (S)w[1], (S)0, (S)w[2]};
        r.info_b = V2{(S)0, (S)0};
      }
    }
    HIPCHK(hipStreamSynchronize(stream_));   // launches already enqueued read the old list
    if (P > 0) {
      upload_grow(prior_ptr_, ptr);
      upload_grow(prior_node_, pnode);
      upload_grow(prior_rec_, rec);
      upload_grow(prior_meas_, meas);
      upload_grow(prior_info3_, info);
      upload_grow(prior_robust_, rob);
    }
    settings_.priors = ps;
    if (P == 0) settings_.priors.keep_anchor = 1;
    prior_order_.swap(order);
    // the captured graphs hold the old kernel and its arguments
    drop_graphs();
  }

  // ---- fixed nodes (include/rr_pgo.h, rr_pgo_set_fixed)
  void refuse_fixed(const char *who) const override {
    const std::string w = who;
    if (sharded_ || world_ > 1) throw ApiError(RR_PGO_EUNSUPPORTED, w + ": sharded handle (the ranks' node lists and diagonal ownership are not taught the fixed nodes)");
    if (edge_lin_env_) throw ApiError(RR_PGO_EUNSUPPORTED, w + ": handle created under RR_PGO_EDGE_LINEARIZE (the edge-parallel linearisation forms are not taught the fixed nodes)");
  }
  void set_fixed(const std::vector<int32_t> &nodes, int keep_anchor) override {   // nodes: distinct, ascending, in range
    refuse_fixed("rr_pgo_set_fixed");
    const int N = g_.n_nodes();
    std::vector<uint8_t> flag((size_t)N, 0);
    for (int32_t v : nodes) flag[(size_t)v] = 1;
    HIPCHK(hipStreamSynchronize(stream_));   // launches already enqueued read the old set
    if (!nodes.empty()) upload_grow(fixed_, flag);
    else flag.clear();
    settings_.fixed = nodes;
    fixed_host_.swap(flag);
    settings_.fixed_keep_anchor = nodes.empty() ? 1 : (keep_anchor != 0 ? 1 : 0);
    // the captured graphs hold the old kernel and its arguments
    drop_graphs();
  }
  bool is_fixed(int v) const { return !fixed_host_.empty() && fixed_host_[(size_t)v] != 0; }

  // ---- rr_pgo_initialize (include/rr_pgo.h; chordal.hip.h): the chordal relaxation from the measurements.
  // Two (2-D) or three (3-D) linear stages on the pattern of H, each linearised by k_chordal_lin and factored and solved by
  // the handle's own launches, eagerly and without the gauge term (a held node makes the systems definite); the solved
  // vector of each is exported in reference order and its error flag read before the next stage is enqueued.  The state is
  // written by ONE launch, k_chordal_place, behind the last clean flag: every refusal and failure leaves it as it was.
  int chordal_anchor() const { return (settings_.priors.keep_anchor && settings_.fixed_keep_anchor) ? g_.anchor_node : -1; }
  ChordalArgs<T, S> chordal_args() const {
    ChordalArgs<T, S> a;
    a.n_nodes = g_.n_nodes();
    a.pose = pose_.p;
    a.e_rec = e_rec_.p;
    a.e_meas = e_meas_.p;
    a.e_info = e_info3_.p;
    a.e_slot = e_slot_.p;
    a.inc_ptr = inc_ptr_.p;
    a.inc_list = inc_list_.p;
    a.node_dim = node_dim_.p;
    a.node_offset = node_offset_.p;
    a.diag_off = diag_off_.p;
    a.hvals = hvals_.p;
    a.b = b_.p;
    a.zero_words = lds_flow_ ? dep_flags_.p : nullptr;
    a.n_zero_words = lds_flow_ ? 2 * sym_.S + 64 : 0;
    a.fill_words = lds_flow_ ? reinterpret_cast<unsigned *>(x_ptr_) : nullptr;
    a.n_fill_words = lds_flow_ ? (int)((size_t)g_.dim * sizeof(T) / 4) : 0;
    a.prior_ptr = settings_.priors.n() > 0 ? prior_ptr_.p : nullptr;
    a.prior_rec = prior_rec_.p;
    a.prior_meas = prior_meas_.p;
    a.prior_info = prior_info3_.p;
    a.fixed = settings_.fixed.empty() ? nullptr : fixed_.p;
    a.anchor = chordal_anchor();
    a.rot = chordal_rot_.p;
    return a;
  }
  template <int STAGE> void chordal_stage() {
    const ChordalArgs<T, S> a = chordal_args();
    const unsigned nb = (unsigned)(((int64_t)g_.n_nodes() * LIN_GROUP + LIN_THREADS - 1) / LIN_THREADS);
    if (is3d_) hipLaunchKernelGGL((k_chordal_lin<T, S, 6, STAGE>), dim3(nb), dim3(LIN_THREADS), 0, stream_, a);
    else if constexpr (STAGE != 1) hipLaunchKernelGGL((k_chordal_lin<T, S, 3, STAGE>), dim3(nb), dim3(LIN_THREADS), 0, stream_, a);
    check_launch("k_chordal_lin");
    launch_factor_range(0, sym_.steps.size(), false);
    launch_solve();
    launch_step(false, STEP_EXPORT);   // the solved vector in reference order (dx_ref_), the state untouched
    check_device_error();              // waits; a singular stage throws RR_PGO_ENOTSPD here
  }
  void initialize(int method) override {
    if (sharded_ || world_ > 1)
      throw ApiError(RR_PGO_EUNSUPPORTED, "rr_pgo_initialize: sharded handle (the relaxed systems are not split over ranks)");
    if (method != RR_PGO_INIT_CHORDAL) throw ApiError(RR_PGO_EINVAL, "rr_pgo_initialize: unknown method " + std::to_string(method));
    const int N = g_.n_nodes();
    const int anchor = chordal_anchor();
    {   // every free landmark needs a term that places it
      std::vector<uint8_t> placed((size_t)N, 0);
      for (int k = 0; k < g_.n_edges(); k++)
        if (g_.edge_kind[k] == EDGE_SE2_XY || g_.edge_kind[k] == EDGE_SE3_XYZ) placed[(size_t)g_.edge_to[k]] = 1;
      for (int32_t v : settings_.priors.node) placed[(size_t)v] = 1;
      for (int i = 0; i < N; i++) {
        const int kind = g_.node_kind[i];
        if ((kind == NODE_XY || kind == NODE_XYZ) && !placed[(size_t)i] && !is_fixed(i) && i != anchor)
          throw ApiError(RR_PGO_EINVAL, "rr_pgo_initialize: landmark node " + std::to_string(i) + " (id " + std::to_string(g_.node_id[(size_t)i]) +
                                            ") is free and has neither an SE2_XY / SE3_XYZ edge nor a prior: nothing places it");
      }
    }
    {   // every set of poses connected by pose-pose edges needs a held pose or a pose prior: without one the rotation stage's
      // matrix is a singular block Laplacian, whose last pivot is zero in exact arithmetic only -- decided here, not by rounding
      std::vector<int32_t> root((size_t)N);
      for (int i = 0; i < N; i++) root[(size_t)i] = i;
      auto find = [&](int v) {
        while (root[(size_t)v] != v) { root[(size_t)v] = root[(size_t)root[(size_t)v]]; v = root[(size_t)v]; }
        return v;
      };
      for (int k = 0; k < g_.n_edges(); k++)
        if (g_.edge_kind[k] == EDGE_SE2 || g_.edge_kind[k] == EDGE_SE3) root[(size_t)find(g_.edge_from[k])] = find(g_.edge_to[k]);
      std::vector<uint8_t> grounded((size_t)N, 0);
      auto is_pose = [&](int v) { return g_.node_kind[(size_t)v] == NODE_SE2 || g_.node_kind[(size_t)v] == NODE_SE3; };
      for (int i = 0; i < N; i++)
        if (is_pose(i) && (is_fixed(i) || i == anchor)) grounded[(size_t)find(i)] = 1;
      for (int32_t v : settings_.priors.node)
        if (is_pose(v)) grounded[(size_t)find(v)] = 1;
      for (int i = 0; i < N; i++)
        if (is_pose(i) && !grounded[(size_t)find(i)])
          throw ApiError(RR_PGO_ENOTSPD, "rr_pgo_initialize: the poses connected to node " + std::to_string(i) +
                                             " hold neither a fixed node, a kept anchor nor a pose prior: the relaxed systems are singular");
    }
    if (!chordal_rot_.p) {
      chordal_rot_.alloc((size_t)N * (is3d_ ? 9 : 2));
      if (is3d_) chordal_sol_.alloc((size_t)g_.dim);
      for (EventHolder &e : chordal_ev_) e.create(hipEventDefault);
    }
    for (double &m : chordal_ms_) m = 0;
    clear_stop_word();
    ChordalNodeArgs<T, S> na;
    na.n_nodes = N;
    na.is3d = is3d_ ? 1 : 0;
    na.pose = pose_.p;
    na.node_dim = node_dim_.p;
    na.node_offset = node_offset_.p;
    na.fixed = settings_.fixed.empty() ? nullptr : fixed_.p;
    na.anchor = anchor;
    na.sol_a = is3d_ ? chordal_sol_.p : dx_ref_.p;
    na.sol_b = dx_ref_.p;
    na.rot = chordal_rot_.p;
    const unsigned nb = (unsigned)((N + 255) / 256);
    HIPCHK(hipEventRecord(chordal_ev_[0], stream_));
    chordal_stage<0>();
    if (is3d_) {
      HIPCHK(hipMemcpyAsync(chordal_sol_.p, dx_ref_.p, (size_t)g_.dim * sizeof(T), hipMemcpyDeviceToDevice, stream_));
      chordal_stage<1>();
    }
    hipLaunchKernelGGL((k_chordal_project<T, S>), dim3(nb), dim3(256), 0, stream_, na);
    check_launch("k_chordal_project");
    HIPCHK(hipEventRecord(chordal_ev_[1], stream_));
    chordal_stage<2>();
    HIPCHK(hipEventRecord(chordal_ev_[2], stream_));
    na.sol_a = dx_ref_.p;
    hipLaunchKernelGGL((k_chordal_place<T, S>), dim3(nb), dim3(256), 0, stream_, na);
    check_launch("k_chordal_place");
    HIPCHK(hipEventRecord(chordal_ev_[3], stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    float t01 = 0, t12 = 0, t03 = 0;
    HIPCHK(hipEventElapsedTime(&t01, chordal_ev_[0], chordal_ev_[1]));
    HIPCHK(hipEventElapsedTime(&t12, chordal_ev_[1], chordal_ev_[2]));
    HIPCHK(hipEventElapsedTime(&t03, chordal_ev_[0], chordal_ev_[3]));
    chordal_ms_[0] = t01; chordal_ms_[1] = t12; chordal_ms_[2] = t03;
  }
  void initialize_times(double *ms) const override { for (int k = 0; k < 3; k++) ms[k] = chordal_ms_[k]; }

  void prior_errors(double *s_out, double *w_out) override {
    refuse_priors("rr_pgo_prior_errors");
    const int P = settings_.priors.n();
    if (P == 0) return;
    DevBuf<double> out;
    out.alloc(2 * (size_t)P);
    PriorErrArgs<S> a;
    a.n_priors = P;
    a.is3d = is3d_ ? (has_lm_ ? 2 : 1) : 0;
    a.kind = settings_.robust_kind;
    a.node = prior_node_.p;
    a.rec = prior_rec_.p;
    a.pose = pose_.p;
    a.meas = prior_meas_.p;
    a.info = prior_info3_.p;
    a.node_dim = node_dim_.p;
    a.delta = (S)settings_.robust_delta;
    a.delta2 = (S)(settings_.robust_delta * settings_.robust_delta);
    a.robust = prior_robust_.p;
    const TlsParams tp = tls_params();
    a.tls_lo = (S)tp.lo; a.tls_hi = (S)tp.hi; a.tls_cs = (S)tp.cs; a.tls_mu = (S)tp.mu;
    a.s_out = out.p;
    a.w_out = out.p + P;
    if (has_lm_) hipLaunchKernelGGL((k_prior_errors<S, true>), dim3((P + 255) / 256), dim3(256), 0, stream_, a);
    else hipLaunchKernelGGL((k_prior_errors<S>), dim3((P + 255) / 256), dim3(256), 0, stream_, a);
    check_launch("k_prior_errors");
    std::vector<double> host(2 * (size_t)P);
    HIPCHK(hipMemcpyAsync(host.data(), out.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    for (int c = 0; c < P; c++) {
      s_out[prior_order_[c]] = host[c];
      if (w_out) w_out[prior_order_[c]] = host[(size_t)P + c];
    }
  }


  // ---- queries over the factor: what rr_pgo_marginals, rr_pgo_covariances, rr_pgo_gate_edges and rr_pgo_gate_joint share
  // lds_only: rr_pgo_marginals while rr_pgo_set_marginals_big_fronts is off, the other queries while
  // rr_pgo_set_query_big_fronts is off
  void require_f64_unsharded_lds_factor(const char *who, bool lds_only) const {
    const std::string w = who;
    if (sharded_ || world_ > 1) throw ApiError(RR_PGO_EUNSUPPORTED, w + ": sharded handle (a rank holds a part of the factor only)");
    if (!f64_) throw ApiError(RR_PGO_EUNSUPPORTED, w + ": F32 / MIXED handle (a single-precision factor of a matrix of condition ~1e10 has no meaningful inverse): create the handle with RR_PGO_F64");
    if (sym_.n_big > 0 && lds_only)
      throw ApiError(RR_PGO_EUNSUPPORTED, w + ": " + std::to_string(sym_.n_big) + " fronts beyond LDS (n_big_fronts must be 0)" +
                                              (w == "rr_pgo_marginals" ? ": use rr_pgo_covariances with rr_pgo_set_query_big_fronts" : ""));
  }
  void set_query_big_fronts(int on) override { settings_.query_big = on != 0; }
  void set_marginals_big_fronts(int on) override { settings_.marg_big = on != 0; }
  // depth of every front, front of every permuted column, the four events of a call: made once
  void tree_tables(const char *who) {
    if (!front_depth_.empty()) return;
    const Symbolic &sym = sym_;
    for (int f = 0; f < sym.S; f++)
      if (sym.sn_parent[f] < 0 && sym.sn_nrows[f] != 0) throw ApiError(RR_PGO_EUNSUPPORTED, std::string(who) + ": a root front with rows below its pivot block");
    for (EventHolder &e : query_ev_) e.create(hipEventDefault);
    col_front_.assign((size_t)g_.dim, -1);
    std::vector<int32_t> depth((size_t)sym.S, 0);
    for (int f = sym.S - 1; f >= 0; f--) {   // children precede parents
      if (sym.sn_parent[f] >= 0) depth[f] = depth[sym.sn_parent[f]] + 1;
      for (int c = 0; c < sym.sn_ncols[f]; c++) col_front_[sym.sn_col0[f] + c] = f;
    }
    front_depth_ = std::move(depth);
  }
  int front_of(int v) const { return col_front_[sym_.node_pcol[v]]; }
  // the three intervals between the events in ms.  accumulate: a later pass of the same call -- event 0 belongs to the first
  // pass, so intervals 1 and 2 are added
  void query_times(double *ms, bool accumulate) {
    for (int k = accumulate ? 1 : 0; k < 3; k++) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, query_ev_[k], query_ev_[k + 1]));
      ms[k] = accumulate ? ms[k] + t : t;
    }
  }

  // ---- marginal covariances (include/rr_pgo.h, rr_pgo_marginals)
  void marginals_prepare(const char *who) {
    if (sel_ready_) return;
    tree_tables(who);
    const Symbolic &sym = sym_;
    const int S_ = sym.S;
    std::vector<SelMeta> meta((size_t)S_);
    sel_soff_.assign((size_t)S_ + 1, 0);
    size_t lds_elems = 0;
    for (int f = 0; f < S_; f++) {
      const int64_t nc = sym.sn_ncols[f], nr = sym.sn_nrows[f];
      const int64_t image = (nc + nr) * nc + nr * (nr + 1) / 2;
      if (!sym.sn_big[f]) {   // (a front beyond LDS keeps its image in svals: k_selinv_big_*)
        if (nc + nr > SELINV_MAX_ROWS) throw ApiError(RR_PGO_EUNSUPPORTED, std::string(who) + ": a front of " + std::to_string(nc + nr) + " rows exceeds what one workgroup holds");
        lds_elems = std::max(lds_elems, (size_t)image);
      }
      sel_soff_[f + 1] = sel_soff_[f] + ((image + 3) & ~(int64_t)3);
    }
    for (int f = 0; f < S_; f++) {
      SelMeta &m = meta[f];
      const int p = sym.sn_parent[f];
      m.nc = sym.sn_ncols[f];
      m.nr = sym.sn_nrows[f];
      m.wblk = host_sn_meta_[f].wblk;
      m.has_parent = p >= 0 ? 1 : 0;
      m.pnc = p >= 0 ? sym.sn_ncols[p] : 0;
      m.pn = p >= 0 ? sym.sn_ncols[p] + sym.sn_nrows[p] : 0;
      m.pad0 = m.pad1 = 0;
      m.loff = sym.sn_loff[f];
      m.soff = sel_soff_[f];
      m.psoff = p >= 0 ? sel_soff_[p] : 0;
      m.rel_ptr = sym.rel_ptr[f];
    }
    sel_lds_ = lds_elems * sizeof(T);
    if (sel_lds_ + (size_t)(256 + SELINV_GPART * 256) * sizeof(T) > (size_t)160 * 1024)
      throw ApiError(RR_PGO_EUNSUPPORTED, std::string(who) + ": fronts beyond LDS");
    std::vector<int32_t> order;
    sel_level_ptr_.assign(1, 0);
    const int max_depth = *std::max_element(front_depth_.begin(), front_depth_.end());
    // a level is two ranges: its LDS fronts, then its fronts beyond LDS with the tiles of their kernels
    std::vector<SelBig> big;
    std::vector<SelTile> tile;
    std::vector<int32_t> big_of((size_t)S_, -1);
    int64_t work_elems = 0;
    for (int f = S_ - 1; f >= 0; f--)
      if (sym.sn_big[f]) {
        const int64_t nc = sym.sn_ncols[f], nr = sym.sn_nrows[f];
        big_of[f] = (int32_t)big.size();
        big.push_back(SelBig{f, 0, work_elems, work_elems + nc * nc});
        work_elems += nc * (nc + nr);
      }
    auto below = [&](int f) {    // 128 rows below x 32 columns: k_selinv_big_y
      for (int r0 = 0; r0 < sym.sn_nrows[f]; r0 += SELB_SLAB)
        for (int c0 = 0; c0 < sym.sn_ncols[f]; c0 += SELB_COLS) tile.push_back(SelTile{big_of[f], r0, c0, 0});
    };
    auto strips = [&](int f) {   // 16 rows below x 256 columns: k_selinv_big_rp
      for (int r0 = 0; r0 < sym.sn_nrows[f]; r0 += 16)
        for (int c0 = 0; c0 < sym.sn_ncols[f]; c0 += SELB_RP_COLS) tile.push_back(SelTile{big_of[f], r0, c0, 0});
    };
    auto square = [&](int f) {   // the lower triangle of the pivot square: k_selinv_big_zz, k_selinv_big_pp
      for (int r0 = 0; r0 < sym.sn_ncols[f]; r0 += SELB_SLAB)
        for (int c0 = 0; c0 < sym.sn_ncols[f] && c0 < r0 + SELB_SLAB; c0 += SELB_COLS) tile.push_back(SelTile{big_of[f], r0, c0, 0});
    };
    sel_tile_ptr_.assign(1, 0);
    for (int pass = 0; pass < 3; pass++) {   // ahead of the levels: Z by block rows, Y, Z^T Z
      for (const SelBig &b : big) {
        if (pass == 0)
          for (int r = 0; r < (sym.sn_ncols[b.front] + 31) / 32; r++) tile.push_back(SelTile{big_of[b.front], r, 0, 0});
        else if (pass == 1) below(b.front);
        else square(b.front);
      }
      sel_tile_ptr_.push_back((int32_t)tile.size());
    }
    sel_big_ptr_.clear();
    for (int d = 0; d <= max_depth; d++) {
      for (int f = S_ - 1; f >= 0; f--)
        if (front_depth_[f] == d && !sym.sn_big[f]) order.push_back(f);
      sel_big_ptr_.push_back((int32_t)order.size());
      for (int f = S_ - 1; f >= 0; f--)
        if (front_depth_[f] == d && sym.sn_big[f]) order.push_back(f);
      sel_level_ptr_.push_back((int32_t)order.size());
      for (int pass = 0; pass < 2; pass++) {   // k_selinv_big_rp, k_selinv_big_pp: nothing for a front without rows below
        for (int k = sel_big_ptr_.back(); k < sel_level_ptr_.back(); k++)
          if (sym.sn_nrows[order[k]] > 0) pass == 0 ? strips(order[k]) : square(order[k]);
        sel_tile_ptr_.push_back((int32_t)tile.size());
      }
    }
    if (big.empty()) {
      ArenaScope scope(&arena_);   // like every other buffer of the handle: back to the pool with it
      sel_meta_.upload(meta);
      sel_order_.upload(order);
      svals_.alloc((size_t)sel_soff_[S_] + 4);
    } else {
      // the images and the workspace of fronts beyond LDS are of the factor's size: buffers of their own, so that a device
      // without room for them is an answer (nothing of the handle has changed by then), not a failed arena chunk
      auto own = [&](DevBuf<T> &buf, size_t count, const char *what) {
        buf.alloc(0);
        T *p = nullptr;
        if (hipMalloc((void **)&p, count * sizeof(T)) != hipSuccess) {
          (void)hipGetLastError();
          throw ApiError(RR_PGO_ENOMEM, std::string(who) + ": " + std::to_string(count * sizeof(T)) + " bytes for " + what + " of the fronts beyond LDS");
        }
        buf.p = p;
        buf.n = count;
        buf.owned = true;
      };
      own(svals_, (size_t)sel_soff_[S_] + 4, "the selected inverse");
      own(sel_work_, (size_t)work_elems + 4, "the workspace");
      ArenaScope scope(&arena_);
      sel_meta_.upload(meta);
      sel_order_.upload(order);
      sel_big_.upload(big);
      sel_tile_.upload(tile);
    }
    if constexpr (std::is_same<T, double>::value)
      HIPCHK(hipFuncSetAttribute((const void *)k_selinv_level<T, SELINV_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sel_lds_));
    sel_ready_ = true;
  }

  void marginals(int nq, const int32_t *na, const int32_t *nb, const int64_t *off, double *out) override {
    static constexpr const char *who = "rr_pgo_marginals";
    require_f64_unsharded_lds_factor(who, !settings_.marg_big);
    if constexpr (f64_) {
      marginals_prepare(who);
      const Symbolic &sym = sym_;
      // ---- where every output scalar lives in svals
      const int64_t n_vals = off[nq];
      std::vector<int64_t> src((size_t)n_vals);
      int32_t pc_a[6], pc_b[6];
      auto node_cols = [&](int v, int32_t *pc) {   // reference scalar r of node v -> permuted column
        const int d = node_dim(g_.node_kind[v]), p0 = sym.node_pcol[v];
        for (int i = 0; i < d; i++) pc[sym.perm[p0 + i] - g_.node_offset[v]] = p0 + i;
        return d;
      };
      for (int q = 0; q < nq; q++) {
        const int va = na ? na[q] : q, vb = nb ? nb[q] : va;
        const int da = node_cols(va, pc_a), db = node_cols(vb, pc_b);
        const int ve = sym.node_pcol[va] <= sym.node_pcol[vb] ? va : vb;   // eliminated first: its front holds the pair, or none does
        const int f = front_of(ve);
        const int nc = sym.sn_ncols[f], nr = sym.sn_nrows[f], n = nc + nr, c0 = sym.sn_col0[f];
        const int32_t *rows = sym.sn_rows.data() + sym.sn_rows_ptr[f];
        auto local = [&](int pcol) -> int {
          if (pcol >= c0 && pcol < c0 + nc) return pcol - c0;
          const int32_t *it = std::lower_bound(rows, rows + nr, pcol);
          return it != rows + nr && *it == pcol ? nc + (int)(it - rows) : -1;
        };
        for (int i = 0; i < da; i++)
          for (int j = 0; j < db; j++) {
            const int li = local(pc_a[i]), lj = local(pc_b[j]);
            if (li < 0 || lj < 0)
              throw ApiError(RR_PGO_EINVAL, "rr_pgo_marginals: nodes " + std::to_string(va) + " and " + std::to_string(vb) +
                                                " (query " + std::to_string(q) + ") share no front of the factor: only pairs joined by an edge are guaranteed");
            const int hi = std::max(li, lj), lo = std::min(li, lj);
            if (lo >= nc) throw ApiError(RR_PGO_ENODEVICE, "rr_pgo_marginals: internal: pair outside its front's panel");
            // (a block with a fixed node is zero: Sigma is conditional on the fixed nodes; the selected inverse of the identity
            // rows holds I in the node's own block)
            src[(size_t)(off[q] + (int64_t)i * db + j)] = is_fixed(va) || is_fixed(vb) ? (int64_t)-1 : sel_soff_[f] + (int64_t)lo * n + hi;
          }
      }
      DevBuf<int64_t> d_src;
      DevBuf<double> d_out;
      d_src.alloc((size_t)n_vals);
      d_out.alloc((size_t)n_vals);
      HIPCHK(hipMemcpyAsync(d_src.p, src.data(), src.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
      HIPCHK(hipEventRecord(query_ev_[0], stream_));
      enqueue_factor(lin_system(0.0, 0));
      HIPCHK(hipEventRecord(query_ev_[1], stream_));
      SelArgs<T> a;
      a.meta = sel_meta_.p;
      a.order = sel_order_.p;
      a.rel = rel_.p;
      a.lvals = lvals_.p;
      a.winv = winv_.p;
      a.svals = svals_.p;
      SelBigArgs<T> ab;
      ab.s = a;
      ab.big = sel_big_.p;
      ab.tile = sel_tile_.p;
      ab.work = sel_work_.p;
      // ranges of sel_tile_: Z, Y, Z^T Z of every front beyond LDS (they need nothing from a parent), then two per level
      auto big_launch = [&](auto kernel, int threads, size_t r) {
        const int first = sel_tile_ptr_[r], count = sel_tile_ptr_[r + 1] - first;
        if (count > 0) hipLaunchKernelGGL(kernel, dim3((unsigned)count), dim3((unsigned)threads), 0, stream_, ab, first);
      };
      big_launch(k_selinv_big_z<T>, SELB_Z_THREADS, 0);
      big_launch(k_selinv_big_y<T>, SELB_THREADS, 1);
      big_launch(k_selinv_big_zz<T>, SELB_THREADS, 2);
      for (size_t l = 0; l + 1 < sel_level_ptr_.size(); l++) {
        const int begin = sel_level_ptr_[l], count = sel_big_ptr_[l] - begin;
        if (count > 0) hipLaunchKernelGGL((k_selinv_level<T, SELINV_THREADS>), dim3((unsigned)count), dim3(SELINV_THREADS), sel_lds_, stream_, a, begin);
        big_launch(k_selinv_big_rp<T>, SELB_THREADS, 3 + 2 * l);
        big_launch(k_selinv_big_pp<T>, SELB_THREADS, 4 + 2 * l);
      }
      check_launch("k_selinv_level");
      HIPCHK(hipEventRecord(query_ev_[2], stream_));
      if (n_vals > 0) {
        hipLaunchKernelGGL((k_marg_gather<T>), dim3((unsigned)((n_vals + 255) / 256)), dim3(256), 0, stream_, (const T *)svals_.p, (const int64_t *)d_src.p, d_out.p, n_vals);
        check_launch("k_marg_gather");
      }
      HIPCHK(hipEventRecord(query_ev_[3], stream_));
      std::vector<double> host((size_t)n_vals);
      if (n_vals > 0) HIPCHK(hipMemcpyAsync(host.data(), d_out.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
      HIPCHK(hipStreamSynchronize(stream_));
      check_device_error();
      query_times(query_ms_[Q_MARGINALS], false);
      if (n_vals > 0) std::memcpy(out, host.data(), host.size() * sizeof(double));
    }
  }
  void last_query_times(Query which, double *ms) const override { for (int k = 0; k < 3; k++) ms[k] = query_ms_[which][k]; }

  // ---- the multi-column tree solve (treesolve.hip.h) under rr_pgo_covariances, rr_pgo_gate_edges and rr_pgo_gate_joint
  struct TsPlan {
    std::vector<TsTask> tasks;                 // by level, deepest first
    std::vector<int32_t> child, unit, czrow, level_ptr;
    std::vector<int32_t> big_ptr;              // per level: its first task beyond LDS (LDS tasks first, then these)
    std::vector<TsSlab> slab;                  // the slabs of rows below of the tasks beyond LDS, by level
    std::vector<int32_t> slab_ptr;             // per level, into slab
    std::vector<CovQuery> query;
    int64_t zrows = 0, urows = 0;
    int n_chunks = 0;
  };

  void covariances_prepare(const char *who) {
    if (ts_ready_) return;
    tree_tables(who);
    const Symbolic &sym = sym_;
    const int S_ = sym.S;
    std::vector<TsMeta> meta((size_t)S_);
    int64_t max_n = 1;
    for (int f = 0; f < S_; f++) {
      TsMeta &m = meta[f];
      m.nc = sym.sn_ncols[f];
      m.nr = sym.sn_nrows[f];
      m.wblk = host_sn_meta_[f].wblk;
      m.parent = sym.sn_parent[f];
      m.loff = sym.sn_loff[f];
      m.rel_ptr = sym.rel_ptr[f];
      if (!sym.sn_big[f]) max_n = std::max<int64_t>(max_n, (int64_t)m.nc + m.nr);   // (a front beyond LDS keeps its block in the workspace)
    }
    ts_lds_ = (size_t)max_n * TS_LD * sizeof(T);
    if (ts_lds_ + 256 * sizeof(T) > (size_t)160 * 1024)
      throw ApiError(RR_PGO_EUNSUPPORTED, std::string(who) + ": a front of " + std::to_string(max_n) + " rows exceeds what one workgroup holds beside a chunk of columns");
    {
      ArenaScope scope(&arena_);   // like every other buffer of the handle: back to the pool with it
      ts_meta_.upload(meta);
    }
    if constexpr (std::is_same<T, double>::value)
      HIPCHK(hipFuncSetAttribute((const void *)k_tree_fwd<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ts_lds_));
    if constexpr (std::is_same<T, double>::value)
      HIPCHK(hipFuncSetAttribute((const void *)k_tree_bwd<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ts_lds_));
    ts_ready_ = true;
  }

  // the plan of queries [q0, q1): columns, chunks, active fronts by level, the pairs' common paths
  void covariances_plan(int q0, int q1, const int32_t *na, const int32_t *nb, const int64_t *off, TsPlan &pl) const {
    const Symbolic &sym = sym_;
    const int S_ = sym.S;
    // distinct nodes by permuted column: fronts own consecutive column ranges in elimination order, so this is the order
    // of (front, column) and neighbours share most of their paths
    std::vector<int32_t> nodes;
    nodes.reserve(2 * (size_t)(q1 - q0));
    for (int q = q0; q < q1; q++) {
      nodes.push_back(na[q]);
      nodes.push_back(nb[q]);
    }
    std::sort(nodes.begin(), nodes.end(), [&](int32_t x, int32_t y) { return sym.node_pcol[x] < sym.node_pcol[y]; });
    nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
    std::vector<int32_t> node_chunk((size_t)g_.n_nodes(), -1), node_col((size_t)g_.n_nodes(), 0);
    std::vector<size_t> chunk_ptr{0};   // into nodes: whole nodes, at most TS_MC columns
    int used = 0;
    for (size_t k = 0; k < nodes.size(); k++) {
      const int v = nodes[k], d = node_dim(g_.node_kind[v]);
      if (used + d > TS_MC) {
        chunk_ptr.push_back(k);
        used = 0;
      }
      node_chunk[v] = (int32_t)chunk_ptr.size() - 1;
      node_col[v] = used;
      used += d;
    }
    chunk_ptr.push_back(nodes.size());
    pl.n_chunks = (int)chunk_ptr.size() - 1;
    pl.czrow.assign((size_t)pl.n_chunks * S_, -1);
    std::vector<TsTask> tmp;            // tasks in (chunk, front) order; pl.child holds indices into it until the sort below
    std::vector<int32_t> mark((size_t)S_, -1), task_of((size_t)S_, -1), fronts;
    for (int c = 0; c < pl.n_chunks; c++) {
      fronts.clear();
      for (size_t k = chunk_ptr[c]; k < chunk_ptr[c + 1]; k++)
        for (int f = front_of(nodes[k]); f >= 0 && mark[f] != c; f = sym.sn_parent[f]) {
          mark[f] = c;
          fronts.push_back(f);
        }
      std::sort(fronts.begin(), fronts.end());
      const size_t base = tmp.size();
      for (int f : fronts) {
        TsTask t{};
        t.front = f;
        t.zrow = (int32_t)pl.zrows;   // (a plan beyond the workspace bound is dropped before these are read)
        t.urow = (int32_t)pl.urows;
        pl.zrows += sym.sn_ncols[f];
        pl.urows += sym.sn_nrows[f];
        pl.czrow[(size_t)c * S_ + f] = t.zrow;
        task_of[f] = (int32_t)tmp.size();
        tmp.push_back(t);
      }
      for (int f : fronts)
        if (sym.sn_parent[f] >= 0) tmp[task_of[sym.sn_parent[f]]].n_child++;
      size_t cp = pl.child.size();
      for (size_t i = base; i < tmp.size(); i++) {
        tmp[i].child_ptr = (int32_t)cp;
        cp += tmp[i].n_child;
        tmp[i].n_child = 0;
      }
      pl.child.resize(cp);
      for (int f : fronts)   // ascending: the fixed child order of the gather
        if (sym.sn_parent[f] >= 0) {
          TsTask &pt = tmp[task_of[sym.sn_parent[f]]];
          pl.child[pt.child_ptr + pt.n_child++] = task_of[f];
        }
      for (size_t k = chunk_ptr[c]; k < chunk_ptr[c + 1]; k++) {   // (the nodes of one front follow each other)
        const int v = nodes[k], f = front_of(v), d = node_dim(g_.node_kind[v]), p0 = sym.node_pcol[v];
        TsTask &t = tmp[task_of[f]];
        if (t.n_unit == 0) t.unit_ptr = (int32_t)pl.unit.size();
        if (is_fixed(v)) continue;   // rr_pgo_set_fixed: the seed of a fixed node is E_s = 0, so Z_s = 0 and its blocks are zero
        for (int i = 0; i < d; i++) pl.unit.push_back(((p0 + i - sym.sn_col0[f]) << 5) | (node_col[v] + i));
        t.n_unit += d;
      }
    }
    const int nt = (int)tmp.size();
    std::vector<int32_t> order((size_t)nt), newidx((size_t)nt);
    for (int i = 0; i < nt; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {   // within a level the LDS tasks, then those beyond LDS
      const int fx = tmp[x].front, fy = tmp[y].front;
      return front_depth_[fx] != front_depth_[fy] ? front_depth_[fx] > front_depth_[fy] : sym.sn_big[fx] < sym.sn_big[fy];
    });
    pl.tasks.resize((size_t)nt);
    pl.level_ptr.assign(1, 0);
    for (int i = 0; i < nt; i++) {
      newidx[order[i]] = i;
      pl.tasks[i] = tmp[order[i]];
      if (i > 0 && front_depth_[pl.tasks[i].front] != front_depth_[pl.tasks[i - 1].front]) pl.level_ptr.push_back(i);
    }
    pl.level_ptr.push_back(nt);
    pl.slab_ptr.assign(1, 0);
    for (size_t l = 0; l + 1 < pl.level_ptr.size(); l++) {
      int i = pl.level_ptr[l];
      while (i < pl.level_ptr[l + 1] && !sym.sn_big[pl.tasks[i].front]) i++;
      pl.big_ptr.push_back(i);
      for (; i < pl.level_ptr[l + 1]; i++)
        for (int r0 = 0; r0 < sym.sn_nrows[pl.tasks[i].front]; r0 += TSB_SLAB) pl.slab.push_back(TsSlab{i, r0});
      pl.slab_ptr.push_back((int32_t)pl.slab.size());
    }
    for (int32_t &c : pl.child) c = newidx[c];
    pl.query.resize((size_t)(q1 - q0));
    for (int q = q0; q < q1; q++) {
      CovQuery &cq = pl.query[q - q0];
      std::memset(&cq, 0, sizeof(cq));
      const int va = na[q], vb = nb[q];
      int fa = front_of(va), fb = front_of(vb);
      while (fa != fb && fa >= 0 && fb >= 0) {
        if (front_depth_[fa] >= front_depth_[fb]) fa = sym.sn_parent[fa];
        else fb = sym.sn_parent[fb];
      }
      cq.lca = fa == fb ? fa : -1;
      cq.chunk_a = node_chunk[va];
      cq.chunk_b = node_chunk[vb];
      cq.da = node_dim(g_.node_kind[va]);
      cq.db = node_dim(g_.node_kind[vb]);
      for (int i = 0; i < cq.da; i++) cq.ca[sym.perm[sym.node_pcol[va] + i] - g_.node_offset[va]] = (uint8_t)(node_col[va] + i);
      for (int i = 0; i < cq.db; i++) cq.cb[sym.perm[sym.node_pcol[vb] + i] - g_.node_offset[vb]] = (uint8_t)(node_col[vb] + i);
      cq.ooff = off[q] - off[q0];
    }
  }

  // RR_PGO_QUERY_TRACE=1: one line per pass, one per active front of the pass (by level, deepest first; over the chunks: a
  // front active in several chunks is listed once) and one per distinct queried node
  void trace_plan(const char *who, int q0, int q1, const int32_t *na, const int32_t *nb, const TsPlan &pl, size_t ws) const {
    const Symbolic &sym = sym_;
    int n_big = 0, n_launch = 0;
    for (const TsTask &t : pl.tasks) n_big += sym.sn_big[t.front];
    for (size_t l = 0; l + 1 < pl.level_ptr.size(); l++)
      n_launch += (pl.big_ptr[l] > pl.level_ptr[l]) + (pl.level_ptr[l + 1] > pl.big_ptr[l]) + (pl.slab_ptr[l + 1] > pl.slab_ptr[l]);
    std::fprintf(stderr, "query trace: %s pass [%d, %d): %d chunks, %zu tasks (%d beyond LDS), %zu slabs, %zu levels, %d forward launches, %zu bytes\n",
                 who, q0, q1, pl.n_chunks, pl.tasks.size(), n_big, pl.slab.size(), pl.level_ptr.size() - 1, n_launch, ws);
    std::vector<char> seen((size_t)sym.S, 0);
    for (size_t l = 0; l + 1 < pl.level_ptr.size(); l++)
      for (int i = pl.level_ptr[l]; i < pl.level_ptr[l + 1]; i++) {
        const int f = pl.tasks[i].front;
        if (seen[f]) continue;
        seen[f] = 1;
        std::fprintf(stderr, "query trace:   front %d depth %d nc %d nr %d parent %d children %d %s\n", f, front_depth_[f], sym.sn_ncols[f],
                     sym.sn_nrows[f], sym.sn_parent[f], sym.child_ptr[f + 1] - sym.child_ptr[f], sym.sn_big[f] ? "beyond-LDS" : "LDS");
      }
    std::vector<char> told((size_t)g_.n_nodes(), 0);
    for (int q = q0; q < q1; q++)
      for (int v : {na[q], nb[q]})
        if (!told[v]) {
          told[v] = 1;
          std::fprintf(stderr, "query trace:   node %d front %d\n", v, front_of(v));
        }
  }

  template <typename U> void ts_grow(DevBuf<U> &b, size_t count) {
    if (b.p && b.n >= count) return;
    ArenaScope scope(nullptr);   // a buffer of its own: freed when it grows and with the handle
    b.alloc(std::max<size_t>(std::max(count, b.n + b.n / 2), 4));
  }
  template <typename U> void ts_fill(DevBuf<U> &b, const std::vector<U> &v) {
    ts_grow(b, v.size());
    if (!v.empty()) HIPCHK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice, stream_));
  }

  // a plan's tables and workspace on the device; the forward solve of its columns, one launch per level (Z, U)
  void ts_stage(const TsPlan &pl) {
    ts_fill(ts_tasks_, pl.tasks);
    ts_fill(ts_child_, pl.child);
    ts_fill(ts_unit_, pl.unit);
    ts_fill(ts_czrow_, pl.czrow);
    if (!pl.slab.empty()) ts_fill(ts_slab_, pl.slab);
    ts_grow(ts_z_, (size_t)pl.zrows * TS_MC);
    ts_grow(ts_u_, (size_t)pl.urows * TS_MC);
  }
  void ts_forward(const TsPlan &pl) {
    TsArgs<T> a;
    a.meta = ts_meta_.p;
    a.tasks = ts_tasks_.p;
    a.child = ts_child_.p;
    a.unit = ts_unit_.p;
    a.rel = rel_.p;
    a.lvals = lvals_.p;
    a.winv = winv_.p;
    a.Z = ts_z_.p;
    a.U = ts_u_.p;
    if constexpr (std::is_same<T, double>::value)
      for (size_t l = 0; l + 1 < pl.level_ptr.size(); l++) {
        const int begin = pl.level_ptr[l], big = pl.big_ptr[l], end = pl.level_ptr[l + 1];
        if (big > begin) hipLaunchKernelGGL((k_tree_fwd<T>), dim3((unsigned)(big - begin)), dim3(TS_THREADS), ts_lds_, stream_, a, begin);
        if (end > big) hipLaunchKernelGGL((k_tree_fwd_big<T>), dim3((unsigned)(end - big)), dim3(TSB_THREADS), 0, stream_, a, big);
        const int s0 = pl.slab_ptr[l], ns = pl.slab_ptr[l + 1] - s0;
        if (ns > 0) hipLaunchKernelGGL((k_tree_fwd_big_update<T>), dim3((unsigned)ns), dim3(TSB_THREADS), 0, stream_, a, (const TsSlab *)ts_slab_.p, s0);
      }
    check_launch("k_tree_fwd");
  }

  // What a pass's kernel left in ts_out_, in order: n doubles for `to` (null: dropped)
  struct TsDest { double *to; size_t n; };

  // One call over the pairs (a[q], b[q]), q < n: linearise and factor, then the plan of the pairs, stage(q0, q1, plan), which
  // uploads the pairs' records and sizes ts_out_, the forward solve of the plan's columns, and launch(q0, q1), which launches
  // the pairs' kernel into ts_out_ and returns the TsDest list of what it writes.  A plan beyond the workspace bound is cut
  // in halves by index, and the parts run one after the other over the same factor.  ms: the call's three intervals (every
  // upload lies in the second); time_copy: the third ends behind the copy to the host.
  // cuts (optional): a table of n_parts + 1 ascending cut points, cuts[0] = 0 and cuts[n_parts] = n -- the list is then cut
  // at these points only, in halves by the index of the part (`what` names a part); stage and launch still get pair indices.
  // extra (optional): bytes(plan) = workspace of a pass beside Z + U, counted against the bound; solve(plan) is enqueued
  // behind the forward solve, inside the second interval.
  struct TsExtra {
    std::function<size_t(const TsPlan &)> bytes;
    std::function<void(const TsPlan &)> solve;
  };
  template <typename Stage, typename Launch>
  void tree_query(const char *who, const char *what, int n, const int32_t *a, const int32_t *b, const int64_t *off, double *ms,
                  bool time_copy, Stage &&stage, Launch &&launch, const int32_t *cuts = nullptr, int n_parts = 0,
                  const TsExtra *extra = nullptr) {
    for (int k = 0; k < 3; k++) ms[k] = 0;
    if (n == 0) return;
    auto first_of = [&](int u) { return cuts ? (int)cuts[u] : u; };   // the first pair of part u (no table: a part is a pair)
    HIPCHK(hipEventRecord(query_ev_[0], stream_));
    enqueue_factor(lin_system(0.0, 0));
    HIPCHK(hipEventRecord(query_ev_[1], stream_));
    bool first = true;   // the factorisation of this call has not been waited for yet
    std::vector<std::pair<int, int>> todo{{0, cuts ? n_parts : n}};   // ranges of parts still to run, the next one last
    std::vector<double> host;
    while (!todo.empty()) {
      const int u0 = todo.back().first, u1 = todo.back().second;
      const int q0 = first_of(u0), q1 = first_of(u1);
      todo.pop_back();
      TsPlan pl;
      covariances_plan(q0, q1, a, b, off, pl);
      const size_t ws = (size_t)(pl.zrows + pl.urows) * TS_MC * sizeof(T) + (extra ? extra->bytes(pl) : 0);
      if (ws > ts_ws_bytes_) {
        if (u1 - u0 <= 1) throw ApiError(RR_PGO_ENOMEM, std::string(who) + ": one " + what + " needs " + std::to_string(ws) + " bytes of workspace");
        const int mid = u0 + (u1 - u0) / 2;
        todo.emplace_back(mid, u1);
        todo.emplace_back(u0, mid);
        continue;
      }
      if (ts_trace_) trace_plan(who, q0, q1, a, b, pl, ws);
      ts_stage(pl);
      stage(q0, q1, pl);
      if (!first) HIPCHK(hipEventRecord(query_ev_[1], stream_));
      ts_forward(pl);
      if (extra) extra->solve(pl);
      HIPCHK(hipEventRecord(query_ev_[2], stream_));
      const auto dest = launch(q0, q1);
      size_t n_out = 0;
      for (const TsDest &d : dest) n_out += d.n;
      host.resize(n_out);
      if (!time_copy) HIPCHK(hipEventRecord(query_ev_[3], stream_));
      if (n_out > 0) HIPCHK(hipMemcpyAsync(host.data(), ts_out_.p, n_out * sizeof(double), hipMemcpyDeviceToHost, stream_));
      if (time_copy) HIPCHK(hipEventRecord(query_ev_[3], stream_));
      HIPCHK(hipStreamSynchronize(stream_));
      if (first) check_device_error();   // a non-positive pivot: nothing has been written
      query_times(ms, !first);
      first = false;
      const double *src = host.data();
      for (const TsDest &d : dest) {
        if (d.to && d.n > 0) std::memcpy(d.to, src, d.n * sizeof(double));
        src += d.n;
      }
    }
  }

  // ---- covariances of arbitrary node pairs (include/rr_pgo.h, rr_pgo_covariances; treesolve.hip.h, k_cov_pairs)
  void covariances(int nq, const int32_t *na, const int32_t *nb, const int64_t *off, double *out) override {
    static constexpr const char *who = "rr_pgo_covariances";
    require_f64_unsharded_lds_factor(who, !settings_.query_big);
    if constexpr (f64_) {
      covariances_prepare(who);
      tree_query(who, "pair", nq, na, nb, off, query_ms_[Q_COVARIANCES], false, [&](int q0, int q1, const TsPlan &pl) {
        ts_fill(ts_query_, pl.query);
        ts_grow(ts_out_, (size_t)(off[q1] - off[q0]));
      }, [&](int q0, int q1) {
        CovArgs<T> c;
        c.meta = ts_meta_.p;
        c.query = ts_query_.p;
        c.czrow = ts_czrow_.p;
        c.Z = ts_z_.p;
        c.out = ts_out_.p;
        c.S = sym_.S;
        hipLaunchKernelGGL((k_cov_pairs<T>), dim3((unsigned)(q1 - q0)), dim3(COV_THREADS), 0, stream_, c);
        check_launch("k_cov_pairs");
        return std::array<TsDest, 1>{{{out + off[q0], (size_t)(off[q1] - off[q0])}}};
      });
    }
  }

  // ---- Sigma[rows, cols] (include/rr_pgo.h, rr_pgo_cross_covariances; treesolve.hip.h, k_tree_bwd, k_cross_gather): the plan
  // of the columns is the covariance plan of the pairs (col, col), cut between column nodes; the backward sweep runs over the
  // union of the root paths of the row nodes, the same fronts for every chunk
  void cross_covariances(int n_row, const int32_t *row_node, int n_col, const int32_t *col_node, const int64_t *roff,
                         const int64_t *coff, double *out) override {
    static constexpr const char *who = "rr_pgo_cross_covariances";
    require_f64_unsharded_lds_factor(who, !settings_.query_big);
    if constexpr (f64_) {
      covariances_prepare(who);
      const Symbolic &sym = sym_;
      const int S_ = sym.S;
      const int64_t R = roff[n_row], C = coff[n_col];
      // ---- the backward-active fronts by depth, root level first (within a level: the LDS fronts in descending front index, as
      // sel_order_, then the fronts beyond LDS)
      std::vector<int32_t> fvrow((size_t)S_, -1), order, level_ptr;
      if (!row_node) std::fill(fvrow.begin(), fvrow.end(), 0);
      else
        for (int k = 0; k < n_row; k++)
          for (int f = front_of(row_node[k]); f >= 0 && fvrow[f] < 0; f = sym.sn_parent[f]) fvrow[f] = 0;
      const int max_depth = *std::max_element(front_depth_.begin(), front_depth_.end());
      level_ptr.assign((size_t)max_depth + 2, 0);
      for (int f = 0; f < S_; f++)
        if (fvrow[f] == 0) level_ptr[(size_t)front_depth_[f] + 1]++;
      for (int d = 0; d <= max_depth; d++) level_ptr[(size_t)d + 1] += level_ptr[d];
      order.resize((size_t)level_ptr[(size_t)max_depth + 1]);
      std::vector<int32_t> big_ptr(level_ptr.begin() + 1, level_ptr.end());   // per level: its first front beyond LDS (LDS fronts first)
      {
        std::vector<int32_t> fill(level_ptr.begin(), level_ptr.end() - 1);
        for (int f = S_ - 1; f >= 0; f--)
          if (fvrow[f] == 0 && sym.sn_big[f]) order[(size_t)--big_ptr[front_depth_[f]]] = f;
        for (int f = S_ - 1; f >= 0; f--)
          if (fvrow[f] == 0 && !sym.sn_big[f]) order[(size_t)fill[front_depth_[f]]++] = f;
      }
      std::vector<TsSlab> slab;               // the slabs of pivot rows of the fronts beyond LDS, by level
      std::vector<int32_t> slab_ptr(1, 0);
      for (int d = 0; d <= max_depth; d++) {
        for (int i = big_ptr[d]; i < level_ptr[(size_t)d + 1]; i++)
          for (int r0 = 0; r0 < sym.sn_ncols[order[i]]; r0 += TSB_SLAB) slab.push_back(TsSlab{order[i], r0});
        slab_ptr.push_back((int32_t)slab.size());
      }
      int64_t vrows = 0;   // rows of V per chunk
      for (int32_t f : order) {
        fvrow[f] = (int32_t)std::min<int64_t>(vrows, 0x7fffffff);   // (a plan beyond the workspace bound is dropped before these are read)
        vrows += (int64_t)sym.sn_ncols[f] + sym.sn_nrows[f];
      }
      // ---- row of out -> row of a chunk's part of V: reference scalar r of the node -> its permuted pivot row
      std::vector<int32_t> rsrc((size_t)R);
      for (int k = 0; k < n_row; k++) {
        const int v = row_node ? row_node[k] : k, f = front_of(v), d = node_dim(g_.node_kind[v]), p0 = sym.node_pcol[v];
        for (int i = 0; i < d; i++)
          rsrc[(size_t)(roff[k] + sym.perm[p0 + i] - g_.node_offset[v])] = is_fixed(v) ? -1 : fvrow[f] + (p0 + i - sym.sn_col0[f]);
      }
      std::vector<int64_t> csrc;
      std::vector<TsDest> dest;
      TsExtra extra;
      extra.bytes = [&](const TsPlan &pl) { return (size_t)pl.n_chunks * (size_t)vrows * TS_MC * sizeof(T); };
      extra.solve = [&](const TsPlan &pl) {
        TsBwdArgs<T> a;
        a.meta = ts_meta_.p;
        a.order = cross_order_.p;
        a.fvrow = cross_fvrow_.p;
        a.czrow = ts_czrow_.p;
        a.rel = rel_.p;
        a.lvals = lvals_.p;
        a.winv = winv_.p;
        a.Z = ts_z_.p;
        a.V = ts_v_.p;
        a.vrows = vrows;
        a.S = S_;
        if (ts_trace_) {
          int n_launch = 0;
          for (size_t l = 0; l + 1 < level_ptr.size(); l++)
            n_launch += (big_ptr[l] > level_ptr[l]) + (level_ptr[l + 1] > big_ptr[l]) + (slab_ptr[l + 1] > slab_ptr[l]);
          std::fprintf(stderr, "query trace:   backward: %zu fronts, %zu slabs, %d launches\n", order.size(), slab.size(), n_launch);
        }
        if constexpr (std::is_same<T, double>::value)
          for (size_t l = 0; l + 1 < level_ptr.size(); l++) {
            const int begin = level_ptr[l], big = big_ptr[l], end = level_ptr[l + 1];
            const unsigned nch = (unsigned)pl.n_chunks;
            if (big > begin) hipLaunchKernelGGL((k_tree_bwd<T>), dim3((unsigned)(big - begin), nch), dim3(TS_THREADS), ts_lds_, stream_, a, begin);
            const int s0 = slab_ptr[l], ns = slab_ptr[l + 1] - s0;
            if (ns > 0) hipLaunchKernelGGL((k_tree_bwd_big_gemv<T>), dim3((unsigned)ns, nch), dim3(TSB_THREADS), 0, stream_, a, (const TsSlab *)cross_slab_.p, s0);
            if (end > big) hipLaunchKernelGGL((k_tree_bwd_big<T>), dim3((unsigned)(end - big), nch), dim3(TSB_THREADS), 0, stream_, a, big);
          }
        check_launch("k_tree_bwd");
      };
      tree_query(who, "column node", n_col, col_node, col_node, coff, query_ms_[Q_CROSS], true, [&](int q0, int q1, const TsPlan &pl) {
        // column of this part's out -> (chunk, column) in V: reference scalar r of the node -> its column in the chunk
        const int64_t Cp = coff[q1] - coff[q0];
        csrc.assign((size_t)Cp, -1);
        for (int q = q0; q < q1; q++) {
          const CovQuery &cq = pl.query[q - q0];
          if (is_fixed(col_node[q])) continue;
          for (int r = 0; r < cq.da; r++) csrc[(size_t)(coff[q] - coff[q0] + r)] = (int64_t)cq.chunk_a * vrows * TS_MC + cq.ca[r];
        }
        ts_fill(cross_order_, order);
        ts_fill(cross_fvrow_, fvrow);
        if (!slab.empty()) ts_fill(cross_slab_, slab);
        ts_fill(cross_rsrc_, rsrc);
        ts_fill(cross_csrc_, csrc);
        ts_grow(ts_v_, (size_t)pl.n_chunks * (size_t)vrows * TS_MC);
        ts_grow(ts_out_, (size_t)(R * Cp));
      }, [&](int q0, int q1) -> const std::vector<TsDest> & {
        const int64_t Cp = coff[q1] - coff[q0];
        CrossArgs<T> c;
        c.V = ts_v_.p;
        c.rsrc = cross_rsrc_.p;
        c.csrc = cross_csrc_.p;
        c.out = ts_out_.p;
        c.R = R;
        c.C = Cp;
        if (R * Cp > 0) hipLaunchKernelGGL((k_cross_gather<T>), dim3((unsigned)((R * Cp + 255) / 256)), dim3(256), 0, stream_, c);
        check_launch("k_cross_gather");
        dest.clear();
        if (Cp == C) dest.push_back({out, (size_t)(R * C)});
        else
          for (int64_t i = 0; i < R; i++) dest.push_back({out + i * C + coff[q0], (size_t)Cp});   // a part holds some columns of every row
        return dest;
      }, nullptr, 0, &extra);
    }
  }

  // a record of kind RR_PGO_EDGE_SE2_BEARING / _RANGE among the call's records (the whole call decides, not a cut of its plan)
  static bool cand_has_br(const std::vector<GateCand> &cand) {
    for (const GateCand &c : cand)
      if (edge_is_br(c.kind)) return true;
    return false;
  }
  // ---- Mahalanobis gate of candidate edges (include/rr_pgo.h, rr_pgo_gate_edges; treesolve.hip.h, k_gate_pairs): the plan
  // of the candidates' nodes is the covariance plan of the pairs (from, to)
  void gate_edges(int n, const int32_t *from, const int32_t *to, const int64_t *soff, std::vector<GateCand> &cand, double *d2,
                  double *chi2, double *innov) override {
    static constexpr const char *who = "rr_pgo_gate_edges";
    require_f64_unsharded_lds_factor(who, !settings_.query_big);
    if constexpr (f64_) {
      covariances_prepare(who);
      const bool br = has_br_ || cand_has_br(cand);   // the BR kernel: the graph or the call holds a bearing / range edge
      auto n_innov = [&](int c0, int c1) { return innov ? (size_t)(soff[c1] - soff[c0]) : 0; };
      tree_query(who, "candidate", n, from, to, soff, query_ms_[Q_GATE], true, [&](int c0, int c1, const TsPlan &pl) {
        const size_t nc = (size_t)(c1 - c0);
        for (int c = c0; c < c1; c++) {
          cand[c].cq = pl.query[c - c0];
          cand[c].fa = front_of(from[c]);
          cand[c].fb = front_of(to[c]);
        }
        ts_grow(gate_cand_, nc);
        HIPCHK(hipMemcpyAsync(gate_cand_.p, cand.data() + c0, nc * sizeof(GateCand), hipMemcpyHostToDevice, stream_));
        ts_grow(ts_out_, 2 * nc + n_innov(c0, c1));
      }, [&](int c0, int c1) {
        const size_t nc = (size_t)(c1 - c0);
        GateArgs<T> a;
        a.meta = ts_meta_.p;
        a.cand = gate_cand_.p;
        a.czrow = ts_czrow_.p;
        a.Z = ts_z_.p;
        a.pose = pose_.p;
        a.d2 = ts_out_.p;
        a.chi2 = ts_out_.p + nc;
        a.sout = innov ? ts_out_.p + 2 * nc : nullptr;
        a.S = sym_.S;
        if (has_lm_) hipLaunchKernelGGL((k_gate_pairs<T, 6, true>), dim3((unsigned)nc), dim3(COV_THREADS), 0, stream_, a);
        else if (br) hipLaunchKernelGGL((k_gate_pairs<T, 3, true>), dim3((unsigned)nc), dim3(COV_THREADS), 0, stream_, a);
        else if (is3d_) hipLaunchKernelGGL((k_gate_pairs<T, 6>), dim3((unsigned)nc), dim3(COV_THREADS), 0, stream_, a);
        else hipLaunchKernelGGL((k_gate_pairs<T, 3>), dim3((unsigned)nc), dim3(COV_THREADS), 0, stream_, a);
        check_launch("k_gate_pairs");
        return std::array<TsDest, 3>{{{d2 + c0, nc}, {chi2 ? chi2 + c0 : nullptr, nc}, {innov ? innov + soff[c0] : nullptr, n_innov(c0, c1)}}};
      });
    }
  }

  // ---- audit of the graph's own edges (include/rr_pgo.h, rr_pgo_check_edges; treesolve.hip.h, k_check_edges): the gate's plan
  // and records, for edges of the graph; the robust kind and delta travel in the arguments
  void refuse_factor_query(const char *who) const override { require_f64_unsharded_lds_factor(who, !settings_.query_big); }
  void check_edges(int n, const int32_t *from, const int32_t *to, const int64_t *soff, std::vector<GateCand> &cand, double *d2,
                   double *red, double *chi2, double *resid) override {
    static constexpr const char *who = "rr_pgo_check_edges";
    require_f64_unsharded_lds_factor(who, !settings_.query_big);
    if constexpr (f64_) {
      covariances_prepare(who);
      const bool br = has_br_ || cand_has_br(cand);   // the BR kernel: the graph or the call holds a bearing / range edge
      auto n_resid = [&](int c0, int c1) { return resid ? (size_t)(soff[c1] - soff[c0]) : 0; };
      tree_query(who, "edge", n, from, to, soff, query_ms_[Q_CHECK], true, [&](int c0, int c1, const TsPlan &pl) {
        const size_t nc = (size_t)(c1 - c0);
        for (int c = c0; c < c1; c++) {
          cand[c].cq = pl.query[c - c0];
          cand[c].fa = front_of(from[c]);
          cand[c].fb = front_of(to[c]);
        }
        ts_grow(gate_cand_, nc);
        HIPCHK(hipMemcpyAsync(gate_cand_.p, cand.data() + c0, nc * sizeof(GateCand), hipMemcpyHostToDevice, stream_));
        ts_grow(ts_out_, 3 * nc + n_resid(c0, c1));
      }, [&](int c0, int c1) {
        const size_t nc = (size_t)(c1 - c0);
        CheckArgs<T> a;
        a.meta = ts_meta_.p;
        a.cand = gate_cand_.p;
        a.czrow = ts_czrow_.p;
        a.Z = ts_z_.p;
        a.pose = pose_.p;
        a.d2 = ts_out_.p;
        a.chi2 = ts_out_.p + nc;
        a.red = ts_out_.p + 2 * nc;
        a.rout = resid ? ts_out_.p + 3 * nc : nullptr;
        a.delta = (T)settings_.robust_delta;
        a.delta2 = (T)(settings_.robust_delta * settings_.robust_delta);
        a.S = sym_.S;
        a.rkind = settings_.robust_kind;
        const TlsParams tp = tls_params();
        a.tls_lo = (T)tp.lo; a.tls_hi = (T)tp.hi; a.tls_cs = (T)tp.cs; a.tls_mu = (T)tp.mu;
        if (has_lm_) hipLaunchKernelGGL((k_check_edges<T, 6, true>), dim3((unsigned)nc), dim3(COV_THREADS), 0, stream_, a);
        else if (br) hipLaunchKernelGGL((k_check_edges<T, 3, true>), dim3((unsigned)nc), dim3(COV_THREADS), 0, stream_, a);
        else if (is3d_) hipLaunchKernelGGL((k_check_edges<T, 6>), dim3((unsigned)nc), dim3(COV_THREADS), 0, stream_, a);
        else hipLaunchKernelGGL((k_check_edges<T, 3>), dim3((unsigned)nc), dim3(COV_THREADS), 0, stream_, a);
        check_launch("k_check_edges");
        return std::array<TsDest, 4>{{{d2 + c0, nc}, {chi2 ? chi2 + c0 : nullptr, nc}, {red ? red + c0 : nullptr, nc},
                                      {resid ? resid + soff[c0] : nullptr, n_resid(c0, c1)}}};
      });
    }
  }

  // ---- joint compatibility of sets of candidate edges (include/rr_pgo.h, rr_pgo_gate_joint; treesolve.hip.h, k_gate_joint):
  // the plan is the covariance plan of the sets' pairs (from, to), one after the other, cut at set boundaries only
  void gate_joint(int n_sets, const int32_t *set_ptr, const int32_t *from, const int32_t *to, const int32_t *dim,
                  const int64_t *ioff, std::vector<GateCand> &cand, double *d2, double *prefix, double *innov) override {
    static constexpr const char *who = "rr_pgo_gate_joint";
    require_f64_unsharded_lds_factor(who, !settings_.query_big);
    if constexpr (f64_) {
      covariances_prepare(who);
      const bool br = has_br_ || cand_has_br(cand);   // the BR kernel: the graph or the call holds a bearing / range edge
      const Symbolic &sym = sym_;
      const int n = n_sets > 0 ? set_ptr[n_sets] : 0;
      const std::vector<int64_t> no_off((size_t)n + 1, 0);   // (a pair's record carries no output offset here)
      std::vector<JointSet> sets;
      std::vector<int32_t> fnc, fz, fronts, slot((size_t)sym.S, -1);   // slot: front -> its place among the set's fronts
      auto set_of = [&](int q) { return (int)(std::lower_bound(set_ptr, set_ptr + n_sets + 1, q) - set_ptr); };   // (no set is empty)
      auto n_innov = [&](int s0, int s1) { return innov ? (size_t)(ioff[s1] - ioff[s0]) : 0; };
      tree_query(who, "set", n, from, to, no_off.data(), query_ms_[Q_GATE_JOINT], true, [&](int q0, int q1, const TsPlan &pl) {
        const int s0 = set_of(q0), s1 = set_of(q1);
        sets.clear();
        fnc.clear();
        fz.clear();
        for (int s = s0; s < s1; s++) {
          const int c0 = set_ptr[s], m = set_ptr[s + 1] - c0;
          // the union of the root paths of the set's nodes, ascending front index (children precede parents)
          fronts.clear();
          for (int k = c0; k < c0 + m; k++) {
            cand[k].cq = pl.query[k - q0];
            cand[k].fa = front_of(from[k]);
            cand[k].fb = front_of(to[k]);
            for (int f0 : {cand[k].fa, cand[k].fb})
              for (int f = f0; f >= 0 && slot[f] < 0; f = sym.sn_parent[f]) {
                slot[f] = 0;
                fronts.push_back(f);
              }
          }
          std::sort(fronts.begin(), fronts.end());
          const int nf = (int)fronts.size();
          JointSet js{};
          js.cand0 = c0 - q0;
          js.m = m;
          js.dim = dim[s];
          js.n_front = nf;
          js.fptr = (int64_t)fnc.size();
          js.zptr = (int64_t)fz.size();
          js.soff = innov ? ioff[s] - ioff[s0] : 0;
          for (int i = 0; i < nf; i++) {
            slot[fronts[i]] = i;
            fnc.push_back(sym.sn_ncols[fronts[i]]);
          }
          // per (front, candidate): the first Z row of `from` and of `to` there, -1 where the front is not on the node's path
          fz.resize(fz.size() + (size_t)nf * m * 2, -1);
          int32_t *z = fz.data() + js.zptr;
          for (int k = c0; k < c0 + m; k++) {
            const int chunk[2] = {cand[k].cq.chunk_a, cand[k].cq.chunk_b}, f0[2] = {cand[k].fa, cand[k].fb};
            for (int side = 0; side < 2; side++)
              for (int f = f0[side]; f >= 0; f = sym.sn_parent[f]) {
                const int32_t zr = pl.czrow[(size_t)chunk[side] * sym.S + f];
                if (zr < 0) throw ApiError(RR_PGO_ENODEVICE, std::string(who) + ": internal: a front of a node's path is not active in its chunk");
                z[((size_t)slot[f] * m + (k - c0)) * 2 + side] = zr;
              }
          }
          for (int f : fronts) slot[f] = -1;
          sets.push_back(js);
        }
        ts_fill(joint_set_, sets);
        ts_fill(joint_fnc_, fnc);
        ts_fill(joint_fz_, fz);
        const size_t nc = (size_t)(q1 - q0);
        ts_grow(gate_cand_, nc);
        HIPCHK(hipMemcpyAsync(gate_cand_.p, cand.data() + q0, nc * sizeof(GateCand), hipMemcpyHostToDevice, stream_));
        ts_grow(ts_out_, (size_t)(s1 - s0) + nc + n_innov(s0, s1));
      }, [&](int q0, int q1) {
        const int s0 = set_of(q0), s1 = set_of(q1);
        const size_t ns = (size_t)(s1 - s0), nc = (size_t)(q1 - q0);
        JointArgs<T> a;
        a.set = joint_set_.p;
        a.cand = gate_cand_.p;
        a.fnc = joint_fnc_.p;
        a.fz = joint_fz_.p;
        a.Z = ts_z_.p;
        a.pose = pose_.p;
        a.d2 = ts_out_.p;
        a.prefix = ts_out_.p + ns;
        a.sout = innov ? ts_out_.p + ns + nc : nullptr;
        if (has_lm_) hipLaunchKernelGGL((k_gate_joint<T, 6, true>), dim3((unsigned)ns), dim3(COV_THREADS), 0, stream_, a);
        else if (br) hipLaunchKernelGGL((k_gate_joint<T, 3, true>), dim3((unsigned)ns), dim3(COV_THREADS), 0, stream_, a);
        else if (is3d_) hipLaunchKernelGGL((k_gate_joint<T, 6>), dim3((unsigned)ns), dim3(COV_THREADS), 0, stream_, a);
        else hipLaunchKernelGGL((k_gate_joint<T, 3>), dim3((unsigned)ns), dim3(COV_THREADS), 0, stream_, a);
        check_launch("k_gate_joint");
        return std::array<TsDest, 3>{{{d2 + s0, ns}, {prefix ? prefix + q0 : nullptr, nc}, {innov ? innov + ioff[s0] : nullptr, n_innov(s0, s1)}}};
      }, set_ptr, n_sets);
    }
  }

  // Test-only failure injection: make ONE hand-off of a dataflow launch never arrive, so that the waits behind it run
  // into their time bound (RR_PGO_FLOW_TIMEOUT_MS).  mode 1: k_factor_flow -- the root front's last foreign child's flag
  // is looked for in a word nobody sets; 2: k_solve_flow -- the same for the parent flag of one front; 3: k_big_flow --
  // the first PANEL task of the first flow level publishes its X blocks in the dead words behind the live flags;
  // 0: everything back.  The captured graphs hold pointers, not contents: no re-capture.
  void debug_withhold(int mode) override {
    HIPCHK(hipStreamSynchronize(stream_));
    if (mode == 0) {
      if (withheld_child_ >= 0) {
        HIPCHK(hipMemcpy(child_dep_.p + withheld_child_, &host_child_dep_[withheld_child_], sizeof(int32_t), hipMemcpyHostToDevice));
        withheld_child_ = -1;
      }
      if (withheld_parent_ >= 0) {
        HIPCHK(hipMemcpy(parent_dep_.p + withheld_parent_, &withheld_parent_val_, sizeof(int32_t), hipMemcpyHostToDevice));
        withheld_parent_ = -1;
      }
      if (withheld_level_ >= 0) {
        FlowRec *dst = withheld_level_ == (1 << 30) ? xl_recs_.p : plan_[withheld_level_].flow->tasks.p;
        HIPCHK(hipMemcpy(dst + withheld_task_, &withheld_rec_, sizeof(FlowRec), hipMemcpyHostToDevice));
        withheld_level_ = -1;
      }
      return;
    }
    if (mode == 1 || mode == 2) {
      if (!lds_flow_) throw ApiError(RR_PGO_EUNSUPPORTED, "this handle does not run the dataflow launches of the LDS fronts");
      const int32_t dead = 2 * sym_.S + 96;   // inside dep_flags_, behind the words the linearisation zeroes, never set
      if (mode == 1) {
        for (int q = (int)host_child_dep_.size() - 1; q >= 0; q--)
          if (host_child_dep_[q] >= 0) {
            HIPCHK(hipMemcpy(child_dep_.p + q, &dead, sizeof(int32_t), hipMemcpyHostToDevice));
            withheld_child_ = q;
            return;
          }
        throw ApiError(RR_PGO_EUNSUPPORTED, "no front waits for a child of another task");
      }
      std::vector<int32_t> pd(sym_.S);
      HIPCHK(hipMemcpy(pd.data(), parent_dep_.p, pd.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (int f = 0; f < sym_.S; f++)
        if (pd[f] >= 0) {
          withheld_parent_ = f;
          withheld_parent_val_ = pd[f];
          HIPCHK(hipMemcpy(parent_dep_.p + f, &dead, sizeof(int32_t), hipMemcpyHostToDevice));
          return;
        }
      throw ApiError(RR_PGO_EUNSUPPORTED, "no front waits for a parent of another task");
    }
    if (mode == 3 && xl_) {
      for (size_t t = 0; t < xl_host_.size(); t++)
        if ((xl_host_[t].t.kind_front >> 24) == FLOW_PANEL) {
          withheld_level_ = 1 << 30;   // (the cross-level list)
          withheld_task_ = (int)t;
          withheld_rec_ = xl_host_[t];
          FlowRec bad = xl_host_[t];
          bad.ff.pf = (int32_t)((int64_t)flow_flags_.n - kDeadFlagWords);
          bad.ff.pstride = 1;
          HIPCHK(hipMemcpy(xl_recs_.p + t, &bad, sizeof(FlowRec), hipMemcpyHostToDevice));
          return;
        }
      throw ApiError(RR_PGO_EUNSUPPORTED, "no PANEL task in the cross-level list");
    }
    if (mode == 3) {
      for (size_t si = 0; si < plan_.size(); si++) {
        if (!plan_[si].flow) continue;
        FlowLevel &l = *plan_[si].flow;
        std::vector<FlowRec> recs((size_t)l.n_tasks);
        HIPCHK(hipMemcpy(recs.data(), l.tasks.p, recs.size() * sizeof(FlowRec), hipMemcpyDeviceToHost));
        for (int t = 0; t < l.n_tasks; t++)
          if ((recs[t].t.kind_front >> 24) == FLOW_PANEL) {
            withheld_level_ = (int)si;
            withheld_task_ = t;
            withheld_rec_ = recs[t];
            FlowRec bad = recs[t];
            bad.ff.pf = (int32_t)((int64_t)flow_flags_.n - kDeadFlagWords);   // its X flags land in the dead words
            bad.ff.pstride = 1;
            HIPCHK(hipMemcpy(l.tasks.p + t, &bad, sizeof(FlowRec), hipMemcpyHostToDevice));
            return;
          }
      }
      throw ApiError(RR_PGO_EUNSUPPORTED, "this handle has no dataflow level of fronts beyond LDS");
    }
    throw ApiError(RR_PGO_EINVAL, "mode must be 0 .. 3");
  }

  void profile(int iters, double *ms, int64_t *launches) override {
    HIPCHK(hipEventCreate(&prof_.e0));
    HIPCHK(hipEventCreate(&prof_.e1));
    for (int k = 0; k < RR_PGO_NUM_KCLASS; k++) { prof_.ms[k] = 0; prof_.n[k] = 0; }
    prof_.on = true;
    try {
      for (int i = 0; i < iters; i++) { enqueue_gn_iteration(); launch_counts[0]++; }
      HIPCHK(hipStreamSynchronize(stream_));
    } catch (...) {
      prof_.on = false;
      throw;
    }
    prof_.on = false;
    (void)hipEventDestroy(prof_.e0);
    (void)hipEventDestroy(prof_.e1);
    for (int k = 0; k < RR_PGO_NUM_KCLASS; k++) { ms[k] = prof_.ms[k]; launches[k] = prof_.n[k]; }
  }
};

}  // namespace rrpgo

// ============================================================== C ABI

using namespace rrpgo;

struct rr_pgo {
  // behind a pointer: the engine keeps a reference to the graph, and rr_pgo_extend swaps graph, analysis and engine together
  std::unique_ptr<HostGraph> g = std::make_unique<HostGraph>();
  std::shared_ptr<const Symbolic> symp;   // shared with the analysis cache (structurally identical graphs analysed once)
  const Symbolic &sym_ref() const { return *symp; }
  rr_pgo_options opt;
  std::unique_ptr<EngineBase> engine;
  rr_pgo_stats stats;
  std::vector<int32_t> blk_rows, blk_cols;   // assemble() block list
  std::vector<int64_t> blk_offs;
  double extend_ms[3] = {0, 0, 0};   // the last rr_pgo_extend: analysis, engine (host wall clock), state carry + guess (HIP events)
  double remove_ms[3] = {0, 0, 0};   // the last rr_pgo_remove_edges: analysis, engine (host wall clock), state carry (HIP events)
};

struct rr_pgo_synth {
  HostGraph g;
};

namespace {

template <typename F> int guarded(F &&f) {
  try {
    f();
    return RR_PGO_OK;
  } catch (const ApiError &e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc &) {
    g_last_error = "out of host memory";
    return RR_PGO_ENOMEM;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return RR_PGO_EINVAL;
  }
}

void fill_desc(const HostGraph &g, rr_pgo_graph_desc *d) {
  d->n_nodes = g.n_nodes();
  d->node_kind = g.node_kind.data();
  d->node_id = g.node_id.data();
  d->node_state = g.node_state.data();
  d->n_edges = g.n_edges();
  d->edge_kind = g.edge_kind.data();
  d->edge_from = g.edge_from.data();
  d->edge_to = g.edge_to.data();
  d->edge_meas = g.edge_meas.data();
  d->edge_info = g.edge_info.data();
}

// ---- analysis cache: the last few analyses of this process, keyed by everything they depend on
struct AnalysisCacheEntry {
  uint64_t key;
  int32_t precision, rank, world_size, sharded;
  std::vector<int32_t> node_kind, edge_kind, edge_from, edge_to;
  std::vector<double> node_state;
  std::string env;
  std::shared_ptr<const Symbolic> sym;
};
static std::mutex g_analysis_mu;
static std::vector<AnalysisCacheEntry> g_analysis_cache;   // most recent last; at most four graphs of at most 50 000 edges
extern "C" char **environ;
static std::string analysis_env() {   // every RR_PGO_* switch of the process (the analysis reads a dozen of them)
  std::string e;
  for (char **p = environ; p && *p; p++)
    if (std::strncmp(*p, "RR_PGO_", 7) == 0) { e += *p; e += '\n'; }
  return e;
}
static uint64_t fnv(uint64_t h, const void *data, size_t n) {
  const unsigned char *p = (const unsigned char *)data;
  for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}
static uint64_t analysis_cache_key(const HostGraph &g, const rr_pgo_options &opt) {
  if (const char *e = std::getenv("RR_PGO_ANALYSIS_CACHE")) if (std::atoi(e) == 0) return 0;
  if (g.n_edges() > 50000 || g.n_edges() == 0) return 0;   // (the reference's datasets: at most 17 605 edges; the tables of a large graph are not worth keeping)
  uint64_t h = 1469598103934665603ull;
  const int32_t o[4] = {opt.precision, opt.rank, opt.world_size, opt.sharded};
  h = fnv(h, o, sizeof o);
  h = fnv(h, g.node_kind.data(), g.node_kind.size() * 4);
  h = fnv(h, g.edge_kind.data(), g.edge_kind.size() * 4);
  h = fnv(h, g.edge_from.data(), g.edge_from.size() * 4);
  h = fnv(h, g.edge_to.data(), g.edge_to.size() * 4);
  h = fnv(h, g.node_state.data(), g.node_state.size() * 8);
  return h ? h : 1;
}
static bool analysis_same(const AnalysisCacheEntry &c, uint64_t key, const HostGraph &g, const rr_pgo_options &opt, const std::string &env) {
  return c.key == key && c.precision == opt.precision && c.rank == opt.rank && c.world_size == opt.world_size && c.sharded == opt.sharded &&
         c.node_kind == g.node_kind && c.edge_kind == g.edge_kind && c.edge_from == g.edge_from && c.edge_to == g.edge_to && c.node_state == g.node_state && c.env == env;
}
static std::shared_ptr<const Symbolic> analysis_cache_find(uint64_t key, const HostGraph &g, const rr_pgo_options &opt) {
  const std::string env = analysis_env();
  std::lock_guard<std::mutex> lk(g_analysis_mu);
  for (const AnalysisCacheEntry &c : g_analysis_cache)
    if (analysis_same(c, key, g, opt, env)) return c.sym;
  return nullptr;
}
static void analysis_cache_store(uint64_t key, const HostGraph &g, const rr_pgo_options &opt, std::shared_ptr<const Symbolic> sym) {
  AnalysisCacheEntry c{key, opt.precision, opt.rank, opt.world_size, opt.sharded, g.node_kind, g.edge_kind, g.edge_from, g.edge_to, g.node_state, analysis_env(), std::move(sym)};
  std::lock_guard<std::mutex> lk(g_analysis_mu);
  if (g_analysis_cache.size() >= 4) g_analysis_cache.erase(g_analysis_cache.begin());
  g_analysis_cache.push_back(std::move(c));
}

// host part of PoseGraph::new: options, symbolic analysis, the statistics that need no device
void analyze_handle(rr_pgo &h, const rr_pgo_options *opt_in, double parse_ms) {
  rr_pgo_options opt;
  if (opt_in) opt = *opt_in; else rr_pgo_default_options(&opt);
  h.opt = opt;
  if (opt.precision != RR_PGO_F64 && opt.precision != RR_PGO_F32 && opt.precision != RR_PGO_MIXED)
    throw ApiError(RR_PGO_EINVAL, "bad precision");
  if (opt.world_size > 1) {
    if (opt.world_size & (opt.world_size - 1)) throw ApiError(RR_PGO_EINVAL, "world_size must be a power of two");
    if (opt.world_size > 64) throw ApiError(RR_PGO_EINVAL, "world_size must be at most 64");
    if (opt.rank < 0 || opt.rank >= opt.world_size) throw ApiError(RR_PGO_EINVAL, "rank out of range");
  }
  // symbolic analysis (host only)
  SymbolicOptions so;
  so.lds_budget_elems = opt.precision == RR_PGO_F64 ? 19000 : 38000;
  // nested dissection down to leaves of this many nodes on large graphs (measured on the 400 x 250 lattice, r02:
  // fp32 6.05 ms per step with 48, 6.09 with 40, 6.12 with 56, 6.21 with 64; fp64 -- half the LDS budget per front --
  // 9.78 with 32, 10.41 with 48 or 64)
  const int big_leaf = opt.precision == RR_PGO_F64 ? 32 : 48;
  so.nd_leaf = h.g->n_nodes() <= 6000 ? (1 << 30) : big_leaf;
  so.split_separators = h.g->n_nodes() > 6000;   // wide top fronts: see symbolic.cpp, supernode pass
  if (opt.world_size > 1) {   // sharding needs the nested-dissection top levels
    so.n_parts = opt.world_size;
    so.my_part = opt.rank;
    so.nd_leaf = big_leaf;
    so.pin_node = h.g->anchor_node;   // every rank needs the anchor's entries of the solution (gauge transfer)
  }
  // tuning knobs of the symbolic phase
  // graphs whose fronts all fit LDS: ONE dataflow launch for the factorisation, one for the back substitution (lds_flow.hip.h);
  // RR_PGO_LDS_FLOW=0 keeps one launch per level of the task tree (the parity alternative: bit-identical results)
  so.lds_flow = opt.world_size <= 1 && !opt.sharded;
  if (const char *e = std::getenv("RR_PGO_LDS_FLOW")) so.lds_flow = so.lds_flow && std::atoi(e) != 0;
  if (const char *e = std::getenv("RR_PGO_TASK_US")) so.task_us = std::atof(e);
  if (std::getenv("RR_PGO_NO_GEO")) so.geo_nd = false;
  // small graphs (trajectories with loop closures): the multilevel bisection finds narrower separators (intel: 97 -> 60 nodes along the heaviest root path) than the
  // level sets / coordinate cuts (symbolic.cpp, MultilevelBisection); the lattice's straight cuts are already the best there are
  so.ml_nd = h.g->n_nodes() <= 6000;
  if (const char *e = std::getenv("RR_PGO_ML_ND")) so.ml_nd = std::atoi(e) != 0;
  if (const char *e = std::getenv("RR_PGO_LDS_PIECES")) so.max_lds_pieces = std::max(1, std::atoi(e));
  // RR_PGO_JOIN_SEPARATORS=1: a region's last separator always chained into its parent separator's supernode; =0: never (small graphs:
  // no longer a choice of the candidates below)
  const char *join_env = std::getenv("RR_PGO_JOIN_SEPARATORS");
  if (join_env) so.split_separators = std::atoi(join_env) == 0 && join_env[0] == '0';
  if (const char *e = std::getenv("RR_PGO_ND_LEAF")) so.nd_leaf = std::atoi(e);
  if (const char *e = std::getenv("RR_PGO_BALANCE_BLOCKS")) { so.balance_blocks = std::atoi(e) != 0; if (std::atoi(e) > 1) so.balance_max_rem = std::atoi(e); }
  // the widest front the chain pass may merge into its parent (when the cost model says the parent finishes earlier): 80 pivot
  // columns for 2D graphs, 48 for 6 x 6 blocks -- re-measured on the r05 / r06 trees (profiles/r06_chain_cap_sweep.txt: intel + 3.1 %,
  // M3500 - 0.3 %, dlr + 0.0 % at 80; the SE(3) graphs lose 0.4 - 2 % beyond 48, where the model's error grows with the front)
  if (!h.g->has_se3) so.merge_chain_nc = 80;
  if (const char *e = std::getenv("RR_PGO_MERGE_CHAIN")) { so.merge_chain_nc = std::atoi(e); if (const char *c = std::strchr(e, ',')) so.merge_chain_gain_us = std::atof(c + 1); }
  if (const char *e = std::getenv("RR_PGO_AMALG_NP")) so.amalg_np = std::atoi(e);
  // Pivot nodes of every supernode in arrival order and children added mid-panel (symbolic.cpp, step 5), where every front lives
  // in LDS and the factor is fp64.  RR_PGO_ARRIVAL_ORDER=0: the elimination order, every child before the panel (the order of
  // r18 and before: the same bits).  An fp32 factor (f32, mixed) always keeps that order: far from the answer its iterates carry
  // cond(H) x 2^-24 of rounding, which another pivot order moves like another summation order does (dlr, Levenberg-Marquardt: the K
  // form and the chain form of the back substitution settle 7e-4 apart in the old order, 1.4e-3 in the new), and the fp32
  // workloads that are measured have fronts beyond LDS
  so.arrival_order = opt.precision == RR_PGO_F64;
  if (const char *e = std::getenv("RR_PGO_ARRIVAL_ORDER")) so.arrival_order = so.arrival_order && std::atoi(e) != 0;
  double t0 = now_ms();
  std::string err;
  // The analysis is a function of the graph's structure (and, through the coordinate cuts, of the initial positions), the options
  // and the switches above -- not of the measurements.  A caller that builds the same graph again (the reference's own bench is a
  // loop of PoseGraph::new(file) + optimize(10), benches/graph_slam.rs:9-10; UMFPACK users keep the symbolic object for the same
  // reason) gets the tables of the first analysis.  RR_PGO_ANALYSIS_CACHE=0: every handle is analysed afresh.
  const uint64_t cache_key = analysis_cache_key(*h.g, opt);
  if (cache_key != 0)
    if (std::shared_ptr<const Symbolic> hit = analysis_cache_find(cache_key, *h.g, opt)) h.symp = hit;
  Symbolic fresh;
  if (h.symp) {
  } else
  if (h.g->n_nodes() <= 6000 && opt.world_size <= 1 && !opt.sharded && !(std::getenv("RR_PGO_ND_LEAF") && std::getenv("RR_PGO_AMALG_NP"))) {
    // Small graphs are bound by the critical path through the supernode tree, not by flops: a few
    // nested-dissection cuts above minimum-degree leaves shorten that path on the larger ones (M3500, dlr,
    // sphere2500: +20..26 % measured) and lengthen it on intel; merging mid-sized fronts (relaxed amalgamation up to 72
    // pivot columns) pays on sphere2500 and costs 2 - 4 % on intel, M3500 and dlr now that the fronts on the chain are merged
    // by their own rule (symbolic.cpp, step 5).  The front cost model ranks the candidates the way the measurements do, so
    // the estimated critical path picks the leaf size and the amalgamation width.  Below 2400 nodes no cut ever won.
    // The candidates are independent host computations: one thread each (r04: the six analyses in sequence were 35 ms
    // of M3500's and 55 ms of dlr's constructor on the GPU box, against 2 - 3 ms of optimize(10)).
    static const int kLeafLevelSets[] = {1 << 30, 3000, 2000, 1400, 1000, 700};
    static const int kLeafMultilevel[] = {1 << 30, 250, 150, 100, 70, 50};   // (500 never won on any graph of the test set)
    struct Cand { int leaf, np; bool split; };
    const bool np_fixed = std::getenv("RR_PGO_AMALG_NP") != nullptr;
    std::vector<Cand> cl;
    for (int li = 0; li < 6; li++) {
      int leaf = so.ml_nd ? kLeafMultilevel[li] : kLeafLevelSets[li];
      if (std::getenv("RR_PGO_ND_LEAF")) { if (leaf != (1 << 30)) continue; leaf = so.nd_leaf; }
      else if (leaf != (1 << 30) && ((!so.ml_nd && h.g->n_nodes() < 2400) || leaf >= h.g->n_nodes())) continue;   // (a leaf size >= the graph is no cut at all)
      // (with the multilevel bisection the undissected tree lost on every graph of 1000+ nodes by 30 - 60 % of the estimate, and its
      // minimum-degree pass over the whole graph is the slowest of the candidate analyses: 5.8 ms on dlr)
      if (so.ml_nd && leaf == (1 << 30) && h.g->n_nodes() >= 1000 && !std::getenv("RR_PGO_ND_LEAF")) continue;
      cl.push_back({leaf, np_fixed ? so.amalg_np : 16, so.split_separators});   // the narrow rule first: it wins wherever every front lives in LDS
    }
    const size_t n_depths = cl.size();
    // the deepest dissections once more with mid-sized fronts merged up to 32 columns (intel, r05: the model's and the measured best)
    if (so.ml_nd && !np_fixed && !std::getenv("RR_PGO_ND_LEAF"))
      for (int leaf : {70, 50})
        if (leaf < h.g->n_nodes()) cl.push_back({leaf, 32, so.split_separators});
    // ... and the deeper dissections with a region's last separator NOT chained into its parent separator's supernode (the rule of the
    // large graphs, symbolic.cpp step 4): the sibling separator then runs beside it instead of before it.  Measured (r05, same kernels):
    // sphere2500 1539 -> 1697 it/s, torus3D 1066 -> 1191, dlr 7369 -> 7852, intel 7382 -> 6962 -- and the estimates say so beforehand
    // (-8 %, -5 %, -3 %, +7 %), so the candidates carry both forms and the model picks.
    const bool split_free = so.ml_nd && !join_env && !std::getenv("RR_PGO_ND_LEAF");
    if (split_free)
      for (int leaf : {100, 70, 50})
        if (leaf < h.g->n_nodes()) cl.push_back({leaf, np_fixed ? so.amalg_np : 16, true});
    Symbolic best;
    double best_crit = -1.0;
    // the candidates differ in where they STOP dissecting, not in how a set is split: the deepest dissection runs once (its halves on
    // threads of their own) and records its splits, every candidate replays them (symbolic.h, NdSplitTable)
    NdSplitTable splits;
    bool shared_splits = false;
    if (so.ml_nd && cl.size() > 1) {
      SymbolicOptions o = so;
      o.nd_leaf = 1 << 30;
      for (const Cand &c : cl) o.nd_leaf = std::min(o.nd_leaf, c.leaf);
      o.nd_record = &splits;
      const double td = now_ms();
      err = dissect_only(*h.g, o);
      shared_splits = err.empty();
      if (std::getenv("RR_PGO_ANALYZE_TIMES")) std::fprintf(stderr, "analyze: shared dissection down to %d nodes: %.3f ms (%zu splits)\n", o.nd_leaf, now_ms() - td, splits.map.size());
    }
    auto run = [&](const std::vector<Cand> &list) {
      std::vector<Symbolic> cands(list.size());
      std::vector<std::string> errs(list.size());
      // (one candidate per thread, never more threads than cores: host_threads.h)
      parallel_indices((int)list.size(), (int)list.size(), [&](int c) {
        SymbolicOptions o = so;
        o.nd_leaf = list[c].leaf;
        o.amalg_np = list[c].np;
        o.split_separators = list[c].split;
        if (shared_splits) o.nd_replay = &splits;
        try { errs[c] = analyze(*h.g, o, cands[c]); } catch (const std::exception &e) { errs[c] = e.what(); }
      });
      for (size_t c = 0; c < list.size(); c++) {
        if (!errs[c].empty()) { err = errs[c]; return; }
        if (std::getenv("RR_PGO_ANALYZE_TIMES"))
          std::fprintf(stderr, "analyze: nd_leaf %d, amalgamation up to %d columns, separators %s -> estimated critical path %.1f us (%d big fronts, %d supernodes)\n", list[c].leaf,
                       list[c].np, list[c].split ? "apart" : "chained", cands[c].est_critical_us, cands[c].n_big, cands[c].S);
        // a tree with a front beyond LDS below an LDS front loses the dataflow launches (one launch per level instead, and no
        // cross-level launch for its big fronts): the estimate does not see that, the measurement does (torus3D, r05: the
        // candidate with the smallest estimate ran 40 launches per iteration and 2 % slower than r04's tree)
        const double eff = cands[c].est_critical_us * (so.lds_flow && !cands[c].lds_flow ? 1.15 : 1.0);
        if (best_crit < 0 || eff < best_crit) { best_crit = eff; best = std::move(cands[c]); }
      }
    };
    if (err.empty()) run(cl);
    // fronts beyond LDS (sphere2500, torus3D: 6 x 6 blocks): there the r01 rule -- mid-sized fronts merge up to 72 columns --
    // still pays, and with another depth than the narrow rule's (torus3D): a second round of the same depths decides
    if (err.empty() && !np_fixed && best.n_big > 0) {
      cl.resize(n_depths);
      for (Cand &c : cl) c.np = 72;
      if (split_free)
        for (size_t i = 0; i < n_depths; i++)
          if (cl[i].leaf != (1 << 30)) cl.push_back({cl[i].leaf, 72, true});
      run(cl);
    }
    if (err.empty()) fresh = std::move(best);
  } else {
    err = analyze(*h.g, so, fresh);
    if (err.empty() && std::getenv("RR_PGO_ANALYZE_TIMES"))
      std::fprintf(stderr, "analyze: estimated critical path %.1f us (%d big fronts, %d supernodes)\n", fresh.est_critical_us, fresh.n_big, fresh.S);
  }
  if (!err.empty()) throw ApiError(RR_PGO_EINVAL, err);
  if (!h.symp) {
    h.symp = std::make_shared<const Symbolic>(std::move(fresh));
    if (cache_key != 0) analysis_cache_store(cache_key, *h.g, opt, h.symp);
  }
  double t1 = now_ms();
  rr_pgo_stats &s = h.stats;
  std::memset(&s, 0, sizeof s);
  const Symbolic &y = h.sym_ref();
  const double sz = opt.precision == RR_PGO_F64 ? 8.0 : 4.0;
  int64_t diag_elems = 0, off_elems = 0;
  for (int i = 0; i < y.N; i++) { int d = node_dim(h.g->node_kind[i]); diag_elems += d * d; }
  off_elems = y.n_hvals - diag_elems;
  s.nnz_h_blocks = y.N + y.n_offblocks;
  s.nnz_l_scalars = y.l_elems;
  s.factor_flops = y.factor_flops;
  s.n_supernodes = y.S;
  s.n_levels = (int)y.steps.size();
  s.max_front = y.max_front;
  s.max_pivot_cols = y.max_pivot_cols;
  s.n_big_fronts = y.n_big;
  s.analyze_ms = t1 - t0;
  s.parse_ms = parse_ms;
  s.abi_version = RR_PGO_ABI_VERSION;
  s.lds_dataflow = y.lds_flow ? 1 : 0;
  // algorithmic bytes per GN iteration, SURVEY.md 8(d): every datum moved once.  The factor is priced at its NONZEROS,
  // nnzblk(L) * d^2 scalars (Symbolic::nnz_l_entries) -- written once by the factorisation, read by the forward and by
  // the backward substitution -- not at what is stored: the supernodal panels carry padding and a front beyond LDS keeps
  // its whole M x M square in place (stored_factor_bytes; 2.2 x the nonzeros on the 1M-edge lattice)
  const double dim = y.dim;
  double edge_stream = 0;
  for (int k = 0; k < h.g->n_edges(); k++)
    edge_stream += 8.0 + sz * (edge_meas_len(h.g->edge_kind[k]) + edge_info_len(h.g->edge_kind[k]));
  s.bytes_linearize = edge_stream + dim * sz /*poses*/ + (diag_elems + off_elems) * sz + dim * sz;
  s.bytes_chi2 = 0;  // fused into the linearisation pass
  s.bytes_factor = (diag_elems + off_elems) * sz + (double)y.nnz_l_entries * sz;
  s.bytes_solve = 2.0 * (double)y.nnz_l_entries * sz + 4.0 * dim * sz;
  s.bytes_update = 3.0 * dim * sz;
  s.stored_factor_bytes = (double)y.l_elems * sz;
}

void build_engine(rr_pgo &h);
void build_handle(rr_pgo &h, const rr_pgo_options *opt_in, double parse_ms) {
  analyze_handle(h, opt_in, parse_ms);
  build_engine(h);
}

// device part of PoseGraph::new: the engine of an analysed handle, the statistics that need it
void build_engine(rr_pgo &h) {
  const rr_pgo_options opt = h.opt;
  // device
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    throw ApiError(RR_PGO_ENODEVICE, "no HIP device available (this library has no CPU fallback)");
  if (opt.device >= 0) {
    if (opt.device >= ndev) throw ApiError(RR_PGO_EINVAL, "device ordinal out of range");
    HIPCHK(hipSetDevice(opt.device));
  }
  const int wr = opt.world_size > 1 ? opt.rank : 0, ww = opt.world_size > 1 ? opt.world_size : 1;
  const bool shd = opt.sharded != 0;
  if (opt.precision == RR_PGO_F64) h.engine = std::make_unique<Engine<double>>(*h.g, h.sym_ref(), wr, ww, shd);
  else if (opt.precision == RR_PGO_F32) h.engine = std::make_unique<Engine<float>>(*h.g, h.sym_ref(), wr, ww, shd);
  else h.engine = std::make_unique<Engine<float, double>>(*h.g, h.sym_ref(), wr, ww, shd);
  // stats
  rr_pgo_stats &s = h.stats;
  const Symbolic &y = h.sym_ref();
  s.n_launches_per_iter = h.engine->n_launches_per_iter;
  // trailing updates of the huge fronts: a super-panel of w columns updates the lower triangle of the T rows to its
  // right, w * T (T + 1) / 2 multiply-adds -- counted for the launches of k_big_update and, separately, for the tiles
  // that run inside k_big_flow launches.  (The updates INSIDE a super-panel belong to the panel kernels / PANEL tasks
  // and are not counted here.)
  double buf = 0, bflow = 0;
  std::vector<char> in_flow(y.S, 0);
  h.engine->mark_flow_fronts(in_flow);
  const int sch_tile = h.engine->schur_tile();   // 0: no split (flow levels that keep their Schur tiles are marked 2 in in_flow)
  auto schur_origin_fn = [&](int nc) { return (double)big_schur_origin(nc, sch_tile); };
  const std::function<double(int)> schur_origin_of = sch_tile ? std::function<double(int)>(schur_origin_fn) : std::function<double(int)>();
  for (int f = 0; f < y.S; f++)
    if (y.sn_huge[f]) {
      const double M = y.sn_ncols[f] + y.sn_nrows[f] + 1;
      for (int k0 = 0; k0 < y.sn_ncols[f]; k0 += BIG_SUPER) {
        const double w = std::min<int>(BIG_SUPER, y.sn_ncols[f] - k0), T = M - (k0 + w);
        // with the Schur split the tiles from the Schur origin on belong to k_big_schur (a k_big_update-class launch) on every level
        const double Ts = (schur_origin_of && in_flow[f] != 2) ? std::max(0.0, M - std::max<double>(schur_origin_of(y.sn_ncols[f]), k0 + w)) : 0.0;
        buf += w * Ts * (Ts + 1);
        (in_flow[f] ? bflow : buf) += w * (T * (T + 1) - Ts * (Ts + 1));
      }
    }
  s.big_update_flops = buf;
  s.big_flow_flops = bflow;
}


// ---- rr_pgo_extend: the steps of the initial guess, from structure alone (include/rr_pgo.h).  The ready set starts as the old
// nodes; the new edges are scanned in order until a scan adds nothing.  Returns the first new node no step reaches, -1 if none.
static int plan_guess_steps(const HostGraph &g, int n_old, int e_old, std::vector<HostGuessStep> &steps, std::vector<int32_t> &tree_ptr) {
  const int N = g.n_nodes(), E = g.n_edges();
  std::vector<char> ready((size_t)N, 0);
  std::vector<int32_t> tree_of((size_t)N, -1), step_tree;
  for (int i = 0; i < n_old; i++) ready[i] = 1;
  int n_trees = 0;
  for (bool added = true; added;) {
    added = false;
    for (int k = e_old; k < E; k++) {
      const int f = g.edge_from[k], t = g.edge_to[k], ek = g.edge_kind[k];
      int src, dst, op;
      if (edge_is_br(ek)) continue;   // one scalar does not place a landmark: a bearing or range edge yields no step
      if (ready[f] && !ready[t] && t >= n_old) {
        src = f; dst = t;
        op = ek == EDGE_SE2 ? GUESS_SE2 : ek == EDGE_SE2_XY ? GUESS_XY : ek == EDGE_SE3_XYZ ? GUESS_XYZ : GUESS_SE3;
      } else if (ready[t] && !ready[f] && f >= n_old && ek != EDGE_SE2_XY && ek != EDGE_SE3_XYZ) {   // (a landmark does not determine the pose that saw it)
        src = t; dst = f;
        op = ek == EDGE_SE2 ? GUESS_SE2_INV : GUESS_SE3_INV;
      } else {
        continue;
      }
      HostGuessStep st{};
      st.src = src; st.dst = dst; st.op = op;
      const double *m = &g.edge_meas[g.edge_meas_off[k]];
      for (int q = 0; q < edge_meas_len(ek); q++) st.m[q] = m[q];
      steps.push_back(st);
      tree_of[dst] = src < n_old ? n_trees++ : tree_of[src];
      step_tree.push_back(tree_of[dst]);
      ready[dst] = 1;
      added = true;
    }
  }
  for (int i = n_old; i < N; i++)
    if (!ready[i]) return i;
  // tree by tree, list order kept within a tree: one thread of k_guess_nodes walks one tree
  std::vector<int32_t> idx(steps.size());
  for (size_t i = 0; i < idx.size(); i++) idx[i] = (int32_t)i;
  std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return step_tree[a] < step_tree[b]; });
  std::vector<HostGuessStep> sorted(steps.size());
  tree_ptr.assign((size_t)n_trees + 1, 0);
  for (size_t i = 0; i < idx.size(); i++) { sorted[i] = steps[idx[i]]; tree_ptr[step_tree[idx[i]] + 1]++; }
  for (int t = 0; t < n_trees; t++) tree_ptr[t + 1] += tree_ptr[t];
  steps.swap(sorted);
  return -1;
}

// rr_pgo_set_priors behind its checks, and rr_pgo_extend's carry: the engine takes the list, the statistics its bytes
// (the CSR pointers, and per prior the node, the robust flag, the measurement and the information: whole numbers, exact)
static double prior_bytes(const rr_pgo &h, const PriorSet &ps) {
  if (ps.n() == 0) return 0.0;
  const double sz = h.opt.precision == RR_PGO_F32 ? 4.0 : 8.0;   // the linearisation's type
  double bytes = 4.0 * (h.g->n_nodes() + 1);
  for (int p = 0; p < ps.n(); p++) {
    const int ek = prior_edge_kind(h.g->node_kind[ps.node[p]]);
    bytes += 5.0 + sz * (edge_meas_len(ek) + edge_info_len(ek));
  }
  return bytes;
}
static void apply_priors(rr_pgo &h, const PriorSet &ps) {
  const double before = prior_bytes(h, h.engine->settings().priors);
  h.engine->set_priors(ps);
  h.stats.bytes_linearize += prior_bytes(h, h.engine->settings().priors) - before;
}

// The settings of a handle's engine applied to the engine of the graph rebuilt from it (HandleSettings: the one list of what
// is carried).  origin: the old index of every edge of nh's graph, -1 for a new one.  Node indices do not change, so the
// priors and the fixed set go over as they are (new nodes are free); a setting still at its default skips its setter.
static void carry_settings(const HandleSettings &s, rr_pgo &nh, const std::vector<int32_t> &origin) {
  if (s.robust_kind != ROBUST_NONE) nh.engine->set_robust(s.robust_kind, s.robust_delta, s.robust_mu, reindex_edge_mask(s.robust_mask, origin));
  if (s.priors.n() > 0) apply_priors(nh, s.priors);   // (through the statistics: bytes_linearize)
  if (!s.fixed.empty()) nh.engine->set_fixed(s.fixed, s.fixed_keep_anchor);
  nh.engine->set_query_big_fronts(s.query_big);
  nh.engine->set_marginals_big_fronts(s.marg_big);
}

// The tail of rr_pgo_extend and rr_pgo_remove_edges: nh holds the finalized new graph and nothing else.  Its analysis and its
// engine are built completely, the first n_state nodes of the state come from `state` (device memory of h's engine, whose
// stream the caller has drained), the settings are carried, and only then the handles change sides: a throw leaves *h as it
// was.  ms (rr_pgo::extend_ms or remove_ms): analysis, engine (host wall clock), ms_dev plus the state copy (HIP events).
static void rebuild_and_swap(rr_pgo *h, std::unique_ptr<rr_pgo> nh, const std::vector<int32_t> &origin, const void *state, size_t n_state,
                             double ms_dev, double (rr_pgo::*ms)[3]) {
  const double t0 = now_ms();
  analyze_handle(*nh, &h->opt, 0.0);
  const double t1 = now_ms();
  build_engine(*nh);
  const double t2 = now_ms();
  double t = 0;
  nh->engine->adopt_state(state, n_state, &t);
  carry_settings(h->engine->settings(), *nh, origin);
  // ---- the swap: nothing below can fail.  The old engine (its stream drained by the caller, the copy out of its buffers waited
  // for) goes with nh.  Every field changes sides (the engines refer to the pointees of g and symp, which do not move).
  std::swap(*h, *nh);
  (h->*ms)[0] = t1 - t0;
  (h->*ms)[1] = t2 - t1;
  (h->*ms)[2] = ms_dev + t;
}

static void extend_handle(rr_pgo *h, int32_t n_new_nodes, const int32_t *node_kind, const uint32_t *node_id, const double *node_state,
                          int32_t n_new_edges, const int32_t *edge_kind, const int32_t *edge_from, const int32_t *edge_to,
                          const double *edge_meas, const double *edge_info) {
  const HostGraph &og = *h->g;
  const int n_old = og.n_nodes(), e_old = og.n_edges(), n_total = n_old + n_new_nodes;
  if (n_new_nodes > 0 && !node_kind) throw ApiError(RR_PGO_EINVAL, "rr_pgo_extend: null node_kind");
  if (n_new_edges > 0 && (!edge_kind || !edge_from || !edge_to || !edge_meas || !edge_info)) throw ApiError(RR_PGO_EINVAL, "rr_pgo_extend: null edge arrays");
  const bool guess = n_new_nodes > 0 && !node_state;
  // ---- the grown graph, checked completely before anything is launched
  auto nh = std::make_unique<rr_pgo>();
  HostGraph &g = *nh->g;
  g.node_kind = og.node_kind;
  g.node_id = og.node_id;
  g.node_state = og.node_state;
  g.edge_kind = og.edge_kind;
  g.edge_from = og.edge_from;
  g.edge_to = og.edge_to;
  g.edge_meas = og.edge_meas;
  g.edge_info = og.edge_info;
  std::unordered_map<uint32_t, int> ids;
  ids.reserve((size_t)n_total * 2);
  for (int i = 0; i < n_old; i++) ids.emplace(og.node_id[i], i);
  const size_t state_old = g.node_state.size();
  for (int i = 0; i < n_new_nodes; i++) {
    const int node = n_old + i;
    if (node_kind[i] < NODE_SE2 || node_kind[i] > NODE_XYZ)
      throw ApiError(RR_PGO_EINVAL, "rr_pgo_extend: new node " + std::to_string(i) + " (node " + std::to_string(node) + "): bad node kind " + std::to_string(node_kind[i]));
    const uint32_t id = node_id ? node_id[i] : (uint32_t)node;
    const auto ins = ids.emplace(id, node);
    if (!ins.second)
      throw ApiError(RR_PGO_EINVAL, "rr_pgo_extend: new node " + std::to_string(i) + " (node " + std::to_string(node) + "): id " + std::to_string(id) + " is the id of node " + std::to_string(ins.first->second));
    g.node_kind.push_back(node_kind[i]);
    g.node_id.push_back(id);
    const int len = node_state_len(node_kind[i]);
    for (int q = 0; q < len; q++) g.node_state.push_back(node_state ? *node_state++ : (q == 6 ? 1.0 : 0.0));   // (guess mode: filled in below)
  }
  for (int k = 0; k < n_new_edges; k++) {
    const std::string who = "rr_pgo_extend: new edge " + std::to_string(k) + " (edge " + std::to_string(e_old + k) + ")";
    const int ek = edge_kind[k], a = edge_from[k], b = edge_to[k];
    if (!edge_kind_known(ek)) throw ApiError(RR_PGO_EINVAL, who + ": bad edge kind " + std::to_string(ek));
    if (a < 0 || a >= n_total || b < 0 || b >= n_total) throw ApiError(RR_PGO_EINVAL, who + " references an unknown vertex");
    if (a == b) throw ApiError(RR_PGO_EINVAL, who + " is a self loop");
    const int ka = g.node_kind[a], kb = g.node_kind[b];
    if (!edge_endpoints_ok(ek, ka, kb)) throw ApiError(RR_PGO_EINVAL, who + ": endpoint kinds do not match the edge kind");
    g.edge_kind.push_back(ek);
    g.edge_from.push_back(a);
    g.edge_to.push_back(b);
    g.edge_meas.insert(g.edge_meas.end(), edge_meas, edge_meas + edge_meas_len(ek));
    g.edge_info.insert(g.edge_info.end(), edge_info, edge_info + edge_info_len(ek));
    edge_meas += edge_meas_len(ek);
    edge_info += edge_info_len(ek);
  }
  const std::string err = g.finalize();   // (what is left: mixed 2-D / 3-D)
  if (!err.empty()) throw ApiError(RR_PGO_EINVAL, "rr_pgo_extend: " + err);
  std::vector<HostGuessStep> steps;
  std::vector<int32_t> tree_ptr;
  if (guess) {
    const int lost = plan_guess_steps(g, n_old, e_old, steps, tree_ptr);
    if (lost >= 0)
      throw ApiError(RR_PGO_EINVAL, "rr_pgo_extend: new node " + std::to_string(lost - n_old) + " (node " + std::to_string(lost) +
                                        ") has no initial value: no chain of new edges determines it from a node of the graph");
  }
  // ---- from here on the device.  The old stream is drained: its last launches wrote the state that is carried.
  HIPCHK(hipStreamSynchronize(h->engine->stream()));
  double ms_dev = 0;
  // (before the analysis, which reads the positions: on the OLD engine's stream, into a staging buffer of the grown state)
  if (guess) h->engine->guess_nodes(steps, tree_ptr, n_old, n_total, g.has_se3, g.node_kind.data() + n_old, g.node_state.data() + state_old, &ms_dev);
  std::vector<int32_t> origin((size_t)g.n_edges(), -1);   // the old edges keep their indices, the new ones follow
  for (int k = 0; k < e_old; k++) origin[(size_t)k] = k;
  rebuild_and_swap(h, std::move(nh), origin, guess ? h->engine->guess_dev() : h->engine->pose_dev(), (size_t)(guess ? n_total : n_old), ms_dev,
                   &rr_pgo::extend_ms);
}

// rr_pgo_remove_edges behind its argument checks: the graph without the listed edges, then rebuild_and_swap with the surviving
// edges' old indices
static void remove_handle(rr_pgo *h, int32_t n_remove, const int32_t *edge) {
  const HostGraph &og = *h->g;
  const int N = og.n_nodes(), E = og.n_edges();
  std::vector<char> gone((size_t)E, 0);
  for (int q = 0; q < n_remove; q++) {
    if (edge[q] < 0 || edge[q] >= E)
      throw ApiError(RR_PGO_EINVAL, "rr_pgo_remove_edges: entry " + std::to_string(q) + ": edge index " + std::to_string(edge[q]) + " out of range");
    gone[edge[q]] = 1;   // a duplicate counts once
  }
  const int orphan = first_orphan_node(N, E, og.edge_from.data(), og.edge_to.data(), gone.data());
  if (orphan >= 0)
    throw ApiError(RR_PGO_EINVAL, "rr_pgo_remove_edges: node " + std::to_string(orphan) + " would be left without any edge");
  // ---- the remaining graph: edges in their order, renumbered compactly; nodes as they are
  auto nh = std::make_unique<rr_pgo>();
  HostGraph &g = *nh->g;
  const std::vector<int32_t> keep = copy_without_edges(og, gone.data(), g);
  const std::string err = g.finalize();   // (the anchor rule on what remains)
  if (!err.empty()) throw ApiError(RR_PGO_EINVAL, "rr_pgo_remove_edges: " + err);
  // ---- from here on the device.  The old stream is drained: its last launches wrote the state that is carried.
  HIPCHK(hipStreamSynchronize(h->engine->stream()));
  rebuild_and_swap(h, std::move(nh), keep, h->engine->pose_dev(), (size_t)N, 0.0, &rr_pgo::remove_ms);
}

}  // namespace

extern "C" {

int rr_pgo_extend(rr_pgo *h, int32_t n_new_nodes, const int32_t *node_kind, const uint32_t *node_id, const double *node_state,
                  int32_t n_new_edges, const int32_t *edge_kind, const int32_t *edge_from, const int32_t *edge_to,
                  const double *edge_meas, const double *edge_info) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  if (n_new_nodes < 0 || n_new_edges < 0) { g_last_error = "rr_pgo_extend: negative counts"; return RR_PGO_EINVAL; }
  if (h->opt.world_size > 1 || h->opt.sharded) {
    g_last_error = "rr_pgo_extend: sharded handle (every rank would have to grow and re-partition the same graph): create new handles on the grown graph";
    return RR_PGO_EUNSUPPORTED;
  }
  if (n_new_nodes == 0 && n_new_edges == 0) return RR_PGO_OK;
  if ((int64_t)h->g->n_nodes() + n_new_nodes > 0x7fffffffLL || (int64_t)h->g->n_edges() + n_new_edges > 0x7fffffffLL) {
    g_last_error = "rr_pgo_extend: more than 2^31 - 1 nodes or edges";
    return RR_PGO_EINVAL;
  }
  return guarded([&] { extend_handle(h, n_new_nodes, node_kind, node_id, node_state, n_new_edges, edge_kind, edge_from, edge_to, edge_meas, edge_info); });
}

int rr_pgo_extend_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  for (int i = 0; i < 3; i++) ms[i] = h->extend_ms[i];
  return RR_PGO_OK;
}

int rr_pgo_remove_edges(rr_pgo *h, int32_t n_remove, const int32_t *edge) {
  if (!h) { g_last_error = "rr_pgo_remove_edges: no handle"; return RR_PGO_EINVAL; }
  if (n_remove < 0) { g_last_error = "rr_pgo_remove_edges: n_remove < 0"; return RR_PGO_EINVAL; }
  if (n_remove > 0 && !edge) { g_last_error = "rr_pgo_remove_edges: null argument (edge is required)"; return RR_PGO_EINVAL; }
  if (h->opt.world_size > 1 || h->opt.sharded) {
    g_last_error = "rr_pgo_remove_edges: sharded handle (every rank would have to shrink and re-partition the same graph): create new handles on the remaining graph";
    return RR_PGO_EUNSUPPORTED;
  }
  if (n_remove == 0) return RR_PGO_OK;
  return guarded([&] { remove_handle(h, n_remove, edge); });
}

int rr_pgo_remove_edges_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  for (int i = 0; i < 3; i++) ms[i] = h->remove_ms[i];
  return RR_PGO_OK;
}

void rr_pgo_default_options(rr_pgo_options *opt) {
  std::memset(opt, 0, sizeof *opt);
  opt->precision = RR_PGO_F64;
  opt->device = -1;
  opt->solver = RR_PGO_GAUSS_NEWTON;
  opt->rank = 0;
  opt->world_size = 1;
}

const char *rr_pgo_last_error(void) { return g_last_error.c_str(); }

int rr_pgo_load_g2o(const char *path, const rr_pgo_options *opt, rr_pgo **out) {
  if (!path || !out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  *out = nullptr;
  return guarded([&] {
    auto h = std::make_unique<rr_pgo>();
    bool io = false;
    double t0 = now_ms();
    std::string err = load_g2o(path, *h->g, io);
    if (!err.empty()) throw ApiError(io ? RR_PGO_EIO : RR_PGO_EPARSE, err);
    build_handle(*h, opt, now_ms() - t0);
    *out = h.release();
  });
}

int rr_pgo_create(const rr_pgo_graph_desc *d, const rr_pgo_options *opt, rr_pgo **out) {
  if (!d || !out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  *out = nullptr;
  return guarded([&] {
    auto h = std::make_unique<rr_pgo>();
    HostGraph &g = *h->g;
    if (d->n_nodes < 0 || d->n_edges < 0) throw ApiError(RR_PGO_EINVAL, "negative counts");
    if (d->n_nodes > 0 && (!d->node_kind || !d->node_state)) throw ApiError(RR_PGO_EINVAL, "null node arrays");
    if (d->n_edges > 0 && (!d->edge_kind || !d->edge_from || !d->edge_to || !d->edge_meas || !d->edge_info))
      throw ApiError(RR_PGO_EINVAL, "null edge arrays");
    g.node_kind.assign(d->node_kind, d->node_kind + d->n_nodes);
    g.node_id.resize(d->n_nodes);
    for (int i = 0; i < d->n_nodes; i++) g.node_id[i] = d->node_id ? d->node_id[i] : (uint32_t)i;
    size_t ns = 0;
    for (int i = 0; i < d->n_nodes; i++) {
      if (g.node_kind[i] < NODE_SE2 || g.node_kind[i] > NODE_XYZ) throw ApiError(RR_PGO_EINVAL, "bad node kind");
      ns += node_state_len(g.node_kind[i]);
    }
    g.node_state.assign(d->node_state, d->node_state + ns);
    g.edge_kind.assign(d->edge_kind, d->edge_kind + d->n_edges);
    g.edge_from.assign(d->edge_from, d->edge_from + d->n_edges);
    g.edge_to.assign(d->edge_to, d->edge_to + d->n_edges);
    size_t nm = 0, ni = 0;
    for (int k = 0; k < d->n_edges; k++) {
      if (!edge_kind_known(g.edge_kind[k])) throw ApiError(RR_PGO_EINVAL, "bad edge kind");
      nm += edge_meas_len(g.edge_kind[k]);
      ni += edge_info_len(g.edge_kind[k]);
    }
    g.edge_meas.assign(d->edge_meas, d->edge_meas + nm);
    g.edge_info.assign(d->edge_info, d->edge_info + ni);
    std::string err = g.finalize();
    if (!err.empty()) throw ApiError(RR_PGO_EINVAL, err);
    build_handle(*h, opt, 0.0);
    *out = h.release();
  });
}

void rr_pgo_destroy(rr_pgo *h) { delete h; }

int32_t rr_pgo_num_nodes(const rr_pgo *h) { return h ? h->g->n_nodes() : 0; }
int32_t rr_pgo_num_edges(const rr_pgo *h) { return h ? h->g->n_edges() : 0; }
int32_t rr_pgo_dim(const rr_pgo *h) { return h ? h->g->dim : 0; }
int32_t rr_pgo_state_len(const rr_pgo *h) { return h ? (int32_t)h->g->node_state.size() : 0; }
int32_t rr_pgo_anchor_node(const rr_pgo *h) { return h ? h->g->anchor_node : -1; }

int rr_pgo_get_graph(const rr_pgo *h, rr_pgo_graph_desc *out) {
  if (!h || !out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  fill_desc(*h->g, out);
  return RR_PGO_OK;
}

int rr_pgo_chi2(rr_pgo *h, double *out) {
  if (!h || !out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->chi2(out); });
}

int rr_pgo_linearize_solve(rr_pgo *h, double lambda, int lm, double *dx_out) {
  if (!h || !dx_out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->linearize_solve(lambda, lm, dx_out); });
}

int rr_pgo_update(rr_pgo *h, const double *dx, double sign) {
  if (!h || !dx) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->update(dx, sign); });
}

int rr_pgo_optimize(rr_pgo *h, int32_t iters, double *errors, int32_t *n_errors, double *norms) {
  if (!h || !errors || !n_errors || iters < 0) { g_last_error = "bad argument"; return RR_PGO_EINVAL; }
  *n_errors = 0;
  return guarded([&] {
    int ne = 0;
    h->engine->optimize(h->opt.solver, iters, errors, &ne, norms);
    *n_errors = ne;
  });
}

int rr_pgo_get_state(rr_pgo *h, double *out) {
  if (!h || !out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->get_state(out); });
}

int rr_pgo_set_state(rr_pgo *h, const double *st) {
  if (!h || !st) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->set_state(st); });
}

int rr_pgo_assemble(rr_pgo *h, double lambda, int lm, int32_t *n_blocks, int32_t *brow, int32_t *bcol,
                    int64_t *boff, double *bvals, int64_t *n_vals, double *b_out) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  const Symbolic &y = h->sym_ref();
  const int64_t nb = y.N + y.n_offblocks;
  if (n_blocks) *n_blocks = (int32_t)nb;
  if (n_vals) *n_vals = y.n_hvals;
  if (!bvals) return RR_PGO_OK;
  return guarded([&] {
    std::vector<double> hv, b;
    h->engine->assemble(lambda, lm, hv, b);
    for (int i = 0; i < y.N; i++) {
      int v = y.order[i];
      if (brow) brow[i] = v;
      if (bcol) bcol[i] = v;
      if (boff) boff[i] = y.diag_off[v];
    }
    for (int64_t s = 0; s < y.n_offblocks; s++) {
      if (brow) brow[y.N + s] = y.blk_row[s];
      if (bcol) bcol[y.N + s] = y.blk_col[s];
      if (boff) boff[y.N + s] = y.blk_off[s];
    }
    std::memcpy(bvals, hv.data(), hv.size() * sizeof(double));
    if (b_out) std::memcpy(b_out, b.data(), b.size() * sizeof(double));
  });
}

int rr_pgo_set_robust_kernel(rr_pgo *h, int32_t kind, double delta, const int32_t *edge_mask) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  if (kind != RR_PGO_ROBUST_NONE && kind != RR_PGO_ROBUST_HUBER && kind != RR_PGO_ROBUST_CAUCHY) {
    g_last_error = "unknown robust kernel " + std::to_string(kind);
    return RR_PGO_EINVAL;
  }
  if (kind != RR_PGO_ROBUST_NONE && !(std::isfinite(delta) && delta > 0.0)) {
    g_last_error = "robust kernel delta must be finite and > 0";
    return RR_PGO_EINVAL;
  }
  static_assert(RR_PGO_ROBUST_HUBER == ROBUST_HUBER && RR_PGO_ROBUST_CAUCHY == ROBUST_CAUCHY, "robust kernel numbering");
  return guarded([&] { h->engine->set_robust(kind, delta, 0.0, mask_bytes(edge_mask, h->g->n_edges())); });
}

int rr_pgo_set_robust_tls(rr_pgo *h, double delta, double mu, const int32_t *edge_mask) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  if (!(std::isfinite(delta) && delta > 0.0) || !(std::isfinite(mu) && mu > 0.0)) {
    g_last_error = "rr_pgo_set_robust_tls: delta and mu must be finite and > 0";
    return RR_PGO_EINVAL;
  }
  static_assert(RR_PGO_ROBUST_TLS == ROBUST_TLS, "robust kernel numbering");
  return guarded([&] { h->engine->set_robust(ROBUST_TLS, delta, mu, mask_bytes(edge_mask, h->g->n_edges())); });
}

int rr_pgo_set_robust_mu(rr_pgo *h, double mu) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  if (!(std::isfinite(mu) && mu > 0.0)) { g_last_error = "rr_pgo_set_robust_mu: mu must be finite and > 0"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->set_robust_mu(mu); });
}

int rr_pgo_get_robust(const rr_pgo *h, int32_t *kind, double *delta, double *mu) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] {
    const HandleSettings &s = h->engine->settings();
    if (kind) *kind = s.robust_kind;
    if (delta) *delta = s.robust_delta;
    if (mu) *mu = s.robust_mu;
  });
}

void rr_pgo_default_gnc_options(rr_pgo_gnc_options *opt) {
  if (!opt) return;
  std::memset(opt, 0, sizeof(*opt));
  opt->delta = 1.0;
  opt->mu_factor = 1.4;
  opt->max_stages = 100;
  opt->inner_iterations = 1;
  opt->final_iterations = 20;
}

int rr_pgo_optimize_gnc(rr_pgo *h, const rr_pgo_gnc_options *opt, const int32_t *edge_mask, rr_pgo_gnc_result *res,
                        double *stage_mu, double *stage_cost) {
  if (!h || !opt || !res) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  bool ok = std::isfinite(opt->delta) && opt->delta > 0.0 && std::isfinite(opt->mu_factor) && opt->mu_factor > 1.0 &&
            opt->max_stages >= 1 && opt->inner_iterations >= 1 && opt->final_iterations >= 0;
  for (int32_t r : opt->reserved) ok = ok && r == 0;
  if (!ok) { g_last_error = "rr_pgo_optimize_gnc: option out of range"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->optimize_gnc(h->opt.solver, *opt, edge_mask, res, stage_mu, stage_cost); });
}

int rr_pgo_gnc_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  h->engine->gnc_times(ms);
  return RR_PGO_OK;
}

int rr_pgo_edge_errors(rr_pgo *h, double *chi2_out, double *weight_out) {
  if (!h || !chi2_out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->edge_errors(chi2_out, weight_out); });
}

int rr_pgo_solve_form(const rr_pgo *h, int32_t *kform, double *k_bytes, double *k_flops) {
  if (!h || !kform) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->solve_form(kform, k_bytes, k_flops); });
}

int rr_pgo_launch_counts(const rr_pgo *h, int64_t *out) {
  if (!h || !out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  for (int k = 0; k < 4; k++) out[k] = h->engine->launch_counts[k];
  return RR_PGO_OK;
}

// rr_pgo_marginals / rr_pgo_covariances behind their own argument rules: the offsets of the blocks, the node-range check, the
// size query (out == NULL) and the call; out_offset is written on success only
static int pair_query(rr_pgo *h, const char *who, void (EngineBase::*call)(int, const int32_t *, const int32_t *, const int64_t *, double *),
                      int32_t n_query, const int32_t *node_a, const int32_t *node_b, double *out, int64_t *out_offset, int64_t *n_vals) {
  const int N = h->g->n_nodes();
  std::vector<int64_t> off((size_t)n_query + 1, 0);
  for (int q = 0; q < n_query; q++) {
    const int va = node_a ? node_a[q] : q, vb = node_b ? node_b[q] : va;
    if (va < 0 || va >= N || vb < 0 || vb >= N) {
      g_last_error = std::string(who) + ": query " + std::to_string(q) + ": node index out of range";
      return RR_PGO_EINVAL;
    }
    off[q + 1] = off[q] + (int64_t)node_dim(h->g->node_kind[va]) * node_dim(h->g->node_kind[vb]);
  }
  if (n_vals) *n_vals = off[n_query];
  const int rc = out ? guarded([&] { (h->engine.get()->*call)(n_query, node_a, node_b, off.data(), out); }) : RR_PGO_OK;
  if (rc == RR_PGO_OK && out_offset) std::copy(off.begin(), off.end(), out_offset);
  return rc;
}

int rr_pgo_marginals(rr_pgo *h, int32_t n_query, const int32_t *node_a, const int32_t *node_b, double *out,
                     int64_t *out_offset, int64_t *n_vals) {
  if (!h || n_query < 0 || (!node_a && node_b)) { g_last_error = "bad argument"; return RR_PGO_EINVAL; }
  if (!node_a && n_query != h->g->n_nodes()) {
    g_last_error = "rr_pgo_marginals: node_a == NULL asks for every node: n_query must be rr_pgo_num_nodes";
    return RR_PGO_EINVAL;
  }
  return pair_query(h, "rr_pgo_marginals", &EngineBase::marginals, n_query, node_a, node_b, out, out_offset, n_vals);
}

int rr_pgo_marginals_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->last_query_times(EngineBase::Q_MARGINALS, ms); });
}

int rr_pgo_covariances(rr_pgo *h, int32_t n_query, const int32_t *node_a, const int32_t *node_b, double *out,
                       int64_t *out_offset, int64_t *n_vals) {
  if (!h || n_query < 0 || (n_query > 0 && (!node_a || !node_b))) { g_last_error = "rr_pgo_covariances: bad argument (node_a and node_b are both required)"; return RR_PGO_EINVAL; }
  return pair_query(h, "rr_pgo_covariances", &EngineBase::covariances, n_query, node_a, node_b, out, out_offset, n_vals);
}

int rr_pgo_covariances_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->last_query_times(EngineBase::Q_COVARIANCES, ms); });
}

int rr_pgo_cross_covariances(rr_pgo *h, int32_t n_row, const int32_t *row_node, int32_t n_col, const int32_t *col_node,
                             double *out, int64_t *row_offset, int64_t *col_offset, int64_t *n_vals) {
  static const std::string who = "rr_pgo_cross_covariances: ";
  if (!h || !n_vals) { g_last_error = who + "null argument (n_vals is required)"; return RR_PGO_EINVAL; }
  if (n_row < 0 || n_col < 0) { g_last_error = who + "negative counts"; return RR_PGO_EINVAL; }
  if (n_col > 0 && !col_node) { g_last_error = who + "col_node is required"; return RR_PGO_EINVAL; }
  const int N = h->g->n_nodes();
  if (!row_node && n_row != N) { g_last_error = who + "row_node == NULL asks for every node: n_row must be rr_pgo_num_nodes"; return RR_PGO_EINVAL; }
  std::vector<int64_t> roff((size_t)n_row + 1, 0), coff((size_t)n_col + 1, 0);
  for (int k = 0; k < n_row; k++) {
    const int v = row_node ? row_node[k] : k;
    if (v < 0 || v >= N) { g_last_error = who + "row " + std::to_string(k) + ": node index out of range"; return RR_PGO_EINVAL; }
    roff[(size_t)k + 1] = roff[k] + node_dim(h->g->node_kind[v]);
  }
  for (int k = 0; k < n_col; k++) {
    const int v = col_node[k];
    if (v < 0 || v >= N) { g_last_error = who + "column " + std::to_string(k) + ": node index out of range"; return RR_PGO_EINVAL; }
    coff[(size_t)k + 1] = coff[k] + node_dim(h->g->node_kind[v]);
  }
  const bool empty = n_col == 0 || n_row == 0;
  int rc = RR_PGO_OK;
  if (out && !empty) rc = guarded([&] { h->engine->cross_covariances(n_row, row_node, n_col, col_node, roff.data(), coff.data(), out); });
  if (rc != RR_PGO_OK) return rc;
  *n_vals = empty ? 0 : roff[n_row] * coff[n_col];
  if (row_offset) std::copy(roff.begin(), roff.end(), row_offset);
  if (col_offset) std::copy(coff.begin(), coff.end(), col_offset);
  return RR_PGO_OK;
}

int rr_pgo_cross_covariances_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->last_query_times(EngineBase::Q_CROSS, ms); });
}

// Cholesky of the d x d matrix in w (row stride ld), in place in the lower triangle; false: not positive definite
static bool small_cholesky(double *w, int d, int ld) {
  for (int c = 0; c < d; c++) {
    double v = w[c * ld + c];
    for (int k = 0; k < c; k++) v -= w[c * ld + k] * w[c * ld + k];
    if (!(v > 0.0) || !std::isfinite(v)) return false;
    const double l = std::sqrt(v);
    w[c * ld + c] = l;
    for (int r = c + 1; r < d; r++) {
      double x = w[r * ld + c];
      for (int k = 0; k < c; k++) x -= w[r * ld + k] * w[c * ld + k];
      w[r * ld + c] = x / l;
    }
  }
  return true;
}

// What rr_pgo_gate_edges and rr_pgo_gate_joint share: every check of the candidates (the message names the candidate) and
// their records -- kind, nodes, measurement, Omega and Omega^-1 -- with soff, the [n_cand + 1] offsets of d_e x d_e blocks
static int gate_candidates(const char *api, const rr_pgo *h, int32_t n_cand, const int32_t *edge_kind, const int32_t *edge_from,
                           const int32_t *edge_to, const double *edge_meas, const double *edge_info, std::vector<GateCand> &cand,
                           std::vector<int64_t> &soff, const char *what = "candidate") {
  const HostGraph &g = *h->g;
  const int N = g.n_nodes(), D = g.has_se3 ? 6 : 3;
  cand.assign((size_t)n_cand, GateCand{});
  soff.assign((size_t)n_cand + 1, 0);
  int64_t mo = 0, io = 0;
  for (int c = 0; c < n_cand; c++) {
    const std::string who = std::string(api) + ": " + what + " " + std::to_string(c) + ": ";
    auto bad = [&](const std::string &what) { g_last_error = who + what; return RR_PGO_EINVAL; };
    const int kind = edge_kind[c], a = edge_from[c], b = edge_to[c];
    if (!edge_kind_known(kind)) return bad("unknown edge kind " + std::to_string(kind));
    if (a < 0 || a >= N || b < 0 || b >= N) return bad("node index out of range");
    if (a == b) return bad("from == to");
    const int ka = g.node_kind[a], kb = g.node_kind[b];
    if (kind == EDGE_SE2 && (ka != NODE_SE2 || kb != NODE_SE2)) return bad("an SE2 edge needs two SE2 poses");
    if (kind == EDGE_SE2_XY && (ka != NODE_SE2 || kb != NODE_XY)) return bad("an SE2_XY edge goes from an SE2 pose to an XY landmark");
    if (kind == EDGE_SE3 && (ka != NODE_SE3 || kb != NODE_SE3)) return bad("an SE3 edge needs two SE3 poses");
    if (kind == EDGE_SE3_XYZ && (ka != NODE_SE3 || kb != NODE_XYZ)) return bad("an SE3_XYZ edge goes from an SE3 pose to an XYZ landmark");
    if (kind == EDGE_SE2_BEARING && (ka != NODE_SE2 || kb != NODE_XY)) return bad("an SE2_BEARING edge goes from an SE2 pose to an XY landmark");
    if (kind == EDGE_SE2_RANGE && (ka != NODE_SE2 || kb != NODE_XY)) return bad("an SE2_RANGE edge goes from an SE2 pose to an XY landmark");
    const int nm = edge_meas_len(kind), ni = edge_info_len(kind), de = edge_dim(kind);
    const double *m = edge_meas + mo, *w = edge_info + io;
    mo += nm;
    io += ni;
    for (int t = 0; t < nm; t++)
      if (!std::isfinite(m[t])) return bad("non-finite measurement");
    GateCand &gc = cand[c];
    std::memset(&gc, 0, sizeof(gc));
    gc.kind = kind;
    gc.na = a;
    gc.nb = b;
    if (kind == EDGE_SE3 && !(quat_norm(m + 3) > 0.0)) return bad("zero quaternion in the measurement");
    pack_meas(kind, m, gc.meas);
    // Omega from its packed upper triangle; Omega^-1 = L^-T L^-1 from its Cholesky factor
    double L[36] = {0}, Li[36] = {0};
    for (int i = 0, t = 0; i < de; i++)
      for (int j = i; j < de; j++, t++) {
        if (!std::isfinite(w[t])) return bad("non-finite information matrix");
        gc.info[i * D + j] = gc.info[j * D + i] = w[t];
        L[j * 6 + i] = w[t];
        L[i * 6 + j] = w[t];
      }
    if (!small_cholesky(L, de, 6)) return bad("information matrix not positive definite");
    for (int j = 0; j < de; j++)     // Li = L^-1, column by column
      for (int i = j; i < de; i++) {
        double x = i == j ? 1.0 : 0.0;
        for (int k = j; k < i; k++) x -= L[i * 6 + k] * Li[k * 6 + j];
        Li[i * 6 + j] = x / L[i * 6 + i];
      }
    for (int i = 0; i < de; i++)
      for (int j = 0; j <= i; j++) {
        double x = 0.0;
        for (int k = i; k < de; k++) x += Li[k * 6 + i] * Li[k * 6 + j];
        gc.cov[i * D + j] = gc.cov[j * D + i] = x;
      }
    soff[c + 1] = soff[c] + de * de;
  }
  return RR_PGO_OK;
}

int rr_pgo_set_priors(rr_pgo *h, int32_t n_priors, const int32_t *node, const double *meas, const double *info,
                      const int32_t *robust, int32_t keep_anchor) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  if (n_priors < 0) { g_last_error = "rr_pgo_set_priors: n_priors < 0"; return RR_PGO_EINVAL; }
  if (n_priors > 0 && (!node || !meas || !info)) { g_last_error = "rr_pgo_set_priors: null argument (node, meas and info are required)"; return RR_PGO_EINVAL; }
  if (const int rc = guarded([&] { h->engine->refuse_priors("rr_pgo_set_priors"); })) return rc;
  const HostGraph &g = *h->g;
  PriorSet ps;
  ps.keep_anchor = keep_anchor != 0 ? 1 : 0;
  for (int p = 0; p < n_priors; p++) {
    auto bad = [&](const std::string &what) { g_last_error = "rr_pgo_set_priors: prior " + std::to_string(p) + ": " + what; return RR_PGO_EINVAL; };
    if (node[p] < 0 || node[p] >= g.n_nodes()) return bad("node index out of range");
    const int ek = prior_edge_kind(g.node_kind[node[p]]), nm = edge_meas_len(ek), ni = edge_info_len(ek), de = edge_dim(ek);
    for (int t = 0; t < nm; t++)
      if (!std::isfinite(meas[t])) return bad("non-finite measurement");
    if (ek == EDGE_SE3 && !(quat_norm(meas + 3) > 0.0)) return bad("zero quaternion in the measurement");
    double L[36] = {0};
    for (int i = 0, t = 0; i < de; i++)
      for (int j = i; j < de; j++, t++) {
        if (!std::isfinite(info[t])) return bad("non-finite information matrix");
        L[j * 6 + i] = L[i * 6 + j] = info[t];
      }
    if (!small_cholesky(L, de, 6)) return bad("information matrix not positive definite");
    ps.node.push_back(node[p]);
    ps.meas.insert(ps.meas.end(), meas, meas + nm);
    ps.info.insert(ps.info.end(), info, info + ni);
    ps.robust.push_back(robust && robust[p] != 0 ? 1 : 0);
    meas += nm;
    info += ni;
  }
  return guarded([&] { apply_priors(*h, ps); });
}

int32_t rr_pgo_num_priors(const rr_pgo *h) { return h ? h->engine->settings().priors.n() : 0; }

int rr_pgo_set_fixed(rr_pgo *h, int32_t n_fixed, const int32_t *node, int32_t keep_anchor) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  if (n_fixed < 0) { g_last_error = "rr_pgo_set_fixed: n_fixed < 0"; return RR_PGO_EINVAL; }
  if (n_fixed > 0 && !node) { g_last_error = "rr_pgo_set_fixed: null argument (node is required)"; return RR_PGO_EINVAL; }
  if (const int rc = guarded([&] { h->engine->refuse_fixed("rr_pgo_set_fixed"); })) return rc;
  const int N = h->g->n_nodes();
  for (int p = 0; p < n_fixed; p++)
    if (node[p] < 0 || node[p] >= N) {
      g_last_error = "rr_pgo_set_fixed: entry " + std::to_string(p) + ": node index " + std::to_string(node[p]) + " out of range";
      return RR_PGO_EINVAL;
    }
  std::vector<int32_t> nodes(node, node + n_fixed);
  std::sort(nodes.begin(), nodes.end());
  nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());   // a node listed twice counts once
  return guarded([&] { h->engine->set_fixed(nodes, keep_anchor); });
}

int rr_pgo_set_query_big_fronts(rr_pgo *h, int32_t on) {
  if (!h) { g_last_error = "rr_pgo_set_query_big_fronts: no handle"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->set_query_big_fronts(on); });
}
int32_t rr_pgo_get_query_big_fronts(const rr_pgo *h) { return h && h->engine->settings().query_big ? 1 : 0; }

int rr_pgo_set_marginals_big_fronts(rr_pgo *h, int32_t on) {
  if (!h) { g_last_error = "rr_pgo_set_marginals_big_fronts: no handle"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->set_marginals_big_fronts(on); });
}
int32_t rr_pgo_get_marginals_big_fronts(const rr_pgo *h) { return h && h->engine->settings().marg_big ? 1 : 0; }

int rr_pgo_initialize(rr_pgo *h, int32_t method) {
  if (!h) { g_last_error = "rr_pgo_initialize: no handle"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->initialize(method); });
}

int rr_pgo_initialize_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  h->engine->initialize_times(ms);
  return RR_PGO_OK;
}

int32_t rr_pgo_num_fixed(const rr_pgo *h) { return h ? (int32_t)h->engine->settings().fixed.size() : 0; }

int rr_pgo_get_fixed(const rr_pgo *h, int32_t *out) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  const std::vector<int32_t> &f = h->engine->settings().fixed;
  if (!f.empty() && !out) { g_last_error = "rr_pgo_get_fixed: null argument (out is required)"; return RR_PGO_EINVAL; }
  if (!f.empty()) std::memcpy(out, f.data(), f.size() * sizeof(int32_t));
  return RR_PGO_OK;
}

int rr_pgo_prior_errors(rr_pgo *h, double *s_out, double *weight_out) {
  if (!h || !s_out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->prior_errors(s_out, weight_out); });
}

int rr_pgo_gate_edges(rr_pgo *h, int32_t n_cand, const int32_t *edge_kind, const int32_t *edge_from, const int32_t *edge_to,
                      const double *edge_meas, const double *edge_info, double *d2_out, double *chi2_out, double *innov_out,
                      int64_t *innov_offset) {
  if (!h || n_cand < 0) { g_last_error = "rr_pgo_gate_edges: bad argument (n_cand < 0 or no handle)"; return RR_PGO_EINVAL; }
  if (n_cand > 0 && (!edge_kind || !edge_from || !edge_to || !edge_meas || !edge_info || !d2_out)) {
    g_last_error = "rr_pgo_gate_edges: null argument (edge_kind, edge_from, edge_to, edge_meas, edge_info and d2_out are required)";
    return RR_PGO_EINVAL;
  }
  std::vector<GateCand> cand;
  std::vector<int64_t> soff;
  if (const int rc = gate_candidates("rr_pgo_gate_edges", h, n_cand, edge_kind, edge_from, edge_to, edge_meas, edge_info, cand, soff)) return rc;
  const int rc = guarded([&] { h->engine->gate_edges(n_cand, edge_from, edge_to, soff.data(), cand, d2_out, chi2_out, innov_out); });
  if (rc == RR_PGO_OK && innov_offset) std::copy(soff.begin(), soff.end(), innov_offset);
  return rc;
}

int rr_pgo_gate_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->last_query_times(EngineBase::Q_GATE, ms); });
}

static_assert(RR_PGO_GATE_JOINT_MAX_DIM == GJ_MAX_DIM && RR_PGO_GATE_JOINT_MAX_CAND == GJ_MAX_CAND, "the caps of k_gate_joint");

int rr_pgo_gate_joint(rr_pgo *h, int32_t n_cand, const int32_t *edge_kind, const int32_t *edge_from, const int32_t *edge_to,
                      const double *edge_meas, const double *edge_info, int32_t n_sets, const int32_t *set_ptr,
                      const int32_t *set_cand, double *d2_out, double *prefix_d2_out, double *innov_out, int64_t *innov_offset) {
  static constexpr const char *api = "rr_pgo_gate_joint";
  auto bad = [&](const std::string &what) { g_last_error = std::string(api) + ": " + what; return RR_PGO_EINVAL; };
  if (!h || n_cand < 0 || n_sets < 0) return bad("bad argument (n_cand < 0, n_sets < 0 or no handle)");
  std::vector<GateCand> cand, flat;
  std::vector<int64_t> soff, ioff((size_t)n_sets + 1, 0);
  std::vector<int32_t> from, to, dim((size_t)n_sets, 0);
  if (n_sets > 0) {
    if ((n_cand > 0 && (!edge_kind || !edge_from || !edge_to || !edge_meas || !edge_info)) || !set_ptr || !set_cand || !d2_out)
      return bad("null argument (edge_kind, edge_from, edge_to, edge_meas, edge_info, set_ptr, set_cand and d2_out are required)");
    if (const int rc = gate_candidates(api, h, n_cand, edge_kind, edge_from, edge_to, edge_meas, edge_info, cand, soff)) return rc;
    if (set_ptr[0] != 0) return bad("set_ptr[0] must be 0");
    for (int s = 0; s < n_sets; s++) {
      const std::string set = "set " + std::to_string(s) + ": ";
      const int64_t m = (int64_t)set_ptr[s + 1] - set_ptr[s];
      if (m < 0) return bad(set + "set_ptr decreases");
      if (m == 0) return bad(set + "empty set");
      if (m > RR_PGO_GATE_JOINT_MAX_CAND)
        return bad(set + std::to_string(m) + " candidates (at most RR_PGO_GATE_JOINT_MAX_CAND = " + std::to_string(RR_PGO_GATE_JOINT_MAX_CAND) + ")");
      for (int k = set_ptr[s]; k < set_ptr[s + 1]; k++) {
        const int c = set_cand[k];
        if (c < 0 || c >= n_cand) return bad(set + "candidate index " + std::to_string(c) + " out of range");
        dim[s] += edge_dim(cand[c].kind);
      }
      if (dim[s] > RR_PGO_GATE_JOINT_MAX_DIM)
        return bad(set + "stacked error dimension " + std::to_string(dim[s]) + " (at most RR_PGO_GATE_JOINT_MAX_DIM = " + std::to_string(RR_PGO_GATE_JOINT_MAX_DIM) + ")");
      ioff[s + 1] = ioff[s] + (int64_t)dim[s] * dim[s];
    }
    // the sets' records one after the other: the pairs (from, to) of the plan
    const size_t n = (size_t)set_ptr[n_sets];
    flat.reserve(n);
    from.reserve(n);
    to.reserve(n);
    for (size_t k = 0; k < n; k++) {
      flat.push_back(cand[set_cand[k]]);
      from.push_back(flat.back().na);
      to.push_back(flat.back().nb);
    }
  }
  const int rc = guarded([&] { h->engine->gate_joint(n_sets, set_ptr, from.data(), to.data(), dim.data(), ioff.data(), flat, d2_out, prefix_d2_out, innov_out); });
  if (rc == RR_PGO_OK && innov_offset) std::copy(ioff.begin(), ioff.end(), innov_offset);
  return rc;
}

int rr_pgo_gate_joint_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->last_query_times(EngineBase::Q_GATE_JOINT, ms); });
}

int rr_pgo_check_edges(rr_pgo *h, int32_t n_query, const int32_t *edge, double *d2_out, double *redundancy_out, double *chi2_out,
                       double *resid_out, int64_t *resid_offset) {
  static constexpr const char *api = "rr_pgo_check_edges";
  auto bad = [&](const std::string &what) { g_last_error = std::string(api) + ": " + what; return RR_PGO_EINVAL; };
  if (!h) return bad("no handle");
  if (const int rc = guarded([&] { h->engine->refuse_factor_query(api); })) return rc;
  const HostGraph &g = *h->g;
  const int E = g.n_edges();
  if (n_query < 0) return bad("n_query < 0");
  if (n_query == 0) {
    if (resid_offset) resid_offset[0] = 0;
    return RR_PGO_OK;
  }
  if (!d2_out) return bad("null argument (d2_out is required)");
  if (!edge && n_query != E) return bad("edge == NULL means every edge: n_query must be rr_pgo_num_edges = " + std::to_string(E));
  for (int q = 0; edge && q < n_query; q++)
    if (edge[q] < 0 || edge[q] >= E) return bad("query " + std::to_string(q) + ": edge index " + std::to_string(edge[q]) + " out of range");
  // ---- the queried edges as the gate's candidates, from the host copy of the graph
  std::vector<int32_t> kind((size_t)n_query), from((size_t)n_query), to((size_t)n_query);
  std::vector<double> meas, info;
  for (int q = 0; q < n_query; q++) {
    const int k = edge ? edge[q] : q, ek = g.edge_kind[k];
    kind[q] = ek;
    from[q] = g.edge_from[k];
    to[q] = g.edge_to[k];
    const double *m = &g.edge_meas[g.edge_meas_off[k]], *w = &g.edge_info[g.edge_info_off[k]];
    meas.insert(meas.end(), m, m + edge_meas_len(ek));
    info.insert(info.end(), w, w + edge_info_len(ek));
  }
  std::vector<GateCand> cand;
  std::vector<int64_t> soff;
  if (const int rc = gate_candidates(api, h, n_query, kind.data(), from.data(), to.data(), meas.data(), info.data(), cand, soff, "query")) return rc;
  const HandleSettings &rs = h->engine->settings();   // (the mask is read in place)
  for (int q = 0; q < n_query; q++)
    cand[q].pad = rs.robust_kind != ROBUST_NONE && (rs.robust_mask.empty() || rs.robust_mask[edge ? edge[q] : q]) ? 1 : 0;
  const int rc = guarded([&] { h->engine->check_edges(n_query, from.data(), to.data(), soff.data(), cand, d2_out, redundancy_out, chi2_out, resid_out); });
  if (rc == RR_PGO_OK && resid_offset) std::copy(soff.begin(), soff.end(), resid_offset);
  return rc;
}

int rr_pgo_check_edges_times(const rr_pgo *h, double *ms) {
  if (!h || !ms) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->last_query_times(EngineBase::Q_CHECK, ms); });
}

int rr_pgo_iterate_async(rr_pgo *h, int32_t iters) {
  if (!h || iters < 0) { g_last_error = "bad argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->iterate_async(iters); });
}

int rr_pgo_sync(rr_pgo *h) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->sync(); });
}

int32_t rr_pgo_abi_version(void) { return RR_PGO_ABI_VERSION; }

int rr_pgo_trim(void) {
  chunk_pool().trim();
  stream_pool().trim();
  std::lock_guard<std::mutex> lk(g_analysis_mu);
  g_analysis_cache.clear();
  return RR_PGO_OK;
}

int rr_pgo_debug_withhold(rr_pgo *h, int32_t mode) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->debug_withhold(mode); });
}

int rr_pgo_analyze_g2o(const char *path, const rr_pgo_options *opt, rr_pgo_stats *out) {
  if (!path || !out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] {
    auto h = std::make_unique<rr_pgo>();
    const double t0 = now_ms();
    bool io_error = false;
    const std::string err = load_g2o(path, *h->g, io_error);
    if (!err.empty()) throw ApiError(io_error ? RR_PGO_EIO : RR_PGO_EPARSE, err);
    analyze_handle(*h, opt, now_ms() - t0);
    *out = h->stats;
  });
}

int rr_pgo_get_stats(const rr_pgo *h, rr_pgo_stats *out) {
  if (!h || !out) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  *out = h->stats;
  return RR_PGO_OK;
}

int rr_pgo_profile(rr_pgo *h, int32_t iters, double *ms_total, int64_t *launches, int32_t n_classes) {
  if (!h || !ms_total || !launches || iters < 0 || n_classes < 0) { g_last_error = "bad argument"; return RR_PGO_EINVAL; }
  return guarded([&] {
    double ms[RR_PGO_NUM_KCLASS];
    int64_t n[RR_PGO_NUM_KCLASS];
    h->engine->profile(iters, ms, n);
    for (int k = 0; k < std::min<int>(n_classes, RR_PGO_NUM_KCLASS); k++) { ms_total[k] = ms[k]; launches[k] = n[k]; }
  });
}

int rr_pgo_synth_grid(int32_t width, int32_t height, int64_t n_edges_target, uint64_t seed_meas,
                      uint64_t seed_init, rr_pgo_synth **out, rr_pgo_graph_desc *desc) {
  if (!out || !desc || width < 2 || height < 2) { g_last_error = "bad argument"; return RR_PGO_EINVAL; }
  return guarded([&] {
    auto s = std::make_unique<rr_pgo_synth>();
    synth_grid(width, height, n_edges_target, seed_meas, seed_init, s->g);
    fill_desc(s->g, desc);
    *out = s.release();
  });
}

void rr_pgo_synth_free(rr_pgo_synth *s) { delete s; }

int rr_pgo_exchange_buffer(rr_pgo *h, int32_t which, void **dev_ptr, int64_t *n_elems, int32_t *elem_size) {
  if (!h || !dev_ptr || !n_elems || !elem_size) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->exchange_buffer(which, dev_ptr, n_elems, elem_size); });
}
int rr_pgo_set_exchange_buffer(rr_pgo *h, int32_t which, void *dev_ptr, int64_t n_elems) {
  if (!h || !dev_ptr) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->set_exchange_buffer(which, dev_ptr, n_elems); });
}
int rr_pgo_stage(rr_pgo *h, int32_t stage, double lambda, int lm) {
  if (!h) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->stage(stage, lambda, lm); });
}
int rr_pgo_stage_scalars(rr_pgo *h, double *chi2, double *norm_dx) {
  if (!h || !chi2 || !norm_dx) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  return guarded([&] { h->engine->read_last_scalars(chi2, norm_dx); });
}
#ifdef RRPGO_FLOW_TRACE
// Diagnostic build only: per supernode (parent, pivot columns, rows below, step) -- out[S][4]
extern "C" int32_t rr_pgo_debug_sn_info(rr_pgo *h, int32_t *out) {
  if (!h) return -1;
  const Symbolic &y = h->sym_ref();
  if (out) {
    std::vector<int> step_of(y.S, -1);
    for (size_t si = 0; si < y.steps.size(); si++)
      for (int t = y.steps[si].task_begin; t < y.steps[si].task_end; t++)
        for (int q = y.task_ptr[t]; q < y.task_ptr[t + 1]; q++) step_of[y.task_sn[q]] = (int)si;
    for (int s2 = 0; s2 < y.S; s2++) { out[4 * s2] = y.sn_parent[s2]; out[4 * s2 + 1] = y.sn_ncols[s2]; out[4 * s2 + 2] = y.sn_nrows[s2]; out[4 * s2 + 3] = step_of[s2]; }
  }
  return y.S;
}
// Diagnostic build only (make ../librr_pgo_trace.so): task list (4 ints per task) and stamps (4 waves x 4 per task) of a flow level
extern "C" int64_t rr_pgo_debug_flow_trace(rr_pgo *h, int32_t level, int32_t *tasks, unsigned long long *stamps, int64_t cap_tasks, int32_t *nf, double *est_us) {
  if (!h) return -1;
  int64_t n = -1;
  guarded([&] {
    std::vector<int32_t> t;
    std::vector<unsigned long long> st;
    n = h->engine->flow_trace(level, t, st, nf, est_us);
    if (n < 0 || !tasks || !stamps) return;
    const int64_t m = std::min<int64_t>(n, cap_tasks);
    std::memcpy(tasks, t.data(), (size_t)m * 4 * sizeof(int32_t));
    std::memcpy(stamps, st.data(), (size_t)m * 16 * sizeof(unsigned long long));
  });
  return n;
}
#endif
#ifdef RRPGO_STAMPS
// Diagnostic build only: the launch trace region behind the stamps (count, pad, then (tag, clock) pairs).
extern "C" int64_t rr_pgo_debug_trace(rr_pgo *h, unsigned long long *out, int64_t cap) {
  if (!h) return -1;
  int64_t n = 0;
  guarded([&] {
    std::vector<unsigned long long> st;
    h->engine->read_stamps(st);
    const size_t off = (size_t)h->sym_ref().S * 12;
    n = std::min<int64_t>(cap, (int64_t)(st.size() - off));
    for (int64_t i = 0; i < n; i++) out[i] = st[off + i];
  });
  return n;
}
// Diagnostic build only: per-supernode phase stamps of the last factorisation
// plus the supernode -> (step, task, ncols, nrows) map.  out: [S][16] doubles.
int rr_pgo_debug_stamps(rr_pgo *h, double *out, int32_t *n_sn) {
  if (!h) return RR_PGO_EINVAL;
  return guarded([&] {
    const Symbolic &y = h->sym_ref();
    *n_sn = y.S;
    if (!out) return;
    std::vector<unsigned long long> st;
    h->engine->read_stamps(st);
    std::vector<int> step_of(y.S, -1), task_of(y.S, -1);
    for (size_t si = 0; si < y.steps.size(); si++) {
      const Step &sp = y.steps[si];
      for (int t = sp.task_begin; t < sp.task_end; t++)   // (a level of fronts beyond LDS: one front per task)
        for (int q = y.task_ptr[t]; q < y.task_ptr[t + 1]; q++) { step_of[y.task_sn[q]] = (int)si; task_of[y.task_sn[q]] = t; }
    }
    for (int s = 0; s < y.S; s++) {
      double *o = out + (size_t)s * 16;
      o[0] = step_of[s]; o[1] = task_of[s]; o[2] = y.sn_ncols[s]; o[3] = y.sn_nrows[s];
      o[4] = y.child_ptr[s + 1] - y.child_ptr[s];
      for (int q = 0; q < 10; q++) o[5 + q] = (double)st[(size_t)s * 12 + q];
      o[15] = y.sn_parent[s];
    }
  });
}
// Diagnostic build only: the raw stamps ([S][12], 100 MHz ticks) + per front: parent, task (= ticket of the dataflow
// schedule), pivot columns, rows below, children.  out: [S][20] doubles.
int rr_pgo_debug_stamps12(rr_pgo *h, double *out, int32_t *n_sn) {
  if (!h) return RR_PGO_EINVAL;
  return guarded([&] {
    const Symbolic &y = h->sym_ref();
    *n_sn = y.S;
    if (!out) return;
    std::vector<unsigned long long> st;
    h->engine->read_stamps(st);
    std::vector<int> task_of(y.S, -1);
    for (size_t t = 0; t + 1 < y.task_ptr.size(); t++)
      for (int q = y.task_ptr[t]; q < y.task_ptr[t + 1]; q++) task_of[y.task_sn[q]] = (int)t;
    for (int s = 0; s < y.S; s++) {
      double *o = out + (size_t)s * 20;
      for (int q = 0; q < 12; q++) o[q] = (double)st[(size_t)s * 12 + q];
      o[12] = y.sn_parent[s]; o[13] = task_of[s]; o[14] = y.sn_ncols[s]; o[15] = y.sn_nrows[s];
      o[16] = y.child_ptr[s + 1] - y.child_ptr[s]; o[17] = y.lds_flow ? 1 : 0; o[18] = o[19] = 0;
    }
  });
}
#endif

void *rr_pgo_stream(rr_pgo *h) { return h && h->engine ? (void *)h->engine->stream() : nullptr; }

int rr_pgo_node_owner(const rr_pgo *h, int32_t *owner) {
  if (!h || !owner) { g_last_error = "null argument"; return RR_PGO_EINVAL; }
  const int ws = h->opt.world_size > 1 ? h->opt.world_size : 1;
  for (int i = 0; i < h->g->n_nodes(); i++) owner[i] = ws > 1 ? h->sym_ref().node_part[i] : 0;
  return RR_PGO_OK;
}

}  // extern "C"
