/*
 * rr_pgo.h -- C ABI of librr_pgo.so, the MI355X (gfx950) pose-graph-optimization
 * backend for RustRobotics' `robotics::mapping::PoseGraph`.
 *
 * The reference crate has no FFI seam of its own for this path;
 * the one it has one level down is russell_sparse -> UMFPACK, an opaque handle
 * with new/factorize/solve/drop returning i32 status codes
 * (reference src/mapping/pose_graph_optimization.rs:130,138,141).  This header
 * follows that model: opaque handle, plain pointers + sizes, int status.
 * Each entry point names the reference interface it replaces (file:line is
 * relative to the reference repository root).  INTEGRATION.md shows the Rust
 * `extern "C"` block + `PoseGraph` wrapper a maintainer would add.
 *
 * Threading: one handle = one caller thread at a time; handles are independent.
 * All functions return RR_PGO_OK (0) or a negative RR_PGO_E* code;
 * rr_pgo_last_error() returns the message of the calling thread's last failure.
 * Nothing here falls back to the CPU: without a HIP device every compute entry
 * point fails with RR_PGO_ENODEVICE.
 */
#ifndef RR_PGO_H
#define RR_PGO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_PGO_ABI_VERSION 4  /* see rr_pgo_abi_version() */

/* caps of one set of rr_pgo_gate_joint */
#define RR_PGO_GATE_JOINT_MAX_DIM  48   /* stacked error dimension of one set */
#define RR_PGO_GATE_JOINT_MAX_CAND 16   /* candidates of one set */

typedef struct rr_pgo rr_pgo; /* opaque: replaces `struct PoseGraph`, pose_graph_optimization.rs:155-163 */

enum {
  RR_PGO_OK = 0,
  RR_PGO_EINVAL = -1,   /* bad argument / malformed description.  Deliberate deviations from the reference, which
                         * accepts these inputs and then fails (or silently misbehaves) in the solver: a self-loop
                         * edge (from == to; the reference sums H_ii, H_ij, H_ji, H_jj into one block) and, for the
                         * loader, a repeated VERTEX id (the reference overwrites the node but keeps the first
                         * offset, leaving structurally empty rows => singular system) are rejected up front:
                         * RR_PGO_EINVAL from rr_pgo_create, RR_PGO_EPARSE from rr_pgo_load_g2o. */
  RR_PGO_EIO = -2,      /* file could not be read                         (Err(io) at g2o.rs:51) */
  RR_PGO_EPARSE = -3,   /* malformed g2o text                             (Err/panic at g2o.rs:53-139) */
  RR_PGO_ENODEVICE = -4,/* no usable HIP device / HIP runtime error */
  RR_PGO_ENOTSPD = -5,  /* factorisation hit a non-positive pivot         (Err from umfpack.factorize, :138).
                         * Like the reference (Err at :271 comes before update_nodes) the handle's state is the one
                         * before the failed iteration: the step is not applied, the caller may retry, e.g. with LM. */
  RR_PGO_ENOMEM = -6,
  RR_PGO_EUNSUPPORTED = -7,
  RR_PGO_ETIMEOUT = -8  /* a wait between workgroups of one launch (the dataflow launches k_factor_flow / k_solve_flow /
                         * k_big_flow / k_big_solve_flow hand fronts, tiles and solutions to each other) ran out of time:
                         * the launch drained without applying the step -- the handle's state is the one before the call, the
                         * handle stays usable.  No counterpart in the reference (its solver is one thread). */
};

/* enum PoseGraphSolver, pose_graph_optimization.rs:28-32 */
enum { RR_PGO_GAUSS_NEWTON = 0, RR_PGO_LEVENBERG_MARQUARDT = 1 };
/* enum Node variants, :147-154 ; enum Edge variants, :20-26 */
enum { RR_PGO_NODE_SE2 = 0, RR_PGO_NODE_XY = 1, RR_PGO_NODE_SE3 = 2, RR_PGO_NODE_XYZ = 3 };
enum { RR_PGO_EDGE_SE2 = 0, RR_PGO_EDGE_SE2_XY = 1, RR_PGO_EDGE_SE3 = 2, RR_PGO_EDGE_SE3_XYZ = 3,
       RR_PGO_EDGE_SE2_BEARING = 4, RR_PGO_EDGE_SE2_RANGE = 6 };   /* 5 and 7 are reserved: unknown kinds at every entry point */
/* 3-D point landmarks: RR_PGO_NODE_XYZ and RR_PGO_EDGE_SE3_XYZ (build-defined; the reference has none).
 *   node   state x y z, 3 scalars of the step, additive: l <- l + sign * dl, no renormalisation.
 *   edge   from an SE3 pose (t, q) to an XYZ landmark l, measurement z = x y z, information 6 values (3 x 3 upper triangle,
 *          row-major).  With p = R(q)^T (l - t), the landmark in the pose's frame, e = p - z (3 scalars): g2o's
 *          EDGE_SE3_TRACKXYZ with an identity sensor offset.  Under the library's increments (the pose's right increment
 *          X <- X (dt, Exp(dw)), the landmark's addition) the Jacobians are A = [ -I | [p]x ] and B = R(q)^T; the tests pin
 *          both to central differences in 50-digit arithmetic.
 *   graph  an XYZ node counts as 3-D: with SE2 or XY nodes the graph is "mixed 2D / 3D" and refused.  The edge is not a
 *          pose-pose edge and never sets rr_pgo_anchor_node; landmarks without any pose-pose edge leave the anchor at -1, as in 2-D.
 *   prior  on an XYZ node: the SE3_XYZ edge from the fixed identity pose, e = l - z, B = I, 3 + 6 values.
 *   fixed  an XYZ node gets an identity 3 x 3 block and b = 0; its state bits never change.
 *   extend (guess mode) l = t + R z from the edge's `from` pose only: a landmark does not determine the pose that saw it.
 *   gate / check / joint: d_e = 3.
 *   Handles in RR_PGO_F64, RR_PGO_F32 and RR_PGO_MIXED; sharded handles on a graph with an XYZ node are RR_PGO_EUNSUPPORTED.
 *   g2o text: VERTEX_TRACKXYZ id x y z; EDGE_SE3_TRACKXYZ from to param_id x y z i11 i12 i13 i22 i23 i33 (param_id: an
 *   unsigned integer, otherwise ignored); PARAMS_SE3OFFSET id x y z qx qy qz qw is accepted only as exactly 0 0 0 0 0 0 1 --
 *   any other offset is RR_PGO_EPARSE, "sensor offsets are not supported": a deliberate restriction. */
/* Bearing-only and range-only landmark edges: RR_PGO_EDGE_SE2_BEARING and RR_PGO_EDGE_SE2_RANGE (the range-bearing model of
 * the reference's src/models/measurement.rs, one measurement at a time).  Both go from an SE2 pose (t, theta) to an XY landmark
 * l; any other endpoints are RR_PGO_EINVAL, and with a 3-D node the graph is "mixed 2D / 3D".
 *   edge   1 measurement value z, 1 information value omega > 0; the error has ONE scalar.  With d = l - t, p = R(theta)^T d
 *          and rho = |d|:
 *            bearing  z in radians, e = wrap(atan2(p_y, p_x) - z) into (-pi, pi] -- evaluated without a modulo: the
 *                     measurement is kept as (cos z, sin z), as poses keep their angle, and e = atan2 of p rotated by -z;
 *                     de/dt = (d_y, -d_x) / rho^2, de/dtheta = -1, de/dl = (-d_y, d_x) / rho^2
 *            range    z >= 0 in the units of t, e = rho - z; de/dt = -d / rho, de/dtheta = 0, de/dl = d / rho
 *          under the library's additive 2-D increments (x, y, theta) and (l_x, l_y); the tests pin both Jacobians to central
 *          differences in 50-digit arithmetic.
 *   domain rho = 0 (the landmark at the pose) is outside the domain of both kinds: keeping every observed landmark away from
 *          the pose that saw it is the CALLER'S precondition; the kernels carry no guard (rho = 0 gives NaN).
 *   graph  rr_pgo_graph_desc packs 1 measurement and 1 information value per such edge.  Neither kind is a pose-pose edge:
 *          neither sets rr_pgo_anchor_node.  A bearing and a range edge between the same pair are two edges (two terms of one
 *          block); a combined kind with a correlated 2 x 2 information matrix does not exist.
 *   prior  there are no bearing or range priors: a prior stays the edge of the node's own kind.
 *   extend (guess mode) a bearing or range edge yields NO step -- one scalar does not place a landmark.  A new landmark that
 *          only such edges reach is the refusal "has no initial value" naming the node; one that also has an SE2_XY edge from
 *          a ready pose is guessed from that edge.
 *   gate / check / joint: d_e = 1, S and R are 1 x 1; the `to` node's block keeps its 2 scalars.  A call of rr_pgo_gate_edges,
 *          rr_pgo_gate_joint or rr_pgo_check_edges runs ONE kernel instantiation, chosen by the whole call: the one that knows the
 *          two kinds when the handle's graph has such an edge or the call holds such a record, the one every other call always
 *          ran otherwise.  Within an instantiation every bitwise guarantee of the three calls holds as stated (order, repeats,
 *          the rest of the list, a cut of the plan).  The one exception: on a handle WITHOUT such edges, an SE2 or SE2_XY
 *          candidate's outputs in a call that also holds a bearing or range candidate agree with its outputs in a call that
 *          holds none to rounding, not bit for bit -- two instantiations promise no common bits.  On a handle with such edges
 *          every call runs the same instantiation and there is no exception.
 *   Handles in RR_PGO_F64, RR_PGO_F32 and RR_PGO_MIXED.  RR_PGO_EUNSUPPORTED: a sharded handle on a graph with one of the
 *   kinds, and such a graph under RR_PGO_EDGE_LINEARIZE (at rr_pgo_create / rr_pgo_load_g2o / rr_pgo_extend: the
 *   edge-parallel experiment forms are not taught the kinds, as they are not taught priors or fixed nodes).
 *   g2o text: EDGE_BEARING_SE2_XY from to z omega is g2o's own tag; EDGE_RANGE_SE2_XY from to z omega is build-defined by
 *   analogy (stock g2o has no 2-D range tag).  A non-positive omega is RR_PGO_EPARSE there, RR_PGO_EINVAL from rr_pgo_create
 *   and rr_pgo_extend. */
/* arithmetic type of the device path (the reference is f64 throughout).
 * RR_PGO_MIXED: state, measurements, error / Jacobians / gradient and chi2 in f64; H, its factor and
 * the solve in f32.  The gradient is exact, so Gauss-Newton converges to the f64 minimum while the
 * factorisation (all of the cost on large graphs) runs at the f32 rate. */
enum { RR_PGO_F64 = 0, RR_PGO_F32 = 1, RR_PGO_MIXED = 2 };

/* What parse_g2o returns (g2o.rs:35-45: len, edges, lut, nodes), flattened.
 * All arrays are borrowed for the duration of the call only. */
typedef struct rr_pgo_graph_desc {
  int32_t n_nodes;
  const int32_t *node_kind;   /* [n_nodes] RR_PGO_NODE_*; scalar offsets follow this order (g2o.rs:60-77) */
  const uint32_t *node_id;    /* [n_nodes] g2o ids, may be NULL (then id = index) */
  const double *node_state;   /* packed in node order: SE2 x,y,theta | XY x,y | SE3 x,y,z,qx,qy,qz,qw | XYZ x,y,z */
  int32_t n_edges;
  const int32_t *edge_kind;   /* [n_edges] RR_PGO_EDGE_*, file order (order defines the prior, :330-336) */
  const int32_t *edge_from;   /* [n_edges] dense node index (lut/nodes lookups of :312-320 done by the caller) */
  const int32_t *edge_to;
  const double *edge_meas;    /* packed in edge order: SE2 x,y,theta | SE2_XY x,y | SE3 x,y,z,qx,qy,qz,qw | SE3_XYZ x,y,z |
                                 SE2_BEARING z | SE2_RANGE z */
  const double *edge_info;    /* packed upper triangles, row-major: 6 | 3 | 21 | 6 | 1 | 1 values (g2o.rs:82,100,117) */
} rr_pgo_graph_desc;

typedef struct rr_pgo_options {
  int32_t precision;      /* RR_PGO_F64 (default), RR_PGO_F32 or RR_PGO_MIXED */
  int32_t device;         /* HIP device ordinal, -1 = current device */
  int32_t solver;         /* RR_PGO_GAUSS_NEWTON / RR_PGO_LEVENBERG_MARQUARDT (PoseGraph::new's 2nd arg, :215) */
  /* Multi-GPU sharding of ONE graph.  world_size <= 1: single GPU; else a power of two <= 64. */
  int32_t rank, world_size;
  int32_t sharded;        /* 1: build the handle for rr_pgo_stage even with world_size <= 1 (a one-rank group: same
                           * stages, same collectives); world_size > 1 implies it */
  int32_t reserved[10];   /* zero */
} rr_pgo_options;

void rr_pgo_default_options(rr_pgo_options *opt);

/* ---- lifecycle ---------------------------------------------------------- */

/* PoseGraph::new(file_path, solver)  (:215-227) = parse_g2o (g2o.rs:35-143) +
 * upload + one-off symbolic analysis.  Same tag set and failure cases as the
 * reference loader; a panic there is RR_PGO_EPARSE here. */
int rr_pgo_load_g2o(const char *path, const rr_pgo_options *opt, rr_pgo **out);

/* PoseGraph::new for an already parsed graph (what a Rust caller holding the
 * output of its own parse_g2o passes down). */
int rr_pgo_create(const rr_pgo_graph_desc *desc, const rr_pgo_options *opt, rr_pgo **out);

/* Drop for PoseGraph */
void rr_pgo_destroy(rr_pgo *h);

/* message for the last failing call on this thread (Box<dyn Error> text) */
const char *rr_pgo_last_error(void);

/* Process-wide state the library keeps BETWEEN handles, and how to give it back (no counterpart in the reference, which
 * keeps nothing between two PoseGraphs):
 *   - device memory of destroyed handles (chunks of at most 64 MB, at most 256 MB in all), their HIP streams (at most 16)
 *     and the symbolic analysis of the last four graph structures are kept for the next handle: the reference's bench
 *     (benches/graph_slam.rs:9-10) is a loop of new + optimize(10) + drop, and hipMalloc / hipStreamCreate / the analysis
 *     cost more than its ten iterations.  RR_PGO_ANALYSIS_CACHE=0 switches the last one off.
 *   - rr_pgo_load_g2o / rr_pgo_create work on a few host threads of their own for the duration of the call (the parts of a
 *     large file, the halves of the nested dissection, the candidate elimination trees): never more than the host has
 *     cores, all joined before the call returns; a thread the host refuses is not used.
 * rr_pgo_trim() frees everything of the first kind that no live handle is using (safe at any time from any thread; the
 * next constructor pays for allocation and analysis again).  Returns RR_PGO_OK. */
int rr_pgo_trim(void);

/* ---- sizes / fields ------------------------------------------------------ */
int32_t rr_pgo_num_nodes(const rr_pgo *h);  /* nodes.len()  */
int32_t rr_pgo_num_edges(const rr_pgo *h);  /* edges.len()  */
int32_t rr_pgo_dim(const rr_pgo *h);        /* len, :156    */
int32_t rr_pgo_state_len(const rr_pgo *h);  /* entries rr_pgo_get_state writes */
int32_t rr_pgo_anchor_node(const rr_pgo *h);/* from-node of the first pose-pose edge (prior target, :330-336), -1 if none */

/* host copy of the parsed graph in rr_pgo_graph_desc packing (so a caller or a
 * test can hand the identical graph to another implementation).  Pointers stay
 * valid until rr_pgo_destroy or the next rr_pgo_extend. */
int rr_pgo_get_graph(const rr_pgo *h, rr_pgo_graph_desc *out);

/* ---- the hot path -------------------------------------------------------- */

/* global_error(graph)  (:537-574): sum_e e^T Omega e at the current state (sum_e rho(s_e) while a robust kernel is
 * set, see below).  f64 result also in f32 mode. */
int rr_pgo_chi2(rr_pgo *h, double *out);

/* build_linear_system(lambda)?.solve()?  (:271 ; linearize_and_solve :371-373
 * is lambda = 0, lm = 0).  Includes the 1e7 prior (:330-336), b = -b (:361) and,
 * when lm != 0, + lambda*I (:362-366).  dx_out: rr_pgo_dim entries, reference
 * scalar order (node offsets). */
int rr_pgo_linearize_solve(rr_pgo *h, double lambda, int lm, double *dx_out);

/* update_nodes(sign * dx)  (:229-245) */
int rr_pgo_update(rr_pgo *h, const double *dx, double sign);

/* optimize(num_iterations, log=false, plot=false)  (:247-303), exact control
 * flow incl. the LM accept/reject quirks (:275-286) and the |dx| < 1e-4 break
 * (:298-300).  errors_out needs num_iterations+1 slots; *n_errors = 1 +
 * iterations executed (the length of the reference's returned Vec<f64>).
 * norms_out (may be NULL): |dx| per executed iteration.
 * The loop runs on the device: the stop rule, Levenberg-Marquardt's accept / reject and lambda are decided by the kernel
 * that finishes an iteration, which publishes (chi2, |dx|) in host-coherent memory; the host enqueues one iteration ahead
 * and polls -- no stream synchronisation inside the call (handles of 48+ launches per iteration, i.e. graphs of tens of
 * thousands of poses, keep one host round trip per iteration: 0.5 % of theirs).  Same bits either way.
 * With log or plot the reference prints / plots BETWEEN iterations (:258-268, :288-296): a shim steps through
 * rr_pgo_linearize_solve / rr_pgo_update / rr_pgo_chi2 instead. */
int rr_pgo_optimize(rr_pgo *h, int32_t num_iterations, double *errors_out,
                    int32_t *n_errors, double *norms_out);

/* State read-back: SE2 -> x, y, atan2(im,re) ; XY -> x, y ; SE3 -> x,y,z,qx,qy,qz,qw ; XYZ -> x,y,z,
 * node order.  (Field access on PoseGraph.nodes in the reference.) */
int rr_pgo_get_state(rr_pgo *h, double *out);
/* Overwrite the state (same packing); used to restart a benchmark run.  Returns once the copy is enqueued on the handle's
 * stream (everything else the handle does is ordered behind it); setting the state of the previous call again costs a
 * comparison and one device-side copy. */
int rr_pgo_set_state(rr_pgo *h, const double *state);

/* ---- robust kernels (build-defined; the reference has none) -------------
 * s_e = e^T Omega e of edge e at the current state (the term global_error sums, :537-574).  A kernel rho with
 * parameter delta > 0 (g2o's convention: delta is in the units of sqrt(s)):
 *   RR_PGO_ROBUST_NONE    rho(s) = s, w = 1: the default, plain least squares
 *   RR_PGO_ROBUST_HUBER   rho(s) = s if s <= delta^2, else 2 delta sqrt(s) - delta^2;  w = rho'(s) = 1 or delta / sqrt(s)
 *   RR_PGO_ROBUST_CAUCHY  rho(s) = delta^2 log(1 + s / delta^2);                       w = 1 / (1 + s / delta^2)
 *   s < 0 (an indefinite Omega): rho(s) = s, w = 1.
 * IRLS as g2o does it, without the rho'' term: every robustified edge adds w J^T Omega J to H and w J^T Omega e to b,
 * w taken at the state being linearised; its term in chi2 is rho(s_e).  The anchor prior (1e7) and the LM lambda are
 * never weighted.  So while a kernel is set, rr_pgo_chi2, the errors_out of rr_pgo_optimize and the values
 * Levenberg-Marquardt compares are the robust cost sum_e rho(s_e); the stop rule |dx| < 1e-4 is unchanged.
 * The setting is per handle (a new handle starts with NONE) and holds from the next linearisation on, for every entry
 * point that linearises (rr_pgo_stage on sharded handles included).  Arithmetic in the linearisation's type: f64 in the
 * f64 and mixed modes, f32 in the f32 mode; chi2 sums in f64. */
enum { RR_PGO_ROBUST_NONE = 0, RR_PGO_ROBUST_HUBER = 1, RR_PGO_ROBUST_CAUCHY = 2 };
/* edge_mask: [n_edges], nonzero = robustified; NULL = every edge.  Copied.  EINVAL: unknown kind, delta not finite or <= 0
 * (NONE ignores delta), mask length implied by n_edges. */
int rr_pgo_set_robust_kernel(rr_pgo *h, int32_t kind, double delta, const int32_t *edge_mask);
/* s_e = e^T Omega e and w_e at the current state, file order; weight_out may be NULL.  EUNSUPPORTED on sharded handles.
 * Edges only: the priors of rr_pgo_set_priors have rr_pgo_prior_errors. */
int rr_pgo_edge_errors(rr_pgo *h, double *chi2_out, double *weight_out);

/* ---- truncated least squares and graduated non-convexity (build-defined) ----
 * A fourth kernel, with a continuation parameter mu > 0 beside delta (written c below).  With lo = mu / (mu + 1) c^2 and
 * hi = (mu + 1) / mu c^2:
 *   s <= lo  (and s < 0)   w = 1                               rho = s
 *   lo < s < hi            w = c sqrt(mu (mu + 1) / s) - mu    rho = 2 c sqrt(s mu (mu + 1)) - mu (c^2 + s)
 *   s >= hi                w = 0                               rho = c^2
 * w = rho' everywhere, w is continuous, and outside the band the weights are EXACTLY 0 and 1.  As mu grows the band closes
 * on c^2: the surrogate goes from (nearly) least squares to truncated least squares, rho = min(s, c^2) (Yang, Antonante,
 * Tzoumas, Carlone: "Graduated non-convexity for robust spatial perception", RA-L 2020).
 * Everything said above for the robust kernels holds: IRLS, the mask, flagged priors, chi2 = sum rho, the arithmetic types.
 * An edge of weight 0 adds nothing to H and b; the sparsity pattern and the analysis stay as they are.  A node whose every
 * edge has weight 0 leaves H singular there: the iteration returns RR_PGO_ENOTSPD with the state as before it.  That is the
 * caller's precondition: mask the loop closures and leave the odometry chain at weight 1 (edge_mask[k] = |from - to| > 1).
 * rr_pgo_check_edges on an edge of weight exactly 0: d2, redundancy and R are NaN (Omega_w^-1 does not exist), chi2_out
 * stays e^T Omega e, no other edge's output changes; query such an edge with rr_pgo_gate_edges as the candidate it now is.
 * RR_PGO_ROBUST_TLS is what rr_pgo_get_robust reports; rr_pgo_set_robust_kernel does NOT accept it (EINVAL, as ever), and
 * with kinds 0..2 replaces it (the constant is defined below, before the driver's structs). */
/* As rr_pgo_set_robust_kernel (mask copied, stream synchronised, captured graphs dropped); accepted on sharded handles.
 * EINVAL, before anything changes: delta or mu not finite or <= 0. */
int rr_pgo_set_robust_tls(rr_pgo *h, double delta, double mu, const int32_t *edge_mask);
/* mu alone: no mask upload, no allocation; every later launch reads the new value (captured iterations are captured anew).
 * EINVAL unless the handle's kernel is RR_PGO_ROBUST_TLS, or mu not finite or <= 0. */
int rr_pgo_set_robust_mu(rr_pgo *h, double mu);
/* The handle's kernel; any pointer may be NULL.  mu = 0 for the kinds other than TLS, delta = 1 for NONE.  Carried by
 * rr_pgo_extend and rr_pgo_remove_edges (the list under rr_pgo_extend). */
int rr_pgo_get_robust(const rr_pgo *h, int32_t *kind, double *delta, double *mu);

#define RR_PGO_ROBUST_TLS 3   /* reported by rr_pgo_get_robust; NOT accepted by rr_pgo_set_robust_kernel */
typedef struct rr_pgo_gnc_options {
  double delta;              /* c; c^2 is the caller's chi-square quantile of the edge dimension */
  double mu_factor;          /* > 1; default 1.4 */
  int32_t max_stages;        /* >= 1; default 100 */
  int32_t inner_iterations;  /* iterations of the handle's solver per stage, >= 1; default 1 */
  int32_t final_iterations;  /* closing iterations at the last mu under the stop rule, >= 0; default 20 */
  int32_t reserved[11];      /* zero */
} rr_pgo_gnc_options;
/* the defaults above; delta = 1 */
void rr_pgo_default_gnc_options(rr_pgo_gnc_options *opt);
typedef struct rr_pgo_gnc_result {
  int32_t n_stages, converged;          /* converged: 1 = a stage ended with every masked weight exactly 0 or 1 */
  int32_t n_rejected, n_fractional;     /* masked edges with w == 0 / 0 < w < 1 at the end */
  int32_t final_iterations_run;
  double mu0, mu_last, r2_max, cost_last;
} rr_pgo_gnc_result;
/* Optimise a graph that holds outliers, from the current state:
 *   1. scan: r2_max = the largest s over the masked edges, clamped at 0
 *   2. mu0 = c^2 / (2 r2_max - c^2) when 2 r2_max > c^2 (every masked weight starts inside the band or at 1), else mu0 = 1
 *      (every masked weight is exactly 1: the first stage is a plain step)
 *   3. stage t: TLS (c, mu_t, mask); inner_iterations iterations exactly as rr_pgo_optimize runs them (stop rule and
 *      Levenberg-Marquardt's decisions included; each stage is one such call); scan; stop when no masked weight is fractional
 *      or t + 1 == max_stages, else mu_{t+1} = mu_factor mu_t
 *   4. final_iterations iterations under the stop rule at the last mu, and a last scan
 *   5. the handle keeps the TLS kernel at mu_last: rr_pgo_edge_errors' weights name the rejected edges (w == 0),
 *      rr_pgo_remove_edges takes them out, every query sees the final weights.
 * edge_mask as for rr_pgo_set_robust_tls (NULL: every edge -- see the precondition above).  stage_mu / stage_cost: [max_stages],
 * may be NULL: mu_t and sum rho (over all edges, at mu_t) after stage t.  cost_last: sum rho after step 4.  A scan is one pass
 * on the device and one synchronisation; nothing per edge comes back to the host inside the loop.
 * ENOTSPD propagates as from rr_pgo_optimize, the state that of the last completed iteration, the kernel at that stage's mu
 * (res holds n_stages completed, mu0 and mu_last).  EUNSUPPORTED: sharded handles.  EINVAL, before anything changes: NULL opt
 * or res, options out of their ranges, reserved not zero. */
int rr_pgo_optimize_gnc(rr_pgo *h, const rr_pgo_gnc_options *opt, const int32_t *edge_mask, rr_pgo_gnc_result *res,
                        double *stage_mu, double *stage_cost);
/* ms[3]: HIP-event time of the last rr_pgo_optimize_gnc call's scans, stages and closing iterations */
int rr_pgo_gnc_times(const rr_pgo *h, double *ms);

/* ---- absolute priors on poses and landmarks (build-defined; the reference has only the anchor term) ----
 * A prior on node i is the edge of the node's own kind from a FIXED identity pose to node i: an SE2 pose takes an
 * RR_PGO_EDGE_SE2 term, an XY landmark an RR_PGO_EDGE_SE2_XY term, an SE3 pose an RR_PGO_EDGE_SE3 term, an XYZ landmark an
 * RR_PGO_EDGE_SE3_XYZ term, with measurement z
 * and information Omega packed exactly as an edge's are (3 | 2 | 7 | 3 and 6 | 3 | 21 | 6 values).  So e = Log(Z^-1 X_i) for poses,
 * e = l - z for landmarks, B = de/d(node) as the linearisation computes it for such an edge at the current state, and
 *   H_ii += w B^T Omega B,   b_i gets w B^T Omega e before the negation,   chi2 += rho(e^T Omega e)
 * with w and rho of the handle's robust kernel when the prior is flagged robust and a kernel is set, else w = 1, rho(s) = s.
 * Arithmetic in the linearisation's type (f64 in the f64 and mixed modes, f32 in the f32 mode); chi2 sums in f64.  The
 * Levenberg-Marquardt lambda and the anchor term are never weighted.  The sparsity pattern of H does not change.
 * rr_pgo_set_priors REPLACES the handle's whole prior list; the arrays are copied.  node: [n_priors] node indices, a node
 * may carry any number of priors (they add); meas, info: packed in prior order by the node's kind; robust: [n_priors],
 * nonzero = robustified, NULL = none.  n_priors == 0 clears the list: the handle then behaves, bit for bit, as a handle that
 * never had priors, and keep_anchor is forced back to 1.
 * keep_anchor != 0: the 1e7 term on rr_pgo_anchor_node stays; the system is the reference's plus the priors.
 * keep_anchor == 0: the anchor term is dropped from every later linearisation and the priors alone must fix the gauge.
 * That is the CALLER'S responsibility: a system the priors leave singular (no pose prior in a connected component, say)
 * ends as RR_PGO_ENOTSPD or as an ill-conditioned solve, not as an error of this call.
 * The list holds from the next linearisation on, for every entry point that linearises: rr_pgo_chi2,
 * rr_pgo_linearize_solve, rr_pgo_optimize, rr_pgo_iterate_async, rr_pgo_assemble, rr_pgo_profile, and the four factor
 * queries below.  The state, the Levenberg-Marquardt lambda and the robust setting are untouched; captured graphs are
 * dropped, as by rr_pgo_set_robust_kernel.  On RR_PGO_F32 / RR_PGO_MIXED handles whose Gauss-Newton steps use the gauge
 * transfer (a big root front), that transfer is off while the list is non-empty: the system is then the one described here.
 * Carried by rr_pgo_extend and rr_pgo_remove_edges (the list under rr_pgo_extend).
 * RR_PGO_EINVAL, decided before anything changes, the message names the prior: n_priors < 0, a null required pointer, a
 * node out of range, a non-finite value, Omega not positive definite, an SE3 measurement whose quaternion has zero norm.
 * RR_PGO_EUNSUPPORTED (the message says which): sharded handles; handles created under RR_PGO_EDGE_LINEARIZE=1 or =2 (the
 * measured-alternative linearisation forms are not taught the priors). */
int rr_pgo_set_priors(rr_pgo *h, int32_t n_priors, const int32_t *node, const double *meas, const double *info,
                      const int32_t *robust /* may be NULL: none */, int32_t keep_anchor);
int32_t rr_pgo_num_priors(const rr_pgo *h);
/* s_p = e^T Omega e and w_p of every prior at the current state, in the order of the rr_pgo_set_priors call; weight_out may
 * be NULL.  The counterpart of rr_pgo_edge_errors, which stays edges-only.  EUNSUPPORTED as for rr_pgo_set_priors. */
int rr_pgo_prior_errors(rr_pgo *h, double *s_out, double *weight_out /* may be NULL */);

/* ---- fixed nodes (build-defined; what g2o's setFixed and GTSAM's constrained keys do) ----
 * A fixed node is held constant EXACTLY: its dx is exactly zero, its state bits never change, and every covariance and gate
 * is conditional on it.  (A prior with a huge Omega is a soft constraint: the node still moves by b / Omega, and its
 * Sigma is Omega^-1, not 0.)  With F the set of fixed nodes, every entry point that linearises builds this system:
 *   fixed node i in F:   H_ii = I exactly -- no lambda, no 1e7, no prior terms, no edge terms --, b_i = 0;
 *   an edge with at least one endpoint in F:   its off-diagonal block(s) are exactly zero;
 *   free node j:   H_jj and b_j are what they are without the set, bit for bit, including the full w A^T Omega A,
 *                  w A^T Omega e contribution of edges whose other end is fixed (what eliminating dx_i = 0 leaves behind);
 *   chi2 is unchanged: every edge and every prior counts, fixed-fixed edges included (a constant); priors on a fixed node
 *                  still count in chi2 and in rr_pgo_prior_errors and add nothing to H or b.
 * The sparsity pattern of H, the analysis and the factorisation do not change: the factor has the same size, the fixed
 * columns are unit columns, and the solves give dx_i = 0 there.
 * rr_pgo_set_fixed REPLACES the whole set; node: [n_fixed] node indices, copied; a node listed twice counts once.
 * n_fixed == 0 clears the set: the handle then behaves, bit for bit, as one that never had fixed nodes (the same kernels,
 * the same launch counts), and keep_anchor is forced back to 1.
 * keep_anchor: as for rr_pgo_set_priors.  The 1e7 term on rr_pgo_anchor_node is applied only while BOTH settings say keep;
 * if the anchor node itself is fixed its row is the identity row and the term is moot.  With keep_anchor == 0 the fixed set
 * (plus any priors) must fix the gauge of every connected component: the CALLER'S responsibility; a singular system ends
 * as RR_PGO_ENOTSPD.
 * The set holds from the next linearisation on.  Untouched: the state, the Levenberg-Marquardt lambda, the robust
 * setting, the prior list.  Captured graphs are dropped, as by rr_pgo_set_priors.  On RR_PGO_F32 / RR_PGO_MIXED handles the
 * gauge transfer is off while the set is non-empty.
 * rr_pgo_update ignores its dx entries for fixed nodes and does not move them -- the update inside every iteration and
 * Levenberg-Marquardt's undo included --, fixed nodes add nothing to |dx|, and rr_pgo_linearize_solve writes 0.0 for them.
 * rr_pgo_set_state still overwrites every node: that is how a fixed node is moved.
 * rr_pgo_marginals, rr_pgo_covariances, rr_pgo_gate_edges, rr_pgo_gate_joint: Sigma is the covariance conditional on the
 * fixed nodes, (H_ff)^-1 on the free nodes; every block with a fixed node in it, its own diagonal block included, is
 * returned as zeros; a gate candidate with a fixed endpoint a gets S = Omega^-1 + B Sigma_bb B^T, one with both S = Omega^-1.
 * Carried by rr_pgo_extend and rr_pgo_remove_edges (the list under rr_pgo_extend).
 * RR_PGO_EINVAL, decided before anything changes, the message names the entry: n_fixed < 0, null node with n_fixed > 0, a
 * node out of range.  RR_PGO_EUNSUPPORTED (the message says which): sharded handles; handles created under
 * RR_PGO_EDGE_LINEARIZE=1 or =2. */
int rr_pgo_set_fixed(rr_pgo *h, int32_t n_fixed, const int32_t *node, int32_t keep_anchor);
int32_t rr_pgo_num_fixed(const rr_pgo *h);           /* distinct fixed nodes */
int rr_pgo_get_fixed(const rr_pgo *h, int32_t *out); /* ascending node indices, rr_pgo_num_fixed entries */

/* ---- initialisation from the measurements (build-defined; the reference has none) ----------
 * rr_pgo_initialize(h, RR_PGO_INIT_CHORDAL) replaces the state of every free node by the chordal relaxation of the graph
 * (Carlone, Tron, Daniilidis, Dellaert, ICRA 2015): linear least squares for the rotations, a projection onto SO(d),
 * linear least squares for the positions.  It reads the graph, the prior list and the HELD nodes' states, nothing else of
 * the current state.  Every edge takes full weight: the robust kernel, its mask and the TLS weights play no part.
 * HELD nodes are the fixed nodes (rr_pgo_set_fixed) and, while BOTH keep_anchor settings say keep, rr_pgo_anchor_node.
 * They are constants taken from the current state -- held exactly, not by the 1e7 term -- and their state bits do not change.
 * With Omega an edge's or prior's information, translation first; Omega_tt its upper-left d x d block, Omega_rot the rest:
 *   SE(3)  1. over M_i in R^(3x3), i a free pose, M_c = R_c for a held pose c:
 *               min  sum_{SE3 edges (i,j)} k_ij |M_i R_ij - M_j|_F^2  +  sum_{priors p on pose i} k_p |M_i - R_zp|_F^2 ,
 *               k = trace(Omega_rot) / 3
 *          2. R_i = U diag(1, 1, det(U V^T)) V^T  of  M_i = U S V^T  (the nearest rotation in the Frobenius norm)
 *          3. over t_i (free poses) and l (free XYZ landmarks), with |v|^2_W = v^T W v and the R_i of step 2 or the held ones:
 *               min  sum_{SE3 edges} |R_i^T (t_j - t_i) - t_ij|^2_Omega_tt  +  sum_{SE3_XYZ edges} |R_i^T (l_j - t_i) - z|^2_Omega
 *                  + sum_{pose priors} |R_z^T (t_i - t_z)|^2_Omega_tt       +  sum_{landmark priors} |l - z|^2_Omega
 *             (the translation-rotation cross block of Omega is ignored)
 *   SE(2)  the same scheme with u_i = (cos, sin) in R^2: min sum k |Rot(theta_ij) u_i - u_j|^2 + sum k_p |u_i - u_zp|^2,
 *          k = Omega_theta,theta; the projection is u / |u|; positions as above with the 2 x 2 Omega_tt, SE2_XY edges and
 *          XY-landmark priors.  SE2_BEARING and SE2_RANGE edges take no part (one scalar places nothing).
 * A free pose gets (t, R) -- SE(3): a unit quaternion with q_w >= 0 --, a free landmark its position.  All three precisions;
 * RR_PGO_F32 / RR_PGO_MIXED solve with the single-precision factor, without the gauge transfer.
 * Untouched: the robust setting, the prior list, the fixed set, the Levenberg-Marquardt lambda, the solver, captured graphs
 * and the two big-front switches (rr_pgo_set_query_big_fronts, rr_pgo_set_marginals_big_fronts).
 * Failures; after each of them the state is what it was before the call, bit for bit:
 *   RR_PGO_EINVAL        unknown method; a free landmark with no SE2_XY / SE3_XYZ edge and no prior (the message names it)
 *   RR_PGO_EUNSUPPORTED  sharded handles
 *   RR_PGO_ENOTSPD       a stage's system is singular: a set of poses connected by pose-pose edges with no held pose and
 *                        no pose prior (decided before anything runs), or a non-positive pivot in a stage's factorisation
 *   device errors and RR_PGO_ETIMEOUT propagate as from rr_pgo_optimize
 * The call synchronises with the device once per stage. */
enum { RR_PGO_INIT_CHORDAL = 0 };
int rr_pgo_initialize(rr_pgo *h, int32_t method);
/* ms[3]: HIP-event time of the last call's rotation stage(s) incl. projection, position stage, and the whole call */
int rr_pgo_initialize_times(const rr_pgo *h, double *ms);

/* ---- marginal covariances (build-defined; the reference has none) ----------
 * Blocks of Sigma = H^-1 at the current state (H as rr_pgo_linearize_solve(h, 0, 0) builds it: anchor prior 1e7 included,
 * lambda = 0, robust weights included while a kernel is set; with a prior list, rr_pgo_set_priors, H is the one with the
 * priors, and without the anchor term under keep_anchor == 0).
 * Query q asks for block (node_a[q], node_b[q]): d_a x d_b, row-major, tangent coordinates in the order
 * rr_pgo_linearize_solve's dx uses for the node.  node_b == NULL: diagonal blocks of node_a.
 * node_a == NULL too: n_query must be rr_pgo_num_nodes, all diagonal blocks in node order.
 * out_offset (may be NULL): [n_query + 1] offsets into out.  Call with out == NULL to get *n_vals (and the offsets).
 * A pair a != b is answered when both nodes lie in one front of the factor -- guaranteed for every pair joined by an edge;
 * any other pair is RR_PGO_EINVAL (the message names it) and nothing is written.  Out-of-range node: RR_PGO_EINVAL.
 * The call linearises, factors, runs the selected inverse (the Takahashi recursion over the supernode tree) and gathers on
 * the handle's stream, then synchronises; the state, the Levenberg-Marquardt lambda and rr_pgo_optimize's results are
 * untouched.  A non-positive pivot: RR_PGO_ENOTSPD.
 * RR_PGO_EUNSUPPORTED (the message says which): sharded handles, RR_PGO_F32 / RR_PGO_MIXED handles, graphs with fronts
 * beyond LDS (rr_pgo_stats::n_big_fronts != 0; there the message points to rr_pgo_covariances with
 * rr_pgo_set_query_big_fronts) unless rr_pgo_set_marginals_big_fronts, below, is on: then every sentence above holds on
 * such graphs too.  RR_PGO_ENOMEM (only with that switch, on the first call): the device has no room for the selected
 * inverse or the workspace of the fronts beyond LDS; the message holds the bytes, the handle stays usable. */
int rr_pgo_marginals(rr_pgo *h, int32_t n_query, const int32_t *node_a, const int32_t *node_b,
                     double *out, int64_t *out_offset, int64_t *n_vals);
/* ms[3]: HIP-event times of the last rr_pgo_marginals call -- linearise + factor, selected inverse, gather. */
int rr_pgo_marginals_times(const rr_pgo *h, double *ms);
/* Let rr_pgo_marginals answer on graphs with fronts beyond LDS.  Default 0: such graphs are refused as before, same code,
 * same message (a test of the earlier interface pins it), so the capability is asked for per handle.  With the switch on, a
 * front beyond LDS keeps its part of the selected inverse in device memory and is inverted by kernels of its own
 * (DESIGN.md 4s): one launch ahead of the tree's levels and up to three more per level that holds such a front; the
 * results do not depend on the schedule, so two calls at one state give the same bits.  On a handle without such fronts
 * the switch changes no bit and no launch.  The setter is RR_PGO_OK on every handle (RR_PGO_EINVAL: no handle); sharded and
 * RR_PGO_F32 / RR_PGO_MIXED handles keep their own refusals, which are checked first.  Independent of
 * rr_pgo_set_query_big_fronts: neither call reads the other's switch.  rr_pgo_extend and rr_pgo_remove_edges carry it. */
int rr_pgo_set_marginals_big_fronts(rr_pgo *h, int32_t on);
int32_t rr_pgo_get_marginals_big_fronts(const rr_pgo *h);   /* 0 or 1; 0 without a handle */

/* Covariance blocks of ARBITRARY node pairs: block q is Sigma(node_a[q], node_b[q]), d_a x d_b row-major, for any two
 * valid nodes -- joined by an edge or far apart in the elimination tree (a == b: the node's diagonal block).  Same H (the
 * one with the priors of rr_pgo_set_priors when the handle has any), same
 * coordinates, same out / out_offset / n_vals conventions as rr_pgo_marginals (out == NULL: size query; out_offset may
 * be NULL), with these differences: node_a and node_b are both required; every pair is answered; a node may appear in
 * any number of queries.
 * Computed as Sigma_ab = Z_a^T Z_b with Z_s = L^-1 E_s, a multi-column forward solve over the fronts between the queried
 * nodes and the root: Sigma(b, a) is the transpose of Sigma(a, b) bit for bit, diagonal blocks are symmetric bit for bit,
 * and a block's bits do not depend on what else the call asks for.  Cost grows with the number of DISTINCT nodes (32
 * columns per pass over their root paths); for all diagonal blocks or edge pairs rr_pgo_marginals is the cheaper call.
 * The call linearises, factors, solves and gathers on the handle's stream, then synchronises; the state, the
 * Levenberg-Marquardt lambda, rr_pgo_optimize's results and captured graphs are untouched.
 * RR_PGO_EINVAL: an out-of-range node or n_query < 0 (nothing is written).  RR_PGO_ENOTSPD: a non-positive pivot.
 * RR_PGO_EUNSUPPORTED (the message says which): sharded handles, RR_PGO_F32 / RR_PGO_MIXED handles, graphs with fronts
 * beyond LDS unless rr_pgo_set_query_big_fronts (rr_pgo_stats::n_big_fronts != 0). */
int rr_pgo_covariances(rr_pgo *h, int32_t n_query, const int32_t *node_a, const int32_t *node_b,
                       double *out, int64_t *out_offset, int64_t *n_vals);
/* ms[3]: HIP-event times of the last rr_pgo_covariances call -- linearise + factor, tree solve, products + gather. */
int rr_pgo_covariances_times(const rr_pgo *h, double *ms);

/* The rectangular block Sigma[rows, cols]: rows = the scalars of row_node[0 .. n_row) stacked in that order, cols = the
 * scalars of col_node[0 .. n_col) likewise, each node's scalars in the order rr_pgo_linearize_solve's dx uses.
 * out: R x C doubles, row-major, R = sum of the row nodes' dims, C = sum of the column nodes' dims.
 * row_node == NULL: n_row must be rr_pgo_num_nodes; the rows are all nodes in node order, i.e. R = rr_pgo_dim and
 * row i is scalar i of dx -- the block columns Sigma[:, col_node], what a search for the nodes within a pose's
 * uncertainty starts from.  Same H as rr_pgo_covariances (current state, lambda = 0, robust weights while a kernel is set,
 * the priors of rr_pgo_set_priors, the anchor term only while both keep_anchor settings say keep).
 * row_offset [n_row + 1], col_offset [n_col + 1] (either may be NULL): the first row / column of every node in out.  Call
 * with out == NULL to get *n_vals = R * C (and the offsets).  n_vals is required.  A node may appear any number of times in
 * either list: repeated rows and columns are copies, same bits.  n_col == 0, or n_row == 0 with a non-NULL row_node:
 * RR_PGO_OK, nothing is launched, *n_vals = 0.
 * Computed as X = L^-T (L^-1 E_cols): the forward solve of rr_pgo_covariances over the root paths of the column nodes,
 * then a backward sweep over the union of the root paths of the row nodes (every front for row_node == NULL), one launch
 * per level of the tree each way.  The bits of block (r, c) depend on the graph, the state, r and c alone -- not on the
 * other rows or columns of the call, their order, repeats, or a cut of the list.  Sigma(r, c) and the transpose of
 * Sigma(c, r) agree to rounding, NOT bit for bit, and a block agrees with rr_pgo_covariances -- which stays the
 * bit-symmetric call -- to rounding.
 * Fixed nodes (rr_pgo_set_fixed): every entry in a fixed node's rows or columns is +0.0; the rest is (H_ff)^-1.
 * The call linearises, factors, solves forward and backward and gathers on the handle's stream, then synchronises once;
 * the state, the Levenberg-Marquardt lambda, rr_pgo_optimize's results, captured graphs and the robust setting are untouched.
 * RR_PGO_EINVAL, decided before anything is launched or written, the message names the entry: negative counts, col_node ==
 * NULL with n_col > 0, row_node == NULL with n_row != rr_pgo_num_nodes, a node out of range, n_vals == NULL.
 * RR_PGO_ENOTSPD: a non-positive pivot, nothing is written.  RR_PGO_EUNSUPPORTED: the cases and messages of
 * rr_pgo_covariances (graphs with fronts beyond LDS unless rr_pgo_set_query_big_fronts).  RR_PGO_ENOMEM: one column node alone needs more workspace (forward and backward blocks of its pass)
 * than the handle's bound, the message gives the bytes; a longer list is cut between column nodes, never between rows, and
 * the cut changes no bit. */
int rr_pgo_cross_covariances(rr_pgo *h, int32_t n_row, const int32_t *row_node, int32_t n_col, const int32_t *col_node,
                             double *out, int64_t *row_offset /* [n_row + 1], may be NULL */,
                             int64_t *col_offset /* [n_col + 1], may be NULL */, int64_t *n_vals /* R * C */);
/* ms[3]: HIP-event times of the last rr_pgo_cross_covariances call -- linearise + factor, forward + backward solve,
 * gather + copy. */
int rr_pgo_cross_covariances_times(const rr_pgo *h, double *ms);

/* ---- Mahalanobis gate of candidate loop closures (build-defined; the reference has none) ----
 * For candidate c -- an edge of kind edge_kind[c] from node edge_from[c] to node edge_to[c] with measurement z and
 * information Omega, in rr_pgo_graph_desc packing (measurements and packed upper triangles follow each other in candidate
 * order) -- that is NOT part of the graph:
 *   e, A = de/d(from), B = de/d(to)   what the linearisation computes for such an edge at the current state (dx's coordinates)
 *   S = Omega^-1 + [A B] Sigma_{ab,ab} [A B]^T     the innovation covariance; Sigma = H^-1, H as for rr_pgo_covariances
 *                                                  (with the priors of rr_pgo_set_priors when the handle has any)
 *   d2_out[c] = e^T S^-1 e                         compare with a chi-square quantile of d_e = 3 / 2 / 6 degrees of freedom
 *   chi2_out[c] = e^T Omega e                      the term the edge would add to rr_pgo_chi2 (may be NULL)
 *   innov_out (may be NULL): S per candidate, d_e x d_e row-major, packed; innov_offset (may be NULL): [n_cand + 1] offsets.
 * [A B] Sigma [A B]^T is formed as G^T G with G = Z_a A^T + Z_b B^T, Z_s = L^-1 E_s of rr_pgo_covariances: the blocks of
 * Sigma of two poses that move together cancel to many digits, and here they cancel row by row before the square.  S is
 * symmetric bit for bit and positive definite; a candidate's bits do not depend on what else the call asks for.
 * One linearisation, one factorisation and one tree solve per call on the handle's stream, then one synchronisation; the
 * state, the Levenberg-Marquardt lambda, rr_pgo_optimize's results, captured graphs and the robust setting are untouched.
 * RR_PGO_EINVAL, decided before anything is launched or written, the message names the candidate: n_cand < 0, a null
 * required pointer, a node out of range, from == to, an unknown kind, a kind that does not fit its nodes (SE2: two SE2
 * poses; SE2_XY: from an SE2 pose to an XY landmark; SE3: two SE3 poses; SE3_XYZ: from an SE3 pose to an XYZ landmark), Omega not positive definite, a non-finite
 * measurement.  n_cand == 0: RR_PGO_OK.  RR_PGO_ENOTSPD: a non-positive pivot of H.
 * RR_PGO_EUNSUPPORTED (the message says which): sharded handles, RR_PGO_F32 / RR_PGO_MIXED handles, graphs with fronts
 * beyond LDS unless rr_pgo_set_query_big_fronts (rr_pgo_stats::n_big_fronts != 0). */
int rr_pgo_gate_edges(rr_pgo *h, int32_t n_cand,
                      const int32_t *edge_kind, const int32_t *edge_from, const int32_t *edge_to,
                      const double *edge_meas, const double *edge_info,
                      double *d2_out, double *chi2_out, double *innov_out, int64_t *innov_offset);
/* ms[3]: HIP-event times of the last rr_pgo_gate_edges call -- linearise + factor, tree solve, gate kernel + copy. */
int rr_pgo_gate_times(const rr_pgo *h, double *ms);

/* Joint compatibility of SETS of candidates: set s is the ordered list set_cand[set_ptr[s] .. set_ptr[s + 1]) of indices
 * into the n_cand candidates (given as for rr_pgo_gate_edges); a candidate may appear in any number of sets, and twice in
 * one (two independent measurements).  With e_s the stacked errors of the set (D_s = the sum of its d_e) and
 * G_s = [G_c1 .. G_cm], G_c = Z_a A_c^T + Z_b B_c^T as for rr_pgo_gate_edges (the same H: with the priors of
 * rr_pgo_set_priors when the handle has any):
 *   S_s = blockdiag(Omega_c^-1) + G_s^T G_s        the joint innovation covariance: the cross block of candidates c and d is
 *                                                  G_c^T G_d, summed over the pivot rows their root paths share
 *   d2_out[s] = e_s^T S_s^-1 e_s                   compare with a chi-square quantile of D_s degrees of freedom
 *   prefix_d2_out[set_ptr[s] + k] (may be NULL)    with S_s = L L^T, y = L^-1 e_s: the sum of y^2 over the rows of the set's
 *                                                  first k + 1 candidates = the joint distance of the set cut after candidate
 *                                                  k (the increment a branch-and-bound search asks for at each depth); the
 *                                                  last one of a set is d2_out[s], same bits
 *   innov_out (may be NULL): S_s, D_s x D_s row-major, sets packed; innov_offset (may be NULL): [n_sets + 1] offsets.
 * S_s is symmetric bit for bit; the bits of its block (c, d) depend on the two candidates alone -- not on the rest of the
 * set, on its order or on the other sets -- and a prefix equals d2_out of the truncated set bit for bit.  A one-candidate
 * set agrees with rr_pgo_gate_edges to rounding (the sums run in another order), not bit for bit.  A non-positive pivot of
 * S_s (rounding only) gives NaN for the set's d2 and for its prefixes from that candidate on.
 * One linearisation, one factorisation and one tree solve per call, then one synchronisation; the state, the
 * Levenberg-Marquardt lambda, rr_pgo_optimize's results, captured graphs and the robust setting are untouched.
 * RR_PGO_EINVAL, decided before anything is launched or written, the message names the candidate or the set: every case
 * of rr_pgo_gate_edges, n_sets < 0, a null required pointer (with n_sets > 0: the candidate arrays, set_ptr, set_cand,
 * d2_out), set_ptr[0] != 0 or set_ptr decreasing, an empty set, a set_cand out of range, more than
 * RR_PGO_GATE_JOINT_MAX_CAND candidates in a set, D_s > RR_PGO_GATE_JOINT_MAX_DIM.  n_sets == 0: RR_PGO_OK, nothing is read.
 * RR_PGO_ENOTSPD and RR_PGO_EUNSUPPORTED as for rr_pgo_gate_edges (graphs with fronts beyond LDS unless
 * rr_pgo_set_query_big_fronts).  RR_PGO_ENOMEM: one set alone needs more workspace than
 * the handle's bound (the message gives the bytes); longer lists are cut at set boundaries, which changes no bit. */
int rr_pgo_gate_joint(rr_pgo *h, int32_t n_cand,
                      const int32_t *edge_kind, const int32_t *edge_from, const int32_t *edge_to,
                      const double *edge_meas, const double *edge_info,
                      int32_t n_sets, const int32_t *set_ptr, const int32_t *set_cand,
                      double *d2_out, double *prefix_d2_out, double *innov_out, int64_t *innov_offset);
/* ms[3]: HIP-event times of the last rr_pgo_gate_joint call -- linearise + factor, tree solve, joint kernel + copy. */
int rr_pgo_gate_joint_times(const rr_pgo *h, double *ms);

/* ---- audit of the edges that ARE in the graph (build-defined; the reference has none) --------
 * For queried edge edge[q] (edge == NULL: every edge in order, n_query must be rr_pgo_num_edges; an edge may be listed any
 * number of times), joining nodes a and b, with e, A, B as for rr_pgo_gate_edges at the current state:
 *   Omega_w = w Omega                              w: the weight the handle's robust kernel gives the edge at this state (1
 *                                                  without a kernel or for an unmasked edge); what the edge contributed to H
 *   P = [A B] Sigma_{ab,ab} [A B]^T                formed as G^T G exactly as for rr_pgo_gate_edges; Sigma = H^-1, H as for
 *                                                  rr_pgo_covariances (robust weights, priors, fixed nodes, the anchor term
 *                                                  while both keep_anchor settings say keep)
 *   R = Omega_w^-1 - P                             the covariance of the edge's residual
 *   d2_out[q] = e^T R^-1 e                         the leave-one-out distance: to first order the d2 that rr_pgo_gate_edges gives
 *                                                  the edge as a candidate for the graph without it, at that graph's optimum
 *                                                  (Woodbury: S_without = Omega_w^-1 R^-1 Omega_w^-1).  Compare with a
 *                                                  chi-square quantile of d_e degrees of freedom.
 *   redundancy_out[q] = trace(R Omega_w) / d_e     (may be NULL) in [0, 1].  1: the rest of the graph determines the residual
 *                                                  completely.  0: a bridge -- an odometry edge on no loop, a landmark seen
 *                                                  once -- nothing else constrains the edge, R is zero up to rounding and d2
 *                                                  carries no information: read the redundancy before d2.
 *   chi2_out[q] = e^T Omega e                      (may be NULL) unweighted, as rr_pgo_edge_errors
 *   resid_out (may be NULL): R per query, d_e x d_e row-major, packed; resid_offset (may be NULL): [n_query + 1] offsets.
 * PARTIAL redundancy.  The redundancy is the MEAN of the eigenvalues of R Omega_w, which lie in [0, 1] one per direction of the
 * residual, and the rest of the graph may determine some directions only: a pose-landmark graph in which nothing but this edge
 * fixes a pose's heading has edges at redundancy 0.05 .. 0.4 whose R is singular to rounding in one direction.  d2 of such an
 * edge carries no information either -- NaN, or 1e13 and up, rounding decides -- and removing it would leave that direction
 * unconstrained.  redundancy_out alone does not show this; resid_out does: take the smallest eigenvalue of
 * Omega^1/2 R Omega^1/2 against the largest (the Python mirror's redundancy_min and suspect_edges do, and never name such an
 * edge).  A non-positive pivot of R -- at redundancy near 0, or in such a direction -- gives d2 = NaN.
 * An endpoint in the fixed set drops out of G;
 * with both endpoints fixed P = 0, the redundancy is 1 and d2 = e^T Omega_w e.  R is symmetric bit for bit; the bits of an
 * edge's outputs depend on the graph, the state and that edge alone, not on the rest of the list, its order or repeats.
 * One linearisation, one factorisation and one tree solve per call on the handle's stream, then one synchronisation; the
 * state, the Levenberg-Marquardt lambda, rr_pgo_optimize's results, captured graphs and the robust setting are untouched.
 * The cost grows with the number of distinct endpoint nodes (32 columns per pass over their root paths).
 * RR_PGO_EUNSUPPORTED first (the message says which): sharded handles, RR_PGO_F32 / RR_PGO_MIXED handles, graphs with fronts
 * beyond LDS unless rr_pgo_set_query_big_fronts.  RR_PGO_EINVAL, decided before anything is launched or written: n_query < 0, null d2_out with n_query > 0,
 * edge == NULL with n_query != rr_pgo_num_edges, an edge index out of range.  n_query == 0: RR_PGO_OK, nothing is launched.
 * RR_PGO_ENOTSPD: a non-positive pivot of H; nothing is written.  RR_PGO_ENOMEM: one edge alone needs more workspace than
 * the handle's bound (the message gives the bytes); longer lists are cut, which changes no bit. */
int rr_pgo_check_edges(rr_pgo *h, int32_t n_query, const int32_t *edge,
                       double *d2_out, double *redundancy_out, double *chi2_out,
                       double *resid_out, int64_t *resid_offset);
/* ms[3]: HIP-event times of the last rr_pgo_check_edges call -- linearise + factor, tree solve, kernel + copy. */
int rr_pgo_check_edges_times(const rr_pgo *h, double *ms);

/* ---- factor queries on fronts beyond LDS (build-defined) --------
 * Let rr_pgo_covariances, rr_pgo_cross_covariances, rr_pgo_gate_edges, rr_pgo_gate_joint and rr_pgo_check_edges answer on
 * graphs with fronts beyond LDS.  Default 0: such graphs are refused as before, same code, same message -- the refusal is
 * what callers and tests of the earlier interface rely on, so the capability is asked for per handle.
 * With the switch on, a front beyond LDS (rr_pgo_stats::n_big_fronts of them) keeps its block of the tree solve in the
 * call's workspace and is solved by kernels of its own, one or two more launches per level of the tree that
 * holds such a front; every "bit for bit" sentence of the five queries holds on these graphs too.  On a handle without such
 * fronts the switch changes no bit of any result and no launch.  The setter is RR_PGO_OK on every handle (RR_PGO_EINVAL:
 * no handle); sharded and RR_PGO_F32 / RR_PGO_MIXED handles keep their own refusals, which are checked first.
 * rr_pgo_extend and rr_pgo_remove_edges carry the switch.  rr_pgo_marginals does not read it: its own switch is rr_pgo_set_marginals_big_fronts.
 * Captured graphs, the state, the Levenberg-Marquardt lambda and the robust, prior and fixed settings are untouched. */
int rr_pgo_set_query_big_fronts(rr_pgo *h, int32_t on);
int32_t rr_pgo_get_query_big_fronts(const rr_pgo *h);   /* 0 or 1; 0 without a handle */

/* ---- growing a live handle (build-defined; the reference builds a new PoseGraph) --------
 * Append n_new_nodes nodes and n_new_edges edges, in rr_pgo_graph_desc packing.  New nodes get the indices
 * N .. N + n_new_nodes - 1 (N = rr_pgo_num_nodes before the call), new edges come after the existing ones; old node indices,
 * old dx offsets, old edge indices and the anchor rule (from-node of the first pose-pose edge in edge order) stay as they are
 * -- a graph that had no pose-pose edge takes its anchor from the first new one.  New edges may name any node below
 * N + n_new_nodes.  node_id == NULL: id = index; an id that repeats an existing or another new id is RR_PGO_EINVAL.
 * After the call the handle is the handle rr_pgo_create would return for the grown graph, with the handle's options and under
 * the environment as it is AT THE CALL (the RR_PGO_* switches are read again): same symbolic analysis, launches,
 * rr_pgo_get_stats and rr_pgo_get_graph -- except that its device state equals the old device state BIT FOR BIT for every old
 * node (the poses are copied device to device into the new state buffer: no read-back, no atan2), while new nodes hold
 * node_state, converted exactly as rr_pgo_set_state converts it.  rr_pgo_get_graph keeps showing the old nodes' initial
 * values, as before the call.
 * node_state == NULL with n_new_nodes > 0: the new nodes are initialised on the device.  The host plans steps from structure
 * alone: the ready set starts as the old nodes; the new edges are scanned in order, again and again, until a scan adds no
 * step; an edge with exactly one ready endpoint whose other endpoint is a new node not yet ready is a step when it determines
 * that node -- to = from (+) z for every kind (SE2: X_to = X_from Z; SE2_XY and SE3_XYZ: l = t + R z; SE3: X_to = X_from Z), from = to (+) z^-1
 * for pose-pose edges only -- and makes it ready (SE2_BEARING and SE2_RANGE edges are never a step).  A new node no step reaches is RR_PGO_EINVAL (the message names it), decided
 * before anything changes.  One kernel (k_guess_nodes) executes the steps in the state's arithmetic type, dependent steps in
 * list order, (cos, sin) and quaternions renormalised; the guessed values of the new nodes are copied into the host graph
 * (rr_pgo_get_graph shows them, the analysis sees what a fresh handle on that graph would).
 * Carried over -- by this call and by rr_pgo_remove_edges, the two calls that rebuild a handle; this is the one list:
 *   the solver option;
 *   the robust kernel: kind, delta, the mu of RR_PGO_ROBUST_TLS, and the edge mask re-indexed to the new edges -- here the
 *     old entries followed by 1 for every new edge (a fresh closure is robustified); a NULL mask stays NULL;
 *   the prior list of rr_pgo_set_priors with its robust flags and keep_anchor (node indices do not change);
 *   the fixed set of rr_pgo_set_fixed with its keep_anchor (new nodes are free);
 *   the rr_pgo_set_query_big_fronts and rr_pgo_set_marginals_big_fronts switches.
 * NOT carried: captured graphs, the tree and selected-inverse tables of the queries, rr_pgo_set_state's memo of the previous
 * state, the Levenberg-Marquardt lambda and the *_times of earlier calls; rr_pgo_stream may return another stream.  Pointers
 * from an earlier rr_pgo_get_graph become invalid.
 * Atomic: the new graph, analysis and engine are built completely and then swapped in; the old stream is synchronised before
 * the old engine goes.  Any failure -- RR_PGO_EINVAL below, RR_PGO_ENOMEM, a HIP error (RR_PGO_ENODEVICE) -- leaves the handle
 * as it was, usable, with the same bits.
 * RR_PGO_EINVAL, decided before anything is launched, the message names the node or edge: negative counts, a null required
 * pointer (node_id may be NULL, node_state may be NULL as above), everything rr_pgo_create rejects for the grown graph (bad
 * kinds, a kind that does not fit its endpoints, a self loop, an unknown vertex, mixed 2-D / 3-D), duplicate ids, an
 * unreachable node in guess mode.  n_new_nodes == 0 && n_new_edges == 0: RR_PGO_OK, nothing changes.
 * RR_PGO_EUNSUPPORTED: sharded handles (the message says why).  RR_PGO_F32 / RR_PGO_MIXED handles and graphs with fronts beyond
 * LDS are supported: the rebuild is rr_pgo_create's constructor. */
int rr_pgo_extend(rr_pgo *h,
                  int32_t n_new_nodes, const int32_t *node_kind, const uint32_t *node_id, const double *node_state,
                  int32_t n_new_edges, const int32_t *edge_kind, const int32_t *edge_from, const int32_t *edge_to,
                  const double *edge_meas, const double *edge_info);
/* ms[3] of the last rr_pgo_extend call: symbolic analysis and engine construction (host wall clock), state carry + initial
 * guess (HIP events). */
int rr_pgo_extend_times(const rr_pgo *h, double *ms);

/* ---- taking edges out of a live handle (build-defined) --------
 * Remove the edges edge[0 .. n_remove) (a duplicate counts once).  The remaining edges keep their order and are renumbered
 * compactly; nodes, node indices and dx offsets do not change.  The anchor rule is applied to what remains -- the from-node of
 * the first remaining pose-pose edge -- so rr_pgo_anchor_node MAY CHANGE when the first pose-pose edge goes.
 * After the call the handle is the handle rr_pgo_create would return for the remaining graph, with the handle's options and
 * under the environment as it is at the call -- except that the device state of every node is the old device state bit for
 * bit (copied device to device, as rr_pgo_extend carries it).
 * Carried over and NOT carried: the list under rr_pgo_extend, with one difference -- the robust kernel's edge mask keeps the
 * entries of the remaining edges, in their order.  Atomic as rr_pgo_extend: any failure leaves the handle as it was, with the
 * same bits.
 * RR_PGO_EINVAL, decided before anything changes: n_remove < 0, null edge with n_remove > 0, an index out of range, a node
 * left without any edge (the message names the node).  A removal that only disconnects the graph is the caller's
 * responsibility, as with keep_anchor == 0: the system then ends as RR_PGO_ENOTSPD, and redundancy_out of rr_pgo_check_edges
 * (0 for a bridge) is the warning.  n_remove == 0: RR_PGO_OK, nothing changes.  RR_PGO_EUNSUPPORTED: sharded handles.
 * RR_PGO_F32 / RR_PGO_MIXED handles and graphs with fronts beyond LDS are supported: the rebuild is the constructor. */
int rr_pgo_remove_edges(rr_pgo *h, int32_t n_remove, const int32_t *edge);
/* ms[3] of the last rr_pgo_remove_edges call: symbolic analysis and engine construction (host wall clock), state carry
 * (HIP events). */
int rr_pgo_remove_edges_times(const rr_pgo *h, double *ms);

/* ---- inspection of the assembled system (parity tests) ------------------- */

/* Runs the linearisation kernels only and returns the assembled normal matrix
 * as a dense-block list: for every stored block s, (row_node, col_node) and
 * d_row x d_col row-major values; plus b (negated).  Call with all output
 * pointers NULL to get the counts.  Values are converted to f64. */
int rr_pgo_assemble(rr_pgo *h, double lambda, int lm, int32_t *n_blocks,
                    int32_t *block_row_node, int32_t *block_col_node,
                    int64_t *block_val_offset, double *block_vals,
                    int64_t *n_vals, double *b_out);

/* ---- measurement --------------------------------------------------------- */

/* Enqueue `iters` Gauss-Newton iterations (linearise, factor, solve, update,
 * chi2) back to back on the handle's stream WITHOUT the convergence break and
 * without host round trips; returns immediately.  rr_pgo_sync waits. */
int rr_pgo_iterate_async(rr_pgo *h, int32_t iters);
int rr_pgo_sync(rr_pgo *h);

typedef struct rr_pgo_stats {
  /* symbolic analysis (done once in create) */
  int64_t nnz_h_blocks;      /* stored blocks of H (diag + lower off-diag)      */
  int64_t nnz_l_scalars;     /* scalars in the supernodal factor incl. padding  */
  int64_t factor_flops;      /* flops of one numeric factorisation               */
  int32_t n_supernodes, n_levels, n_launches_per_iter;
  int32_t max_front, max_pivot_cols;
  int32_t n_big_fronts;      /* fronts taken by the tiled multi-workgroup path   */
  double analyze_ms, parse_ms;
  /* algorithmic bytes of one GN iteration by phase */
  double bytes_linearize, bytes_factor, bytes_solve, bytes_update, bytes_chi2;
  double big_update_flops;   /* flops (2 per multiply-add) of one iteration's k_big_update launches */
  double big_flow_flops;     /* the same count for the trailing-update tiles that run inside k_big_flow launches */
  double stored_factor_bytes;/* bytes of the factor AS STORED (supernodal panels with their padding; fronts beyond LDS: the whole
                              * in-place M x M front) -- NOT what bytes_factor / bytes_solve are computed from: those follow
                              * SURVEY 8(d), nnzblk(L) * d^2 * s, every datum moved once */
  int32_t abi_version;       /* RR_PGO_ABI_VERSION of the library that filled the struct */
  int32_t lds_dataflow;      /* 1: the fronts that live in LDS are factored and solved by the two dataflow launches
                              * (k_factor_flow / k_solve_flow), 0: by one launch per level of the task tree */
} rr_pgo_stats;
int rr_pgo_get_stats(const rr_pgo *h, rr_pgo_stats *out);

/* Form of the back substitution of the fronts that live in LDS.  *kform = 1: the K form -- the factorisation also forms, per
 * front with rows below its pivot block, K = L11^-T L21^T and c = L11^-T y (stored like the factor), and the back
 * substitution of such a front is one product with them; 0: the chain over 16-column blocks.  k_bytes / k_flops (may be
 * NULL): what the K steps of one factorisation read and write, and their flops (2 per multiply-add); 0 in the chain form.
 * Not part of bytes_factor / bytes_solve, which count every datum of the factor once. */
int rr_pgo_solve_form(const rr_pgo *h, int32_t *kform, double *k_bytes, double *k_flops);

/* Iterations this handle's engine has put on its stream so far, by the form in which they were enqueued (out: 4 entries):
 * out[0] plain launches outside rr_pgo_optimize's device-side loop (rr_pgo_iterate_async, the loop of rr_pgo_optimize with
 *        one host round trip per iteration, rr_pgo_profile),
 * out[1] replays of the captured hipGraph of one Gauss-Newton iteration,
 * out[2] items of rr_pgo_optimize's device-side loop (an item is an iteration or the chi2 pass that ends a call),
 * out[3] captures (instantiations) of that hipGraph.
 * Host-side counters, incremented where the launches are enqueued: no device work, no synchronisation.  rr_pgo_extend
 * builds a new engine for the grown graph, so the counters start again at 0 there; rr_pgo_set_robust_kernel and
 * rr_pgo_set_priors drop the captured graph, so the next replay counts another capture. */
int rr_pgo_launch_counts(const rr_pgo *h, int64_t *out);

/* Host-only: parse + symbolic analysis of a g2o file, the rr_pgo_stats a handle on it would report (fields that depend
 * on the device -- n_launches_per_iter, big_update_flops, big_flow_flops -- are 0).  Needs no HIP device. */
int rr_pgo_analyze_g2o(const char *path, const rr_pgo_options *opt, rr_pgo_stats *out);

/* ABI version: bumped whenever a struct layout, an enum that sizes a caller's array (RR_PGO_NUM_KCLASS) or the meaning
 * of an argument changes.  r03 -> 3 (RR_PGO_NUM_KCLASS 10 -> 11), r04 -> 4 (rr_pgo_stats: stored_factor_bytes,
 * abi_version; RR_PGO_ETIMEOUT; rr_pgo_profile takes the length of the caller's arrays). */
int32_t rr_pgo_abi_version(void);

/* Per-kernel timing measured with HIP events on the handle's own stream.
 * Runs `iters` eager (non-graph) GN iterations with an event pair around every
 * launch and accumulates per kernel class.  The caller passes the length of its arrays (RR_PGO_NUM_KCLASS). */
enum {
  RR_PGO_K_LINEARIZE = 0,   /* k_linearize                                             */
  RR_PGO_K_FACTOR = 1,      /* k_factor_tasks (fronts in LDS)                          */
  RR_PGO_K_SOLVE = 2,       /* k_solve_tasks                                           */
  RR_PGO_K_UPDATE = 3,      /* k_update                                                */
  RR_PGO_K_REDUCE = 4,      /* k_finalize_slot                                         */
  RR_PGO_K_BIGFRONT = 5,    /* huge fronts: k_big_build + k_big_assemble (gather pass), k_flow_reset */
  RR_PGO_K_BIG_PANEL = 6,   /* k_big_panel32 (huge fronts: 32-column chain steps)       */
  RR_PGO_K_BIG_UPDATE = 7,  /* k_big_update + k_big_schur (huge fronts: MFMA trailing updates) */
  RR_PGO_K_MID_FACTOR = 8,  /* retired in r03 (the one-workgroup panel class was removed): always 0   */
  RR_PGO_K_BIG_SOLVE = 9,   /* k_big_gemv_partial + k_big_solve_flow (k_big_solve_sp) / k_solve_mid */
  RR_PGO_K_BIG_FLOW = 10,   /* k_big_flow (huge fronts of a level of few fronts: panels + updates as one dataflow launch) */
  RR_PGO_NUM_KCLASS = 11
};
int rr_pgo_profile(rr_pgo *h, int32_t iters, double *ms_total /*[n_classes]*/,
                   int64_t *launches /*[n_classes]*/, int32_t n_classes /* length of the two arrays: at most that many
                   classes are written (a caller built against an older RR_PGO_NUM_KCLASS is not overrun) */);

/* ---- testing ------------------------------------------------------------- */

/* Failure injection for the dataflow launches (tests only; no counterpart in the reference): make ONE hand-off between
 * workgroups never arrive, so that the waits behind it run into their time bound (environment RR_PGO_FLOW_TIMEOUT_MS,
 * read when the handle is created; default 2000) and the next iteration returns RR_PGO_ETIMEOUT with the state untouched.
 * mode 1: a child front of the factorisation of the LDS fronts (k_factor_flow); 2: a parent front of their back
 * substitution (k_solve_flow); 3: one panel step of the fronts beyond LDS (k_big_flow); 0: put everything back. */
int rr_pgo_debug_withhold(rr_pgo *h, int32_t mode);

/* ---- synthetic workload (BASELINE config 4) -------------------- */

/* Deterministic SE(2) lattice graph: W x H poses in boustrophedon order, the
 * 10-offset stencil (+ part of an 11th) described in SURVEY.md 8(d), trimmed or
 * capped to n_edges_target (<=0: all stencil edges).  Fills a graph description
 * whose arrays are owned by the returned object; free with rr_pgo_synth_free. */
typedef struct rr_pgo_synth rr_pgo_synth;
int rr_pgo_synth_grid(int32_t width, int32_t height, int64_t n_edges_target,
                      uint64_t seed_meas, uint64_t seed_init, rr_pgo_synth **out,
                      rr_pgo_graph_desc *desc);
void rr_pgo_synth_free(rr_pgo_synth *s);

/* ---- sharding ONE graph over ranks ------------------------------ */

/* A handle created with opt.world_size = P > 1 (power of two, <= 64) and opt.rank = r owns the subtrees
 * of partition r of the nested dissection (its nodes, their edges, their fronts); the top log2(P)
 * separator levels -- and the anchor node -- are shared: every rank holds their state and factors their
 * fronts redundantly, so there is no panel traffic on the sequential chain of the top fronts.  Every rank
 * creates its handle from the SAME graph.  One Gauss-Newton iteration is two stages and two collectives
 * (the reference has no counterpart: its only parallel construct is pose_graph_optimization.rs:230):
 *
 *   rr_pgo_stage(h, 0, lambda, lm)   linearise the rank's nodes (:305-369 restricted to own + shared nodes),
 *                                    factor its own subtrees, publish the boundary fronts' update matrices in
 *                                    chunk r of exchange buffer 0
 *   ALL-GATHER of buffer 0           in place: rank r contributes elements [r * n / P, (r + 1) * n / P)
 *   rr_pgo_stage(h, 1, ...)          shared top fronts, back substitution (top + own subtrees), update_nodes
 *                                    (:229-245) for own + shared nodes, partial chi2 / |dx|^2 -> buffer 1
 *   ALL-REDUCE (sum) of buffer 1     two doubles; only the stop rule (:298-300) and the log need them
 *   rr_pgo_stage(h, 2, ...)          chi2 of the current state only (partial -> buffer 1, then the same
 *                                    all-reduce): the last entry of optimize()'s error list
 *
 * Every edge's chi2 term and every node's |dx|^2 is counted by exactly one rank.  A rank's copy of the state
 * is valid for its own and the shared nodes (rr_pgo_node_owner says which); rr_pgo_get_state returns the
 * rank's copy.  The library enqueues on its own stream (rr_pgo_stream): issue the collectives on that stream
 * and an iteration needs no host synchronisation.  Buffers are device memory of element size *elem_size (4 or
 * 8 for buffer 0, 8 for buffer 1); the caller may bind memory it allocated itself (so that its collective
 * library can register it) with rr_pgo_set_exchange_buffer before the first stage. */
int rr_pgo_exchange_buffer(rr_pgo *h, int32_t which, void **dev_ptr, int64_t *n_elems, int32_t *elem_size);
int rr_pgo_set_exchange_buffer(rr_pgo *h, int32_t which, void *dev_ptr, int64_t n_elems);
int rr_pgo_stage(rr_pgo *h, int32_t stage, double lambda, int lm);
/* after the all-reduce of buffer 1: chi2 of the state BEFORE the iteration's update and |dx| of the step
 * (stage 1), or chi2 of the current state (stage 2).  Synchronises the handle's stream. */
int rr_pgo_stage_scalars(rr_pgo *h, double *chi2, double *norm_dx);
void *rr_pgo_stream(rr_pgo *h);                           /* hipStream_t the handle launches on */
/* owner[n_nodes]: rank that owns the node, -1 = shared (top separators, anchor); all 0 on an unsharded handle */
int rr_pgo_node_owner(const rr_pgo *h, int32_t *owner);

#ifdef __cplusplus
}
#endif
#endif
