// treesolve.hip.h -- covariances of arbitrary node pairs from a multi-column forward solve over the supernode tree
// (rr_pgo_covariances).
//
// With H = L L^T, Sigma_ab = Z_a^T Z_b where Z_s = L^-1 E_s and E_s holds the unit columns of node s.  Z_s is non-zero only
// on the pivot rows of the fronts on the path from the front of s to the root, so a set of right-hand columns touches only
// the union of those paths (the ACTIVE fronts), and a pair (a, b) needs only the rows from the lowest common front up.
//
//   k_tree_fwd    one workgroup per (chunk of TS_MC columns, active front), one launch per level of the tree, deepest first
//   k_cov_pairs   one workgroup per query: Sigma_ab = sum over the common path's pivot rows of Z_a[row]^T Z_b[row]
//   k_gate_pairs  one workgroup per candidate edge: its Mahalanobis distance from the same Z
//   k_check_edges one workgroup per edge of the graph: its leave-one-out distance and redundancy from the same Z
//   k_gate_joint  one workgroup per set of candidate edges: their joint distance from the same Z
//   k_tree_bwd    one workgroup per (chunk, backward-active front), one launch per level, root level first: X = L^-T Z
//   k_cross_gather  the rectangular block Sigma[rows, cols] out of X (the end of this file)
//   k_tree_fwd_big, k_tree_fwd_big_update, k_tree_bwd_big_gemv, k_tree_bwd_big   the two solves of a front beyond LDS, whose
//                 block stays in the workspace (before k_cross_gather; DESIGN.md 4r, rr_pgo_set_query_big_fronts)
//
// Columns.  The distinct queried nodes are ordered by (front, pivot column) -- fronts are numbered in elimination order, so
// neighbours share paths -- and packed, whole nodes at a time, into chunks of TS_MC = 32 columns (unused columns stay zero).
// Workspace.  Z: per (chunk, active front) nc rows of TS_MC scalars -- all chunks resident, so a pair may span two chunks.
//             U: per (chunk, active front) nr rows of TS_MC scalars, the front's update block for its parent.
// Both are row-major with TS_MC columns.  Z + U of one pass stay within TS_WS_BYTES = 512 MiB: a query list whose plan
// would need more is cut in halves (by query index) until every part fits, and the parts run one after the other over the
// same factor.  A column's arithmetic does not depend on the chunk it sits in or on its place there (below), so the cut
// changes no bit of the result.
//
// Determinism.  No atomics.  Every scalar of Z and U is produced by one wave in a fixed operation order that depends on
// the front and the row alone: columns of an MFMA tile are independent, children are gathered in ascending front order with
// a barrier between them, and an inactive child contributes what an active child with a zero column contributes (x + 0).
// k_cov_pairs adds the rows of a pair in a fixed slice order, products by fma (commutative in its two factors), so
// Sigma(b, a) is the transpose of Sigma(a, b) bit for bit and diagonal blocks are symmetric bit for bit.
#pragma once
#include "kernels.hip.h"

namespace rrpgo {

constexpr int TS_MC = 32;                       // columns of a chunk (two 16-column MFMA tiles)
constexpr int TS_LD = TS_MC + 16;               // LDS row stride of the right-hand block: rows k and k + 1 of a B operand
                                                // (lanes l and l + 16) land on opposite halves of the 64 banks
constexpr int TS_THREADS = 512;
constexpr int COV_THREADS = 512;
constexpr size_t TS_WS_BYTES = (size_t)512 << 20;   // bound of Z + U of one pass (RR_PGO_TS_WS_BYTES=<n>: a handle's own)
static_assert(TS_MC == 32, "row / column of a packed unit entry and of a flat Z / U index are taken with >> 5 and & 31");

struct TsMeta {
  int32_t nc, nr, wblk, parent;   // pivot columns, rows below, first W block in winv, parent front (-1: a root)
  int64_t loff, rel_ptr;          // panel in lvals, the front's rel map (local row in the parent's front)
};
static_assert(sizeof(TsMeta) == 32, "TsMeta is one 32-byte record");

struct TsTask {
  int32_t front;
  int32_t child_ptr, n_child;     // into TsArgs::child: the tasks of this front's active children, ascending front order
  int32_t unit_ptr, n_unit;       // into TsArgs::unit: (local pivot row << 5 | column) of the chunk's nodes eliminated here
  int32_t zrow, urow;             // first row of this task's pivot part in Z, of its update block in U
  int32_t pad;
};
static_assert(sizeof(TsTask) == 32, "TsTask is one 32-byte record");

template <typename T> struct TsArgs {
  const TsMeta *meta;
  const TsTask *tasks;            // by level, deepest first
  const int32_t *child, *unit, *rel;
  const T *lvals, *winv;
  T *Z, *U;
};

// The right-hand block of the front, (nc + nr) x TS_MC, lives in LDS (row stride TS_LD).  L is read from lvals in global
// memory straight into the A operands (a 152 000 B panel and the block do not fit in LDS together).
template <typename T>
__global__ void __launch_bounds__(TS_THREADS) k_tree_fwd(TsArgs<T> a, int begin) {
  using MM = Mfma16<T>;
  constexpr int NW = TS_THREADS / 64, LD = TS_LD, NCT = TS_MC / 16;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  __shared__ T ws[256];                  // W_b: ws[i * 16 + k] = W(i, k)
  T *B = reinterpret_cast<T *>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = wave_index();
  const TsTask t = a.tasks[begin + blockIdx.x];
  const TsMeta m = a.meta[t.front];
  const int nc = m.nc, nr = m.nr, n = nc + nr, M = n + 1;
  const T *Lg = a.lvals + m.loff;
  const T *Wg = a.winv + (int64_t)m.wblk * 256;
  for (int e = tid; e < n * LD; e += TS_THREADS) B[e] = 0;
  __syncthreads();
  // ---- the update blocks of the active children through their rel maps, one child after the other
  for (int c = 0; c < t.n_child; c++) {
    const TsTask ct = a.tasks[a.child[t.child_ptr + c]];
    const TsMeta cm = a.meta[ct.front];
    const int32_t *rel = a.rel + cm.rel_ptr;
    const T *Uc = a.U + (int64_t)ct.urow * TS_MC;
    for (int e = tid; e < cm.nr * TS_MC; e += TS_THREADS) {
      const int row = rel[e >> 5];
      if ((unsigned)row < (unsigned)n) B[row * LD + (e & 31)] += Uc[e];
    }
    __syncthreads();
  }
  // ---- unit entries of the chunk's nodes whose pivot columns are here
  for (int e = tid; e < t.n_unit; e += TS_THREADS) {
    const int u = a.unit[t.unit_ptr + e];
    B[(u >> 5) * LD + (u & 31)] += (T)1;
  }
  __syncthreads();
  // ---- pivot square, right-looking by 16-column blocks: Y_b = W_b B_b, then B_i -= L_ib Y_b for the later pivot rows
  for (int b = 0; b < ((nc + 15) >> 4); b++) {
    const int c0 = 16 * b, cw = min(16, nc - c0), t0 = c0 + 16;
    if (tid < 256) ws[tid] = Wg[b * 256 + tid];
    __syncthreads();
    if (wave < NCT) {   // a column tile of the block is one wave's: read whole, then written
      const int col = 16 * wave + li;
      typename MM::Acc y = {0, 0, 0, 0};
      T bv[4];
#pragma unroll
      for (int s = 0; s < 4; s++) bv[s] = B[(c0 + min(4 * s + lk, cw - 1)) * LD + col];
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int k = 4 * s + lk;
        const T wv = (k <= li && li < cw) ? ws[li * 16 + k] : (T)0;   // W is lower triangular; rows past a partial block are padding
        y = MM::mma(wv, k < cw ? bv[s] : (T)0, y);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = MM::row(lane, r);
        if (i < cw) B[(c0 + i) * LD + col] = y[r];
      }
    }
    __syncthreads();
    if (t0 < nc) {   // (so this block is a full one)
      const int nti = (nc - t0 + 15) >> 4;
      for (int tile = wave; tile < nti * NCT; tile += NW) {
        const int ib = tile / NCT, jb = tile - ib * NCT;
        const int i0 = t0 + 16 * ib, col = 16 * jb + li;
        typename MM::Acc acc;
#pragma unroll
        for (int r = 0; r < 4; r++) acc[r] = B[min(i0 + MM::row(lane, r), n - 1) * LD + col];
        const int ia = min(i0 + li, n - 1);   // rows past nc of the last tile are computed and dropped
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const int k = c0 + 4 * s + lk;
          acc = MM::mma(-Lg[(int64_t)k * M + ia], B[k * LD + col], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = i0 + MM::row(lane, r);
          if (row < nc) B[row * LD + col] = acc[r];
        }
      }
    }
    __syncthreads();
  }
  // ---- U = B_R - L_21 Y_P, the front's update block (a root has no rows below)
  if (nr > 0) {
    T *Ug = a.U + (int64_t)t.urow * TS_MC;
    const int nti = (nr + 15) >> 4;
    for (int tile = wave; tile < nti * NCT; tile += NW) {
      const int ib = tile / NCT, jb = tile - ib * NCT;
      const int i0 = nc + 16 * ib, col = 16 * jb + li;
      typename MM::Acc acc;
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = B[min(i0 + MM::row(lane, r), n - 1) * LD + col];
      const int ia = min(i0 + li, n - 1);
      for (int k4 = 0; k4 < nc; k4 += 4) {
        const int k = k4 + lk, kc = min(k, nc - 1);
        const T lv = Lg[(int64_t)kc * M + ia];
        acc = MM::mma(k < nc ? -lv : (T)0, B[kc * LD + col], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = i0 + MM::row(lane, r);
        if (row < n) Ug[(int64_t)(row - nc) * TS_MC + col] = acc[r];
      }
    }
  }
  // ---- Y_P is this front's part of Z
  T *Zg = a.Z + (int64_t)t.zrow * TS_MC;
  for (int e = tid; e < nc * TS_MC; e += TS_THREADS) Zg[e] = B[(e >> 5) * LD + (e & 31)];
}

struct CovQuery {
  int32_t lca;                    // lowest front common to the two nodes' paths, -1: none (different trees: the block is zero)
  int32_t chunk_a, chunk_b;
  int32_t da, db, pad;
  uint8_t ca[8], cb[8];           // reference scalar r of the node -> its column in the chunk
  int64_t ooff;                   // offset of the block in out
};
static_assert(sizeof(CovQuery) == 48, "CovQuery is one 48-byte record");

template <typename T> struct CovArgs {
  const TsMeta *meta;
  const CovQuery *query;
  const int32_t *czrow;           // [chunk * S + front]: first Z row of the front in the chunk, -1 = not active there
  const T *Z;
  double *out;
  int32_t S;
};

// A wave is one slice of rows (row = slice, slice + 8, ... of every front on the path); lane e of it accumulates output
// scalar e = i * db + j.  The eight slices are added in slice order.
template <typename T>
__global__ void __launch_bounds__(COV_THREADS) k_cov_pairs(CovArgs<T> a) {
  constexpr int NS = COV_THREADS / 64;
  __shared__ T part[NS * 64];
  const CovQuery *q = a.query + blockIdx.x;
  const int tid = threadIdx.x, e = tid & 63, slice = wave_index();
  const int db = q->db, cnt = q->da * db;
  const int ec = min(e, cnt - 1), i = ec / db, j = ec - i * db;
  const int cola = q->ca[i], colb = q->cb[j];
  const int32_t *za_tab = a.czrow + (int64_t)q->chunk_a * a.S, *zb_tab = a.czrow + (int64_t)q->chunk_b * a.S;
  T acc = 0;
  for (int f = q->lca; f >= 0; f = a.meta[f].parent) {
    const int nc = a.meta[f].nc, za = za_tab[f], zb = zb_tab[f];
    if (za < 0 || zb < 0) continue;
    const T *Za = a.Z + ((int64_t)za * TS_MC + cola), *Zb = a.Z + ((int64_t)zb * TS_MC + colb);
    for (int r = slice; r < nc; r += NS) acc = fma(Za[r * TS_MC], Zb[r * TS_MC], acc);
  }
  part[slice * 64 + e] = acc;
  __syncthreads();
  if (tid < cnt) {
    T s = part[tid];
#pragma unroll
    for (int k = 1; k < NS; k++) s += part[k * 64 + tid];
    a.out[q->ooff + tid] = (double)s;
  }
}

// ---- Mahalanobis gate of candidate edges (rr_pgo_gate_edges)
//
// For a candidate edge between nodes a and b with error e, Jacobians A, B and information Omega at the current state:
//   P = [A B] Sigma_{ab,ab} [A B]^T = G^T G,   G = Z_a A^T + Z_b B^T   (one row per pivot row on the two root paths),
//   S = Omega^-1 + P,   d2 = e^T S^-1 e,   s = e^T Omega e.
// The four blocks of Sigma_{ab,ab} are large against P (the two poses move together): G forms the difference row by row,
// on the common path, BEFORE it is squared, and P is positive semi-definite by construction.
struct GateCand {
  CovQuery cq;                    // of the pair (a, b); ooff: offset of S (d_e x d_e, row-major) in sout
  int32_t fa, fb;                 // the fronts of a and of b
  int32_t na, nb, kind, pad;      // the two nodes; RR_PGO_EDGE_*
  double meas[8];                 // 2-D: x, y, cos, sin | SE(3): t (3), -, q (4, normalised) | SE3_XYZ: x, y, z, then zeros
                                  // SE2_BEARING: cos z, sin z, 0, 4 | SE2_RANGE: z, 0, 0, 6 (pack_meas, host_graph.h)
  double info[36], cov[36];       // Omega and Omega^-1, row stride D (3 or 6), zero padded
};
static_assert(sizeof(GateCand) == 712, "GateCand is one 712-byte record");

template <typename T> struct GateArgs {
  const TsMeta *meta;
  const GateCand *cand;
  const int32_t *czrow;           // as CovArgs
  const T *Z;
  const typename VecT<T>::V4 *pose;
  double *d2, *chi2, *sout;       // sout null: S is not asked for
  int32_t S;
};

// error dimension of a candidate of RR_PGO_EDGE_* `kind` in a graph of pose dimension D; a landmark edge's `to` node has as many scalars
// LM: the kernel instantiation of a 3-D graph with XYZ landmarks (kind 3 occurs); false is the code of every other handle
// LM with D == 3 ("BR" below): the kernel instantiation of a 2-D call with bearing-only / range-only records (kinds 4 and 6 occur:
// one error scalar, while the `to` node, an XY landmark, has two -- gate_to_dim).  The flag's second meaning keeps the names and
// the code of the instantiations that exist: <T, 3, false> stays what every other 2-D call launches.
template <int D, bool LM> __device__ __forceinline__ int gate_edge_dim(int kind) {
  if constexpr (LM && D == 3) return kind == 4 || kind == 6 ? 1 : kind == 1 ? 2 : D;
  else if constexpr (LM) return kind == 3 ? 3 : D;
  else return kind == 1 ? 2 : D;
}
// scalars of the candidate's `to` node: d_e everywhere but for a bearing or range record
template <int D, bool LM> __device__ __forceinline__ int gate_to_dim(int kind) {
  if constexpr (LM && D == 3) return kind == 0 ? D : 2;
  else return gate_edge_dim<D, LM>(kind);
}

// A candidate's error e and Jacobians A, B (row-major D x D) at the current state, by the linearisation's own code.
// role 0: e and A, and in 2-D also B; role 1: B of SE3 (a second lane shares the work; in 2-D it has none).
template <typename T, int D, bool LM = false>
__device__ __forceinline__ void gate_linearize(const GateCand *q, const typename VecT<T>::V4 *pose, int role, T *se, T *sA, T *sB) {
  using V4 = typename VecT<T>::V4;
  if constexpr (D == 3) {
    if (role == 0) {
      const V4 z = {(T)q->meas[0], (T)q->meas[1], (T)q->meas[2], (T)q->meas[3]};
      T e[3], A[3][3], B[3][3];
      if constexpr (LM) {   // (D == 3: the BR instantiation)
        if (q->kind == 4 || q->kind == 6) edge_linearize_2d_br<T>(pose[q->na], pose[q->nb], z, e, A, B);   // zero padded, row 0 alone
        else edge_linearize_2d<T>(q->kind, pose[q->na], pose[q->nb], z, e, A, B);
      } else
      edge_linearize_2d<T>(q->kind, pose[q->na], pose[q->nb], z, e, A, B);
#pragma unroll
      for (int i = 0; i < 3; i++) {
        se[i] = e[i];
#pragma unroll
        for (int j = 0; j < 3; j++) {
          sA[i * 3 + j] = A[i][j];
          sB[i * 3 + j] = B[i][j];
        }
      }
    }
  } else {
    T ti[3], qi[4], tj[3], qj[4];
    pose_3d<T>(pose[2 * q->na], pose[2 * q->na + 1], ti, qi);
    pose_3d<T>(pose[2 * q->nb], pose[2 * q->nb + 1], tj, qj);
    const T tz[3] = {(T)q->meas[0], (T)q->meas[1], (T)q->meas[2]};
    const T qz[4] = {(T)q->meas[4], (T)q->meas[5], (T)q->meas[6], (T)q->meas[7]};
    T e[6], J[6][6];
    if constexpr (LM) {
      if (q->kind == 3) edge_linearize_3d_point<T>(role, ti, qi, tj, tz, e, J);   // RR_PGO_EDGE_SE3_XYZ, zero padded
      else edge_linearize_3d<T>(role, ti, qi, tj, qj, tz, qz, e, J);
    } else {
      edge_linearize_3d<T>(role, ti, qi, tj, qj, tz, qz, e, J);
    }
    T *dst = role ? sB : sA;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      if (role == 0) se[i] = e[i];
#pragma unroll
      for (int j = 0; j < 6; j++) dst[i * 6 + j] = J[i][j];
    }
  }
}

// the rows of the fronts from f up to (not including) `stop`, slice by slice: acc += G_r[i] G_r[j]
template <typename T, int D, bool UA, bool UB>
__device__ __forceinline__ T gate_walk(const TsMeta *meta, const T *Z, const int32_t *za_tab, const int32_t *zb_tab, int f, int stop,
                                       int slice, int ns, const int (&cola)[D], const int (&colb)[D], const T (&Ai)[D],
                                       const T (&Aj)[D], const T (&Bi)[D], const T (&Bj)[D], T acc) {
  for (; f >= 0 && f != stop; f = meta[f].parent) {
    const int nc = meta[f].nc, za = UA ? za_tab[f] : 0, zb = UB ? zb_tab[f] : 0;
    if (za < 0 || zb < 0) continue;
    for (int r = slice; r < nc; r += ns) {
      T gi = 0, gj = 0;
      if (UA) {
        const T *p = Z + (int64_t)(za + r) * TS_MC;
#pragma unroll
        for (int k = 0; k < D; k++) {
          const T z = p[cola[k]];
          gi = fma(z, Ai[k], gi);
          gj = fma(z, Aj[k], gj);
        }
      }
      if (UB) {
        const T *p = Z + (int64_t)(zb + r) * TS_MC;
#pragma unroll
        for (int k = 0; k < D; k++) {
          const T z = p[colb[k]];
          gi = fma(z, Bi[k], gi);
          gj = fma(z, Bj[k], gj);
        }
      }
      acc = fma(gi, gj, acc);
    }
  }
  return acc;
}

// One workgroup per candidate; D = 3 (a 2-D graph: SE2 and SE2_XY candidates) or 6 (SE3).  Lanes 0 of waves 0 and 1 evaluate
// (e, A) and B with the linearisation's own code.  A wave is one slice of rows (row = slice, slice + 8, ... of every front);
// lane t of it accumulates entry t of P's lower triangle.  The eight slices are added in slice order, then lane 0 of wave 0
// factors S = Omega^-1 + P in LDS.  A non-positive pivot of S (Omega is checked on the host: rounding only) gives d2 = NaN.
template <typename T, int D, bool LM = false>
__global__ void __launch_bounds__(COV_THREADS) k_gate_pairs(GateArgs<T> a) {
  constexpr int NS = COV_THREADS / 64;
  __shared__ T part[NS * 32], sA[D * D], sB[D * D], se[D], sS[D * D];
  const GateCand *q = a.cand + blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, slice = wave_index();
  const int kind = q->kind;
  const int de = gate_edge_dim<D, LM>(kind), db = gate_to_dim<D, LM>(kind), ntri = de * (de + 1) / 2;
  if (lane == 0 && slice < 2) gate_linearize<T, D, LM>(q, a.pose, slice, se, sA, sB);
  __syncthreads();
  // ---- entry t = (i, j), j <= i, of the lower triangle; lanes past the triangle repeat its last entry
  const int t = min(lane, ntri - 1);
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) i++;
  const int j = t - i * (i + 1) / 2;
  T Ai[D], Aj[D], Bi[D], Bj[D];
  int cola[D], colb[D];
#pragma unroll
  for (int k = 0; k < D; k++) {
    Ai[k] = sA[i * D + k];
    Aj[k] = sA[j * D + k];
    Bi[k] = sB[i * D + k];   // (the columns of B past d_b are zero: pose-landmark)
    Bj[k] = sB[j * D + k];
    cola[k] = q->cq.ca[k];
    colb[k] = q->cq.cb[min(k, db - 1)];
  }
  const int32_t *za_tab = a.czrow + (int64_t)q->cq.chunk_a * a.S, *zb_tab = a.czrow + (int64_t)q->cq.chunk_b * a.S;
  const int lca = q->cq.lca;
  T acc = 0;
  acc = gate_walk<T, D, true, false>(a.meta, a.Z, za_tab, zb_tab, q->fa, lca, slice, NS, cola, colb, Ai, Aj, Bi, Bj, acc);
  acc = gate_walk<T, D, false, true>(a.meta, a.Z, za_tab, zb_tab, q->fb, lca, slice, NS, cola, colb, Ai, Aj, Bi, Bj, acc);
  if (lca >= 0) acc = gate_walk<T, D, true, true>(a.meta, a.Z, za_tab, zb_tab, lca, -1, slice, NS, cola, colb, Ai, Aj, Bi, Bj, acc);
  if (lane < 32) part[slice * 32 + lane] = acc;
  __syncthreads();
  if (tid < ntri) {
    T s = part[tid];
#pragma unroll
    for (int k = 1; k < NS; k++) s += part[k * 32 + tid];
    s += (T)q->cov[i * D + j];
    sS[i * D + j] = s;
    sS[j * D + i] = s;
  }
  __syncthreads();
  if (a.sout && tid < de * de) a.sout[q->cq.ooff + tid] = (double)sS[(tid / de) * D + tid % de];   // both halves from the lower triangle
  __syncthreads();
  if (tid == 0) {
    T c2 = 0;   // e^T Omega e, the sum order of edge_chi2_2d / edge_chi2_3d
    for (int r = 0; r < de; r++) {
      T we = 0;
      for (int c = 0; c < de; c++) we += (T)q->info[r * D + c] * se[c];
      c2 += se[r] * we;
    }
    a.chi2[blockIdx.x] = (double)c2;
    // S = L L^T in place (lower triangle), y = L^-1 e, d2 = y^T y
    bool ok = true;
    T d2 = 0;
    for (int c = 0; c < de; c++) {
      T d = sS[c * D + c];
      for (int k = 0; k < c; k++) d = fma(-sS[c * D + k], sS[c * D + k], d);
      if (!(d > (T)0)) { ok = false; break; }
      const T l = sqrt(d), inv = (T)1 / l;
      sS[c * D + c] = l;
      for (int r = c + 1; r < de; r++) {
        T v = sS[r * D + c];
        for (int k = 0; k < c; k++) v = fma(-sS[r * D + k], sS[c * D + k], v);
        sS[r * D + c] = v * inv;
      }
      T y = se[c];
      for (int k = 0; k < c; k++) y = fma(-sS[c * D + k], se[k], y);
      y *= inv;
      se[c] = y;
      d2 = fma(y, y, d2);
    }
    a.d2[blockIdx.x] = ok ? (double)d2 : __builtin_nan("");
  }
}

// ---- audit of the graph's own edges (rr_pgo_check_edges)
//
// For edge c of the graph with error e, Jacobians A, B, information Omega and robust weight w at the current state:
//   Omega_w = w Omega (what the edge gave H),   P = G^T G as above,   R = Omega_w^-1 - P = Omega^-1 / w - P,
//   d2 = e^T R^-1 e (the gate's distance of the edge against the graph without it, to first order),
//   r = trace(R Omega_w) / d_e (1: the rest of the graph determines the residual; 0: a bridge, R = 0 up to rounding).
// The record is the gate's; its pad word holds the mask bit (1: the handle's robust kernel applies to this edge).
template <typename T> struct CheckArgs {
  const TsMeta *meta;
  const GateCand *cand;
  const int32_t *czrow;           // as CovArgs
  const T *Z;
  const typename VecT<T>::V4 *pose;
  double *d2, *chi2, *red, *rout; // rout null: R is not asked for
  T delta, delta2;                // of the robust kernel
  int32_t S, rkind;               // rkind: ROBUST_*
  T tls_lo, tls_hi, tls_cs, tls_mu;   // ROBUST_TLS: as LinArgs
};

// One workgroup per queried edge; D as in k_gate_pairs, and the same walk.  Lane 0 of wave 0 has s = e^T Omega e and w(s) ready
// (the linearisation's own robust_weight) when the slices are added: entry (i, j) of the lower triangle is
// Omega^-1(i, j) / w - P(i, j), mirrored, so R is symmetric bit for bit.  r is summed row by row, column by column, by one
// lane.  An edge whose weight is exactly 0 (ROBUST_TLS beyond its band) gave H nothing: its R, r and d2 are NaN, chi2 stays
// e^T Omega e, and it is queried with rr_pgo_gate_edges as the candidate it now is.  A non-positive pivot of R (an edge at r near 0, or one whose residual the rest of the graph determines in some
// directions only: rounding decides) gives d2 = NaN; r and R are written all the same.
template <typename T, int D, bool LM = false>
__global__ void __launch_bounds__(COV_THREADS) k_check_edges(CheckArgs<T> a) {
  constexpr int NS = COV_THREADS / 64;
  __shared__ T part[NS * 32], sA[D * D], sB[D * D], se[D], sS[D * D], sw[1];
  const GateCand *q = a.cand + blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, slice = wave_index();
  const int kind = q->kind;
  const int de = gate_edge_dim<D, LM>(kind), db = gate_to_dim<D, LM>(kind), ntri = de * (de + 1) / 2;
  if (lane == 0 && slice < 2) gate_linearize<T, D, LM>(q, a.pose, slice, se, sA, sB);
  __syncthreads();
  if (tid == 0) {
    T W[D][D], e[D];   // e^T Omega e by the linearisation's own edge_chi2 (Omega and a landmark edge's e are zero padded)
#pragma unroll
    for (int r = 0; r < D; r++) {
      e[r] = r < de ? se[r] : (T)0;
#pragma unroll
      for (int c = 0; c < D; c++) W[r][c] = (T)q->info[r * D + c];
    }
    const T c2 = edge_chi2<D, T>(W, e);
    T w = 1;
    if (q->pad & 1) w = robust_weight_rt<T>(a.rkind, c2, a.delta, a.delta2, a.tls_lo, a.tls_hi, a.tls_cs, a.tls_mu);
    a.chi2[blockIdx.x] = (double)c2;
    sw[0] = w;
  }
  // ---- entry t = (i, j), j <= i, of the lower triangle; lanes past the triangle repeat its last entry
  const int t = min(lane, ntri - 1);
  int i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) i++;
  const int j = t - i * (i + 1) / 2;
  T Ai[D], Aj[D], Bi[D], Bj[D];
  int cola[D], colb[D];
#pragma unroll
  for (int k = 0; k < D; k++) {
    Ai[k] = sA[i * D + k];
    Aj[k] = sA[j * D + k];
    Bi[k] = sB[i * D + k];   // (the columns of B past d_b are zero: pose-landmark)
    Bj[k] = sB[j * D + k];
    cola[k] = q->cq.ca[k];
    colb[k] = q->cq.cb[min(k, db - 1)];
  }
  const int32_t *za_tab = a.czrow + (int64_t)q->cq.chunk_a * a.S, *zb_tab = a.czrow + (int64_t)q->cq.chunk_b * a.S;
  const int lca = q->cq.lca;
  T acc = 0;
  acc = gate_walk<T, D, true, false>(a.meta, a.Z, za_tab, zb_tab, q->fa, lca, slice, NS, cola, colb, Ai, Aj, Bi, Bj, acc);
  acc = gate_walk<T, D, false, true>(a.meta, a.Z, za_tab, zb_tab, q->fb, lca, slice, NS, cola, colb, Ai, Aj, Bi, Bj, acc);
  if (lca >= 0) acc = gate_walk<T, D, true, true>(a.meta, a.Z, za_tab, zb_tab, lca, -1, slice, NS, cola, colb, Ai, Aj, Bi, Bj, acc);
  if (lane < 32) part[slice * 32 + lane] = acc;
  __syncthreads();
  if (tid < ntri) {
    T s = part[tid];
#pragma unroll
    for (int k = 1; k < NS; k++) s += part[k * 32 + tid];
    // w == 0 exactly (truncated least squares): the edge is not part of H and Omega_w^-1 does not exist -- R, r and d2 are NaN
    const T r = sw[0] == (T)0 ? (T)__builtin_nan("") : (T)q->cov[i * D + j] / sw[0] - s;
    sS[i * D + j] = r;
    sS[j * D + i] = r;
  }
  __syncthreads();
  if (a.rout && tid < de * de) a.rout[q->cq.ooff + tid] = (double)sS[(tid / de) * D + tid % de];   // both halves from the lower triangle
  __syncthreads();
  if (tid == 0) {
    const T w = sw[0];
    T tr = 0;   // trace(R Omega_w)
    for (int r = 0; r < de; r++)
      for (int c = 0; c < de; c++) tr = fma(sS[r * D + c], w * (T)q->info[c * D + r], tr);
    a.red[blockIdx.x] = (double)(tr / (T)de);
    // R = L L^T in place (lower triangle), y = L^-1 e, d2 = y^T y
    bool ok = true;
    T d2 = 0;
    for (int c = 0; c < de; c++) {
      T d = sS[c * D + c];
      for (int k = 0; k < c; k++) d = fma(-sS[c * D + k], sS[c * D + k], d);
      if (!(d > (T)0)) { ok = false; break; }
      const T l = sqrt(d), inv = (T)1 / l;
      sS[c * D + c] = l;
      for (int r = c + 1; r < de; r++) {
        T v = sS[r * D + c];
        for (int k = 0; k < c; k++) v = fma(-sS[r * D + k], sS[c * D + k], v);
        sS[r * D + c] = v * inv;
      }
      T y = se[c];
      for (int k = 0; k < c; k++) y = fma(-sS[c * D + k], se[k], y);
      y *= inv;
      se[c] = y;
      d2 = fma(y, y, d2);
    }
    a.d2[blockIdx.x] = ok ? (double)d2 : __builtin_nan("");
  }
}

// ---- joint compatibility of sets of candidate edges (rr_pgo_gate_joint)
//
// For a set of candidates c1 .. cm with stacked error e (D_s scalars) and G = [G_c1 .. G_cm], G_c = Z_a A_c^T + Z_b B_c^T:
//   S = blockdiag(Omega_c^-1) + G^T G,   S = L L^T,   y = L^-1 e,   d2 = y^T y,
//   prefix(k) = the sum of y^2 over the rows of the first k + 1 candidates = d2 of the set cut after candidate k.
// G has one row per pivot row of the fronts on the union of the root paths of the set's nodes.  The host lists those fronts
// in ascending front index and gives, per (front, candidate), the first Z row of `from` and of `to` there (-1: the front
// is not on that node's path, and the node's part of G_c is exactly zero).
//
// Determinism.  Row r of a front belongs to wave r % 8 whatever the set; a wave adds fma(G_r[i], G_r[j], acc) over its rows
// in the host's front order, and a candidate absent from a front contributes fma(0, x, acc) = acc.  So the bits of block
// (c, d) of S depend on the two candidates alone, not on the rest of the set, on its order or on the plan.  The Cholesky
// factorisation is left-looking, every dot product in ascending k: column c and y[c] depend on the leading (c + 1) x (c + 1)
// part of S and e alone, which makes the prefixes the distances of the truncated sets bit for bit.
constexpr int GJ_MAX_DIM = 48;                  // RR_PGO_GATE_JOINT_MAX_DIM
constexpr int GJ_MAX_CAND = 16;                 // RR_PGO_GATE_JOINT_MAX_CAND
constexpr int GJ_TILE = 6;                      // a lane accumulates a GJ_TILE x GJ_TILE tile of S: 8 x 8 tiles cover 48 x 48
constexpr int GJ_RB = 4;                        // rows of G a wave forms per step (their loads are in flight together)
constexpr int GJ_LD = GJ_MAX_DIM + 1;           // LDS row stride of S: lanes i and i + 1 of a column read 34 banks apart
static_assert(GJ_TILE * 8 == GJ_MAX_DIM, "lane (ti, tj) = (lane >> 3, lane & 7) owns tile (ti, tj)");

struct JointSet {
  int32_t cand0, m;               // the set's records: JointArgs::cand[cand0 .. cand0 + m)
  int32_t dim, n_front;           // D_s; fronts on the union of the root paths
  int64_t fptr;                   // into JointArgs::fnc: pivot columns of the set's fronts, ascending front index
  int64_t zptr;                   // into JointArgs::fz: [(front * m + candidate) * 2 + {0: from, 1: to}] first Z row, -1: absent
  int64_t soff;                   // offset of S (D_s x D_s, row-major) in sout
};
static_assert(sizeof(JointSet) == 40, "JointSet is one 40-byte record");

template <typename T> struct JointArgs {
  const JointSet *set;
  const GateCand *cand;           // cq.ca / cq.cb: the columns of the two nodes in their chunks
  const int32_t *fnc, *fz;
  const T *Z;
  const typename VecT<T>::V4 *pose;
  double *d2, *prefix, *sout;     // prefix: one per record of cand; sout null: S is not asked for
};

// LDS writes of a wave made visible to its other lanes (the wave runs in lockstep: no instruction but the waits)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One workgroup per set; D = 3 (a 2-D graph) or 6 (SE3).  Lanes c < m of wave 0 (and, SE3, of wave 1 for B) linearise the
// candidates.  Lane k < D_s of every wave forms G_r[k] for GJ_RB of the wave's rows into the wave's LDS vector, then lane
// (ti, tj), tj <= ti, adds the rows' outer products into its tile.  The eight waves' tiles are added in wave order, one turn
// each, into S in LDS; wave 0 factors S, lane = row, with e as row D_s of the same recurrence (that row of L is y).
template <typename T, int D, bool LM = false>
__global__ void __launch_bounds__(COV_THREADS) k_gate_joint(JointArgs<T> a) {
  constexpr int NS = COV_THREADS / 64, MD = GJ_MAX_DIM, LD = GJ_LD, TL = GJ_TILE, RB = GJ_RB, MC = GJ_MAX_CAND;
  __shared__ T sA[MC * D * D], sB[MC * D * D], se[MC * D], sS[(MD + 1) * LD], gw[NS * RB * MD];
  __shared__ int32_t s_c[MD], s_i[MD], s_o[MC + 1];   // stacked scalar -> candidate, error row; candidate -> first scalar
  const JointSet js = a.set[blockIdx.x];
  const GateCand *cq = a.cand + js.cand0;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
  const int m = js.m, Ds = js.dim;
  // ---- linearise; wave 2 lays the stacked vector out meanwhile
  if (lane < m && wave < (D == 3 ? 1 : 2))
    gate_linearize<T, D, LM>(cq + lane, a.pose, wave, se + lane * D, sA + lane * D * D, sB + lane * D * D);
  if (tid == 128) {
    int o = 0;
    for (int c = 0; c < m; c++) {
      const int de = gate_edge_dim<D, LM>(cq[c].kind);
      s_o[c] = o;
      for (int i = 0; i < de && o < MD; i++, o++) {   // (the host has checked D_s <= MD)
        s_c[o] = c;
        s_i[o] = i;
      }
    }
    s_o[m] = o;
  }
  __syncthreads();
  // ---- lane k < D_s: row i of A_c and B_c, the columns of c's nodes (the columns of B past d_b are zero: pose-landmark)
  const bool live = lane < Ds;
  const int c = live ? s_c[lane] : 0;
  T Ai[D], Bi[D];
  int cola[D], colb[D];
  {
    const int i = live ? s_i[lane] : 0, db = gate_to_dim<D, LM>(cq[c].kind);
#pragma unroll
    for (int k = 0; k < D; k++) {
      Ai[k] = live ? sA[c * D * D + i * D + k] : (T)0;
      Bi[k] = live ? sB[c * D * D + i * D + k] : (T)0;
      cola[k] = cq[c].cq.ca[k];
      colb[k] = cq[c].cq.cb[min(k, db - 1)];
    }
  }
  const int ti = lane >> 3, tj = lane & 7;
  const bool tile = tj <= ti && TL * ti < Ds;
  T acc[TL][TL];
#pragma unroll
  for (int x = 0; x < TL; x++)
#pragma unroll
    for (int y = 0; y < TL; y++) acc[x][y] = 0;
  T *gmine = gw + wave * RB * MD;
  const int32_t *fnc = a.fnc + js.fptr, *fz = a.fz + js.zptr;
  for (int fi = 0; fi < js.n_front; fi++) {
    const int nc = __builtin_amdgcn_readfirstlane(fnc[fi]);
    int za = -1, zb = -1;
    if (live) {
      const int32_t *p = fz + ((int64_t)fi * m + c) * 2;
      za = p[0];
      zb = p[1];
    }
    for (int r0 = wave; r0 < nc; r0 += NS * RB) {
      T g[RB];
#pragma unroll
      for (int q = 0; q < RB; q++) {
        const int r = r0 + NS * q;
        T v = 0;
        if (r < nc) {
          if (za >= 0) {
            const T *p = a.Z + (int64_t)(za + r) * TS_MC;
#pragma unroll
            for (int k = 0; k < D; k++) v = fma(p[cola[k]], Ai[k], v);
          }
          if (zb >= 0) {
            const T *p = a.Z + (int64_t)(zb + r) * TS_MC;
#pragma unroll
            for (int k = 0; k < D; k++) v = fma(p[colb[k]], Bi[k], v);
          }
        }
        g[q] = v;
      }
      if (lane < MD) {
#pragma unroll
        for (int q = 0; q < RB; q++) gmine[q * MD + lane] = g[q];
      }
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < RB; q++)
        if (r0 + NS * q < nc && tile) {
          T gi[TL], gj[TL];
#pragma unroll
          for (int x = 0; x < TL; x++) {
            gi[x] = gmine[q * MD + TL * ti + x];
            gj[x] = gmine[q * MD + TL * tj + x];
          }
#pragma unroll
          for (int x = 0; x < TL; x++)
#pragma unroll
            for (int y = 0; y < TL; y++) acc[x][y] = fma(gi[x], gj[y], acc[x][y]);
        }
      wave_lds_sync();   // the vector is rewritten by the next step
    }
  }
  // ---- the eight waves' tiles in wave order
  for (int w = 0; w < NS; w++) {
    if (wave == w && tile) {
#pragma unroll
      for (int x = 0; x < TL; x++)
#pragma unroll
        for (int y = 0; y < TL; y++) {
          T *d = sS + (TL * ti + x) * LD + TL * tj + y;
          *d = w == 0 ? acc[x][y] : *d + acc[x][y];
        }
    }
    __syncthreads();
  }
  // ---- Omega^-1 on the diagonal blocks; both halves of S from the lower triangle; e is row D_s
  for (int t = tid; t < Ds * Ds; t += COV_THREADS) {
    const int i = t / Ds, j = t - i * Ds;
    if (j <= i && s_c[i] == s_c[j]) sS[i * LD + j] += (T)cq[s_c[i]].cov[s_i[i] * D + s_i[j]];
  }
  __syncthreads();
  for (int t = tid; t < Ds * Ds; t += COV_THREADS) {
    const int i = t / Ds, j = t - i * Ds;
    if (j > i) sS[i * LD + j] = sS[j * LD + i];
  }
  if (tid < Ds) sS[Ds * LD + tid] = se[s_c[tid] * D + s_i[tid]];
  __syncthreads();
  if (a.sout)
    for (int t = tid; t < Ds * Ds; t += COV_THREADS) {
      const int i = t / Ds, j = t - i * Ds;
      a.sout[js.soff + t] = (double)sS[i * LD + j];
    }
  __syncthreads();
  // ---- S = L L^T in place, column by column, lane = row; row D_s of L is y = L^-1 e
  if (wave == 0) {
    const int i = lane;
    int fail = Ds;   // the first column with a non-positive pivot (Omega is checked on the host: rounding only)
    for (int col = 0; col < Ds; col++) {
      T v = 0;
      if (i >= col && i <= Ds) {
        v = sS[i * LD + col];
        for (int k = 0; k < col; k++) v = fma(-sS[i * LD + k], sS[col * LD + k], v);
      }
      const T d = __shfl(v, col);
      if (!(d > (T)0)) {
        fail = col;
        break;
      }
      const T l = sqrt(d), inv = (T)1 / l;
      if (i == col) sS[i * LD + col] = l;
      else if (i > col && i <= Ds) sS[i * LD + col] = v * inv;
      wave_lds_sync();
    }
    if (lane == 0) {
      T d2 = 0;
      for (int cc = 0, k = 0; cc < m; cc++) {
        for (; k < s_o[cc + 1]; k++) {
          const T y = sS[Ds * LD + k];
          d2 = fma(y, y, d2);
        }
        a.prefix[js.cand0 + cc] = s_o[cc + 1] <= fail ? (double)d2 : __builtin_nan("");
      }
      a.d2[blockIdx.x] = fail == Ds ? (double)d2 : __builtin_nan("");
    }
  }
}

// ---- Sigma[rows, cols] by a backward solve (rr_pgo_cross_covariances)
//
// With Z = L^-1 E_cols from k_tree_fwd, X = L^-T Z holds the columns Sigma[:, cols].  For front f with pivot rows P, rows
// below R and panel [L11; L21]:   X_P = L11^-T (Y_P - L21^T X_R),   Y_P = the front's rows of Z, X_R = rows of its ancestors'
// solution -- so X on a set of row nodes needs the fronts on their root paths only (the BACKWARD-ACTIVE fronts), root first.
// The set is the same for every chunk: one workgroup per (chunk, front of a level).
// Workspace.  V: per (chunk, backward-active front) its whole block [X_P; X_R], nc + nr rows of TS_MC scalars.  A child
// gathers its X_R as V_parent[rel[r]] -- the extend-add map read backwards, the mirror image of U in k_tree_fwd.
//
// Determinism.  No atomics.  Every scalar of V is produced by one wave in an operation order that depends on the front and
// the row alone: columns of an MFMA tile are independent, X_R is a copy of the parent's scalars, the products over the rows
// below run in ascending row order and the pivot blocks from the right in a fixed order.  A front's block depends on Z and
// on its ancestors' blocks only, never on which other fronts are backward-active, and a front that the forward plan of the
// chunk does not hold reads Y_P = 0, which is what k_tree_fwd leaves in a column whose node lies elsewhere.  Hence the bits
// of Sigma(r, c) depend on the graph, the state, r and c alone: not on the other rows or columns of the call, their order,
// repeats, the chunk a column falls in or a cut of the plan.
template <typename T> struct TsBwdArgs {
  const TsMeta *meta;
  const int32_t *order;           // the backward-active fronts by level, root level first
  const int32_t *fvrow;           // [front]: first row of the front's block in a chunk's part of V, -1 = not backward-active
  const int32_t *czrow;           // as CovArgs
  const int32_t *rel;
  const T *lvals, *winv, *Z;
  T *V;
  int64_t vrows;                  // rows of V per chunk
  int32_t S;
};

// The block [T_P; X_R], (nc + nr) x TS_MC, lives in LDS (row stride TS_LD) as in k_tree_fwd; L^T goes from lvals in global
// memory straight into the A operands: A(i, k) = L(k, i), a lane's four k are consecutive scalars of one panel column.
template <typename T>
__global__ void __launch_bounds__(TS_THREADS) k_tree_bwd(TsBwdArgs<T> a, int begin) {
  using MM = Mfma16<T>;
  constexpr int NW = TS_THREADS / 64, LD = TS_LD, NCT = TS_MC / 16;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  __shared__ T ws[256];                  // W_b: ws[k * 16 + i] = W(k, i) = W^T(i, k)
  T *B = reinterpret_cast<T *>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = wave_index();
  const int f = a.order[begin + blockIdx.x], chunk = blockIdx.y;
  const TsMeta m = a.meta[f];
  const int nc = m.nc, nr = m.nr, n = nc + nr, M = n + 1;
  const T *Lg = a.lvals + m.loff;
  const T *Wg = a.winv + (int64_t)m.wblk * 256;
  const int64_t vbase = (int64_t)chunk * a.vrows;
  // ---- Y_P: the front's rows of Z where the chunk's forward plan holds the front, else zero
  {
    const int zr = a.czrow[(int64_t)chunk * a.S + f];
    const T *Zg = a.Z + (int64_t)max(zr, 0) * TS_MC;
    for (int e = tid; e < nc * TS_MC; e += TS_THREADS) B[(e >> 5) * LD + (e & 31)] = zr >= 0 ? Zg[e] : (T)0;
  }
  // ---- X_R: the parent's block through this front's rel map (a root has no rows below)
  if (nr > 0) {
    const int p = m.parent;
    const int pn = p >= 0 ? a.meta[p].nc + a.meta[p].nr : 0;
    const T *Vp = a.V + (vbase + (p >= 0 ? a.fvrow[p] : 0)) * TS_MC;
    const int32_t *rel = a.rel + m.rel_ptr;
    for (int e = tid; e < nr * TS_MC; e += TS_THREADS) {
      const int row = rel[e >> 5];
      B[(nc + (e >> 5)) * LD + (e & 31)] = (unsigned)row < (unsigned)pn ? Vp[(int64_t)row * TS_MC + (e & 31)] : (T)0;
    }
  }
  __syncthreads();
  // ---- T = Y_P - L21^T X_R: a tile of 16 pivot rows x 16 columns is one wave's, the rows below in ascending order
  if (nr > 0) {
    const int nti = (nc + 15) >> 4;
    for (int tile = wave; tile < nti * NCT; tile += NW) {
      const int ib = tile / NCT, jb = tile - ib * NCT;
      const int i0 = 16 * ib, col = 16 * jb + li;
      typename MM::Acc acc;
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = B[min(i0 + MM::row(lane, r), nc - 1) * LD + col];
      const T *Lc = Lg + (int64_t)min(i0 + li, nc - 1) * M + nc;   // rows past nc of the last tile are computed and dropped
      for (int k4 = 0; k4 < nr; k4 += 4) {
        const int k = k4 + lk, kc = min(k, nr - 1);
        const T lv = Lc[kc];
        acc = MM::mma(k < nr ? -lv : (T)0, B[(nc + kc) * LD + col], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = i0 + MM::row(lane, r);
        if (row < nc) B[row * LD + col] = acc[r];
      }
    }
    __syncthreads();
  }
  // ---- pivot square, by 16-column blocks from the right: X_b = W_b^T T_b, then T_j -= L_bj^T X_b for the earlier blocks
  for (int b = ((nc + 15) >> 4) - 1; b >= 0; b--) {
    const int c0 = 16 * b, cw = min(16, nc - c0);
    if (tid < 256) ws[tid] = Wg[b * 256 + tid];
    __syncthreads();
    if (wave < NCT) {   // a column tile of the block is one wave's: read whole, then written
      const int col = 16 * wave + li;
      typename MM::Acc x = {0, 0, 0, 0};
      T bv[4];
#pragma unroll
      for (int s = 0; s < 4; s++) bv[s] = B[(c0 + min(4 * s + lk, cw - 1)) * LD + col];
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int k = 4 * s + lk;
        const T wv = (li <= k && k < cw) ? ws[k * 16 + li] : (T)0;   // W^T is upper triangular; rows past a partial block are padding
        x = MM::mma(wv, k < cw ? bv[s] : (T)0, x);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = MM::row(lane, r);
        if (i < cw) B[(c0 + i) * LD + col] = x[r];
      }
    }
    __syncthreads();
    for (int tile = wave; tile < b * NCT; tile += NW) {   // (the earlier blocks are full ones)
      const int ib = tile / NCT, jb = tile - ib * NCT;
      const int i0 = 16 * ib, col = 16 * jb + li;
      typename MM::Acc acc;
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = B[(i0 + MM::row(lane, r)) * LD + col];
      const T *Lc = Lg + (int64_t)(i0 + li) * M + c0;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int k = 4 * s + lk, kc = min(k, cw - 1);
        const T lv = Lc[kc];
        acc = MM::mma(k < cw ? -lv : (T)0, B[(c0 + kc) * LD + col], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) B[(i0 + MM::row(lane, r)) * LD + col] = acc[r];
    }
    __syncthreads();
  }
  // ---- V = [X_P; X_R], what the children gather from
  T *Vg = a.V + (vbase + a.fvrow[f]) * TS_MC;
  for (int e = tid; e < n * TS_MC; e += TS_THREADS) Vg[e] = B[(e >> 5) * LD + (e & 31)];
}

// ---- fronts beyond LDS (rr_pgo_set_query_big_fronts)
//
// The right-hand block of such a front does not fit in LDS beside nothing: it lives where the plan puts it anyway, its nc
// pivot rows in Z (forward) and its nr rows below in U, or its nc + nr rows in V (backward).  The panel is addressed as an
// LDS front's is; the inverses of its diagonal blocks are 32 x 32: winv[wblk * 256 + b * 1024 + c * 32 + j] = W_b(j, c).
//
//   k_tree_fwd_big         one workgroup per (chunk, active front): zero, gather the children, unit entries, pivot square
//   k_tree_fwd_big_update  one workgroup per (chunk, front, slab of TSB_SLAB rows below): U = B_R - L_21 Y_P
//   k_tree_bwd_big_gemv    one workgroup per (chunk, front, slab of TSB_SLAB pivot rows): T = Y_P - L_21^T X_R into V
//   k_tree_bwd_big         one workgroup per (chunk, front): the pivot square from the right, and X_R into V
// A level of the tree is the launch of its LDS fronts as before, then these for its fronts beyond LDS.  Only launches order
// the work: a kernel reads what an earlier launch wrote, or what its own workgroup wrote behind a __syncthreads().
//
// Determinism.  As above: a scalar of Z, U or V is one wave's, blocks ascend going forward and descend going backward, k
// ascends inside a block and over the rows below, children come in ascending front order.  A tile's wave and a slab's
// workgroup are chosen by the row alone, and neither enters the order of the row's operations.
constexpr int TSB_THREADS = 512;
constexpr int TSB_SLAB = 16 * (TSB_THREADS / 64);   // rows of a slab: one 16-row tile per wave, both column tiles
constexpr int TSB_KP = 64;                          // rows below staged in LDS per piece (k_tree_bwd_big_gemv)
static_assert(TSB_KP % 4 == 0, "a piece is whole MFMA steps, so the pieces do not change how k is grouped");

struct TsSlab {
  int32_t item;                   // forward: the task; backward: the front
  int32_t row0;                   // first row of the slab among the rows below (forward) / the pivot rows (backward)
};

template <typename T>
__global__ void __launch_bounds__(TSB_THREADS) k_tree_fwd_big(TsArgs<T> a, int begin) {
  using MM = Mfma16<T>;
  constexpr int NW = TSB_THREADS / 64, LD = TS_LD, NCT = TS_MC / 16;
  __shared__ T ws[1024];                 // W_b: ws[c * 32 + j] = W_b(j, c)
  __shared__ T yb[32 * LD];              // Y_b, the B operand of the block's updates
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = wave_index();
  const TsTask t = a.tasks[begin + blockIdx.x];
  const TsMeta m = a.meta[t.front];
  const int nc = m.nc, nr = m.nr, n = nc + nr, M = n + 1;
  const T *Lg = a.lvals + m.loff;
  const T *Wg = a.winv + (int64_t)m.wblk * 256;
  T *Zg = a.Z + (int64_t)t.zrow * TS_MC, *Ug = a.U + (int64_t)t.urow * TS_MC;
  for (int e = tid; e < nc * TS_MC; e += TSB_THREADS) Zg[e] = 0;
  for (int e = tid; e < nr * TS_MC; e += TSB_THREADS) Ug[e] = 0;
  __syncthreads();
  // ---- the update blocks of the active children through their rel maps, one child after the other
  for (int c = 0; c < t.n_child; c++) {
    const TsTask ct = a.tasks[a.child[t.child_ptr + c]];
    const TsMeta cm = a.meta[ct.front];
    const int32_t *rel = a.rel + cm.rel_ptr;
    const T *Uc = a.U + (int64_t)ct.urow * TS_MC;
    for (int e = tid; e < cm.nr * TS_MC; e += TSB_THREADS) {
      const int row = rel[e >> 5];
      if ((unsigned)row < (unsigned)n) {
        T *d = row < nc ? Zg + (int64_t)row * TS_MC : Ug + (int64_t)(row - nc) * TS_MC;
        d[e & 31] += Uc[e];
      }
    }
    __syncthreads();
  }
  // ---- unit entries of the chunk's nodes whose pivot columns are here
  for (int e = tid; e < t.n_unit; e += TSB_THREADS) {
    const int u = a.unit[t.unit_ptr + e];
    Zg[(int64_t)(u >> 5) * TS_MC + (u & 31)] += (T)1;
  }
  __syncthreads();
  // ---- pivot square, right-looking by 32-column blocks: Y_b = W_b B_b, then B_i -= L_ib Y_b for the later pivot rows
  for (int b = 0; b < ((nc + 31) >> 5); b++) {
    const int c0 = 32 * b, cw = min(32, nc - c0), t0 = c0 + 32;
    for (int e = tid; e < 1024; e += TSB_THREADS) ws[e] = Wg[(int64_t)b * 1024 + e];
    __syncthreads();
    if (wave < NCT) {   // a column tile of the block is one wave's: read whole, then written
      const int col = 16 * wave + li;
      typename MM::Acc y0 = {0, 0, 0, 0}, y1 = {0, 0, 0, 0};
      T bv[8];
#pragma unroll
      for (int s = 0; s < 8; s++) bv[s] = Zg[(int64_t)(c0 + min(4 * s + lk, cw - 1)) * TS_MC + col];
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const int k = 4 * s + lk;
        const T bk = k < cw ? bv[s] : (T)0;
        // W is lower triangular; rows past a partial block are padding
        y0 = MM::mma((k <= li && li < cw) ? ws[k * 32 + li] : (T)0, bk, y0);
        y1 = MM::mma((k <= 16 + li && 16 + li < cw) ? ws[k * 32 + 16 + li] : (T)0, bk, y1);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = MM::row(lane, r);
        yb[i * LD + col] = y0[r];
        yb[(16 + i) * LD + col] = y1[r];
        if (i < cw) Zg[(int64_t)(c0 + i) * TS_MC + col] = y0[r];
        if (16 + i < cw) Zg[(int64_t)(c0 + 16 + i) * TS_MC + col] = y1[r];
      }
    }
    __syncthreads();
    if (t0 < nc) {   // (so this block is a full one)
      const int nti = (nc - t0 + 15) >> 4;
      for (int tile = wave; tile < nti * NCT; tile += NW) {
        const int ib = tile / NCT, jb = tile - ib * NCT;
        const int i0 = t0 + 16 * ib, col = 16 * jb + li;
        typename MM::Acc acc;
#pragma unroll
        for (int r = 0; r < 4; r++) acc[r] = Zg[(int64_t)min(i0 + MM::row(lane, r), nc - 1) * TS_MC + col];
        const T *La = Lg + (int64_t)c0 * M + min(i0 + li, nc - 1);   // rows past nc of the last tile are computed and dropped
        T lv[8];
#pragma unroll
        for (int s = 0; s < 8; s++) lv[s] = La[(int64_t)(4 * s + lk) * M];
#pragma unroll
        for (int s = 0; s < 8; s++) acc = MM::mma(-lv[s], yb[(4 * s + lk) * LD + col], acc);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = i0 + MM::row(lane, r);
          if (row < nc) Zg[(int64_t)row * TS_MC + col] = acc[r];
        }
      }
    }
    __syncthreads();
  }
}

// The rows below of one slab: a wave holds 16 rows x TS_MC columns in two accumulators over all nc columns of the panel and
// writes them once.  L goes from lvals straight into the A operand, Y_P from the front's rows of Z into the B operands.
template <typename T>
__global__ void __launch_bounds__(TSB_THREADS) k_tree_fwd_big_update(TsArgs<T> a, const TsSlab *slab, int begin) {
  using MM = Mfma16<T>;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const TsSlab s = slab[begin + blockIdx.x];
  const TsTask t = a.tasks[s.item];
  const TsMeta m = a.meta[t.front];
  const int nc = m.nc, nr = m.nr, M = nc + nr + 1;
  const int r0 = s.row0 + 16 * wave_index();
  if (r0 >= nr) return;   // (no barrier below)
  const T *Lg = a.lvals + m.loff;
  const T *Zg = a.Z + (int64_t)t.zrow * TS_MC;
  T *Ug = a.U + (int64_t)t.urow * TS_MC;
  typename MM::Acc acc0, acc1;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const T *u = Ug + (int64_t)min(r0 + MM::row(lane, r), nr - 1) * TS_MC;
    acc0[r] = u[li];
    acc1[r] = u[16 + li];
  }
  const T *La = Lg + nc + min(r0 + li, nr - 1);   // rows past nr of the last tile are computed and dropped
  for (int k4 = 0; k4 < nc; k4 += 4) {
    const int k = k4 + lk, kc = min(k, nc - 1);
    const T lv = La[(int64_t)kc * M];
    const T av = k < nc ? -lv : (T)0;
    const T *z = Zg + (int64_t)kc * TS_MC;
    acc0 = MM::mma(av, z[li], acc0);
    acc1 = MM::mma(av, z[16 + li], acc1);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = r0 + MM::row(lane, r);
    if (row < nr) {
      Ug[(int64_t)row * TS_MC + li] = acc0[r];
      Ug[(int64_t)row * TS_MC + 16 + li] = acc1[r];
    }
  }
}

// T = Y_P - L21^T X_R for one slab of pivot rows, into the front's pivot rows of V.  X_R is gathered from the parent's block
// through the rel map, TSB_KP rows below at a time, into LDS; A(i, k) = L(nc + k, i): a lane's consecutive k are consecutive
// scalars of one panel column.  A root (no rows below) copies Y_P.
template <typename T>
__global__ void __launch_bounds__(TSB_THREADS) k_tree_bwd_big_gemv(TsBwdArgs<T> a, const TsSlab *slab, int begin) {
  using MM = Mfma16<T>;
  constexpr int LD = TS_LD;
  __shared__ T xs[TSB_KP * LD];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const TsSlab s = slab[begin + blockIdx.x];
  const int f = s.item, chunk = blockIdx.y;
  const TsMeta m = a.meta[f];
  const int nc = m.nc, nr = m.nr, M = nc + nr + 1;
  const int64_t vbase = (int64_t)chunk * a.vrows;
  T *Vf = a.V + (vbase + a.fvrow[f]) * TS_MC;
  const int i0 = s.row0 + 16 * wave_index();
  const bool mine = i0 < nc;   // (every wave stages X_R)
  typename MM::Acc acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  // ---- Y_P: the front's rows of Z where the chunk's forward plan holds the front, else zero
  const int zr = a.czrow[(int64_t)chunk * a.S + f];
  if (mine && zr >= 0) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const T *z = a.Z + (int64_t)(zr + min(i0 + MM::row(lane, r), nc - 1)) * TS_MC;
      acc0[r] = z[li];
      acc1[r] = z[16 + li];
    }
  }
  const int p = m.parent;
  const int pn = p >= 0 ? a.meta[p].nc + a.meta[p].nr : 0;
  const T *Vp = a.V + (vbase + (p >= 0 ? a.fvrow[p] : 0)) * TS_MC;
  const int32_t *rel = a.rel + m.rel_ptr;
  const T *Lc = a.lvals + m.loff + (int64_t)min(i0 + li, nc - 1) * M + nc;   // rows past nc of the last tile are computed and dropped
  for (int k0 = 0; k0 < nr; k0 += TSB_KP) {
    const int kp = min(TSB_KP, nr - k0);
    if (k0 > 0) __syncthreads();   // the piece before has been read
    for (int e = tid; e < kp * TS_MC; e += TSB_THREADS) {
      const int row = rel[k0 + (e >> 5)];
      xs[(e >> 5) * LD + (e & 31)] = (unsigned)row < (unsigned)pn ? Vp[(int64_t)row * TS_MC + (e & 31)] : (T)0;
    }
    __syncthreads();
    if (mine)
      for (int k4 = 0; k4 < kp; k4 += 4) {
        const int k = k4 + lk, kc = min(k, kp - 1);
        const T lv = Lc[k0 + kc];
        const T av = k < kp ? -lv : (T)0;
        acc0 = MM::mma(av, xs[kc * LD + li], acc0);
        acc1 = MM::mma(av, xs[kc * LD + 16 + li], acc1);
      }
  }
  if (mine) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = i0 + MM::row(lane, r);
      if (row < nc) {
        Vf[(int64_t)row * TS_MC + li] = acc0[r];
        Vf[(int64_t)row * TS_MC + 16 + li] = acc1[r];
      }
    }
  }
}

// The pivot rows of V hold T (k_tree_bwd_big_gemv).  By 32-column blocks from the right: X_b = W_b^T T_b, then
// T_j -= L_bj^T X_b for the earlier blocks; the rows below are copied from the parent's block, so V = [X_P; X_R] is what a
// child -- in LDS or beyond -- gathers from.
template <typename T>
__global__ void __launch_bounds__(TSB_THREADS) k_tree_bwd_big(TsBwdArgs<T> a, int begin) {
  using MM = Mfma16<T>;
  constexpr int NW = TSB_THREADS / 64, LD = TS_LD, NCT = TS_MC / 16;
  __shared__ T ws[1024];                 // W_b: ws[c * 32 + j] = W_b(j, c) = W_b^T(c, j)
  __shared__ T xb[32 * LD];              // X_b, the B operand of the block's updates
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = wave_index();
  const int f = a.order[begin + blockIdx.x], chunk = blockIdx.y;
  const TsMeta m = a.meta[f];
  const int nc = m.nc, nr = m.nr, M = nc + nr + 1;
  const T *Lg = a.lvals + m.loff;
  const T *Wg = a.winv + (int64_t)m.wblk * 256;
  const int64_t vbase = (int64_t)chunk * a.vrows;
  T *Vf = a.V + (vbase + a.fvrow[f]) * TS_MC;
  // ---- X_R: the parent's block through this front's rel map (a root has no rows below)
  if (nr > 0) {
    const int p = m.parent;
    const int pn = p >= 0 ? a.meta[p].nc + a.meta[p].nr : 0;
    const T *Vp = a.V + (vbase + (p >= 0 ? a.fvrow[p] : 0)) * TS_MC;
    const int32_t *rel = a.rel + m.rel_ptr;
    for (int e = tid; e < nr * TS_MC; e += TSB_THREADS) {
      const int row = rel[e >> 5];
      Vf[(int64_t)nc * TS_MC + e] = (unsigned)row < (unsigned)pn ? Vp[(int64_t)row * TS_MC + (e & 31)] : (T)0;
    }
  }
  for (int b = ((nc + 31) >> 5) - 1; b >= 0; b--) {
    const int c0 = 32 * b, cw = min(32, nc - c0);
    for (int e = tid; e < 1024; e += TSB_THREADS) ws[e] = Wg[(int64_t)b * 1024 + e];
    __syncthreads();
    if (wave < NCT) {   // a column tile of the block is one wave's: read whole, then written
      const int col = 16 * wave + li;
      typename MM::Acc x0 = {0, 0, 0, 0}, x1 = {0, 0, 0, 0};
      T bv[8];
#pragma unroll
      for (int s = 0; s < 8; s++) bv[s] = Vf[(int64_t)(c0 + min(4 * s + lk, cw - 1)) * TS_MC + col];
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const int k = 4 * s + lk;
        const T bk = k < cw ? bv[s] : (T)0;
        // W^T is upper triangular; rows past a partial block are padding
        x0 = MM::mma((li <= k && k < cw) ? ws[li * 32 + k] : (T)0, bk, x0);
        x1 = MM::mma((16 + li <= k && k < cw) ? ws[(16 + li) * 32 + k] : (T)0, bk, x1);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = MM::row(lane, r);
        xb[i * LD + col] = x0[r];
        xb[(16 + i) * LD + col] = x1[r];
        if (i < cw) Vf[(int64_t)(c0 + i) * TS_MC + col] = x0[r];
        if (16 + i < cw) Vf[(int64_t)(c0 + 16 + i) * TS_MC + col] = x1[r];
      }
    }
    __syncthreads();
    for (int tile = wave; tile < 2 * b * NCT; tile += NW) {   // (the earlier blocks are full ones)
      const int ib = tile / NCT, jb = tile - ib * NCT;
      const int i0 = 16 * ib, col = 16 * jb + li;
      typename MM::Acc acc;
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = Vf[(int64_t)(i0 + MM::row(lane, r)) * TS_MC + col];
      const T *Lc = Lg + (int64_t)(i0 + li) * M + c0;
      T lv[8];
#pragma unroll
      for (int s = 0; s < 8; s++) lv[s] = Lc[min(4 * s + lk, cw - 1)];
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const int k = 4 * s + lk;
        acc = MM::mma(k < cw ? -lv[s] : (T)0, xb[k * LD + col], acc);   // (rows of X_b past cw are zero)
      }
#pragma unroll
      for (int r = 0; r < 4; r++) Vf[(int64_t)(i0 + MM::row(lane, r)) * TS_MC + col] = acc[r];
    }
    __syncthreads();
  }
}

template <typename T> struct CrossArgs {
  const T *V;
  const int32_t *rsrc;            // [R]: row of out -> row of the node's scalar in a chunk's part of V, -1 = a fixed node
  const int64_t *csrc;            // [C]: column of out -> flat offset of (chunk, column) in V, -1 = a fixed node
  double *out;                    // R x C, row-major
  int64_t R, C;
};

// One thread per scalar of out; every entry of a fixed node's rows and columns is +0.0 (Sigma is conditional on them).
template <typename T>
__global__ void __launch_bounds__(256) k_cross_gather(CrossArgs<T> a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.R * a.C) return;
  const int64_t i = t / a.C, j = t - i * a.C;
  const int32_t r = a.rsrc[i];
  const int64_t c = a.csrc[j];
  a.out[t] = (r < 0 || c < 0) ? 0.0 : (double)a.V[c + (int64_t)r * TS_MC];
}

}  // namespace rrpgo
