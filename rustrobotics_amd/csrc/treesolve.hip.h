// treesolve.hip.h -- covariances of arbitrary node pairs from a multi-column forward solve over the supernode tree
// (rr_pgo_covariances).
//
// With H = L L^T, Sigma_ab = Z_a^T Z_b where Z_s = L^-1 E_s and E_s holds the unit columns of node s.  Z_s is non-zero only
// on the pivot rows of the fronts on the path from the front of s to the root, so a set of right-hand columns touches only
// the union of those paths (the ACTIVE fronts), and a pair (a, b) needs only the rows from the lowest common front up.
//
//   k_tree_fwd    one workgroup per (chunk of TS_MC columns, active front), one launch per level of the tree, deepest first
//   k_cov_pairs   one workgroup per query: Sigma_ab = sum over the common path's pivot rows of Z_a[row]^T Z_b[row]
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
constexpr size_t TS_WS_BYTES = (size_t)512 << 20;   // bound of Z + U of one pass
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

}  // namespace rrpgo
