// selinv.hip.h -- marginal covariances from the factor: the multifrontal selected inverse.
//
// After a factorisation H = L L^T the entries of Sigma = H^-1 on the pattern of L follow from the Takahashi recursion,
// top-down over the supernode tree.  For a 16-column block b of a front, with T = the front's later pivot columns and its
// rows below (rhs row excluded) and W_b = L_bb^-1 (kept in winv by the factorisation):
//     Y = L_Tb W_b,     Sigma_Tb = -Sigma_TT Y,     Sigma_bb = W_b^T W_b - Y^T Sigma_Tb = W_b^T (W_b - L_Tb^T Sigma_Tb)
// Sigma_TT is known by then: the later blocks of the same front, and Sigma_RR of the rows below, which is a subset of the
// parent's result (the child's `rel` map, the one the extend-add uses, read backwards).
//
//   k_selinv_level   one workgroup per front, one launch per level of the supernode tree, root level first
//   k_marg_gather    queried entries -> the caller's f64 array
//
// A front's image in svals: panel (nc + nr) x nc, column-major (rows = pivot columns then rows below; of the pivot square
// only the lower triangle is defined), then the packed lower triangle of Sigma_RR -- the footprint of the factor image
// less its rhs row, so it fits the LDS budget the front was planned for.
#pragma once
#include "kernels.hip.h"

namespace rrpgo {

struct SelMeta {
  int32_t nc, nr, wblk, has_parent;   // pivot columns, rows below, first W block in winv
  int32_t pnc, pn, pad0, pad1;        // parent: pivot columns, nc + nr
  int64_t loff, soff, psoff, rel_ptr; // panel in lvals, image in svals, the parent's image, the front's rel map
};
static_assert(sizeof(SelMeta) == 64, "SelMeta is one 64-byte record");

template <typename T> struct SelArgs {
  const SelMeta *meta;
  const int32_t *order;   // fronts by level, root level first
  const int32_t *rel;
  const T *lvals, *winv;
  T *svals;
};

constexpr int SELINV_THREADS = 1024;
constexpr int SELINV_TILES_PER_WAVE = 2;   // 16-row tiles of Sigma_Tb one wave keeps in registers across the barrier
constexpr int SELINV_MAX_ROWS = 16 * SELINV_TILES_PER_WAVE * (SELINV_THREADS / 64);
constexpr int SELINV_GPART = 4;            // waves that share the L_Tb^T Sigma_Tb product

__device__ __forceinline__ int packed_lower(int n, int i, int j) { return j * n - ((j * (j - 1)) >> 1) + (i - j); }   // i >= j

template <typename T, int THREADS>
__global__ void __launch_bounds__(THREADS) k_selinv_level(SelArgs<T> a, int begin) {
  using MM = Mfma16<T>;
  constexpr int NW = THREADS / 64;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  __shared__ T ws[256];                  // W_b: ws[j * 16 + c] = W(j, c)
  __shared__ T gs[SELINV_GPART * 256];   // partial sums of G = L_Tb^T Sigma_Tb: [part][c * 16 + d]
  T *P = reinterpret_cast<T *>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = wave_index();
  const SelMeta m = a.meta[a.order[begin + blockIdx.x]];
  const int nc = m.nc, nr = m.nr, n = nc + nr, M = n + 1;
  T *U = P + n * nc;
  const T *Lg = a.lvals + m.loff;
  const T *Wg = a.winv + (int64_t)m.wblk * 256;
  for (int t = tid; t < n * nc; t += THREADS) P[t] = 0;
  // ---- Sigma_RR from the parent's image
  if (m.has_parent && nr > 0) {
    const T *Sp = a.svals + m.psoff;
    const int32_t *rel = a.rel + m.rel_ptr;
    const int pnc = m.pnc, pn = m.pn, pnr = pn - pnc;
    for (int t = tid; t < nr * nr; t += THREADS) {
      const int j = t / nr, i = t - j * nr;
      if (i < j) continue;
      const int pi = rel[i], pj = rel[j];
      const int hi = max(pi, pj), lo = min(pi, pj);
      U[packed_lower(nr, i, j)] = lo < pnc ? Sp[(int64_t)lo * pn + hi] : Sp[(int64_t)pn * pnc + packed_lower(pnr, hi - pnc, lo - pnc)];
    }
  }
  __syncthreads();
  auto sig = [&](int i, int k) -> T {   // Sigma(i, k) of this front, local indices, both already known
    const int hi = max(i, k), lo = min(i, k);
    return lo < nc ? P[lo * n + hi] : U[packed_lower(nr, hi - nc, lo - nc)];
  };
  for (int b = ((nc + 15) >> 4) - 1; b >= 0; b--) {
    const int c0 = 16 * b, cw = min(16, nc - c0), t0 = c0 + cw, nT = n - t0;
    if (tid < 256) ws[tid] = Wg[b * 256 + tid];
    __syncthreads();
    // ---- Y = L_Tb W_b into the place of Sigma_Tb
    for (int t = tid; t < nT * cw; t += THREADS) {
      const int c = t / nT, i = t0 + (t - c * nT);
      T y = 0;
      for (int j = c; j < cw; j++) y += Lg[(int64_t)(c0 + j) * M + i] * ws[j * 16 + c];
      P[(c0 + c) * n + i] = y;
    }
    __syncthreads();
    // ---- Sigma_Tb = -Sigma_TT Y on 16 x 16 tiles, transposed (D[c][i] = sum_k Y(k, c) Sigma(k, i): a lane's results are
    // four columns c of one row i); kept in registers until every wave is done with Y
    typename MM::Acc acc[SELINV_TILES_PER_WAVE];
    const int ntile = (nT + 15) >> 4;
    const int yc = (c0 + min(li, cw - 1)) * n;   // column of Y this lane feeds (rows c >= cw of D are never stored)
#pragma unroll
    for (int q = 0; q < SELINV_TILES_PER_WAVE; q++) {
      acc[q] = typename MM::Acc{0, 0, 0, 0};
      const int ib = wave + q * NW;
      if (ib < ntile) {
        const int ic = min(t0 + 16 * ib + li, n - 1);
        for (int k4 = 0; k4 < nT; k4 += 4) {
          const int k = t0 + k4 + lk, kc = min(k, n - 1);
          const T yv = P[yc + kc];
          const T sv = sig(ic, kc);
          acc[q] = MM::mma(k < n ? yv : (T)0, sv, acc[q]);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SELINV_TILES_PER_WAVE; q++) {
      const int i = t0 + 16 * (wave + q * NW) + li;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int c = MM::row(lane, r);
        if (i < n && c < cw) P[(c0 + c) * n + i] = -acc[q][r];
      }
    }
    __syncthreads();
    // ---- G = L_Tb^T Sigma_Tb (D[c][d] = sum_i L(i, c0 + c) Sigma(i, c0 + d)): four waves take every fourth k-step
    if (wave < SELINV_GPART) {
      typename MM::Acc g = {0, 0, 0, 0};
      const int cc = c0 + min(li, cw - 1);
      for (int k4 = 4 * wave; k4 < nT; k4 += 4 * SELINV_GPART) {
        const int i = t0 + k4 + lk, ic = min(i, n - 1);
        const T lv = Lg[(int64_t)cc * M + ic];
        const T sv = P[cc * n + ic];
        g = MM::mma(i < n ? lv : (T)0, sv, g);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) gs[wave * 256 + MM::row(lane, r) * 16 + li] = g[r];
    }
    __syncthreads();
    // ---- Sigma_bb = W^T (W - G), lower triangle
    if (tid < 256) {
      const int c = tid >> 4, d = tid & 15;
      if (c < cw && d <= c) {
        T s = 0;
        for (int j = c; j < cw; j++) {
          const int e = j * 16 + d;
          const T gj = ((gs[e] + gs[256 + e]) + gs[512 + e]) + gs[768 + e];
          s += ws[j * 16 + c] * (ws[e] - gj);
        }
        P[(c0 + d) * n + c0 + c] = s;
      }
    }
    __syncthreads();
  }
  T *Sg = a.svals + m.soff;
  const int total = n * nc + ((nr * (nr + 1)) >> 1);
  for (int t = tid; t < total; t += THREADS) Sg[t] = P[t];
}
static_assert(SELINV_GPART == 4, "the sum of the partial products in k_selinv_level is written out for four parts");

// out[t] = svals[src[t]]: the host lists, per output scalar, where it lives (symmetric fill of diagonal blocks and the
// permutation back to the reference's scalar order within a node are in the list); src < 0: the entry is 0 (a block with a
// fixed node of rr_pgo_set_fixed: the covariance is conditional on that node)
template <typename T>
__global__ void __launch_bounds__(256) k_marg_gather(const T *svals, const int64_t *src, double *out, int64_t count) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < count) out[t] = src[t] < 0 ? 0.0 : (double)svals[src[t]];
}

// ---- fronts beyond LDS (rr_pgo_set_marginals_big_fronts)
//
// Such a front's image does not fit in one workgroup's LDS: the recursion works on the image in svals itself, in the
// supernodal form.  With Z = L_PP^-1 and Y = L_RP Z:
//     Sigma_RP = -Sigma_RR Y,     Sigma_PP = Z^T Z - Y^T Sigma_RP
// The inverses of the front's diagonal blocks are 32 x 32 (treesolve.hip.h): winv[wblk * 256 + b * 1024 + c * 32 + j] =
// W_b(j, c), an identity past a partial last block.  Z (nc x nc, the block rows on and below the diagonal) and Y (nr x nc)
// live in a workspace, both row-major with leading dimension nc.
//
// What needs nothing from a parent goes ahead of the tree's levels, ONE launch each for all such fronts:
//   k_selinv_big_z    one workgroup per (front, 32-row block b of Z): Z_bb = W_b, then Z_bj = -(sum_{j<k<=b} Z_bk L_kj) W_j
//                     for j descending.  Reads lvals and winv only
//   k_selinv_big_y    (front, 128 rows below, 32 columns): Y = L_RP Z
//   k_selinv_big_zz   (front, 128 pivot rows, 32 columns): Z^T Z into the place of Sigma_PP, lower triangle -- all there is
//                     to a root front
// A level of the tree is then k_selinv_level for its LDS fronts and, for its fronts beyond LDS with rows below,
//   k_selinv_big_rp   (front, 16 rows below, 256 columns): Sigma_RP = -Sigma_RR Y, the strip of Sigma_RR staged in LDS from the
//                     parent's image through the rel map (the lo / hi rule of k_selinv_level) and copied into the front's
//                     own image, where its children look for it
//   k_selinv_big_pp   (front, 128 pivot rows, 32 columns): Sigma_PP -= Y^T Sigma_RP, lower triangle
// Only launches order the work: a kernel reads what an earlier launch wrote, or what its own workgroup wrote behind a
// __syncthreads() (k_selinv_big_z: the blocks of its row of Z; k_selinv_big_rp: the strip in LDS).  No flags, no waits
// between workgroups, no atomics.
//
// Determinism.  Every stored scalar is one wave's, k ascends in every product, and where a sum starts, where its pieces
// end and how many zero steps fill its last group follow from the front and the scalar's position alone; which workgroup
// takes a tile does not enter its arithmetic.
constexpr int SELB_THREADS = 512;
constexpr int SELB_SLAB = 16 * (SELB_THREADS / 64);   // rows of a tile: one 16-row tile per wave
constexpr int SELB_COLS = 32;                         // columns of a tile: two accumulators per wave, one block of Z
constexpr int SELB_Z_THREADS = 256;                   // k_selinv_big_z: one wave per 16 x 16 tile of a 32 x 32 block
constexpr int SELB_RP_COLS = SELB_COLS * (SELB_THREADS / 64);   // k_selinv_big_rp: columns of a tile, one 32-column block per wave
constexpr int SELB_KP = 256;                          // k_selinv_big_rp: rows of Sigma_RR staged in LDS per piece
constexpr int SELB_AHEAD = 4;                         // MFMA steps whose operands are fetched ahead (mfma_chain)
static_assert(SELB_KP % (4 * SELB_AHEAD) == 0 && SELB_THREADS % 16 == 0, "a piece is whole groups of MFMA steps; a thread stages one row of the strip");

struct SelBig {
  int32_t front, pad;
  int64_t zoff, yoff;             // Z and Y of the front in the workspace
};
struct SelTile {
  int32_t big, r0, c0, pad;       // index into SelBig; first row, first column (k_selinv_big_z: r0 = the block row)
};
static_assert(sizeof(SelTile) == 16, "SelTile is one 16-byte record");

template <typename T> struct SelBigArgs {
  SelArgs<T> s;
  const SelBig *big;
  const SelTile *tile;
  T *work;
};

// One wave's chain of MFMA steps k4 = k0, k0 + 4, ... < k1.  load(k4, v) fetches the NV operands of a step -- at clamped
// addresses, one factor zero past the range, so any k4 may be asked for; step(v) issues its MFMAs.  The operands of the next
// SELB_AHEAD steps are in flight while the current ones issue; the steps past k1 that fill the last group add zeros, and how
// many there are follows from k1 - k0 alone.
template <typename T, int NV, typename Load, typename Step>
__device__ __forceinline__ void mfma_chain(int k0, int k1, Load load, Step step) {
  constexpr int U = SELB_AHEAD;
  if (k0 >= k1) return;
  T cur[U][NV], nxt[U][NV];
#pragma unroll
  for (int u = 0; u < U; u++) load(k0 + 4 * u, cur[u]);
  for (int k4 = k0 + 4 * U; k4 < k1; k4 += 4 * U) {
#pragma unroll
    for (int u = 0; u < U; u++) load(k4 + 4 * u, nxt[u]);
#pragma unroll
    for (int u = 0; u < U; u++) step(cur[u]);
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int v = 0; v < NV; v++) cur[u][v] = nxt[u][v];
  }
#pragma unroll
  for (int u = 0; u < U; u++) step(cur[u]);
}

template <typename T>
__global__ void __launch_bounds__(SELB_Z_THREADS) k_selinv_big_z(SelBigArgs<T> a, int begin) {
  using MM = Mfma16<T>;
  constexpr int LT = 33;
  __shared__ T ws[1024];                 // W_j: ws[c * 32 + k] = W_j(k, c)
  __shared__ T ts[32 * LT];              // the sum over the later blocks, the A operand of the product with W_j
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wave = wave_index(), mi = wave >> 1, ni = wave & 1;
  const SelTile tl = a.tile[begin + blockIdx.x];
  const SelBig bg = a.big[tl.big];
  const SelMeta m = a.s.meta[bg.front];
  const int nc = m.nc, M = nc + m.nr + 1;
  const int b = tl.r0, b0 = 32 * b, rw = min(32, nc - b0), kend = b0 + rw;
  const T *Lg = a.s.lvals + m.loff;
  const T *Wg = a.s.winv + (int64_t)m.wblk * 256;
  T *Zb = a.work + bg.zoff + (int64_t)b0 * nc;   // the block row: Zb[r * nc + col]
  // ---- Z_bb = W_b, zero above the diagonal (the products below and of the later kernels run over whole blocks)
  for (int e = tid; e < 1024; e += SELB_Z_THREADS) {
    const int c = e >> 5, r = e & 31;
    if (r < rw && c < rw) Zb[(int64_t)r * nc + b0 + c] = c <= r ? Wg[(int64_t)b * 1024 + e] : (T)0;
  }
  __syncthreads();
  const int mrow = min(16 * mi + li, rw - 1);   // rows past a partial block are computed and dropped
  for (int j = b - 1; j >= 0; j--) {            // (the earlier blocks are full ones)
    const int j0 = 32 * j, col = 16 * ni + li;
    for (int e = tid; e < 1024; e += SELB_Z_THREADS) ws[e] = Wg[(int64_t)j * 1024 + e];
    typename MM::Acc acc = {0, 0, 0, 0};
    const T *za = Zb + (int64_t)mrow * nc;
    const T *lb = Lg + (int64_t)(j0 + col) * M;
    mfma_chain<T, 2>(j0 + 32, kend,
                     [&](int k4, T *v) {
                       const int k = k4 + lk, kc = min(k, kend - 1);
                       const T zv = za[kc];
                       v[0] = k < kend ? zv : (T)0;
                       v[1] = lb[kc];
                     },
                     [&](const T *v) { acc = MM::mma(v[0], v[1], acc); });
#pragma unroll
    for (int r = 0; r < 4; r++) ts[(16 * mi + MM::row(lane, r)) * LT + col] = acc[r];
    __syncthreads();
    typename MM::Acc z = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 8; s++) {
      const int k = 4 * s + lk;
      z = MM::mma(-ts[(16 * mi + li) * LT + k], k >= col ? ws[col * 32 + k] : (T)0, z);   // W is lower triangular
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = 16 * mi + MM::row(lane, r);
      if (row < rw) Zb[(int64_t)row * nc + j0 + col] = z[r];
    }
    __syncthreads();
  }
}

template <typename T>
__global__ void __launch_bounds__(SELB_THREADS) k_selinv_big_y(SelBigArgs<T> a, int begin) {
  using MM = Mfma16<T>;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const SelTile tl = a.tile[begin + blockIdx.x];
  const SelBig bg = a.big[tl.big];
  const SelMeta m = a.s.meta[bg.front];
  const int nc = m.nc, nr = m.nr, M = nc + nr + 1;
  const int c0 = tl.c0;
  // ---- a wave's 16 rows, the tile's 32 columns; Z(k, c) is zero for k < c0
  const int i0 = tl.r0 + 16 * wave_index();
  if (i0 >= nr) return;   // (no barrier below)
  const T *La = a.s.lvals + m.loff + nc + min(i0 + li, nr - 1);   // rows past nr of the last tile are computed and dropped
  const T *Zg = a.work + bg.zoff;
  const int ca = min(c0 + li, nc - 1), cb = min(c0 + 16 + li, nc - 1);
  typename MM::Acc acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  mfma_chain<T, 3>(c0, nc,
                   [&](int k4, T *v) {
                     const int k = k4 + lk, kc = min(k, nc - 1);
                     const T lv = La[(int64_t)kc * M];
                     const T *z = Zg + (int64_t)kc * nc;
                     v[0] = k < nc ? lv : (T)0;
                     v[1] = z[ca];
                     v[2] = z[cb];
                   },
                   [&](const T *v) {
                     acc0 = MM::mma(v[0], v[1], acc0);
                     acc1 = MM::mma(v[0], v[2], acc1);
                   });
  T *Yg = a.work + bg.yoff;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = i0 + MM::row(lane, r);
    if (row < nr) {
      if (c0 + li < nc) Yg[(int64_t)row * nc + c0 + li] = acc0[r];
      if (c0 + 16 + li < nc) Yg[(int64_t)row * nc + c0 + 16 + li] = acc1[r];
    }
  }
}

// Sigma_RP = -Sigma_RR Y for a strip of 16 rows below, in the transposed form of k_selinv_level (D[c][i] = sum_k Y(k, c)
// Sigma(k, i): a lane's results are four columns c of one row i); a wave takes one 32-column block of the tile's 256
// columns.  Sigma_RR(k, i) of the strip is fetched from the parent's image through the rel map, SELB_KP rows k at a time,
// into LDS -- every thread's loads at once, not one wave's chain of them -- and the tiles of the first column group copy
// it into the front's own image for its children.
template <typename T>
__global__ void __launch_bounds__(SELB_THREADS) k_selinv_big_rp(SelBigArgs<T> a, int begin) {
  using MM = Mfma16<T>;
  __shared__ T ss[SELB_KP * 16];          // ss[k * 16 + i] = Sigma_RR(k0 + k, i0 + i)
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const SelTile tl = a.tile[begin + blockIdx.x];
  const SelBig bg = a.big[tl.big];
  const SelMeta m = a.s.meta[bg.front];
  const int nc = m.nc, nr = m.nr, n = nc + nr;
  const int i0 = tl.r0, c0 = tl.c0 + SELB_COLS * wave_index();
  const bool mine = c0 < nc;   // (every wave stages Sigma_RR)
  T *Sg = a.s.svals + m.soff;
  T *U = Sg + (int64_t)n * nc;
  const T *Sp = a.s.svals + m.psoff;
  const T *Yg = a.work + bg.yoff;
  const int32_t *rel = a.s.rel + m.rel_ptr;
  const int pnc = m.pnc, pn = m.pn, pnr = pn - pnc;
  auto parent = [&](int pi, int pj) -> T {   // Sigma of the parent at two of its local indices
    const int hi = max(pi, pj), lo = min(pi, pj);
    return Sp[lo < pnc ? (int64_t)lo * pn + hi : (int64_t)pn * pnc + packed_lower(pnr, hi - pnc, lo - pnc)];
  };
  const int gi = min(i0 + (tid & 15), nr - 1), pgi = rel[gi];   // the row this thread stages (rows past nr repeat the last one)
  const bool copy = tl.c0 == 0 && i0 + (tid & 15) < nr;
  const int ca = min(c0 + li, nc - 1), cb = min(c0 + 16 + li, nc - 1);
  typename MM::Acc acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  for (int k0 = 0; k0 < nr; k0 += SELB_KP) {
    const int kp = min(SELB_KP, nr - k0);
    if (k0 > 0) __syncthreads();   // the piece before has been read
    for (int e = tid; e < kp * 16; e += SELB_THREADS) {   // (e & 15 == tid & 15)
      const int k = k0 + (e >> 4);
      const T v = parent(pgi, rel[k]);
      ss[e] = v;
      if (copy && k <= gi) U[packed_lower(nr, gi, k)] = v;
    }
    __syncthreads();
    if (mine)
      mfma_chain<T, 3>(0, kp,
                       [&](int k4, T *v) {
                         const int k = k4 + lk, kc = min(k, kp - 1);
                         const T sv = ss[kc * 16 + li];
                         const T *y = Yg + (int64_t)(k0 + kc) * nc;
                         v[0] = k < kp ? sv : (T)0;
                         v[1] = y[ca];
                         v[2] = y[cb];
                       },
                       [&](const T *v) {
                         acc0 = MM::mma(v[1], v[0], acc0);
                         acc1 = MM::mma(v[2], v[0], acc1);
                       });
  }
  const int i = i0 + li;
  if (!mine || i >= nr) return;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = c0 + MM::row(lane, r);
    if (c < nc) Sg[(int64_t)c * n + nc + i] = -acc0[r];
    if (c + 16 < nc) Sg[(int64_t)(c + 16) * n + nc + i] = -acc1[r];
  }
}

// The lower triangle of the pivot square, transposed like the kernel above (D[j][i], i >= j: a lane's results are four
// columns j of one row i), in two steps.  k_selinv_big_zz: Z^T Z; Z(k, .) of the tile's rows and columns is zero for k < i0,
// so the sum starts there.  k_selinv_big_pp: what stands there less Y^T Sigma_RP.
template <typename T, bool ZZ>
__device__ __forceinline__ void selinv_big_square(const SelBigArgs<T> &a, int begin) {
  using MM = Mfma16<T>;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const SelTile tl = a.tile[begin + blockIdx.x];
  const SelBig bg = a.big[tl.big];
  const SelMeta m = a.s.meta[bg.front];
  const int nc = m.nc, nr = m.nr, n = nc + nr;
  const int c0 = tl.c0, i0 = tl.r0 + 16 * wave_index();
  if (i0 >= nc || i0 + 15 < c0) return;   // past the front, or above the diagonal (no barrier below)
  T *Sg = a.s.svals + m.soff;
  const int i = i0 + li, ic = min(i, nc - 1), ja = min(c0 + li, nc - 1), jb = min(c0 + 16 + li, nc - 1);
  T *d0[4], *d1[4];   // the true address wherever the entry is stored
  bool s0[4], s1[4];
  typename MM::Acc acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int j = c0 + MM::row(lane, r);
    s0[r] = i < nc && j <= i;
    s1[r] = i < nc && j + 16 <= i;
    d0[r] = Sg + (int64_t)min(j, ic) * n + ic;
    d1[r] = Sg + (int64_t)min(j + 16, ic) * n + ic;
    if (!ZZ) {
      acc0[r] = *d0[r];
      acc1[r] = *d1[r];
    }
  }
  auto step = [&](const T *v) {
    acc0 = MM::mma(v[1], v[0], acc0);
    acc1 = MM::mma(v[2], v[0], acc1);
  };
  if (ZZ) {
    const T *Zg = a.work + bg.zoff;
    mfma_chain<T, 3>(i0, nc,
                     [&](int k4, T *v) {
                       const int k = k4 + lk, kc = min(k, nc - 1);
                       const T *z = Zg + (int64_t)kc * nc;
                       const T zv = z[ic];
                       v[0] = k < nc ? zv : (T)0;
                       v[1] = z[ja];
                       v[2] = z[jb];
                     },
                     step);
  } else {
    const T *Yg = a.work + bg.yoff;
    const T *Sr = Sg + (int64_t)ic * n + nc;   // Sigma_RP(., i)
    mfma_chain<T, 3>(0, nr,
                     [&](int k4, T *v) {
                       const int k = k4 + lk, kc = min(k, nr - 1);
                       const T *y = Yg + (int64_t)kc * nc;
                       const T sv = Sr[kc];
                       v[0] = k < nr ? sv : (T)0;
                       v[1] = -y[ja];
                       v[2] = -y[jb];
                     },
                     step);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (s0[r]) *d0[r] = acc0[r];
    if (s1[r]) *d1[r] = acc1[r];
  }
}
template <typename T>
__global__ void __launch_bounds__(SELB_THREADS) k_selinv_big_zz(SelBigArgs<T> a, int begin) { selinv_big_square<T, true>(a, begin); }
template <typename T>
__global__ void __launch_bounds__(SELB_THREADS) k_selinv_big_pp(SelBigArgs<T> a, int begin) { selinv_big_square<T, false>(a, begin); }

}  // namespace rrpgo
