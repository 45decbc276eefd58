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

}  // namespace rrpgo
