// arrival_order_check.cpp -- TEST HELPER (host only, never part of librr_pgo.so).
//
// The arrival order of the pivot columns (symbolic.cpp, step 5) and the due blocks of the children (Symbolic::child_due),
// without a GPU.  The graph is analysed twice, with SymbolicOptions::arrival_order on and off, and
//   (a) the factorisation is replayed on the host in the kernel's order -- a front's children with due == 0 before the panel,
//       every other child at the top of its due block, after the blocks to its left have been eliminated and their Schur
//       updates applied -- on random SPD values on the pattern (as mf_host_check.cpp), and || b - H x ||_inf / || b ||_inf is
//       held against mf_host_check's bound;
//   (b) no destination of a child's scatter map or rel map lies in a pivot column < 16 * due, due is non-decreasing along
//       every child list and names a block of the parent's panel; without arrival order (the switch, a front beyond LDS)
//       every due is 0;
//   (c) both analyses have the same supernode partition -- (first_pos, npos, ncols, nrows, parent) per front, nnz(L), flops,
//       max_front -- and `order` differs by permutations inside supernodes only;
//   (d) the histogram of due is printed, the tree's statistics as rr_pgo_stats names them (the line "tree:": the GPU test holds
//       its handles against them), and which of the shapes a GPU test wants are present (the line "cases:").
//
// usage: arrival_order_check <file.g2o> | grid W H   [env LEAF, LDS, ML, FLOW, MERGE_NC, MERGE_GAIN, BALANCE, AMALG_NP, SPLIT
//        as mf_host_check reads them]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>

#include "host_graph.h"
#include "symbolic.h"
using namespace rrpgo;

static int64_t tri(int n, int i, int j) { return (int64_t)j * n - (int64_t)j * (j - 1) / 2 + (i - j); }

#define FAIL(...) do { printf("FAIL: " __VA_ARGS__); printf("\n"); return 1; } while (0)

// (b) on the tables of one analysis
static int check_due(const Symbolic &y, bool expect_zero) {
  if (y.child_due.size() != y.child_list.size()) FAIL("child_due has %zu entries for %zu children", y.child_due.size(), y.child_list.size());
  for (int f = 0; f < y.S; f++) {
    const int nc = y.sn_ncols[f], M = nc + y.sn_nrows[f] + 1, nblk = (nc + 15) / 16;
    int prev = 0;
    for (int q = y.child_ptr[f]; q < y.child_ptr[f + 1]; q++) {
      const int c = y.child_list[q], due = y.child_due[q];
      if (y.sn_parent[c] != f) FAIL("child list of front %d holds %d, whose parent is %d", f, c, y.sn_parent[c]);
      if (expect_zero && due != 0) FAIL("child %d of front %d is due at block %d without arrival order", c, f, due);
      if (due < 0 || due >= nblk) FAIL("child %d of front %d is due at block %d of %d", c, f, due, nblk);
      if (due < prev) FAIL("due decreases along the child list of front %d (%d after %d)", f, due, prev);
      prev = due;
      const int ncu = y.sn_nrows[c] + 1;
      const int32_t *rel = y.rel.data() + y.rel_ptr[c];
      for (int i = 0; i < ncu; i++)
        if (rel[i] < nc && rel[i] < 16 * due) FAIL("rel of child %d (due %d) names pivot column %d of front %d", c, due, rel[i], f);
      if (y.scat_ptr[c] >= 0 && !y.sn_big[f]) {
        const int32_t *map = y.scat.data() + y.scat_ptr[c];
        for (int64_t t = 0; t < (int64_t)ncu * (ncu + 1) / 2; t++)
          if (map[t] >= 0 && map[t] < M * nc && map[t] / M < 16 * due) FAIL("scatter map of child %d (due %d) names pivot column %d of front %d", c, due, map[t] / M, f);
      }
    }
  }
  return 0;
}

// (a): factor and solve in the kernel's order; returns the relative residual, < 0 on a failure
static double replay(const HostGraph &g, const Symbolic &y) {
  const int N = y.N, dim = y.dim, S = y.S;
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  std::vector<double> hv((size_t)y.n_hvals, 0.0), b(dim), rowsum(dim, 0.0);
  for (int64_t s = 0; s < y.n_offblocks; s++) {
    int rn = y.blk_row[s], cn = y.blk_col[s];
    int dr = node_dim(g.node_kind[rn]), dc = node_dim(g.node_kind[cn]);
    for (int i = 0; i < dr; i++)
      for (int j = 0; j < dc; j++) {
        double v = U(rng);
        hv[y.blk_off[s] + i * dc + j] = v;
        rowsum[g.node_offset[rn] + i] += std::fabs(v);
        rowsum[g.node_offset[cn] + j] += std::fabs(v);
      }
  }
  for (int v = 0; v < N; v++) {
    int d = node_dim(g.node_kind[v]);
    for (int i = 0; i < d; i++)
      for (int j = 0; j <= i; j++) {
        double x = i == j ? 0.0 : U(rng);
        hv[y.diag_off[v] + i * d + j] = x;
        hv[y.diag_off[v] + j * d + i] = x;
        if (i != j) { rowsum[g.node_offset[v] + i] += std::fabs(x); rowsum[g.node_offset[v] + j] += std::fabs(x); }
      }
    for (int i = 0; i < d; i++) hv[y.diag_off[v] + i * d + i] = rowsum[g.node_offset[v] + i] + 1.0 + std::fabs(U(rng));
  }
  for (int i = 0; i < dim; i++) b[i] = U(rng);

  std::vector<double> L((size_t)y.l_elems + 4, 0.0), Uv((size_t)y.u_elems + 4, 0.0), x(dim, 0.0);
  std::vector<double> img;   // [panel | packed update], the LDS image the scatter maps index
  for (int s = 0; s < S; s++) {   // children precede parents
    if (y.sn_big[s]) { printf("FAIL: the replay is for fronts in LDS\n"); return -1; }
    const int nc = y.sn_ncols[s], nr = y.sn_nrows[s], M = nc + nr + 1, nu = nr + 1;
    const size_t psize = (size_t)M * nc;
    img.assign(psize + (size_t)nu * (nu + 1) / 2, 0.0);
    double *P = img.data(), *Ul = img.data() + psize;
    for (int64_t t = y.fasm_ptr[s]; t < y.fasm_ptr[s + 1]; t++) P[y.fasm_dst[t]] += hv[y.fasm_src[t]];
    for (int64_t t = y.fdup_ptr[s]; t < y.fdup_ptr[s + 1]; t++) P[y.fdup_dst[t]] += hv[y.fdup_src[t]];
    for (int j = 0; j < nc; j++) P[(size_t)j * M + M - 1] = b[y.perm[y.sn_col0[s] + j]];
    int q = y.child_ptr[s];
    auto add_children = [&](int k) {   // every child due at block k, through its scatter map
      for (; q < y.child_ptr[s + 1] && y.child_due[q] == k; q++) {
        const int c = y.child_list[q], ncu = y.sn_nrows[c] + 1;
        const double *Uc = Uv.data() + y.sn_uoff[c];
        const int32_t *map = y.scat.data() + y.scat_ptr[c];
        for (int64_t t = 0; t < (int64_t)ncu * (ncu + 1) / 2; t++)
          if (map[t] >= 0) img[(size_t)map[t]] += Uc[t];
      }
    };
    for (int k0 = 0; k0 < nc; k0 += 16) {
      add_children(k0 / 16);
      const int k1 = std::min(k0 + 16, nc);
      for (int k = k0; k < k1; k++) {
        double d = P[(size_t)k * M + k];
        if (!(d > 0)) { printf("FAIL: non-positive pivot in supernode %d\n", s); return -1; }
        d = std::sqrt(d);
        P[(size_t)k * M + k] = d;
        for (int i = k + 1; i < M; i++) P[(size_t)k * M + i] /= d;
        for (int j = k + 1; j < nc; j++)
          for (int i = j; i < M; i++) P[(size_t)j * M + i] -= P[(size_t)k * M + i] * P[(size_t)k * M + j];
      }
      for (int j = 0; j < nu; j++)   // the block's Schur complement on the update matrix, before the next block's children
        for (int i = j; i < nu; i++) {
          double sacc = 0;
          for (int k = k0; k < k1; k++) sacc += P[(size_t)k * M + nc + i] * P[(size_t)k * M + nc + j];
          Ul[tri(nu, i, j)] -= sacc;
        }
    }
    if (q != y.child_ptr[s + 1]) { printf("FAIL: front %d never adds child %d (due %d)\n", s, y.child_list[q], y.child_due[q]); return -1; }
    std::copy(P, P + psize, L.begin() + y.sn_loff[s]);
    std::copy(Ul, Ul + (size_t)nu * (nu + 1) / 2, Uv.begin() + y.sn_uoff[s]);
  }
  for (int s = S - 1; s >= 0; s--) {
    const int nc = y.sn_ncols[s], nr = y.sn_nrows[s], M = nc + nr + 1;
    const double *Lg = L.data() + y.sn_loff[s];
    const int32_t *rows = y.sn_rows.data() + y.sn_rows_ptr[s];
    std::vector<double> t(nc);
    for (int j = 0; j < nc; j++) {
      double sacc = 0;
      for (int i = 0; i < nr; i++) sacc += Lg[(size_t)j * M + nc + i] * x[rows[i]];
      t[j] = Lg[(size_t)j * M + M - 1] - sacc;
    }
    for (int j = nc - 1; j >= 0; j--) {
      double sacc = 0;
      for (int i = j + 1; i < nc; i++) sacc += Lg[(size_t)j * M + i] * t[i];
      t[j] = (t[j] - sacc) / Lg[(size_t)j * M + j];
    }
    for (int j = 0; j < nc; j++) x[y.sn_col0[s] + j] = t[j];
  }
  std::vector<double> xr(dim), r(b);
  for (int i = 0; i < dim; i++) xr[y.perm[i]] = x[i];
  for (int v = 0; v < N; v++) {
    int d = node_dim(g.node_kind[v]), o = g.node_offset[v];
    for (int i = 0; i < d; i++)
      for (int j = 0; j < d; j++) r[o + i] -= hv[y.diag_off[v] + i * d + j] * xr[o + j];
  }
  for (int64_t s = 0; s < y.n_offblocks; s++) {
    int rn = y.blk_row[s], cn = y.blk_col[s];
    int dr = node_dim(g.node_kind[rn]), dc = node_dim(g.node_kind[cn]);
    int ro = g.node_offset[rn], co = g.node_offset[cn];
    for (int i = 0; i < dr; i++)
      for (int j = 0; j < dc; j++) {
        double v = hv[y.blk_off[s] + i * dc + j];
        r[ro + i] -= v * xr[co + j];
        r[co + j] -= v * xr[ro + i];
      }
  }
  double rmax = 0, bmax = 0;
  for (int i = 0; i < dim; i++) { rmax = std::max(rmax, std::fabs(r[i])); bmax = std::max(bmax, std::fabs(b[i])); }
  return rmax / bmax;
}

int main(int argc, char **argv) {
  HostGraph g;
  if (argc >= 4 && !strcmp(argv[1], "grid")) {
    synth_grid(atoi(argv[2]), atoi(argv[3]), 0, 42, 43, g);
  } else if (argc >= 2) {
    bool io;
    std::string e = load_g2o(argv[1], g, io);
    if (!e.empty()) { printf("load error: %s\n", e.c_str()); return 2; }
  } else {
    return 2;
  }
  SymbolicOptions opt;
  if (getenv("LEAF")) opt.nd_leaf = atoi(getenv("LEAF"));
  if (getenv("LDS")) opt.lds_budget_elems = atoll(getenv("LDS"));
  if (getenv("FLOW")) opt.lds_flow = true;
  if (getenv("MERGE_NC")) opt.merge_chain_nc = atoi(getenv("MERGE_NC"));
  if (getenv("MERGE_GAIN")) opt.merge_chain_gain_us = atof(getenv("MERGE_GAIN"));
  if (getenv("BALANCE")) { opt.balance_blocks = atoi(getenv("BALANCE")) != 0; if (atoi(getenv("BALANCE")) > 1) opt.balance_max_rem = atoi(getenv("BALANCE")); }
  if (getenv("AMALG_NP")) opt.amalg_np = atoi(getenv("AMALG_NP"));
  if (getenv("ML")) opt.ml_nd = true;
  if (getenv("SPLIT")) opt.split_separators = true;
  Symbolic on, off;
  opt.arrival_order = true;
  std::string e = analyze(g, opt, on);
  if (!e.empty()) { printf("analyze error: %s\n", e.c_str()); return 2; }
  opt.arrival_order = false;
  e = analyze(g, opt, off);
  if (!e.empty()) { printf("analyze error: %s\n", e.c_str()); return 2; }

  // ---- (c) the same partition, another order inside the supernodes only
  if (on.S != off.S || on.N != off.N) FAIL("the switch changes the number of supernodes (%d, %d)", on.S, off.S);
  if (on.nnz_l_blocks != off.nnz_l_blocks || on.nnz_l_entries != off.nnz_l_entries || on.factor_flops != off.factor_flops ||
      on.max_front != off.max_front || on.n_big != off.n_big || on.l_elems != off.l_elems || on.u_elems != off.u_elems)
    FAIL("the switch changes nnz(L), the flops, the largest front or the storage");
  int moved = 0;
  for (int f = 0; f < on.S; f++) {
    if (on.sn_first_pos[f] != off.sn_first_pos[f] || on.sn_npos[f] != off.sn_npos[f] || on.sn_ncols[f] != off.sn_ncols[f] ||
        on.sn_nrows[f] != off.sn_nrows[f] || on.sn_parent[f] != off.sn_parent[f] || on.sn_col0[f] != off.sn_col0[f])
      FAIL("front %d differs between the two analyses", f);
    std::vector<int32_t> a(on.order.begin() + on.sn_first_pos[f], on.order.begin() + on.sn_first_pos[f] + on.sn_npos[f]);
    std::vector<int32_t> o(off.order.begin() + off.sn_first_pos[f], off.order.begin() + off.sn_first_pos[f] + off.sn_npos[f]);
    moved += a != o;
    std::sort(a.begin(), a.end());
    std::sort(o.begin(), o.end());
    if (a != o) FAIL("front %d has other pivot nodes under the switch", f);
    const int32_t *ra = on.sn_rows.data() + on.sn_rows_ptr[f];
    for (int i = 1; i < on.sn_nrows[f]; i++)
      if (ra[i] <= ra[i - 1]) FAIL("rows of front %d are not ascending", f);
  }
  const bool eligible = on.n_big == 0;
  if (!eligible && (moved || on.order != off.order)) FAIL("a graph with fronts beyond LDS was reordered");

  // ---- (b)
  if (check_due(on, !eligible) || check_due(off, true)) return 1;

  // ---- (d) histogram and shapes
  std::map<int, int> hist;
  bool middle = false, partial_last = false, same_block = false, three = false, all_zero = false;
  for (int f = 0; f < on.S; f++) {
    const int nc = on.sn_ncols[f], nblk = (nc + 15) / 16;
    std::map<int, int> mine;
    for (int q = on.child_ptr[f]; q < on.child_ptr[f + 1]; q++) {
      const int due = on.child_due[q];
      hist[due]++;
      mine[due]++;
      middle = middle || (due > 0 && due < nblk - 1);
      partial_last = partial_last || (due > 0 && due == nblk - 1 && nc % 16 != 0);
    }
    for (auto &kv : mine) same_block = same_block || (kv.first > 0 && kv.second >= 2);
    three = three || mine.size() >= 3;
    all_zero = all_zero || (mine.size() == 1 && mine.count(0) && mine[0] >= 2);
  }
  printf("due histogram:");
  for (auto &kv : hist) printf(" %d:%d", kv.first, kv.second);
  printf("  (%d of %d supernodes reordered)\n", moved, on.S);
  printf("tree: n_supernodes=%d max_front=%d max_pivot_cols=%d\n", on.S, on.max_front, on.max_pivot_cols);
  printf("cases: middle=%d partial_last=%d same_block=%d three_distinct=%d all_zero=%d\n", middle, partial_last, same_block, three, all_zero);

  // ---- (a)
  if (eligible) {
    const double r_on = replay(g, on), r_off = replay(g, off);
    if (r_on < 0 || r_off < 0) return 1;
    printf("N=%d dim=%d S=%d  rel_residual=%.3e (arrival order)  %.3e (elimination order)\n", on.N, on.dim, on.S, r_on, r_off);
    if (!(r_on < 1e-9) || !(r_off < 1e-9)) FAIL("residual too large");   // the bound of mf_host_check.cpp
  } else {
    printf("N=%d dim=%d S=%d  %d fronts beyond LDS: no arrival order, no replay\n", on.N, on.dim, on.S, on.n_big);
  }
  printf("OK\n");
  return 0;
}
