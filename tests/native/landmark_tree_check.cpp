// landmark_tree_check.cpp -- TEST HELPER (host only, never part of librr_pgo.so).
//
// The elimination tree the symbolic analysis gives a 3-D graph with point landmarks, with the options an f64 handle of at
// most 6000 nodes sets (pgo_api.hip, analyze_handle): prints the number of fronts, the depth of the tree (fronts on the
// longest path from a leaf to its root) and how many fronts have pivot columns of both kinds (SE3 poses and XYZ landmarks).
// rr_pgo_stats has neither: its n_levels counts schedule steps.
//
// usage: landmark_tree_check <file.g2o>
#include <algorithm>
#include <cstdio>
#include <vector>

#include "host_graph.h"
#include "symbolic.h"
using namespace rrpgo;

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  HostGraph g;
  bool io;
  std::string e = load_g2o(argv[1], g, io);
  if (!e.empty()) { printf("load error: %s\n", e.c_str()); return 2; }
  SymbolicOptions opt;
  opt.lds_budget_elems = 19000;
  opt.nd_leaf = 1 << 30;
  opt.lds_flow = true;
  opt.ml_nd = true;
  opt.arrival_order = true;
  Symbolic y;
  e = analyze(g, opt, y);
  if (!e.empty()) { printf("analyze error: %s\n", e.c_str()); return 2; }
  std::vector<int> depth((size_t)y.S, 0);
  int deepest = 0;
  for (int f = 0; f < y.S; f++) {   // the depth of a front below its root, by walking up (the trees are small)
    int d = 1;
    for (int p = y.sn_parent[f]; p >= 0; p = y.sn_parent[p]) d++;
    depth[(size_t)f] = d;
    deepest = std::max(deepest, d);
  }
  int mixed = 0, widest_mixed = 0;
  for (int f = 0; f < y.S; f++) {
    bool pose = false, point = false;
    for (int p = y.sn_first_pos[f]; p < y.sn_first_pos[f] + y.sn_npos[f]; p++) {
      const int k = g.node_kind[(size_t)y.order[(size_t)p]];
      pose = pose || k == NODE_SE3;
      point = point || k == NODE_XYZ;
    }
    if (pose && point) { mixed++; widest_mixed = std::max(widest_mixed, (int)y.sn_ncols[f]); }
  }
  printf("fronts %d depth %d mixed %d widest_mixed %d\n", y.S, deepest, mixed, widest_mixed);
  return 0;
}
