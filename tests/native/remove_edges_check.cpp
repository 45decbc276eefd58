// The host-only part of rr_pgo_remove_edges (csrc/host_graph.h, csrc/g2o_loader.cpp), on the CPU: the orphan check, the
// compaction of what remains, the anchor rule of HostGraph::finalize, and the re-indexing of the robust edge mask that
// rr_pgo_extend shares with it.  Prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <vector>

#include "host_graph.h"

using namespace rrpgo;

static int fail(const char *what) {
  std::printf("FAILED: %s\n", what);
  return 1;
}

int main() {
  // poses 0 .. 3, landmarks 4 (seen from 1 only) and 5 (seen from 0, 2, 3); edge 0 is a sighting, so the anchor is the from-node of edge 1
  const std::vector<int32_t> kind = {EDGE_SE2_XY, EDGE_SE2, EDGE_SE2, EDGE_SE2, EDGE_SE2, EDGE_SE2_XY, EDGE_SE2_XY, EDGE_SE2_XY};
  const std::vector<int32_t> from = {1, 2, 0, 1, 3, 0, 2, 3}, to = {4, 3, 1, 2, 0, 5, 5, 5};
  const int N = 6, E = (int)kind.size();
  auto orphan = [&](std::vector<int> removed) {
    std::vector<char> gone((size_t)E, 0);
    for (int k : removed) gone[(size_t)k] = 1;
    return first_orphan_node(N, E, from.data(), to.data(), gone.data());
  };
  if (orphan({}) != -1) return fail("nothing removed: no orphan");
  if (orphan({0}) != 4) return fail("the landmark seen once loses its only edge");
  if (orphan({5, 6}) != -1) return fail("a landmark seen three times keeps one sighting");
  if (orphan({5, 6, 7}) != 5) return fail("... and is an orphan without all three");
  if (orphan({2, 4, 5, 0}) != 0) return fail("the lowest orphan is named (0 before 4)");
  if (orphan({1, 1, 1}) != -1) return fail("a duplicate counts once");
  if (orphan({1, 2, 3, 4}) != -1) return fail("poses that only landmarks join are disconnected, not orphans");
  // the graph without edges 1 and 5 by copy_without_edges, the loop rr_pgo_remove_edges runs: order kept, compact numbering,
  // the measurements and information of the survivors; then the anchor from the first remaining pose-pose edge
  HostGraph og;
  og.node_kind = {NODE_SE2, NODE_SE2, NODE_SE2, NODE_SE2, NODE_XY, NODE_XY};
  og.node_id = {10, 11, 12, 13, 14, 15};
  og.node_state.assign(4 * 3 + 2 * 2, 0.0);
  og.edge_kind = kind;
  og.edge_from = from;
  og.edge_to = to;
  for (int k = 0; k < E; k++) {   // edge k's measurement is k + 0.25 throughout, its information 100 + k
    og.edge_meas.insert(og.edge_meas.end(), (size_t)edge_meas_len(kind[k]), k + 0.25);
    og.edge_info.insert(og.edge_info.end(), (size_t)edge_info_len(kind[k]), 100.0 + k);
  }
  if (!og.finalize().empty() || og.anchor_node != 2) return fail("the whole graph: anchor 2");
  std::vector<char> gone((size_t)E, 0);
  gone[1] = gone[5] = 1;
  HostGraph g;
  const std::vector<int32_t> keep = copy_without_edges(og, gone.data(), g);
  if (keep != std::vector<int32_t>{0, 2, 3, 4, 6, 7}) return fail("the kept edges in their order");
  if (g.node_kind != og.node_kind || g.node_id != og.node_id || g.node_state != og.node_state) return fail("nodes are copied as they are");
  const std::string err = g.finalize();
  if (!err.empty()) return fail(err.c_str());
  if (g.n_edges() != E - 2 || g.anchor_node != 0) return fail("anchor: the from-node of old edge 2, now edge 1");
  if (g.edge_meas_off[1] != 2 || g.edge_info_off[2] != 3 + 6) return fail("offsets of the compacted arrays");
  if (g.dim != 16 || g.node_offset[5] != 14) return fail("nodes and dx offsets do not change");
  for (int q = 0; q < g.n_edges(); q++) {
    const int k = keep[(size_t)q];
    if (g.edge_kind[q] != kind[k] || g.edge_from[q] != from[k] || g.edge_to[q] != to[k]) return fail("a survivor's kind and endpoints");
    if (g.edge_meas[(size_t)g.edge_meas_off[q]] != k + 0.25 || g.edge_info[(size_t)g.edge_info_off[q]] != 100.0 + k) return fail("a survivor's measurement and information");
  }
  if (g.edge_meas.size() != 2 + 3 * 3 + 2 * 2 || g.edge_info.size() != 3 + 3 * 6 + 2 * 3) return fail("packed lengths");
  // reindex_edge_mask, the robust mask of a rebuilt graph, for the two shapes of `origin` its callers have: rr_pgo_extend's
  // (0 .. E - 1, then -1 per new edge) and rr_pgo_remove_edges' (`keep` above)
  const std::vector<uint8_t> none, mask = {1, 0, 0, 1, 1, 0, 1, 0};
  std::vector<int32_t> grown((size_t)E + 3, -1);
  for (int k = 0; k < E; k++) grown[(size_t)k] = k;
  if (!reindex_edge_mask(none, grown).empty() || !reindex_edge_mask(none, keep).empty()) return fail("an empty mask (every edge) stays empty");
  if (reindex_edge_mask(mask, grown) != std::vector<uint8_t>{1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1}) return fail("extend: the old entries, then 1 per new edge");
  grown.resize((size_t)E);
  if (reindex_edge_mask(mask, grown) != mask) return fail("extend without a new edge: the mask as it was");
  const std::vector<uint8_t> kept = reindex_edge_mask(mask, keep);
  if (kept.size() != keep.size()) return fail("remove: one entry per surviving edge");
  for (size_t q = 0; q < keep.size(); q++)
    if (kept[q] != mask[(size_t)keep[q]]) return fail("remove: mask[keep]");
  if (kept != std::vector<uint8_t>{1, 0, 1, 1, 1, 0}) return fail("remove: the survivors' entries in their order");
  // a removal list with duplicates in any order flags each edge once: `keep` is ascending and without repeats, and so is the mask's
  std::vector<char> gone2((size_t)E, 0);
  for (int k : {7, 0, 7, 3, 0}) gone2[(size_t)k] = 1;
  HostGraph g2;
  const std::vector<int32_t> keep2 = copy_without_edges(og, gone2.data(), g2);
  if (keep2 != std::vector<int32_t>{1, 2, 4, 5, 6}) return fail("duplicates count once, order kept");
  if (reindex_edge_mask(mask, keep2) != std::vector<uint8_t>{0, 0, 1, 0, 1}) return fail("remove with duplicates: mask[keep]");
  std::printf("ok\n");
  return 0;
}
