// host_graph.h -- host-side pose graph, flattened (what the reference keeps as
// Vec<Edge<f64>> + two FxHashMaps, pose_graph_optimization.rs:155-163).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace rrpgo {

enum NodeKind : int32_t { NODE_SE2 = 0, NODE_XY = 1, NODE_SE3 = 2, NODE_XYZ = 3 };
// 5 and 7 are reserved: unknown kinds everywhere
enum EdgeKind : int32_t { EDGE_SE2 = 0, EDGE_SE2_XY = 1, EDGE_SE3 = 2, EDGE_SE3_XYZ = 3, EDGE_SE2_BEARING = 4, EDGE_SE2_RANGE = 6 };
inline bool edge_kind_known(int kind) { return (kind >= EDGE_SE2 && kind <= EDGE_SE2_BEARING) || kind == EDGE_SE2_RANGE; }
// bearing-only and range-only edges SE2 pose -> XY landmark: ONE error scalar, one measurement value, one information value
inline bool edge_is_br(int kind) { return kind == EDGE_SE2_BEARING || kind == EDGE_SE2_RANGE; }

inline int node_dim(int kind) { return kind == NODE_SE2 ? 3 : kind == NODE_XY ? 2 : kind == NODE_XYZ ? 3 : 6; }
inline int node_state_len(int kind) { return kind == NODE_SE2 ? 3 : kind == NODE_XY ? 2 : kind == NODE_XYZ ? 3 : 7; }
inline int edge_dim(int kind) { return edge_is_br(kind) ? 1 : kind == EDGE_SE2 ? 3 : kind == EDGE_SE2_XY ? 2 : kind == EDGE_SE3_XYZ ? 3 : 6; }
inline int edge_meas_len(int kind) { return edge_is_br(kind) ? 1 : kind == EDGE_SE2 ? 3 : kind == EDGE_SE2_XY ? 2 : kind == EDGE_SE3_XYZ ? 3 : 7; }
inline int edge_info_len(int kind) { return edge_is_br(kind) ? 1 : kind == EDGE_SE2 ? 6 : kind == EDGE_SE2_XY ? 3 : kind == EDGE_SE3_XYZ ? 6 : 21; }
// the endpoint kinds an edge kind asks for
inline bool edge_endpoints_ok(int ek, int ka, int kb) {
  return (ek == EDGE_SE2 && ka == NODE_SE2 && kb == NODE_SE2) || ((ek == EDGE_SE2_XY || edge_is_br(ek)) && ka == NODE_SE2 && kb == NODE_XY) ||
         (ek == EDGE_SE3 && ka == NODE_SE3 && kb == NODE_SE3) || (ek == EDGE_SE3_XYZ && ka == NODE_SE3 && kb == NODE_XYZ);
}
inline bool node_is_3d(int kind) { return kind == NODE_SE3 || kind == NODE_XYZ; }
// a prior on a node is the edge of the node's own kind from a fixed identity pose (rr_pgo_set_priors)
inline int prior_edge_kind(int node_kind) {
  return node_kind == NODE_SE2 ? EDGE_SE2 : node_kind == NODE_XY ? EDGE_SE2_XY : node_kind == NODE_XYZ ? EDGE_SE3_XYZ : EDGE_SE3;
}
// The device keeps the information of every edge of a 3-D graph as the 21 entries of a 6 x 6 upper triangle: an SE3_XYZ
// edge's 6 values (3 x 3 upper triangle) go to the upper-left block, the rest is zero.  w: edge_info_len(kind) values.
template <typename S> inline void pack_info_3d(int kind, const double *w, S out[21]) {
  if (kind != EDGE_SE3_XYZ) {
    for (int t = 0; t < 21; t++) out[t] = (S)w[t];
    return;
  }
  for (int t = 0; t < 21; t++) out[t] = (S)0;
  out[0] = (S)w[0]; out[1] = (S)w[1]; out[2] = (S)w[2];   // row 0: (0,0) (0,1) (0,2)
  out[6] = (S)w[3]; out[7] = (S)w[4];                     // row 1: (1,1) (1,2)
  out[11] = (S)w[5];                                      // row 2: (2,2)
}

// The device form of a node's state and of an edge's measurement (the two numberings coincide), as two 4-vectors:
//   SE2  x, y, cos, sin | -      XY  x, y, 0, 0 | -      SE3  t (3), 0 | q (4) / |q|      XYZ  x, y, z, 0 | 0, 0, 0, 0
// the quaternion normalised like UnitQuaternion::from_quaternion, the norm in double.  Every conversion in the library is
// one of these two functions; the callers cast to the arithmetic type where they build the vectors.
inline double quat_norm(const double *q) { return std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); }
// s: node_state_len(kind) scalars in HostGraph's packing; returns how many it read
inline int pack_state(int kind, const double *s, double p[8]) {
  p[0] = s[0]; p[1] = s[1];
  p[2] = p[3] = p[4] = p[5] = p[6] = p[7] = 0.0;
  if (kind == NODE_SE2) {
    p[2] = std::cos(s[2]); p[3] = std::sin(s[2]);
  } else if (kind == NODE_SE3) {
    const double n = quat_norm(s + 3);
    p[2] = s[2];
    for (int t = 0; t < 4; t++) p[4 + t] = s[3 + t] / n;
  } else if (kind == NODE_XYZ) {
    p[2] = s[2];
  }
  return node_state_len(kind);
}
// The device form of an edge's measurement by EDGE kind.  The node numbering serves kinds 0 .. 3 as it is; a bearing z is packed
// as poses pack their angle, a range as it is, and lane 3 carries the kind (4 or 6, exact in every arithmetic type): the lane is
// zero in every SE2_XY record, and the code of the SE2_XY error reads lanes 0 and 1 alone.
//   BEARING  cos z, sin z, 0, 4 | -      RANGE  z, 0, 0, 6 | -
inline int pack_meas(int edge_kind, const double *m, double p[8]) {
  if (!edge_is_br(edge_kind)) return pack_state(edge_kind, m, p);
  for (int t = 0; t < 8; t++) p[t] = 0.0;
  if (edge_kind == EDGE_SE2_BEARING) { p[0] = std::cos(m[0]); p[1] = std::sin(m[0]); }
  else p[0] = m[0];
  p[3] = (double)edge_kind;
  return 1;
}
// the inverse (the angle of (cos, sin); the quaternion as it is); returns how many scalars it wrote
inline int unpack_state(int kind, const double p[8], double *s) {
  s[0] = p[0]; s[1] = p[1];
  if (kind == NODE_SE2) {
    s[2] = std::atan2(p[3], p[2]);
  } else if (kind == NODE_SE3) {
    s[2] = p[2];
    for (int t = 0; t < 4; t++) s[3 + t] = p[4 + t];
  } else if (kind == NODE_XYZ) {
    s[2] = p[2];
  }
  return node_state_len(kind);
}

// Same packing as rr_pgo_graph_desc (include/rr_pgo.h).
struct HostGraph {
  std::vector<int32_t> node_kind;
  std::vector<uint32_t> node_id;
  std::vector<int32_t> node_offset;     // scalar offset, vertex file order (g2o.rs:60-77)
  std::vector<int64_t> node_state_off;  // offset into node_state
  std::vector<double> node_state;       // SE2 x,y,theta | XY x,y | SE3 x,y,z,qx,qy,qz,qw | XYZ x,y,z
  std::vector<int32_t> edge_kind, edge_from, edge_to;
  std::vector<int64_t> edge_meas_off, edge_info_off;
  std::vector<double> edge_meas, edge_info;
  int32_t dim = 0;          // `len`
  int32_t anchor_node = -1; // from-node of the first pose-pose edge (prior, :330-336)
  bool has_se3 = false, has_2d = false;   // has_se3: the graph is 3-D (SE3 poses, XYZ landmarks)
  bool has_xyz = false;                   // ... and has XYZ landmarks
  bool has_br = false;                    // a 2-D graph with bearing-only or range-only edges

  int n_nodes() const { return (int)node_kind.size(); }
  int n_edges() const { return (int)edge_kind.size(); }
  // Recomputes offsets / anchor / flags from the kind + packed arrays; returns
  // an error string (empty = ok) after validating endpoints and kinds.
  std::string finalize();
};

// rr_pgo_remove_edges: the lowest node that has an edge now and none once the edges flagged in `gone` are taken out, -1: none
inline int first_orphan_node(int n_nodes, int n_edges, const int32_t *from, const int32_t *to, const char *gone) {
  std::vector<int32_t> before((size_t)n_nodes, 0), after((size_t)n_nodes, 0);
  for (int k = 0; k < n_edges; k++)
    for (const int v : {from[k], to[k]}) {
      before[(size_t)v]++;
      if (!gone[k]) after[(size_t)v]++;
    }
  for (int v = 0; v < n_nodes; v++)
    if (before[(size_t)v] > 0 && after[(size_t)v] == 0) return v;
  return -1;
}

// rr_pgo_remove_edges: g = og without the edges flagged in `gone` -- the nodes as they are, the remaining edges in their order
// (so compactly renumbered), their measurements and information packed anew; g is not finalized.  Returns the old index of
// every edge of g.
inline std::vector<int32_t> copy_without_edges(const HostGraph &og, const char *gone, HostGraph &g) {
  g.node_kind = og.node_kind;
  g.node_id = og.node_id;
  g.node_state = og.node_state;
  std::vector<int32_t> keep;
  for (int k = 0; k < og.n_edges(); k++) {
    if (gone[k]) continue;
    const int ek = og.edge_kind[k];
    keep.push_back(k);
    g.edge_kind.push_back(ek);
    g.edge_from.push_back(og.edge_from[k]);
    g.edge_to.push_back(og.edge_to[k]);
    const double *m = &og.edge_meas[og.edge_meas_off[k]], *w = &og.edge_info[og.edge_info_off[k]];
    g.edge_meas.insert(g.edge_meas.end(), m, m + edge_meas_len(ek));
    g.edge_info.insert(g.edge_info.end(), w, w + edge_info_len(ek));
  }
  return keep;
}

// rr_pgo_extend / rr_pgo_remove_edges: the robust edge mask of a rebuilt graph.  origin[k] is the old index of new edge k, -1
// for an edge the old graph did not have (a fresh edge is robustified: 1).  An empty mask (every edge) stays empty.
inline std::vector<uint8_t> reindex_edge_mask(const std::vector<uint8_t> &mask, const std::vector<int32_t> &origin) {
  std::vector<uint8_t> out;
  if (mask.empty()) return out;
  out.reserve(origin.size());
  for (const int32_t k : origin) out.push_back(k < 0 ? 1 : mask[(size_t)k]);
  return out;
}

// parse_g2o, g2o.rs:35-143.  Returns "" or an error message; io_error set when
// the file could not be read (Err(io) in the reference) as opposed to malformed.
std::string load_g2o(const char *path, HostGraph &g, bool &io_error);

// BASELINE config 4 generator.
void synth_grid(int width, int height, int64_t n_edges_target, uint64_t seed_meas,
                uint64_t seed_init, HostGraph &g);

}  // namespace rrpgo
