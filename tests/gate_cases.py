"""Candidate edges shared by tests/test_gate_cpu.py and tests/test_gate_gpu.py (rr_pgo_gate_edges).

Per graph, at the state the tests gate at:
  - pose-pose candidates between the 24 seeded nodes of covariances_cases.far_nodes that are poses: every 9th ordered pair
    a != b (about 60: three or more chunks of columns; pairs whose common front is the root, pairs in one front, both
    orders of a pair);
  - one candidate that copies an existing edge (nodes, measurement and information);
  - one candidate whose `from` is the anchor;
  - on a graph with landmarks, SE2_XY candidates from the seeded poses to the seeded landmarks (every 3rd pair).
Omega is the information of the first existing edge of the candidate's kind.  The measurement is the relative pose at that
state -- the oracle's error of the same pair for an identity measurement, the SE(3) qw rebuilt from the vector part --
displaced by k * sigma * N(0, 1) per component, sigma = 1 / sqrt(diag Omega), seed 31, k cycling through LADDER.  No k = 0:
d2 would be exactly 0 and a relative comparison means nothing there.  (SE(3): the vector part of the displaced quaternion is
kept at most QV_MAX long, so that qw can be rebuilt from it.)"""
import numpy as np

from covariances_cases import far_nodes
from marginals_reference import graph_at_state

GATE_GRAPHS = {   # graph -> number of Gauss-Newton iterations before the gate
    "simulation-pose-pose": 10,
    "simulation-pose-landmark": 10,
    "parking-garage": 10,
    "intel": 0,   # the reference needs a dense inverse here (6-8 s): once, at the initial state
}
LADDER = (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)
SEED = 31
QV_MAX = 0.95   # a displaced SE(3) measurement whose quaternion vector part is longer is scaled back to this length
EDGE_DIM = {0: 3, 1: 2, 2: 6}
MEAS_LEN = {0: 3, 1: 2, 2: 7}
INFO_LEN = {0: 6, 1: 3, 2: 21}
IDENTITY = {0: [0.0, 0.0, 0.0], 1: [0.0, 0.0], 2: [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]}
# PoseGraph.gate's defaults: the 0.95 chi-square quantiles for d = 3, 2, 6 (by edge kind)
THRESHOLD = {0: 7.815, 1: 5.991, 2: 12.592}


def info_matrix(kind, packed):
    d = EDGE_DIM[int(kind)]
    W = np.zeros((d, d))
    W[np.triu_indices(d)] = packed
    return W + np.triu(W, 1).T


def split_packed(edge_kind, packed, length):
    out, o = [], 0
    for k in edge_kind:
        out.append(np.asarray(packed[o:o + length[int(k)]], np.float64))
        o += length[int(k)]
    return out


def with_candidates(arrays, state, cand):
    """OracleGraph of the graph at `state` with the candidates appended as edges n_edges, n_edges + 1, ..."""
    nk, _, ek, ef, et, em, ei = arrays
    kind, a, b, meas, info = cand
    return graph_at_state((nk, None, np.concatenate([ek, kind]), np.concatenate([ef, a]), np.concatenate([et, b]),
                           np.concatenate([em, meas]), np.concatenate([ei, info])), state)


def anchor_of(arrays):
    """from-node of the first pose-pose edge (rr_pgo_anchor_node)"""
    ek, ef = arrays[2], arrays[3]
    return int(ef[np.flatnonzero(ek != 1)[0]])


def candidates(arrays, state):
    """(kind, from, to, meas, info) of the graph's candidates at `state`, in rr_pgo_graph_desc packing"""
    nk, _, ek, ef, et, em, ei = arrays
    n = len(nk)
    pose_edge_kind = 2 if np.any(nk == 2) else 0
    seeded = far_nodes(n)
    poses = [v for v in seeded if nk[v] != 1]
    marks = [v for v in seeded if nk[v] == 1]
    pairs = [(a, b) for a in poses for b in poses if a != b][::9]
    kinds = [pose_edge_kind] * len(pairs)
    anchor = anchor_of(arrays)
    pairs.append((anchor, next(v for v in poses if v != anchor)))
    kinds.append(pose_edge_kind)
    lm = [(a, b) for a in poses for b in marks][::3]
    pairs += lm
    kinds += [1] * len(lm)
    kinds = np.array(kinds, np.int32)
    a = np.array([p[0] for p in pairs], np.int32)
    b = np.array([p[1] for p in pairs], np.int32)
    edge_meas, edge_info = split_packed(ek, em, MEAS_LEN), split_packed(ek, ei, INFO_LEN)
    first = {int(k): int(np.flatnonzero(ek == k)[0]) for k in np.unique(kinds)}
    info = [edge_info[first[int(k)]] for k in kinds]
    # ---- the relative pose at the state: the oracle's error for an identity measurement
    ident = (kinds, a, b, np.concatenate([IDENTITY[int(k)] for k in kinds]), np.concatenate(info))
    og = with_candidates(arrays, state, ident)
    rng = np.random.default_rng(SEED)
    meas = []
    for c, k in enumerate(kinds):
        rel = og.linearize_edge(len(ek) + c)[2]
        sigma = 1.0 / np.sqrt(np.diag(info_matrix(k, info[c])))
        z = rel + LADDER[c % len(LADDER)] * sigma * rng.standard_normal(len(rel))
        if k == 2:
            nv = np.linalg.norm(z[3:6])
            if nv > QV_MAX:   # far up the ladder: no unit quaternion has such a vector part
                z[3:6] *= QV_MAX / nv
            z = np.concatenate([z, [np.sqrt(1.0 - z[3:6] @ z[3:6])]])
        meas.append(z)
    # ---- the copy of an existing edge (the middle one of the pose-pose edges), as it is
    copy = int(np.flatnonzero(ek == pose_edge_kind)[np.sum(ek == pose_edge_kind) // 2])
    kinds = np.concatenate([kinds, [pose_edge_kind]]).astype(np.int32)
    a = np.concatenate([a, [ef[copy]]]).astype(np.int32)
    b = np.concatenate([b, [et[copy]]]).astype(np.int32)
    meas.append(edge_meas[copy])
    info.append(edge_info[copy])
    return kinds, a, b, np.concatenate(meas), np.concatenate(info)


def reverse(cand):
    """the same candidates in reverse order"""
    kind, a, b, meas, info = cand
    m, w = split_packed(kind, meas, MEAS_LEN), split_packed(kind, info, INFO_LEN)
    return kind[::-1].copy(), a[::-1].copy(), b[::-1].copy(), np.concatenate(m[::-1]), np.concatenate(w[::-1])


def select(cand, idx):
    """the candidates `idx` (a list of indices)"""
    kind, a, b, meas, info = cand
    m, w = split_packed(kind, meas, MEAS_LEN), split_packed(kind, info, INFO_LEN)
    return (kind[idx].copy(), a[idx].copy(), b[idx].copy(), np.concatenate([m[i] for i in idx]),
            np.concatenate([w[i] for i in idx]))


def thresholds(kind):
    return np.array([THRESHOLD[int(k)] for k in kind])
