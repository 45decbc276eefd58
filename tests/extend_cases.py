"""Graphs shared by tests/test_extend_cpu.py and tests/test_extend_gpu.py (rr_pgo_extend).

Per source file the BASE graph is the file without its last M_NODES = 6 nodes, every edge that touches one of them, and
K_EDGES = 8 further seeded edges between non-consecutive nodes of what remains (loop closures; in the pose-landmark file,
whose pose-pose edges are all odometry, repeated sightings of a landmark); the ADDITION is exactly what
was removed, in file order: the removed nodes (they are the last ones, so their indices are those rr_pgo_extend gives them)
and the removed edges.  base + addition is therefore the file's graph with the removed edges moved to the end -- the GROWN
graph, which is what a fresh handle is built from.

In simulation-pose-landmark the last six nodes are poses, and some landmarks are seen from those poses only: without them
they would be left in the base graph with no measurement at all (a disconnected graph, a singular system).  Such nodes -- every
node all of whose edges go to removed nodes -- are removed WITH the last six and listed in front of them in the addition, in
file order, so the kept nodes keep their relative order and the addition also brings landmarks seen from new poses.  intel and
parking-garage have no such node: there the node order is the file's.

All arrays are in rr_pgo_graph_desc / og_create packing and come from the oracle's loader, so nothing here needs a device.
tests/test_extend_cpu.py checks that every base graph stays connected, keeps a pose-pose edge, and that the oracle optimises
base and grown graph without a failed factorisation (SEED was picked so that this holds)."""
import functools

import numpy as np

from conftest import g2o_path
from gate_cases import INFO_LEN, MEAS_LEN, split_packed
from oracle.oracle import OracleGraph
from robust_reference import oracle_arrays

SOURCES = ["intel", "simulation-pose-landmark", "parking-garage"]   # SE2, SE2 + XY, SE3
M_NODES = 6
K_EDGES = 8
SEED = 7
STATE_LEN = {0: 3, 1: 2, 2: 7}


class Case:
    """base / grown: 7-tuples (node_kind, node_state, edge_kind, from, to, meas, info); addition: the arguments of
    PoseGraph.extend -- (edge_kind, from, to, meas, info, node_kind, node_state)"""

    def __init__(self, base, addition, grown, removed_edges):
        self.base, self.addition, self.grown, self.removed_edges = base, addition, grown, removed_edges
        self.n_base, self.e_base = len(base[0]), len(base[2])

    def extend_args(self, with_state=True):
        ek, ef, et, em, ei, nk, ns = self.addition
        return (ek, ef, et, em, ei), dict(node_kind=nk, node_state=ns if with_state else None)


def select_edges(arrays, idx):
    nk, ns, ek, ef, et, em, ei = arrays
    m, w = split_packed(ek, em, MEAS_LEN), split_packed(ek, ei, INFO_LEN)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)   # noqa: E731
    return (ek[idx].astype(np.int32), ef[idx].astype(np.int32), et[idx].astype(np.int32),
            cat([m[i] for i in idx]), cat([w[i] for i in idx]))


def split_case(arrays, m_nodes=M_NODES, k_edges=K_EDGES, seed=SEED):
    nk, ns, ek, ef, et, em, ei = [np.asarray(a) for a in arrays]
    n = len(nk)
    # the removed nodes: the last m_nodes, and every node all of whose edges go to removed nodes (see the module docstring)
    gone_node = np.zeros(n, bool)
    gone_node[n - m_nodes:] = m_nodes > 0
    while True:
        has_kept_edge = np.zeros(n, bool)
        live = ~gone_node[ef] & ~gone_node[et]
        has_kept_edge[ef[live]] = True
        has_kept_edge[et[live]] = True
        orphan = ~gone_node & ~has_kept_edge
        if not m_nodes or not orphan.any():
            break
        gone_node |= orphan
    order = np.concatenate([np.flatnonzero(~gone_node), np.flatnonzero(gone_node)])   # kept nodes, then removed ones: file order in both
    new_index = np.empty(n, np.int64)
    new_index[order] = np.arange(n)
    states = [ns[o:o + STATE_LEN[int(k)]] for k, o in zip(nk, np.concatenate([[0], np.cumsum([STATE_LEN[int(k)] for k in nk])]))]
    nk = nk[order]
    ns = np.concatenate([states[v] for v in order])
    ef, et = new_index[ef].astype(np.int32), new_index[et].astype(np.int32)
    arrays = (nk, ns, ek, ef, et, em, ei)
    n_base = n - int(gone_node.sum())
    soff = np.concatenate([[0], np.cumsum([STATE_LEN[int(k)] for k in nk])]).astype(int)
    touching = (ef >= n_base) | (et >= n_base)
    closures = np.flatnonzero(~touching & (np.abs(ef - et) > 1))
    picked = np.random.default_rng(seed).choice(closures, k_edges, replace=False)
    removed = np.zeros(len(ek), bool)
    removed[touching] = True
    removed[picked] = True
    keep, gone = np.flatnonzero(~removed), np.flatnonzero(removed)
    base = (nk[:n_base].astype(np.int32), ns[:soff[n_base]].copy()) + select_edges(arrays, keep)
    add_edges = select_edges(arrays, gone)
    addition = add_edges + (nk[n_base:].astype(np.int32), ns[soff[n_base]:].copy())
    grown = (nk.astype(np.int32), ns.copy()) + tuple(np.concatenate([b, a]) for b, a in zip(base[2:], add_edges))
    return Case(base, addition, grown, gone)


@functools.lru_cache(maxsize=None)
def source_arrays(name):
    return tuple(oracle_arrays(OracleGraph.load(g2o_path(name))))


@functools.lru_cache(maxsize=None)
def case(name):
    return split_case(source_arrays(name))


def closures_only(name, count):
    """(base, addition, grown) of a file without `count` seeded loop closures and no node removed (sphere2500: a graph with
    fronts beyond LDS)"""
    return split_case(source_arrays(name), m_nodes=0, k_edges=count)


def connected(arrays):
    """the graph is one component"""
    n, ef, et = len(arrays[0]), arrays[3], arrays[4]
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b in zip(ef, et):
        parent[find(int(a))] = find(int(b))
    return len({find(v) for v in range(n)}) == 1
