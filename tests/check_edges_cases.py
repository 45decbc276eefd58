"""Fixtures shared by tests/test_check_edges_cpu.py (the reference alone) and tests/test_check_edges_gpu.py
(rr_pgo_check_edges against it).  Nothing here needs a GPU.

Small graphs, all edges, at both states of query_small_cases.STATES:
  - of tests/query_small_cases.py: two-poses (one bridge), landmark-first, clique5, se3-chain3 (SE(3) bridges), four of the
    seeded se2-* graphs (SE2_SEEDS) and mid-se2 (a tree of many fronts);
  - mid-se3-320: query_small_cases' mid-se3 builder with 320 poses and closures at most 24 back (a tree of many fronts,
    4 levels).  mid-se3 itself (400 poses, closures 48 back) does not meet the condition of tests/test_check_edges_cpu.py:
    the reference's own two computations of d2 differ by 2e-6 there, above FLOOR_MAX;
  - triangle: three SE(2) poses, three edges -- one front under 16 rows, every tile clamped;
  - landmarks-1-3: four poses in a loop, one landmark seen once (a bridge) and one seen three times;
  - parallel: three poses in a chain, two edges on the pair (0, 1) (a cycle of two) and the bridge (1, 2).
PARTIAL (se2-1, se2-11) are graphs with edges at r = 0.05 .. 0.41 whose R is singular to rounding in one direction; ROBUST
(se2-5, se2-8) are the graphs of the Cauchy case, at the moved state -- both explained where they are defined.
BRIDGE_ONLY names the graphs all of whose edges are bridges: nothing else constrains any of their residuals, so none of
their edges can be compared in d2 and R; they check r against 0.
Datasets, at the states gate_cases.GATE_GRAPHS names: all edges of simulation-pose-landmark, 64 seeded edges of intel (32
non-consecutive ones, 32 consecutive ones), 32 seeded edges of parking-garage (16 and 16)."""
import numpy as np

import query_small_cases as qs
from marginals_reference import graph_at_state
from random_graphs import pack_upper, random_spd, se2_edge

SE2_SEEDS = (2, 4, 5, 8)
# Graphs with PARTIAL redundancy: edges at r = 0.05 .. 0.41 whose R is singular to rounding in one direction (a pose whose
# heading nothing but that edge determines), so that d2 is NaN or 1e13 and up -- rounding decides.  Kept for r, R and the
# smallest directional redundancy, and for what PoseGraph.suspect_edges does with such edges; d2 is compared on the others.
PARTIAL = ("se2-1", "se2-11")
# Robust fixtures (Cauchy, delta 1, two edges of three masked in), at the MOVED state: at a file's initial state the odometry
# edges' errors are zero up to rounding, and d2 = e^T R^-1 e of such an edge is rounding too.
ROBUST = ("se2-5", "se2-8")   # (mid-se2 under Cauchy: the reference's two d2 differ by 4e-6, above FLOOR_MAX)
SMALL = ["two-poses", "triangle", "landmark-first", "clique5", "se3-chain3", "landmarks-1-3", "parallel"] + \
        [f"se2-{s}" for s in SE2_SEEDS] + ["mid-se2", "mid-se3-320"]
BRIDGE_ONLY = ("two-poses", "landmark-first", "se3-chain3")
DATASET_EDGES = {"simulation-pose-landmark": None, "intel": 64, "parking-garage": 32}
SEED = 48   # (picked so that tests/test_check_edges_cpu.py's condition holds on parking-garage: with seeds 41 .. 44 a queried
            # edge on a long loop has r just below 0.01, or the reference's two computations of d2 differ by more than FLOOR_MAX)
_CACHE = {}


def robust_mask(n_edges):
    return (np.arange(n_edges) % 3 != 0).astype(np.int32)


def _se2_graph(seed, X, Lm, edges):
    """poses X (n x 3), landmarks Lm (m x 2), edges (from, to) with landmark m numbered n + m"""
    rng = np.random.default_rng(seed)
    n = len(X)
    nk = np.concatenate([np.zeros(n, np.int32), np.ones(len(Lm), np.int32)])
    ns = np.concatenate([(X + rng.normal(scale=[0.1, 0.1, 0.03], size=X.shape)).ravel(),
                         (Lm + rng.normal(scale=0.1, size=Lm.shape)).ravel() if len(Lm) else np.zeros(0)])
    ek, em, ei = [], [], []
    for a, b in edges:
        pose = b < n
        ek.append(0 if pose else 1)
        em.append(se2_edge(rng, X[a], X[b] if pose else Lm[b - n]))
        ei.append(pack_upper(3, random_spd(rng, 3)) if pose else pack_upper(2, random_spd(rng, 2)))
    return (nk, ns, np.array(ek, np.int32), np.array([e[0] for e in edges], np.int32), np.array([e[1] for e in edges], np.int32),
            np.concatenate(em), np.concatenate(ei))


def _triangle():
    X = np.array([[0.0, 0.0, 0.1], [1.0, 0.2, 0.8], [0.4, 1.1, -2.0]])
    return _se2_graph(6001, X, np.zeros((0, 2)), [(0, 1), (1, 2), (2, 0)])


def _landmarks_1_3():
    X = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 1.5], [1.0, 1.0, 3.0], [0.0, 1.0, -1.6]])
    Lm = np.array([[2.0, 0.5], [0.5, 0.5]])
    return _se2_graph(6002, X, Lm, [(0, 1), (1, 2), (2, 3), (3, 0), (1, 4), (0, 5), (2, 5), (3, 5)])


def _parallel():
    X = np.array([[0.0, 0.0, 0.3], [1.2, 0.1, 0.5], [2.0, 0.9, 1.0]])
    return _se2_graph(6003, X, np.zeros((0, 2)), [(0, 1), (1, 2), (1, 0)])


_OWN = {"triangle": _triangle, "landmarks-1-3": _landmarks_1_3, "parallel": _parallel,
        "mid-se3-320": lambda: qs._mid_se3(4002, 320, 2, 24)}


def arrays_of(name):
    if name not in _OWN:
        return qs.arrays_of(name)
    if name not in _CACHE:
        _CACHE[name] = _OWN[name]()
    return _CACHE[name]


def at_state(name, which):
    """(arrays with the node states of `which`, those states), as query_small_cases.at_state"""
    if name not in _OWN:
        return qs.at_state(name, which)
    arrays = list(arrays_of(name))
    if which == "moved":
        if (name, which) not in _CACHE:
            o = graph_at_state(arrays, arrays[1])
            o.update_nodes(np.random.default_rng(qs.MOVE_SEED).normal(scale=qs.MOVE_SCALE, size=o.dim))
            _CACHE[(name, which)] = o.state()
        arrays[1] = _CACHE[(name, which)].copy()
    else:
        assert which == "initial"
        arrays[1] = np.asarray(arrays[1], np.float64).copy()
    return tuple(arrays), arrays[1]


def seeded_edges(arrays, count):
    """`count` seeded edges, half of them non-consecutive (|from - to| > 1), half consecutive, in one shuffled list; None: all"""
    if count is None:
        return None
    ef, et = np.asarray(arrays[3], np.int64), np.asarray(arrays[4], np.int64)
    rng = np.random.default_rng(SEED)
    far = rng.choice(np.flatnonzero(np.abs(ef - et) > 1), count // 2, replace=False)
    near = rng.choice(np.flatnonzero(np.abs(ef - et) == 1), count - count // 2, replace=False)
    return rng.permutation(np.concatenate([far, near])).astype(np.int32)


def reference(key, arrays, state, edges=None, **kw):
    """CheckReference of the case, computed once per `key` and left unchanged"""
    from check_edges_reference import CheckReference
    key = ("ref",) + tuple(key)
    if key not in _CACHE:
        _CACHE[key] = CheckReference(arrays, state, edges, **kw)
    return _CACHE[key]
