"""Small graphs, their states, candidates and joint sets, shared by tests/test_query_small_cases_cpu.py (the references
alone) and tests/test_queries_small_graphs_gpu.py (rr_pgo_marginals, rr_pgo_covariances, rr_pgo_gate_edges and
rr_pgo_gate_joint against them).  Nothing here needs a GPU.

The graphs (GRAPHS, name -> arrays in rr_pgo_graph_desc packing):
  - se2-0 .. se2-11 and se3-0 .. se3-3: the random graphs of tests/test_gpu_parity.py's two random-graph tests, drawn as
    those tests draw them (seeds 1000 + s and 2000 + s);
  - two-poses (one edge, dim 6), landmark-first (two poses, one landmark, the landmark edge first in the edge list, so the
    anchor is the `from` of a later edge), se3-chain3 (three SE(3) poses in a chain), clique5 (five poses, all ten edges);
  - mid-se2 (420 poses, 60 landmarks seen from two or three neighbouring poses; a loop closure from every third pose to a
    pose at most 24 back) and mid-se3 (400 poses; a closure from every second pose to a pose at most 48 back): odometry
    chains with local closures, so that every front stays in LDS.  The host analysis gives 41 and 90 fronts; under the
    level schedule (RR_PGO_LDS_FLOW=0), where rr_pgo_stats::n_levels counts the levels of the task tree and not the one
    dataflow launch, mid-se3 keeps its 90 fronts and has 5 levels (320 poses with closures at most 24 back: 4).
The states (STATES): "initial" is the arrays' own; "moved" is that state after OracleGraph.update_nodes with a seeded
N(0, 0.05^2) step, read back from the oracle.  Both are arrays the GPU test hands to PoseGraph.from_arrays.

Candidates (small_candidates): every ordered pose pair a != b, every `stride`-th of them with stride = ceil(pairs /
MAX_PAIRS), then one candidate whose `from` is the anchor, then every third (pose, landmark) pair as SE2_XY (thinned
in the same way to at most MAX_MARK_PAIRS), then a copy of the middle pose-pose edge.  Omega and the measurement are
built as tests/gate_cases.py builds them: the information of the first existing edge of the kind, the relative pose at
the state displaced by LADDER[c % 8] sigma.

Joint sets (small_joint_sets returns (sets, left_out)): gate_joint_cases.joint_sets where the graph has at least 8
candidates (its shapes index the first 8, the last 8 and candidate 3), else the one-candidate set, the whole list and a
candidate twice; and
  - 2-D: 9, 12 and 16 SE2 candidates (D_s = 27, 36, 48), once the first ones in candidate order (every rung of the ladder)
    and once the first ones of rungs 0 and 1 (sets that pass); 16 SE2_XY candidates (D_s = 32); 16 candidates of which
    one occurs three times; a mixed set of 15 SE2 + 1 SE2_XY (D_s = 47) and one of 12 SE2 + 4 SE2_XY (D_s = 44), the
    landmark candidates in the middle of the set;
  - SE(3): 1, 2, 7 and 8 candidates (D_s = 6 .. 48), in candidate order and of rungs 0 and 1.
A MIXED set of 16 cannot reach 48: 3 a + 2 b = 48 with a + b <= 16 has the one solution a = 16, b = 0, which is the set
of 16 SE2 candidates; the mixed sets stop at 47.  A graph with too few candidates of a kind leaves the shape out;
`left_out` names every shape left out and why (two-poses, landmark-first, se3-chain3 and clique5 have 4 .. 22
candidates; a random graph without landmarks has no SE2_XY set)."""
import numpy as np

from covariances_cases import FLOOR_MAX   # noqa: F401  (re-exported: the one bound on a floor)
from gate_cases import (EDGE_DIM, IDENTITY, INFO_LEN, LADDER, MEAS_LEN, QV_MAX, SEED, anchor_of, info_matrix, split_packed,
                        with_candidates)
from gate_joint_cases import joint_sets
from marginals_reference import graph_at_state
from random_graphs import pack_upper, q_conj, q_mul, q_rot, random_graph, random_spd, se2_edge, se3_edge, unit_quat

STATES = ("initial", "moved")
MAX_PAIRS = 600        # ordered pose pairs per graph
MAX_MARK_PAIRS = 200   # (pose, landmark) pairs per graph
MOVE_SEED, MOVE_SCALE = 77, 0.05
ALL_PAIRS_MAX_NODES = 80     # all ordered node pairs up to here, SEEDED_NODES seeded nodes and all their pairs beyond
SEEDED_NODES = 40


# ---- the graphs ------------------------------------------------------------------------------------------------------------

def _se2(s):
    rng = np.random.default_rng(1000 + s)
    n_pose = int(rng.integers(2, 70))
    return random_graph(rng, n_pose, int(rng.integers(0, 25)) if s % 3 else 0, int(rng.integers(0, 2 * n_pose)))


def _se3(s):
    rng = np.random.default_rng(2000 + s)
    n_pose = int(rng.integers(3, 40))
    return random_graph(rng, n_pose, 0, int(rng.integers(0, n_pose)), se3=True)


def _chain_pairs(rng, n_pose, every, reach):
    """odometry i -> i + 1, and from every `every`-th pose a closure to a pose 2 .. `reach` back (either direction)"""
    pairs = [(i, i + 1) for i in range(n_pose - 1)]
    for i in range(3, n_pose, every):
        j = i - int(rng.integers(2, min(i, reach) + 1))
        pairs.append((i, j) if rng.integers(0, 2) else (j, i))
    return pairs


def _mid_se2(seed, n_pose, n_lm, every, reach):
    rng = np.random.default_rng(seed)
    th = np.cumsum(rng.normal(scale=0.15, size=n_pose))
    X = np.column_stack([np.cumsum(np.cos(th)), np.cumsum(np.sin(th)), th])
    seen = [int(v) for v in np.sort(rng.choice(n_pose - 3, n_lm, replace=False))]
    Lm = np.array([X[p, :2] + rng.uniform(-2, 2, 2) for p in seen])
    pairs = _chain_pairs(rng, n_pose, every, reach)
    sights = [(p + k, n_pose + l) for l, p in enumerate(seen) for k in range(int(rng.integers(2, 4)))]
    rest = pairs[1:] + sights
    edges = pairs[:1] + [rest[i] for i in rng.permutation(len(rest))]
    nk = np.concatenate([np.zeros(n_pose, np.int32), np.ones(n_lm, np.int32)])
    ns = np.concatenate([(X + rng.normal(scale=[0.1, 0.1, 0.03], size=X.shape)).ravel(), (Lm + rng.normal(scale=0.1, size=Lm.shape)).ravel()])
    ek, em, ei = [], [], []
    for a, b in edges:
        pose = b < n_pose
        ek.append(0 if pose else 1)
        em.append(se2_edge(rng, X[a], X[b] if pose else Lm[b - n_pose]))
        ei.append(pack_upper(3, random_spd(rng, 3)) if pose else pack_upper(2, random_spd(rng, 2)))
    return (nk, ns, np.array(ek, np.int32), np.array([e[0] for e in edges], np.int32), np.array([e[1] for e in edges], np.int32),
            np.concatenate(em), np.concatenate(ei))


def _mid_se3(seed, n_pose, every, reach):
    rng = np.random.default_rng(seed)
    T, t, q = [], np.zeros(3), unit_quat(rng.normal(size=4))
    for _ in range(n_pose):
        T.append((t.copy(), q.copy()))
        q = unit_quat(q_mul(q, unit_quat(np.concatenate([rng.normal(scale=0.1, size=3), [1.0]]))))
        t = t + q_rot(q, np.array([1.0, 0.0, 0.0]))
    pairs = _chain_pairs(rng, n_pose, every, reach)
    edges = pairs[:1] + [pairs[1 + i] for i in rng.permutation(len(pairs) - 1)]
    nk = np.full(n_pose, 2, np.int32)
    ns = np.concatenate([np.concatenate([t + rng.normal(scale=0.05, size=3), unit_quat(q + rng.normal(scale=0.02, size=4))]) for t, q in T])
    em = [se3_edge(rng, T[a], T[b]) for a, b in edges]
    ei = [pack_upper(6, random_spd(rng, 6)) for _ in edges]
    return (nk, ns, np.full(len(edges), 2, np.int32), np.array([e[0] for e in edges], np.int32), np.array([e[1] for e in edges], np.int32),
            np.concatenate(em), np.concatenate(ei))


def _two_poses():
    return (np.zeros(2, np.int32), np.array([0.1, -0.2, 0.05, 1.3, 0.4, -0.1]), np.zeros(1, np.int32), np.array([0], np.int32),
            np.array([1], np.int32), np.array([1.0, 0.5, -0.2]), np.array([10.0, 1, 0, 20, 2, 30]))


def _landmark_first():
    """poses 0 and 1, landmark 2; edge 0 is the sighting 1 -> 2, edge 1 the pose-pose edge 1 -> 0 (the anchor is node 1)"""
    return (np.array([0, 0, 1], np.int32), np.array([0.1, -0.2, 0.05, 1.3, 0.4, -0.1, 2.0, 1.5]), np.array([1, 0], np.int32),
            np.array([1, 1], np.int32), np.array([2, 0], np.int32), np.array([0.8, 1.0, -1.1, -0.7, 0.2]),
            np.array([15.0, 2, 12, 10.0, 1, 0, 20, 2, 30]))


def _se3_chain3():
    rng = np.random.default_rng(3003)
    T = [(rng.uniform(-2, 2, 3), unit_quat(rng.normal(size=4))) for _ in range(3)]
    edges = [(0, 1), (1, 2)]
    ns = np.concatenate([np.concatenate([t + rng.normal(scale=0.05, size=3), unit_quat(q + rng.normal(scale=0.02, size=4))]) for t, q in T])
    return (np.full(3, 2, np.int32), ns, np.full(2, 2, np.int32), np.array([0, 1], np.int32), np.array([1, 2], np.int32),
            np.concatenate([se3_edge(rng, T[a], T[b]) for a, b in edges]), np.concatenate([pack_upper(6, random_spd(rng, 6)) for _ in edges]))


def _clique5():
    rng = np.random.default_rng(5005)
    X = np.column_stack([rng.uniform(-3, 3, 5), rng.uniform(-3, 3, 5), rng.uniform(-np.pi, np.pi, 5)])
    edges = [(a, b) if (a + b) % 2 else (b, a) for a in range(5) for b in range(a + 1, 5)]
    ns = (X + rng.normal(scale=[0.1, 0.1, 0.03], size=X.shape)).ravel()
    return (np.zeros(5, np.int32), ns, np.zeros(10, np.int32), np.array([e[0] for e in edges], np.int32), np.array([e[1] for e in edges], np.int32),
            np.concatenate([se2_edge(rng, X[a], X[b]) for a, b in edges]), np.concatenate([pack_upper(3, random_spd(rng, 3)) for _ in edges]))


_BUILDERS = {f"se2-{s}": (lambda s=s: _se2(s)) for s in range(12)}
_BUILDERS.update({f"se3-{s}": (lambda s=s: _se3(s)) for s in range(4)})
_BUILDERS.update({"two-poses": _two_poses, "landmark-first": _landmark_first, "se3-chain3": _se3_chain3, "clique5": _clique5,
                  "mid-se2": lambda: _mid_se2(4001, 420, 60, 3, 24), "mid-se3": lambda: _mid_se3(4002, 400, 2, 48)})
GRAPHS = list(_BUILDERS)
MID = ("mid-se2", "mid-se3")
_CACHE = {}


def arrays_of(name):
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name]()
    return _CACHE[name]


def state_of(name, which):
    """the node states the tests query at: the graph's own, or those after a seeded update_nodes step of the oracle"""
    arrays = arrays_of(name)
    if which == "initial":
        return np.asarray(arrays[1], np.float64).copy()
    assert which == "moved"
    if (name, which) not in _CACHE:
        o = graph_at_state(arrays, arrays[1])
        o.update_nodes(np.random.default_rng(MOVE_SEED).normal(scale=MOVE_SCALE, size=o.dim))
        _CACHE[(name, which)] = o.state()
    return _CACHE[(name, which)].copy()


def at_state(name, which):
    """(arrays with the node states of `which`, those states)"""
    a = list(arrays_of(name))
    a[1] = state_of(name, which)
    return tuple(a), a[1]


# ---- node pairs ------------------------------------------------------------------------------------------------------------

def pair_nodes(n):
    """every node of a graph of at most ALL_PAIRS_MAX_NODES nodes, SEEDED_NODES seeded ones of a larger graph"""
    if n <= ALL_PAIRS_MAX_NODES:
        return list(range(n))
    return sorted(int(v) for v in np.random.default_rng(SEED).choice(n, SEEDED_NODES, replace=False))


def all_pairs(n):
    """(nodes, node_a, node_b): all ordered pairs of pair_nodes(n), a == b included, in covariances_cases.far_pairs' order"""
    nodes = pair_nodes(n)
    return nodes, np.repeat(nodes, len(nodes)).astype(np.int32), np.tile(nodes, len(nodes)).astype(np.int32)


# ---- candidates ------------------------------------------------------------------------------------------------------------

def small_candidates(arrays, state):
    """(kind, from, to, meas, info) of the graph's candidates at `state`, in rr_pgo_graph_desc packing"""
    nk, _, ek, ef, et, em, ei = arrays
    pose_edge_kind = 2 if np.any(nk == 2) else 0
    poses = [int(v) for v in np.flatnonzero(nk != 1)]
    marks = [int(v) for v in np.flatnonzero(nk == 1)]
    pairs = [(a, b) for a in poses for b in poses if a != b]
    pairs = pairs[::-(-len(pairs) // MAX_PAIRS)]
    anchor = anchor_of(arrays)
    pairs.append((anchor, next(v for v in poses if v != anchor)))
    kinds = [pose_edge_kind] * len(pairs)
    lm = [(a, b) for a in poses for b in marks][::3]
    lm = lm[::-(-len(lm) // MAX_MARK_PAIRS)] if lm else lm
    pairs += lm
    kinds = np.array(kinds + [1] * len(lm), np.int32)
    a = np.array([p[0] for p in pairs], np.int32)
    b = np.array([p[1] for p in pairs], np.int32)
    edge_meas, edge_info = split_packed(ek, em, MEAS_LEN), split_packed(ek, ei, INFO_LEN)
    first = {int(k): int(np.flatnonzero(ek == k)[0]) for k in np.unique(kinds)}
    info = [edge_info[first[int(k)]] for k in kinds]
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
            if nv > QV_MAX:
                z[3:6] *= QV_MAX / nv
            z = np.concatenate([z, [np.sqrt(1.0 - z[3:6] @ z[3:6])]])
        meas.append(z)
    copy = int(np.flatnonzero(ek == pose_edge_kind)[np.sum(ek == pose_edge_kind) // 2])
    kinds = np.concatenate([kinds, [pose_edge_kind]]).astype(np.int32)
    a = np.concatenate([a, [ef[copy]]]).astype(np.int32)
    b = np.concatenate([b, [et[copy]]]).astype(np.int32)
    meas.append(edge_meas[copy])
    info.append(edge_info[copy])
    return kinds, a, b, np.concatenate(meas), np.concatenate(info)


# ---- joint sets ------------------------------------------------------------------------------------------------------------

BIG = (9, 12, 16)   # the set sizes k_gate_joint<double, 3> never saw: m in 9 .. 16, D_s in 27 .. 48


def small_joint_sets(kind):
    """(sets, left_out): ordered lists of candidate indices, and the shapes this graph is too small for"""
    n = len(kind)
    sets, left_out = [], []

    def add(what, need, pool, build):
        if len(pool) < need:
            left_out.append(f"{what}: needs {need} candidates of its kind, the graph has {len(pool)}")
        else:
            sets.append(build(pool))

    if n >= 8:
        sets += [s for s in joint_sets(n) if s]
    else:
        left_out.append(f"gate_joint_cases.joint_sets: indexes the first 8, the last 8 and candidate 3, the graph has {n} candidates")
        sets += [[0], list(range(n)), [n - 1, n - 1]]
    low = [c for c in range(n) if c % len(LADDER) < 2]
    if np.any(kind == 2):
        p = [c for c in range(n) if kind[c] == 2]
        for m in (1, 2, 7, 8):
            add(f"{m} SE3 candidates", m, p, lambda q, m=m: q[:m])
            add(f"{m} SE3 candidates of rungs 0 and 1", m, [c for c in p if c in low], lambda q, m=m: q[:m])
        return sets, left_out
    p = [c for c in range(n) if kind[c] == 0]
    xy = [c for c in range(n) if kind[c] == 1]
    for m in BIG:
        add(f"{m} SE2 candidates", m, p, lambda q, m=m: q[:m])
        add(f"{m} SE2 candidates of rungs 0 and 1", m, [c for c in p if c in low], lambda q, m=m: q[:m])
    add("16 SE2_XY candidates", 16, xy, lambda q: q[:16])
    add("16 SE2 candidates, one of them three times", 14, p, lambda q: q[:5] + [q[2]] + q[5:13] + [q[2]] + q[13:14])
    if len(xy) < 4:
        left_out.append(f"mixed sets of 16 (D_s = 47, 44): need 4 SE2_XY candidates, the graph has {len(xy)}")
    else:
        add("15 SE2 + 1 SE2_XY", 15, p, lambda q: q[:7] + xy[:1] + q[7:15])
        add("12 SE2 + 4 SE2_XY", 12, p, lambda q: q[:3] + xy[:2] + q[3:9] + xy[2:4] + q[9:12])
    return sets, left_out


def set_dim(kind, members):
    return sum(EDGE_DIM[int(kind[c])] for c in members)


def big_sets(kind):
    """the sets of 9 .. 16 members among small_joint_sets(kind): what the dataset cases add to gate_joint_cases.joint_sets"""
    return [s for s in small_joint_sets(kind)[0] if len(s) >= 9]


# ---- a graph at a state with its candidates, sets and references (built once, shared by every test of a module) ------------------

DATASETS = ("simulation-pose-pose", "intel")   # the sets of 9, 12 and 16 on real trees, at the states gate_cases.GATE_GRAPHS names


def case(name, which):
    """dict(arrays, state, cand, sets, left_out) of graph `name` at state `which`; arrays hold that state"""
    key = ("case", name, which)
    if key not in _CACHE:
        arrays, state = at_state(name, which)
        cand = small_candidates(arrays, state)
        sets, left_out = small_joint_sets(cand[0])
        _CACHE[key] = dict(arrays=arrays, state=state, cand=cand, sets=sets, left_out=left_out)
    return _CACHE[key]


def references(key, arrays, state, cand, sets):
    """(GateReference, JointReference) of the case, cached by `key`; GateReference.ref is the MarginalsReference of the
    graph at the state, so one dense inverse serves every comparison of the case"""
    from gate_joint_reference import JointReference
    from gate_reference import GateReference
    key = ("ref",) + tuple(key)
    if key not in _CACHE:
        gate = GateReference(arrays, state, cand)
        _CACHE[key] = (gate, JointReference(arrays, state, cand, sets, gate=gate))
    return _CACHE[key]
