"""Small 3-D graphs whose supernode trees hold fronts beyond LDS, shared by tests/test_big_front_queries_cpu.py (the
generator and the references alone) and tests/test_big_front_queries_gpu.py (the five factor queries under
rr_pgo_set_query_big_fronts against them).  Nothing here needs a GPU.

se3_lattice(n, seed): n^3 SE(3) poses on a jittered lattice, node (z * n + y) * n + x at 2 * (x, y, z) +- 0.3 with a random
orientation, joined to its six lattice neighbours; the first edge stays first (the anchor), the others are shuffled;
measurements are random_graphs.se3_edge of the true poses, information matrices random_graphs.random_spd, the initial state
the truth plus noise (0.05 on the translation, 0.02 on the quaternion), as random_graphs.random_graph makes it.  A lattice
has separators that grow with n^2, so its top fronts leave LDS early: n = 5 has one such front (the root), n = 6 has fronts
beyond LDS with rows below their pivot block, n = 7 has several levels of them.  The GPU tests assert what they need of the
handle's own rr_pgo_stats, since the library chooses the tree.

landmark_lattice(): the n = 6 lattice plus 60 RR_PGO_NODE_XYZ landmarks, each seen from three seeded poses by
RR_PGO_EDGE_SE3_XYZ edges.

States (STATES): "initial" is the arrays' own; "gn3" is the state after three Gauss-Newton iterations of the CPU reference
(the oracle for the pose lattices, Landmarks3dReference for the landmark case)."""
import numpy as np

from marginals_reference import graph_at_state
from random_graphs import pack_upper, q_conj, q_rot, random_spd, se3_edge, unit_quat

LATTICES = {"lattice5": 5, "lattice6": 6, "lattice7": 7}
SEEDS = {5: 1505, 6: 1606, 7: 1707}
STATES = ("initial", "gn3")
N_LANDMARKS, SIGHTINGS, LANDMARK_SEED = 60, 3, 1660
QUERY_NODES = 14      # seeded nodes of the covariance tests: 84 columns, three chunks of 32
AUDIT_EDGES = 60      # seeded edges of the rr_pgo_check_edges test
_CACHE = {}


def _lattice(n, seed):
    """(arrays, true poses)"""
    rng = np.random.default_rng(seed)
    T = []
    for z in range(n):
        for y in range(n):
            for x in range(n):
                T.append((2.0 * np.array([x, y, z], np.float64) + rng.uniform(-0.3, 0.3, 3), unit_quat(rng.normal(size=4))))
    idx = lambda x, y, z: (z * n + y) * n + x
    pairs = []
    for z in range(n):
        for y in range(n):
            for x in range(n):
                if x + 1 < n:
                    pairs.append((idx(x, y, z), idx(x + 1, y, z)))
                if y + 1 < n:
                    pairs.append((idx(x, y, z), idx(x, y + 1, z)))
                if z + 1 < n:
                    pairs.append((idx(x, y, z), idx(x, y, z + 1)))
    edges = pairs[:1] + [pairs[1 + i] for i in rng.permutation(len(pairs) - 1)]
    ns = np.concatenate([np.concatenate([t + rng.normal(scale=0.05, size=3), unit_quat(q + rng.normal(scale=0.02, size=4))]) for t, q in T])
    em = [se3_edge(rng, T[a], T[b]) for a, b in edges]
    ei = [pack_upper(6, random_spd(rng, 6)) for _ in edges]
    arrays = (np.full(n ** 3, 2, np.int32), ns, np.full(len(edges), 2, np.int32), np.array([e[0] for e in edges], np.int32),
              np.array([e[1] for e in edges], np.int32), np.concatenate(em), np.concatenate(ei))
    return arrays, T


def se3_lattice(n, seed):
    """the n x n x n lattice in rr_pgo_graph_desc packing"""
    return _lattice(n, seed)[0]


def landmark_lattice():
    """the n = 6 lattice with N_LANDMARKS point landmarks appended as nodes 216 .. 275, their edges behind the lattice's"""
    (nk, ns, ek, ef, et, em, ei), T = _lattice(6, SEEDS[6])
    rng = np.random.default_rng(LANDMARK_SEED)
    n_pose = len(nk)
    lk, lf, lt, lm, li, ls = [], [], [], [], [], []
    for l in range(N_LANDMARKS):
        seen = sorted(int(v) for v in rng.choice(n_pose, SIGHTINGS, replace=False))
        p = np.mean([T[v][0] for v in seen], axis=0) + rng.uniform(-0.5, 0.5, 3)
        ls.append(p + rng.normal(scale=0.1, size=3))
        for v in seen:
            t, q = T[v]
            lk.append(3); lf.append(v); lt.append(n_pose + l)
            lm.append(q_rot(q_conj(q), p - t) + rng.normal(scale=0.03, size=3))
            li.append(pack_upper(3, random_spd(rng, 3)))
    return (np.concatenate([nk, np.full(N_LANDMARKS, 3, np.int32)]), np.concatenate([ns] + ls),
            np.concatenate([ek, np.array(lk, np.int32)]), np.concatenate([ef, np.array(lf, np.int32)]),
            np.concatenate([et, np.array(lt, np.int32)]), np.concatenate([em] + lm), np.concatenate([ei] + li))


def arrays_of(name):
    """the arrays of a case at its initial state: "lattice5", "lattice6", "lattice7" or "landmarks6" """
    if name not in _CACHE:
        _CACHE[name] = landmark_lattice() if name == "landmarks6" else se3_lattice(LATTICES[name], SEEDS[LATTICES[name]])
    return _CACHE[name]


def at_state(name, which):
    """(arrays with the node states of `which`, those states); computed once and left unchanged"""
    arrays = list(arrays_of(name))
    if which == "gn3":
        if (name, which) not in _CACHE:
            if name == "landmarks6":
                from landmarks3d_reference import Landmarks3dReference
                ref = Landmarks3dReference(arrays)
                for _ in range(3):
                    ref.update(ref.step())
                _CACHE[(name, which)] = ref.state()
            else:
                o = graph_at_state(arrays, arrays[1])
                o.optimize(3)
                _CACHE[(name, which)] = o.state()
        arrays[1] = _CACHE[(name, which)].copy()
    else:
        assert which == "initial"
        arrays[1] = np.asarray(arrays[1], np.float64).copy()
    return tuple(arrays), arrays[1]


def marginals_reference(name, which):
    """MarginalsReference of a pose lattice at a state, built once"""
    from marginals_reference import MarginalsReference
    key = ("marginals", name, which)
    if key not in _CACHE:
        arrays, state = at_state(name, which)
        _CACHE[key] = MarginalsReference(graph_at_state(arrays, state))
    return _CACHE[key]


def query_case(name, which):
    """dict(arrays, state, cand, sets, gate, joint) of a pose lattice at a state: gate_cases.candidates, gate_joint_cases.joint_sets
    and query_small_cases.references (GateReference.ref is the MarginalsReference of the case), built once"""
    from gate_cases import candidates
    from gate_joint_cases import joint_sets
    from query_small_cases import references
    key = ("query", name, which)
    if key not in _CACHE:
        arrays, state = at_state(name, which)
        cand = candidates(arrays, state)
        sets = joint_sets(len(cand[0]))
        gate, joint = references(("big-fronts", name, which), arrays, state, cand, sets)
        _CACHE[key] = dict(arrays=arrays, state=state, cand=cand, sets=sets, gate=gate, joint=joint)
    return _CACHE[key]


def audit_edges(arrays):
    """AUDIT_EDGES seeded edges of the graph, in a shuffled order"""
    return np.random.default_rng(1948).choice(len(arrays[2]), AUDIT_EDGES, replace=False).astype(np.int32)


def seeded_nodes(n_nodes, must, count=QUERY_NODES, seed=1431):
    """`count` distinct nodes: those of `must` (in that order), then seeded ones"""
    must = [int(v) for v in dict.fromkeys(int(v) for v in must)]
    rest = [int(v) for v in np.random.default_rng(seed).permutation(n_nodes) if int(v) not in must]
    return (must + rest)[:count]


def ordered_pairs(nodes):
    """(node_a, node_b): every ordered pair of `nodes`, a == b included, in covariances_cases.far_pairs' order"""
    return np.repeat(nodes, len(nodes)).astype(np.int32), np.tile(nodes, len(nodes)).astype(np.int32)
