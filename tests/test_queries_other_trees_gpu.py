"""The factor queries on OTHER supernode partitions of the same matrix: simulation-pose-pose, intel and parking-garage at
the states gate_cases.GATE_GRAPHS names, on handles created under the switches of the analysis that change the tree
(the values tests/test_gpu_parity.py already runs the factorisation under).  Another partition is another nc, nr, rel
and depth for every front k_selinv_level, k_marg_gather, k_tree_fwd, k_cov_pairs, k_gate_pairs and k_gate_joint index
with, and other pairs that share a front.

The state is the default handle's, set on every pinned handle, so ONE reference per file (built once per module) serves
every pin, by the rule of the dataset tests: a GPU value passes at max(1e-12, 100 x noise floor), the floor at most
FLOOR_MAX = 1e-6, every comparison prints its worst figure, the floor and the tolerance before it asserts.  Pairs that
share no front differ from tree to tree, so rr_pgo_marginals is asked for diagonal blocks and for pairs joined by an edge.

(n_supernodes, n_levels, max_front) of PoseGraph.analyze(file) under each pin, on the host, through the library's own
choice among its candidate trees (n_levels is 1 throughout: every front fits LDS, the factorisation is one dataflow launch;
no tree has a front beyond LDS):

    pin                                          simulation-pose-pose   intel            parking-garage
    none (the default tree)                      (28, 1, 138)           (157, 1, 165)    (190, 1, 174)
    ND_LEAF=50 AMALG_NP=16 JOIN_SEPARATORS=0     (27, 1, 126)           (159, 1, 165)    (187, 1, 174)
    ND_LEAF=1000000 AMALG_NP=72                  (25, 1, 135)           (137, 1, 165)    (161, 1, 168)
    MERGE_CHAIN=0 BALANCE_BLOCKS=0               (34, 1,  96)           (221, 1, 138)    (247, 1, 162)
    MERGE_CHAIN=200,-50 BALANCE_BLOCKS=15        (18, 1, 156)           (116, 1, 171)    (136, 1, 168)
    ML_ND=0                                      (25, 1, 135)           (139, 1, 168)    (167, 1, 168)

Every pin gives a tree other than the default on every file (on simulation-pose-pose the second and the fifth pin give the
same one)."""
import numpy as np
import pytest

from conftest import g2o_path
from covariances_cases import FLOOR_MAX, far_pairs
from gate_cases import GATE_GRAPHS, candidates, thresholds
from gate_joint_cases import joint_sets
from gate_joint_reference import check_each
from gate_reference import check
from marginals_reference import rel_diff, tolerance
from query_small_cases import references
from test_marginals_gpu import query_nodes

pytestmark = pytest.mark.gpu

FILES = ["simulation-pose-pose", "intel", "parking-garage"]
PINS = [
    {"RR_PGO_ND_LEAF": "50", "RR_PGO_AMALG_NP": "16", "RR_PGO_JOIN_SEPARATORS": "0"},
    {"RR_PGO_ND_LEAF": "1000000", "RR_PGO_AMALG_NP": "72"},
    {"RR_PGO_MERGE_CHAIN": "0", "RR_PGO_BALANCE_BLOCKS": "0"},
    {"RR_PGO_MERGE_CHAIN": "200,-50", "RR_PGO_BALANCE_BLOCKS": "15"},
    {"RR_PGO_ML_ND": "0"},
]
CASES = [(name, p) for name in FILES for p in range(len(PINS))]
IDS = [f"{name}-pin{p}" for name, p in CASES]
N_EDGES = 60    # seeded edges whose cross blocks rr_pgo_marginals is asked for
KEY = ("n_supernodes", "nnz_l_scalars", "max_front", "n_levels")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


_DEFAULT, _PINNED, _WANT = {}, {}, {}


def default(api, name):
    """the default handle at the state of GATE_GRAPHS, and everything that depends on the state alone"""
    if name not in _DEFAULT:
        g = api[0].new(g2o_path(name))
        if GATE_GRAPHS[name]:
            g.optimize(GATE_GRAPHS[name])
        arrays, state = g.graph_arrays(), g.state()
        cand = candidates(arrays, state)
        sets = joint_sets(len(cand[0]))
        gate, joint = references(("trees", name), arrays, state, cand, sets)
        print(gate.summary(name))
        print(joint.summary(name))
        _DEFAULT[name] = dict(g=g, arrays=arrays, state=state, cand=cand, sets=sets, gate=gate, joint=joint)
    return _DEFAULT[name]


def want(api, name, what, node_a, node_b=None):
    """reference blocks of a query, computed once per file: the queried nodes depend on the file alone, never on the tree"""
    asked = (list(map(int, node_a)), None if node_b is None else list(map(int, node_b)))
    if (name, what) not in _WANT:
        _WANT[(name, what)] = (asked, default(api, name)["gate"].ref.blocks(node_a, node_b))
    assert _WANT[(name, what)][0] == asked, (name, what)
    return _WANT[(name, what)][1]


def pinned(api, name, p, monkeypatch):
    if (name, p) not in _PINNED:
        d = default(api, name)
        for k, v in PINS[p].items():
            monkeypatch.setenv(k, v)
        g = api[0].new(g2o_path(name))
        for k in PINS[p]:
            monkeypatch.delenv(k)
        g.set_state(d["state"])   # (read back, an angle has been through (cos, sin) once more: the last place may differ)
        assert np.max(np.abs(g.state() - d["state"])) <= 1e-14
        _PINNED[(name, p)] = g
    return _PINNED[(name, p)]


def key(g):
    s = g.stats()
    return tuple(s[k] for k in KEY)


def split(vals, off, blocks):
    return [vals[off[q]:off[q + 1]].reshape(w.shape) for q, w in enumerate(blocks)]


def check_blocks(label, got, blocks, floor):
    tol = tolerance(floor)
    worst = max(rel_diff(a, b) for a, b in zip(got, blocks))
    print(f"{label}: {len(blocks)} blocks, worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert len(got) == len(blocks)
    assert floor <= FLOOR_MAX, (label, floor)
    assert worst <= tol, (label, worst, tol)


@pytest.mark.parametrize("name", FILES)
def test_at_least_three_pins_give_another_tree_without_fronts_beyond_lds(api, name, monkeypatch):
    g0 = default(api, name)["g"]
    print(f"{name} default: {dict(zip(KEY, key(g0)))}")
    count = 0
    for p in range(len(PINS)):
        g = pinned(api, name, p, monkeypatch)
        s = g.stats()
        other = key(g) != key(g0)
        print(f"{name} {PINS[p]}: {dict(zip(KEY, key(g)))}, max_pivot_cols {s['max_pivot_cols']}" + ("" if other else ": the default tree, does not count"))
        assert s["n_big_fronts"] == 0, (name, PINS[p])
        count += other
    assert count >= 3, (name, count)


@pytest.mark.parametrize("name,p", CASES, ids=IDS)
def test_marginals_on_another_tree(api, name, p, monkeypatch):
    g, d = pinned(api, name, p, monkeypatch), default(api, name)
    label = f"{name} {PINS[p]}"
    assert g.stats()["n_big_fronts"] == 0
    nodes = query_nodes(g, name)
    got = g.marginals(np.array(nodes, np.int32))
    blocks, floor = want(api, name, "diagonal", nodes)
    check_blocks(f"{label} diagonal", got, blocks, floor)
    for blk in got:
        assert np.array_equal(blk, blk.T)
    ef, et = d["arrays"][3], d["arrays"][4]
    idx = np.random.default_rng(7).choice(len(ef), N_EDGES, replace=False)
    a, b = ef[idx].astype(np.int32), et[idx].astype(np.int32)
    vals, off = g.marginal_blocks(a, b)
    blocks, floor = want(api, name, "edges", a, b)
    cross = split(vals, off, blocks)
    check_blocks(f"{label} cross blocks of {N_EDGES} edges", cross, blocks, floor)
    vals_t, off_t = g.marginal_blocks(b, a)
    for q, w in enumerate(cross):
        assert np.array_equal(vals_t[off_t[q]:off_t[q + 1]].reshape(w.shape[1], w.shape[0]), w.T)


@pytest.mark.parametrize("name,p", CASES, ids=IDS)
def test_far_pairs_on_another_tree(api, name, p, monkeypatch):
    g = pinned(api, name, p, monkeypatch)
    nodes, a, b = far_pairs(g.num_nodes)
    k = len(nodes)
    vals, off = g.covariance_blocks(a, b)
    blocks, floor = want(api, name, "far pairs", a, b)
    got = split(vals, off, blocks)
    check_blocks(f"{name} {PINS[p]} far pairs", got, blocks, floor)
    for i in range(k):
        for j in range(i + 1):
            assert np.array_equal(got[j * k + i], got[i * k + j].T), (nodes[i], nodes[j])


@pytest.mark.parametrize("name,p", CASES, ids=IDS)
def test_gate_edges_on_another_tree(api, name, p, monkeypatch):
    g, d = pinned(api, name, p, monkeypatch), default(api, name)
    label, ref, cand = f"{name} {PINS[p]}", d["gate"], d["cand"]
    d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
    check(label, "d2", d2, ref.d2, ref.floor_d2, ref.tol_d2, FLOOR_MAX)
    check(label, "chi2", chi2, ref.chi2, ref.floor_chi2, ref.tol_chi2, FLOOR_MAX)
    check(label, "S", S, ref.S, ref.floor_S, ref.tol_S, FLOOR_MAX)
    for M in S:
        assert np.array_equal(M, M.T) and np.all(np.linalg.eigvalsh(M) > 0)
    keep = ~ref.undecided
    assert np.sum(~keep) <= 1
    assert np.array_equal((d2 <= thresholds(cand[0]))[keep], ref.accept[keep])


@pytest.mark.parametrize("name,p", CASES, ids=IDS)
def test_gate_joint_on_another_tree(api, name, p, monkeypatch):
    g, d = pinned(api, name, p, monkeypatch), default(api, name)
    label, ref, cand, sets = f"{name} {PINS[p]}", d["joint"], d["cand"], d["sets"]
    d2, prefix, S = g.gate_joint(*cand, sets, return_prefix=True, return_innovation=True)
    check(label, "d2", d2, ref.d2, ref.floor_d2, ref.tol_d2, FLOOR_MAX)
    check_each(label, "prefixes", prefix, ref.prefix, ref.floor_prefix, ref.tol_prefix, FLOOR_MAX)
    check(label, "S", S, ref.S, ref.floor_S, ref.tol_S, FLOOR_MAX)
    for M, pre, v in zip(S, prefix, d2):
        assert np.array_equal(M, M.T) and pre[-1] == v and np.all(np.linalg.eigvalsh(M) > 0)
    keep = ~ref.undecided
    assert np.sum(~keep) <= 1
    assert np.array_equal((d2 <= ref.threshold)[keep], ref.accept[keep])
