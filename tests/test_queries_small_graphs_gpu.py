"""rr_pgo_marginals, rr_pgo_covariances, rr_pgo_gate_edges and rr_pgo_gate_joint on the MI355X on the graphs of
tests/query_small_cases.py -- seeded random SE(2) and SE(3) graphs of 2 .. 93 nodes, hand-written graphs of one front,
two odometry chains of 400 .. 480 nodes -- at both of its states, against the CPU references (tests/marginals_reference.py,
tests/gate_reference.py, tests/gate_joint_reference.py).  tests/test_query_small_cases_cpu.py checks the same inputs
without a GPU.

The rule of the dataset tests: a GPU value passes when its relative difference to the reference is at most
max(1e-12, 100 x noise floor), the floor being the worst relative difference between the reference's two independent f64
computations of the same quantity; the floor itself must be at most FLOOR_MAX = 1e-6.  Every comparison prints its worst
figure, the floor and the tolerance before it asserts.

What the dataset files cannot show: a factor of ONE front of 6 .. 86 rows (every MFMA tile of k_selinv_level and
k_tree_fwd clamped on both sides), of two to four fronts, a queried node in the root front; every relation two nodes can
have in the tree, by asking for all ordered pairs; k_gate_joint<double, 3> at 9 .. 16 candidates and D_s = 27 .. 48;
SE(3) queries at random unit quaternions."""
import numpy as np
import pytest

from conftest import g2o_path
from covariances_cases import joint_from_blocks
from gate_cases import GATE_GRAPHS, candidates, thresholds
from gate_joint_cases import block_starts, set_dims
from gate_joint_reference import check_each
from gate_reference import check
from marginals_reference import rel_diff, tolerance
from query_small_cases import DATASETS, FLOOR_MAX, GRAPHS, STATES, all_pairs, big_sets, case, references

pytestmark = pytest.mark.gpu

CASES = [(name, which) for name in GRAPHS for which in STATES]
IDS = [f"{name}-{which}" for name, which in CASES]
PROPERTY_MIN = 7   # the bit-for-bit properties are checked on every set of at least this many members (SE(3): 7 and 8; 2-D: 8 .. 16)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


_HANDLES = {}


def handle(api, name, which):
    if (name, which) not in _HANDLES:
        _HANDLES[(name, which)] = api[0].from_arrays(*case(name, which)["arrays"])
    return _HANDLES[(name, which)]


def refs(name, which):
    c = case(name, which)
    return references((name, which), c["arrays"], c["state"], c["cand"], c["sets"])


def split(vals, off, want):
    return [vals[off[q]:off[q + 1]].reshape(w.shape) for q, w in enumerate(want)]


def check_blocks(label, got, want, floor):
    tol = tolerance(floor)
    worst = max(rel_diff(a, b) for a, b in zip(got, want))
    print(f"{label}: {len(want)} blocks, worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert len(got) == len(want)
    assert floor <= FLOOR_MAX, (label, floor)
    assert worst <= tol, (label, worst, tol)
    return worst


def tree(g):
    s = g.stats()
    return {k: s[k] for k in ("n_supernodes", "n_levels", "max_front", "max_pivot_cols", "nnz_l_scalars", "n_big_fronts")}


def full(g, cand, sets):
    return g.gate_joint(*cand, sets, return_prefix=True, return_innovation=True)


def check_marginals(label, g, arrays, ref):
    """marginals() of all nodes and marginal_blocks over every edge, both orientations"""
    n = len(arrays[0])
    got = g.marginals()
    want, floor = ref.blocks(range(n))
    check_blocks(f"{label} diagonal", got, want, floor)
    for blk in got:
        assert np.array_equal(blk, blk.T)
    a, b = arrays[3].astype(np.int32), arrays[4].astype(np.int32)
    vals, off = g.marginal_blocks(a, b)
    want, floor = ref.blocks(a, b)
    cross = split(vals, off, want)
    check_blocks(f"{label} cross blocks of the edges", cross, want, floor)
    vals_t, off_t = g.marginal_blocks(b, a)
    for q, w in enumerate(cross):
        assert np.array_equal(vals_t[off_t[q]:off_t[q + 1]].reshape(w.shape[1], w.shape[0]), w.T), (q, a[q], b[q])
    return got


@pytest.mark.parametrize("name,which", CASES, ids=IDS)
def test_marginals_of_all_nodes_and_of_every_edge(api, name, which):
    g, c = handle(api, name, which), case(name, which)
    print(f"{name} {which}: {tree(g)}")
    assert g.stats()["n_big_fronts"] == 0
    check_marginals(f"{name} {which}", g, c["arrays"], refs(name, which)[0].ref)


@pytest.mark.parametrize("name,which", CASES, ids=IDS)
def test_covariances_of_all_ordered_pairs(api, name, which):
    g, c = handle(api, name, which), case(name, which)
    assert g.stats()["n_big_fronts"] == 0
    check_covariances(f"{name} {which}", g, len(c["arrays"][0]), refs(name, which)[0].ref)


def check_covariances(label, g, n, ref):
    """covariance_blocks over all ordered pairs of all_pairs(n), a == b included"""
    nodes, a, b = all_pairs(n)
    k = len(nodes)
    vals, off = g.covariance_blocks(a, b)
    want, floor = ref.blocks(a, b)
    got = split(vals, off, want)
    check_blocks(f"{label} all ordered pairs of {k} nodes", got, want, floor)
    # ---- Sigma(b, a) = Sigma(a, b)^T and symmetric diagonal blocks, bit for bit
    for i in range(k):
        for j in range(i + 1):
            assert np.array_equal(got[j * k + i], got[i * k + j].T), (nodes[i], nodes[j])
    # ---- the diagonal blocks against the selected inverse
    diag = g.marginals(np.array(nodes, np.int32))
    check_blocks(f"{label} diagonal blocks against marginals()", [got[i * k + i] for i in range(k)], diag, floor)
    # ---- every joint matrix of a pair is positive definite
    lo = np.inf
    for i in range(k):
        for j in range(i):
            J = np.block([[got[i * k + i], got[i * k + j]], [got[j * k + i], got[j * k + j]]])
            lo = min(lo, float(np.min(np.linalg.eigvalsh(J)) / np.max(np.abs(J))))
    print(f"{label}: smallest eigenvalue of a pair's joint matrix, relative to its largest entry {lo:.3g}")
    assert lo > 0
    if k <= 24:   # the dense joint matrix of all of them
        J = g.covariance(nodes)
        assert np.array_equal(J, joint_from_blocks(got, k)) and np.all(np.linalg.eigvalsh(J) > 0)


def check_gate(label, g, cand, ref):
    d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
    check(label, "d2", d2, ref.d2, ref.floor_d2, ref.tol_d2, FLOOR_MAX)
    check(label, "chi2", chi2, ref.chi2, ref.floor_chi2, ref.tol_chi2, FLOOR_MAX)
    check(label, "S", S, ref.S, ref.floor_S, ref.tol_S, FLOOR_MAX)
    lo = np.inf
    for M in S:
        assert np.array_equal(M, M.T)
        lo = min(lo, float(np.min(np.linalg.eigvalsh(M))))
    print(f"{label}: smallest eigenvalue of an S {lo:.3g}")
    assert lo > 0
    mask = g.gate(*cand)
    assert mask.dtype == bool and np.array_equal(mask, d2 <= thresholds(cand[0]))
    keep = ~ref.undecided
    print(f"{label}: {int(np.sum(mask))} accepted, {int(np.sum(~mask))} rejected, {int(np.sum(~keep))} left out of the comparison")
    assert np.sum(~keep) <= 1
    assert np.array_equal(mask[keep], ref.accept[keep])


@pytest.mark.parametrize("name,which", CASES, ids=IDS)
def test_gate_edges_on_the_pairs_of_a_small_graph(api, name, which):
    g, c = handle(api, name, which), case(name, which)
    assert g.stats()["n_big_fronts"] == 0
    check_gate(f"{name} {which}", g, c["cand"], refs(name, which)[0])


def check_joint(label, g, cand, sets, ref):
    """the comparison with the reference, the decisions, and the bit-for-bit properties on the sets of PROPERTY_MIN and more"""
    kind = cand[0]
    d2, prefix, S = full(g, cand, sets)
    dims = set_dims(kind, sets)
    assert [M.shape[0] for M in S] == dims
    print(f"{label}: {len(sets)} sets, sizes {sorted({len(s) for s in sets})}, D_s {sorted(set(dims))}")
    check(label, "d2", d2, ref.d2, ref.floor_d2, ref.tol_d2, FLOOR_MAX)
    check_each(label, "prefixes", prefix, ref.prefix, ref.floor_prefix, ref.tol_prefix, FLOOR_MAX)
    check(label, "S", S, ref.S, ref.floor_S, ref.tol_S, FLOOR_MAX)
    mask = g.gate_joint_accept(*cand, sets)
    assert mask.dtype == bool and np.array_equal(mask, d2 <= ref.threshold)
    keep = ~ref.undecided
    print(f"{label}: {int(np.sum(mask))} accepted, {int(np.sum(~mask))} rejected, {int(np.sum(~keep))} left out of the comparison")
    assert np.sum(~keep) <= 1
    assert np.array_equal(mask[keep], ref.accept[keep])
    lo = np.inf
    for M, pre, d in zip(S, prefix, d2):
        assert np.array_equal(M, M.T)   # the upper half is a copy of the lower
        assert pre[-1] == d and np.all(np.diff(pre) >= 0)
        lo = min(lo, float(np.min(np.linalg.eigvalsh(M))))
    print(f"{label}: smallest eigenvalue of an S {lo:.3g}")
    assert lo > 0
    big = [s for s, members in enumerate(sets) if len(members) >= PROPERTY_MIN]
    # ---- a prefix is d2 of the truncated set
    cut, where = [], []
    for s in big:
        for k in range(len(sets[s])):
            cut.append(sets[s][:k + 1])
            where.append((s, k))
    # ---- block (c, d) is the same block of the two-candidate set [d, c], a diagonal block that of the set [c]
    small, at = [], []
    for s in big:
        o = block_starts(kind, sets[s])
        for i in range(len(sets[s])):
            for j in range(i + 1):
                small.append([sets[s][j], sets[s][i]] if j < i else [sets[s][i]])
                at.append((s, o[i], o[i + 1], o[j], o[j + 1]))
    if not big:
        return
    d2c, prefc, Sc = full(g, cand, cut)
    starts = {s: block_starts(kind, sets[s]) for s in big}
    for q, (s, k) in enumerate(where):
        assert d2c[q] == prefix[s][k], (label, s, k)
        assert np.array_equal(prefc[q], prefix[s][:k + 1]), (label, s, k)
        assert np.array_equal(Sc[q], S[s][:starts[s][k + 1], :starts[s][k + 1]]), (label, s, k)
    _, _, S2 = full(g, cand, small)
    for (s, i0, i1, j0, j1), P in zip(at, S2):
        if i0 == j0:
            assert np.array_equal(P, S[s][i0:i1, i0:i1]), (label, s, i0)
            continue
        dj = j1 - j0
        assert np.array_equal(P[dj:, :dj], S[s][i0:i1, j0:j1]), (label, s, i0, j0)
        assert np.array_equal(P[:dj, :dj], S[s][j0:j1, j0:j1]), (label, s, j0)
        assert np.array_equal(P[dj:, dj:], S[s][i0:i1, i0:i1]), (label, s, i0)
    print(f"{label}: {len(cut)} truncated sets and {len(small)} sets of one or two candidates reproduce the bits of {len(big)} sets")


@pytest.mark.parametrize("name,which", CASES, ids=IDS)
def test_gate_joint_on_the_sets_of_a_small_graph(api, name, which):
    g, c = handle(api, name, which), case(name, which)
    assert g.stats()["n_big_fronts"] == 0
    check_joint(f"{name} {which}", g, c["cand"], c["sets"], refs(name, which)[1])


def test_the_collection_has_one_front_a_few_fronts_and_a_deep_tree(api, monkeypatch):
    """rr_pgo_stats::n_levels counts the launches of the factorisation's schedule: every handle whose fronts all fit LDS runs
    the one dataflow launch and reports 1, whatever its tree.  The levels of the tree are read from a handle of the same
    graph under the level schedule (RR_PGO_LDS_FLOW=0), which must report the same fronts; that handle answers the same
    queries and is compared with the same reference."""
    trees = {}
    for name in GRAPHS:
        trees[name] = tree(handle(api, name, "initial"))
        print(f"{name}: {trees[name]}")
        assert trees[name]["n_big_fronts"] == 0
    monkeypatch.setenv("RR_PGO_LDS_FLOW", "0")
    lvl = api[0].from_arrays(*case("mid-se3", "initial")["arrays"])
    monkeypatch.delenv("RR_PGO_LDS_FLOW")
    t = trees["mid-se3 under the level schedule"] = tree(lvl)
    print(f"mid-se3 under the level schedule: {t}")
    same = ("n_supernodes", "max_front", "max_pivot_cols", "nnz_l_scalars", "n_big_fronts")
    assert [t[k] for k in same] == [trees["mid-se3"][k] for k in same]
    c = case("mid-se3", "initial")
    gate, joint = refs("mid-se3", "initial")
    check_marginals("mid-se3 under the level schedule", lvl, c["arrays"], gate.ref)
    check_covariances("mid-se3 under the level schedule", lvl, len(c["arrays"][0]), gate.ref)
    check_gate("mid-se3 under the level schedule", lvl, c["cand"], gate)
    check_joint("mid-se3 under the level schedule", lvl, c["cand"], c["sets"], joint)
    assert any(t["n_supernodes"] == 1 for t in trees.values())
    assert any(2 <= t["n_supernodes"] <= 4 for t in trees.values())
    assert any(t["n_supernodes"] >= 30 and t["n_levels"] >= 5 for t in trees.values())
    assert any(t["max_front"] < 16 for t in trees.values())   # a factor of fewer than 16 rows


# ---- the sets of 9, 12 and 16 on two dataset files: D_s = 48 on real trees --------------------------------------------------

_DATA = {}


def dataset(api, name):
    if name not in _DATA:
        g = api[0].new(g2o_path(name))
        if GATE_GRAPHS[name]:
            g.optimize(GATE_GRAPHS[name])
        arrays, state = g.graph_arrays(), g.state()
        cand = candidates(arrays, state)
        sets = big_sets(cand[0])
        _DATA[name] = (g, cand, sets, references(("gpu", name), arrays, state, cand, sets)[1])
    return _DATA[name]


@pytest.mark.parametrize("name", DATASETS)
def test_sets_of_9_to_16_on_dataset_files(api, name):
    g, cand, sets, ref = dataset(api, name)
    print(f"{name}: {tree(g)}")
    print(ref.summary(name))
    assert sorted(set(set_dims(cand[0], sets))) == [27, 36, 48]
    check_joint(name, g, cand, sets, ref)
