"""The factor queries on trees with fronts beyond LDS, under rr_pgo_set_query_big_fronts: the SE(3) lattices of
tests/big_front_cases.py (n = 5, 6, 7), the n = 6 lattice with point landmarks, and sphere2500.

The rule of the dataset tests: a GPU value passes at marginals_reference.tolerance(floor) = max(1e-12, 100 x floor), the
floor from the reference alone and at most FLOOR_MAX = 1e-6; every comparison prints its worst figure, the floor and the
tolerance before it asserts.  States: "initial" and "gn3" (three Gauss-Newton iterations of the CPU reference).

The trees.  The library chooses among its candidate trees, so the tests assert what they need of the handle's own
rr_pgo_stats (test_the_trees_hold_what_the_kernels_need).  Under the default choice the n = 5 lattice keeps every front in
LDS (22 fronts, the largest of 168 rows) and the root of the n = 6 lattice is its largest front (234 rows, all pivots), so
the handles of n = 5 and n = 6 are created under RR_PGO_ND_LEAF=1000000 RR_PGO_AMALG_NP=72 (the second pin of
tests/test_queries_other_trees_gpu.py: no dissection, amalgamation up to 72 columns).  PoseGraph.analyze on the host gives
(n_supernodes, n_levels, max_front, max_pivot_cols, n_big_fronts):
    n = 5 pinned   (32, 2, 186, 186, 1)     the root alone is beyond LDS: 186 = 5 * 32 + 26 pivot columns, a partial last block
    n = 6 pinned   (63, 3, 276, 264, 3)     rows below a pivot block beyond LDS, a front beyond LDS under another
    n = 7 default  (110, 5, 312, 222, 10)   ten such fronts on several levels
    landmarks6     (82, 5, 444, 444, 10)    the default tree
Which front a node's pivot columns lie in is read from the plan trace of a handle created under RR_PGO_QUERY_TRACE=1."""
import re

import numpy as np
import pytest

from big_front_cases import (AUDIT_EDGES, LATTICES, STATES, at_state, audit_edges, marginals_reference, ordered_pairs, query_case,
                             seeded_nodes)
from conftest import g2o_path
from covariances_cases import FLOOR_MAX, far_pairs
from cross_covariances_reference import CrossReference, check_columns
from gate_cases import candidates, thresholds
from gate_joint_reference import check_each
from gate_reference import check
from marginals_reference import rel_diff, tolerance

pytestmark = pytest.mark.gpu

PIN = {"RR_PGO_ND_LEAF": "1000000", "RR_PGO_AMALG_NP": "72"}
PINS = {"lattice5": PIN, "lattice6": PIN, "lattice7": {}, "landmarks6": {}}
MIN_BIG = {"lattice5": 1, "lattice6": 3, "lattice7": 3, "landmarks6": 3}
CASES = [(name, which) for name in LATTICES for which in STATES]
IDS = [f"{name}-{which}" for name, which in CASES]
WITH_ROWS_BELOW = [c for c in CASES if c[0] != "lattice5"]
IDS_BELOW = [f"{name}-{which}" for name, which in WITH_ROWS_BELOW]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


_HANDLES, _KINDS = {}, {}


def create(api, name, which, monkeypatch, env=None, switch=True):
    """a fresh handle of the case at the state, created under the case's pin (and `env`)"""
    arrays, _ = at_state(name, which)
    extra = dict(PINS[name], **(env or {}))
    for k, v in extra.items():
        monkeypatch.setenv(k, v)
    g = api[0].from_arrays(*arrays)
    for k in extra:
        monkeypatch.delenv(k)
    if switch:
        g.query_big_fronts = True
    return g


def handle(api, name, which, monkeypatch):
    if (name, which) not in _HANDLES:
        _HANDLES[(name, which)] = create(api, name, which, monkeypatch)
    return _HANDLES[(name, which)]


def passes_of(text):
    return len(re.findall(r"^query trace: \S+ pass ", text, re.M))


def node_kinds(api, name, which, monkeypatch, capfd):
    """dict(root, big, leaf, anchor, fronts): a node whose pivot columns lie in the root front, one in a non-root front beyond
    LDS (None where the tree has none), one in an LDS front without children, the anchor -- from the plan trace of the diagonal
    blocks of every node"""
    if (name, which) not in _KINDS:
        g = create(api, name, which, monkeypatch, env={"RR_PGO_QUERY_TRACE": "1"})
        capfd.readouterr()
        every = np.arange(g.num_nodes, dtype=np.int32)
        g.covariance_blocks(every, every)
        err = capfd.readouterr().err
        fronts = {int(m[0]): dict(depth=int(m[1]), nc=int(m[2]), nr=int(m[3]), parent=int(m[4]), children=int(m[5]), big=m[6] == "beyond-LDS")
                  for m in re.findall(r"query trace:   front (\d+) depth (\d+) nc (\d+) nr (\d+) parent (-?\d+) children (\d+) (\S+)", err)}
        front_of = {int(v): int(f) for v, f in re.findall(r"query trace:   node (\d+) front (\d+)", err)}
        assert len(front_of) == g.num_nodes and fronts, (name, which, len(front_of), len(fronts))

        def first(pred):
            return next((v for v in range(g.num_nodes) if pred(fronts[front_of[v]])), None)
        _KINDS[(name, which)] = dict(root=first(lambda f: f["parent"] < 0), big=first(lambda f: f["big"] and f["parent"] >= 0),
                                     leaf=first(lambda f: not f["big"] and f["children"] == 0), anchor=g.anchor_node,
                                     fronts=fronts, front_of=front_of)
    return _KINDS[(name, which)]


def query_nodes(api, name, which, monkeypatch, capfd):
    k = node_kinds(api, name, which, monkeypatch, capfd)
    must = [k[w] for w in ("root", "big", "leaf", "anchor") if k[w] is not None]
    return seeded_nodes(len(at_state(name, which)[0][0]), must), k


def split(vals, off, blocks):
    return [vals[off[q]:off[q + 1]].reshape(w.shape) for q, w in enumerate(blocks)]


def check_blocks(label, got, blocks, floor):
    tol = tolerance(floor)
    worst = max(rel_diff(a, b) for a, b in zip(got, blocks))
    print(f"{label}: {len(blocks)} blocks, worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert len(got) == len(blocks)
    assert floor <= FLOOR_MAX, (label, floor)
    assert worst <= tol, (label, worst, tol)


def refusal(call):
    """(code, message) of the PoseGraphError `call` must raise"""
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    with pytest.raises(PoseGraphError) as ei:
        call()
    return ei.value.code, _lib.load().rr_pgo_last_error().decode()


def the_five(g, cand, sets):
    """the five queries as callables"""
    return {"rr_pgo_covariances": lambda: g.covariance_blocks([0, 1], [1, 2]),
            "rr_pgo_cross_covariances": lambda: g.cross_covariance([0, 3], [1]),
            "rr_pgo_gate_edges": lambda: g.gate_edges(*cand),
            "rr_pgo_gate_joint": lambda: g.gate_joint(*cand, sets),
            "rr_pgo_check_edges": lambda: g.check_edges([0, 1])}


# ---- 1. the switch -----------------------------------------------------------------------------------------------------------

def test_the_switch_is_off_by_default_and_travels_with_the_handle(api, monkeypatch):
    """n = 5 under the pin of this file's docstring (one front beyond LDS, the root), kept set for the whole test so that
    rr_pgo_extend and rr_pgo_remove_edges, which read the environment again, build such a tree too"""
    from rustrobotics_amd import _lib
    for k, v in PIN.items():
        monkeypatch.setenv(k, v)
    c = query_case("lattice5", "initial")
    arrays, cand, sets = c["arrays"], c["cand"], c["sets"]
    g = api[0].from_arrays(*arrays)
    print(f"lattice5: {g.stats()}")
    assert g.stats()["n_big_fronts"] >= 1
    assert g.query_big_fronts is False
    for who, call in the_five(g, cand, sets).items():
        code, msg = refusal(call)
        assert code == _lib.EUNSUPPORTED and msg.startswith(who + ":") and "beyond LDS" in msg, (who, code, msg)
    g.query_big_fronts = True
    assert g.query_big_fronts is True
    for who, call in the_five(g, cand, sets).items():
        call()
    code, msg = refusal(lambda: g.marginals([0]))
    assert code == _lib.EUNSUPPORTED and "beyond LDS" in msg and "use rr_pgo_covariances with rr_pgo_set_query_big_fronts" in msg, msg
    g.query_big_fronts = False
    assert g.query_big_fronts is False and refusal(lambda: g.covariance_blocks([0], [0]))[0] == _lib.EUNSUPPORTED
    g.query_big_fronts = True
    # ---- one new pose, hung on node 0 by a copy of the first edge's measurement: the grown handle answers without being asked again
    n, ml, il = g.num_nodes, 7, 21
    g.extend([2], [0], [n], arrays[5][:ml], arrays[6][:il], node_kind=[2])
    assert g.num_nodes == n + 1 and g.stats()["n_big_fronts"] >= 1 and g.query_big_fronts is True
    vals, _ = g.covariance_blocks([n, 0], [n, n])
    assert np.all(np.isfinite(vals)) and len(vals) == 72
    # ---- a loop edge goes (every lattice node keeps three or more edges)
    g.remove_edges([7])
    assert g.stats()["n_big_fronts"] >= 1 and g.query_big_fronts is True
    g.gate_edges(*cand)
    # ---- off travels too
    g.query_big_fronts = False
    g.remove_edges([9])
    assert g.query_big_fronts is False and refusal(lambda: g.gate_edges(*cand))[0] == _lib.EUNSUPPORTED
    # ---- the setter is RR_PGO_OK on handles that refuse for their own reasons, and those reasons come first
    f32 = api[0].from_arrays(*arrays, precision="f32")
    f32.query_big_fronts = True
    code, msg = refusal(lambda: f32.covariance_blocks([0], [0]))
    assert code == _lib.EUNSUPPORTED and "F32" in msg, msg
    assert _lib.load().rr_pgo_get_query_big_fronts(None) == 0 and _lib.load().rr_pgo_set_query_big_fronts(None, 1) == _lib.EINVAL


# ---- 2. no effect without fronts beyond LDS ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["simulation-pose-pose", "parking-garage"])
def test_the_switch_changes_no_bit_on_a_tree_without_fronts_beyond_lds(api, name):
    off, on = api[0].new(g2o_path(name)), api[0].new(g2o_path(name))
    on.query_big_fronts = True
    assert off.stats()["n_big_fronts"] == 0
    _, a, b = far_pairs(off.num_nodes)
    v0, o0 = off.covariance_blocks(a, b)
    v1, o1 = on.covariance_blocks(a, b)
    assert np.array_equal(o0, o1) and np.array_equal(v0, v1)
    cand = candidates(off.graph_arrays(), off.state())
    r0, r1 = off.gate_edges(*cand, return_innovation=True), on.gate_edges(*cand, return_innovation=True)
    assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1])
    assert all(np.array_equal(x, y) for x, y in zip(r0[2], r1[2]))
    x0, x1 = off.cross_covariance(None, a[:2]), on.cross_covariance(None, a[:2])
    assert np.array_equal(x0, x1)


# ---- the trees -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,which", [(n, w) for n in PINS for w in STATES], ids=[f"{n}-{w}" for n in PINS for w in STATES])
def test_the_trees_hold_what_the_kernels_need(api, name, which, monkeypatch, capfd):
    g = handle(api, name, which, monkeypatch)
    s = g.stats()
    print(f"{name} {which}: {s}")
    assert s["n_big_fronts"] >= MIN_BIG[name]
    if name != "lattice5":   # a front beyond LDS with rows below its pivot block
        assert s["max_front"] > s["max_pivot_cols"] or name == "landmarks6"
    if name in LATTICES:
        k = node_kinds(api, name, which, monkeypatch, capfd)
        big = [f for f in k["fronts"].values() if f["big"]]
        print(f"{name} {which}: fronts beyond LDS (nc x rows) " + ", ".join(f"{f['nc']}x{f['nc'] + f['nr']}" for f in big)
              + f"; query nodes root {k['root']} big {k['big']} leaf {k['leaf']} anchor {k['anchor']}")
        assert len(big) == s["n_big_fronts"]
        assert k["root"] is not None and k["leaf"] is not None
        if name != "lattice5":
            assert k["big"] is not None and any(f["nr"] > 0 for f in big)
            assert any(f["nc"] % 32 for f in big)


# ---- 3. rr_pgo_covariances -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,which", CASES, ids=IDS)
def test_covariances_of_all_pairs_of_fourteen_nodes(api, name, which, monkeypatch, capfd):
    g = handle(api, name, which, monkeypatch)
    nodes, _ = query_nodes(api, name, which, monkeypatch, capfd)
    k = len(nodes)
    a, b = ordered_pairs(nodes)
    vals, off = g.covariance_blocks(a, b)
    want, floor = marginals_reference(name, which).blocks(a, b)
    got = split(vals, off, want)
    t = g.covariances_times()
    print(f"{name} {which}: nodes {nodes}; linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, products + gather {t[2]:.3f} ms")
    check_blocks(f"{name} {which} all pairs of {k} nodes", got, want, floor)
    for i in range(k):
        assert np.array_equal(got[i * k + i], got[i * k + i].T), nodes[i]
        for j in range(k):
            assert np.array_equal(got[j * k + i], got[i * k + j].T), (nodes[i], nodes[j])


# ---- 4. independence of the rest of the call and of a cut of the plan ----------------------------------------------------------

@pytest.mark.parametrize("name", ["lattice6", "lattice7"])
def test_a_block_alone_in_the_list_reversed_and_under_a_cut_has_the_same_bits(api, name, monkeypatch, capfd):
    from rustrobotics_amd import _lib
    which = "initial"
    g = handle(api, name, which, monkeypatch)
    nodes, _ = query_nodes(api, name, which, monkeypatch, capfd)
    a, b = ordered_pairs(nodes)
    vals, off = g.covariance_blocks(a, b)
    rv, ro = g.covariance_blocks(a[::-1].copy(), b[::-1].copy())
    nq = len(a)
    for q in range(nq):
        assert np.array_equal(rv[ro[nq - 1 - q]:ro[nq - q]], vals[off[q]:off[q + 1]]), (a[q], b[q])
    probe = list(range(0, nq, 13))
    for q in probe:
        one, _ = g.covariance_blocks(a[q:q + 1], b[q:q + 1])
        assert np.array_equal(one, vals[off[q]:off[q + 1]]), (a[q], b[q])
    # ---- a handle whose workspace bound is the largest need of a single pair (the reasoning of tests/test_covariances_gpu.py's
    # test of the cut): 14 nodes are 84 columns, three chunks, so the whole list needs more and is cut
    tiny = create(api, name, which, monkeypatch, env={"RR_PGO_TS_WS_BYTES": "1"})
    need = []
    for q in range(nq):
        code, msg = refusal(lambda: tiny.covariance_blocks(a[q:q + 1], b[q:q + 1]))
        m = re.fullmatch(r"rr_pgo_covariances: one pair needs (\d+) bytes of workspace", msg)
        assert code == _lib.ENOMEM and m, msg
        need.append(int(m.group(1)))
    cut = create(api, name, which, monkeypatch, env={"RR_PGO_TS_WS_BYTES": str(max(need)), "RR_PGO_QUERY_TRACE": "1"})
    capfd.readouterr()
    cv, co = cut.covariance_blocks(a, b)
    passes = passes_of(capfd.readouterr().err)
    print(f"{name}: {nq} pairs alone need {min(need)} .. {max(need)} bytes; under a bound of {max(need)} the list ran in {passes} passes")
    assert passes >= 2
    assert np.array_equal(co, off) and np.array_equal(cv, vals)


# ---- 5. rr_pgo_cross_covariances -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,which", WITH_ROWS_BELOW, ids=IDS_BELOW)
def test_cross_covariances(api, name, which, monkeypatch, capfd):
    from rustrobotics_amd import _lib
    g = handle(api, name, which, monkeypatch)
    nodes, k = query_nodes(api, name, which, monkeypatch, capfd)
    cols = [k["root"], k["big"], k["leaf"]]
    ref = CrossReference.from_marginals(marginals_reference(name, which))
    full = ref.full_columns(cols)
    X = g.cross_covariance(None, cols)
    t = g.cross_covariances_times()
    print(f"{name} {which}: columns of nodes {cols}; linearise + factor {t[0]:.3f} ms, forward + backward solve {t[1]:.3f} ms, gather + copy {t[2]:.3f} ms")
    _, floor, tol = check_columns(f"{name} {which} Sigma[:, root / beyond-LDS / leaf node]", X, ref, None, cols, full)
    # ---- a row subset with repeats: copies of the full columns' rows, same bits
    rows = [nodes[5], k["root"], nodes[7], k["big"], nodes[5], k["leaf"], k["anchor"]]
    Y = g.cross_covariance(rows, cols)
    assert np.array_equal(Y, X[ref.row_scalars(rows)])
    # ---- independent of the other columns, of their order and of a cut between column nodes
    many = [nodes[9], k["leaf"], nodes[3], k["root"], nodes[11], k["big"], nodes[2], k["leaf"]] + nodes
    Z = g.cross_covariance(rows, many)
    co = np.concatenate([[0], np.cumsum([ref.dims[v] for v in many])]).astype(int)
    for c, v in enumerate(cols):
        at = many.index(v)
        assert np.array_equal(Z[:, co[at]:co[at + 1]], Y[:, 6 * c:6 * c + 6]), v
    tiny = create(api, name, which, monkeypatch, env={"RR_PGO_TS_WS_BYTES": "1"})
    need = []
    for v in sorted(set(many)):
        code, msg = refusal(lambda: tiny.cross_covariance(rows, [v]))
        m = re.fullmatch(r"rr_pgo_cross_covariances: one column node needs (\d+) bytes of workspace", msg)
        assert code == _lib.ENOMEM and m, msg
        need.append(int(m.group(1)))
    cut = create(api, name, which, monkeypatch, env={"RR_PGO_TS_WS_BYTES": str(max(need)), "RR_PGO_QUERY_TRACE": "1"})
    capfd.readouterr()
    W = cut.cross_covariance(rows, many)
    passes = passes_of(capfd.readouterr().err)
    print(f"{name} {which}: {len(many)} column nodes under a bound of {max(need)} bytes: {passes} passes")
    assert passes >= 2 and np.array_equal(W, Z)
    # ---- agreement with rr_pgo_covariances, to rounding
    a, b = np.repeat(rows, len(cols)).astype(np.int32), np.tile(cols, len(rows)).astype(np.int32)
    vals, off = g.covariance_blocks(a, b)
    worst = 0.0
    for i in range(len(rows)):
        for c in range(len(cols)):
            q = i * len(cols) + c
            blk = vals[off[q]:off[q + 1]].reshape(6, 6)
            scale = full[2][c][3]   # the whole column's largest entry: the unit of the backward solve's error
            worst = max(worst, float(np.max(np.abs(Y[6 * i:6 * i + 6, 6 * c:6 * c + 6] - blk)) / scale))
    print(f"{name} {which}: cross covariances against rr_pgo_covariances: worst difference {worst:.3g} of the column's scale, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert worst <= tol


# ---- 6. the gate, the joint gate and the audit --------------------------------------------------------------------------------

@pytest.mark.parametrize("which", STATES)
def test_gate_edges(api, which, monkeypatch):
    name = "lattice6"
    g, c = handle(api, name, which, monkeypatch), query_case(name, which)
    label, ref, cand = f"{name} {which}", c["gate"], c["cand"]
    print(ref.summary(label))
    d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
    check(label, "d2", d2, ref.d2, ref.floor_d2, ref.tol_d2, FLOOR_MAX)
    check(label, "chi2", chi2, ref.chi2, ref.floor_chi2, ref.tol_chi2, FLOOR_MAX)
    check(label, "S", S, ref.S, ref.floor_S, ref.tol_S, FLOOR_MAX)
    for M in S:
        assert np.array_equal(M, M.T) and np.all(np.linalg.eigvalsh(M) > 0)
    keep = ~ref.undecided
    assert np.sum(~keep) <= 1
    assert np.array_equal((d2 <= thresholds(cand[0]))[keep], ref.accept[keep])


@pytest.mark.parametrize("which", STATES)
def test_gate_joint(api, which, monkeypatch):
    name = "lattice6"
    g, c = handle(api, name, which, monkeypatch), query_case(name, which)
    label, ref, cand, sets = f"{name} {which}", c["joint"], c["cand"], c["sets"]
    print(ref.summary(label))
    d2, prefix, S = g.gate_joint(*cand, sets, return_prefix=True, return_innovation=True)
    check(label, "d2", d2, ref.d2, ref.floor_d2, ref.tol_d2, FLOOR_MAX)
    check_each(label, "prefixes", prefix, ref.prefix, ref.floor_prefix, ref.tol_prefix, FLOOR_MAX)
    check(label, "S", S, ref.S, ref.floor_S, ref.tol_S, FLOOR_MAX)
    for M, pre, v in zip(S, prefix, d2):
        assert np.array_equal(M, M.T) and pre[-1] == v and np.all(np.linalg.eigvalsh(M) > 0)
    keep = ~ref.undecided
    assert np.sum(~keep) <= 1
    assert np.array_equal((d2 <= ref.threshold)[keep], ref.accept[keep])


@pytest.mark.parametrize("which", STATES)
def test_check_edges(api, which, monkeypatch):
    from check_edges_cases import reference
    name = "lattice6"
    g, c = handle(api, name, which, monkeypatch), query_case(name, which)
    edges = audit_edges(c["arrays"])
    ref = reference(("big-fronts", name, which), c["arrays"], c["state"], edges)
    print(ref.summary(f"{name} {which}"))
    got = g.check_edges(edges, return_residual=True)
    ref.check(f"{name} {which} {AUDIT_EDGES} seeded edges", got)
    for R in got["R"]:
        assert np.array_equal(R, R.T)


# ---- 7. fixed nodes and priors ----------------------------------------------------------------------------------------------------

def test_fixed_nodes_and_priors(api, monkeypatch, capfd):
    """20 seeded poses fixed, two of them in the root front, five priors on free poses, keep_anchor = 0 (the fixed set and the
    priors hold the gauge): Sigma is conditional on the fixed poses"""
    from fixed_reference import FixedReference
    from priors_reference import random_priors
    name, which = "lattice6", "initial"
    arrays, _ = at_state(name, which)
    k = node_kinds(api, name, which, monkeypatch, capfd)
    n = len(arrays[0])
    in_root = [v for v in range(n) if k["fronts"][k["front_of"][v]]["parent"] < 0][:2]
    rng = np.random.default_rng(1977)
    F = sorted(seeded_nodes(n, in_root, count=20, seed=1978))
    free = [v for v in range(n) if v not in F]
    prior_nodes = sorted(int(v) for v in rng.choice(free, 5, replace=False))
    priors = random_priors(rng, arrays, prior_nodes, noise=0.05)
    g = create(api, name, which, monkeypatch)
    g.set_priors(*priors)
    g.set_fixed(F, keep_anchor=False)
    ref = FixedReference(arrays, F, keep_anchor=False, priors=priors)
    nodes = seeded_nodes(n, [F[0], in_root[0], k["big"], k["leaf"], prior_nodes[0]], seed=1979)
    a, b = ordered_pairs(nodes)
    sig = ref.sigma_pair()
    want, floor = ref.blocks(a, b, sig=sig)
    vals, off = g.covariance_blocks(a, b)
    got = split(vals, off, want)
    live =[q for q in range(len(a)) if a[q] not in F and b[q] not in F]
    print(f"lattice6 fixed {F}, priors on {prior_nodes}: {len(a)} blocks, {len(a) - len(live)} with a fixed node")
    assert 0 < len(live) < len(a)
    check_blocks("lattice6 with 20 fixed poses and 5 priors", [got[q] for q in live], [want[q] for q in live], floor)
    for q in range(len(a)):
        if q not in live:
            assert not np.any(got[q]) and not np.any(want[q]), (a[q], b[q])
    cols = [in_root[0], k["big"], k["leaf"], prior_nodes[0]]
    cref = CrossReference.from_sigma_pair(sig, arrays[0])
    X = g.cross_covariance(None, cols)
    check_columns("lattice6 with 20 fixed poses and 5 priors, Sigma[:, cols]", X, cref, None, cols)
    assert not np.any(X[cref.row_scalars(F)]) and not np.any(X[:, :6])


# ---- 8. point landmarks: the LM instantiations of the gate, joint and audit kernels ----------------------------------------------

@pytest.mark.parametrize("which", STATES)
def test_landmark_case(api, which, monkeypatch):
    from landmarks3d_reference import Landmarks3dReference
    from test_landmarks3d_gpu import candidates as candidates3d
    name = "landmarks6"
    arrays, _ = at_state(name, which)
    g = handle(api, name, which, monkeypatch)
    ref = Landmarks3dReference(list(arrays))
    sig = ref.sigma_pair()
    cand = candidates3d(list(arrays), 51)
    d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
    S2, d22, chi22, fS, fd = ref.gate(cand, sig=sig)
    worst_S = max(rel_diff(x, y) for x, y in zip(S, S2))
    worst_d = float(np.abs(d2 / d22 - 1).max())
    print(f"{name} {which}: gate S worst {worst_S:.3g} (floor {fS:.3g}, tolerance {tolerance(fS):.3g}), d2 worst {worst_d:.3g} (floor {fd:.3g}, tolerance {tolerance(fd):.3g})")
    assert [s.shape[0] for s in S] == [6] * 6 + [3] * 6
    assert max(fS, fd) <= FLOOR_MAX and worst_S <= tolerance(fS) and worst_d <= tolerance(fd)
    assert all(np.array_equal(s, s.T) and np.all(np.linalg.eigvalsh(s) > 0) for s in S)
    sets = [[0, 6], [7, 1, 8], [2, 3], [9, 10, 11], [4, 9, 5, 6]]
    dj, pre, Sj = g.gate_joint(*cand, sets, return_prefix=True, return_innovation=True)
    Sj2, dj2, fSj, fdj = ref.gate_joint(cand, sets, sig=sig)
    worst_S = max(rel_diff(x, y) for x, y in zip(Sj, Sj2))
    worst_d = float(np.abs(dj / dj2 - 1).max())
    print(f"{name} {which}: joint S worst {worst_S:.3g} (floor {fSj:.3g}, tolerance {tolerance(fSj):.3g}), d2 worst {worst_d:.3g} (floor {fdj:.3g}, tolerance {tolerance(fdj):.3g})")
    assert [s.shape[0] for s in Sj] == [9, 12, 12, 9, 18]
    assert max(fSj, fdj) <= FLOOR_MAX and worst_S <= tolerance(fSj) and worst_d <= tolerance(fdj)
    assert all(np.array_equal(s, s.T) and p[-1] == v for s, p, v in zip(Sj, pre, dj))
    # ---- the audit of AUDIT_EDGES seeded edges, landmark edges among them
    edges = audit_edges(arrays)
    assert np.any(arrays[2][edges] == 3) and np.any(arrays[2][edges] == 2)
    out = g.check_edges(edges, return_residual=True)
    R2, d22, red2, chi22, fR, fd, fc, fr = ref.check(edges, sig=sig)
    worst = np.zeros(4)
    for q, e in enumerate(edges):
        assert np.isfinite(fd[q]) and max(fd[q], fc[q], fr[q], fR) <= FLOOR_MAX, (e, fd[q], fc[q], fr[q], fR)
        scale = np.abs(np.linalg.inv(ref.omega[e])).max()
        figures = (np.abs(out["R"][q] - R2[q]).max() / scale / tolerance(fR), abs(out["chi2"][q] / chi22[q] - 1) / tolerance(fc[q]),
                   abs(out["redundancy"][q] - red2[q]) / tolerance(fr[q]), abs(out["d2"][q] / d22[q] - 1) / tolerance(fd[q]))
        worst = np.maximum(worst, figures)
        assert np.array_equal(out["R"][q], out["R"][q].T), e
    print(f"{name} {which}: audit of {len(edges)} edges, worst difference as a fraction of its tolerance: R {worst[0]:.3g}, chi2 {worst[1]:.3g}, "
          f"redundancy {worst[2]:.3g}, d2 {worst[3]:.3g}; floor of R {fR:.3g}, largest floors d2 {fd.max():.3g} chi2 {fc.max():.3g} r {fr.max():.3g}")
    assert np.all(worst <= 1.0), worst


# ---- 9. sphere2500 ---------------------------------------------------------------------------------------------------------------

_SPHERE = {}


def sphere(api):
    """the handle after 5 Gauss-Newton iterations and its sparse reference, built once"""
    pytest.importorskip("scipy.sparse.linalg", reason="the sparse reference of sphere2500 (dim 15000) needs SciPy")
    if not _SPHERE:
        from gate_reference import GateReference
        g = api[0].new(g2o_path("sphere2500"))
        g.query_big_fronts = True
        g.optimize(5)
        arrays, state = g.graph_arrays(), g.state()
        cand = candidates(arrays, state)
        gate = GateReference(arrays, state, cand)
        _SPHERE.update(g=g, cand=cand, gate=gate)
    return _SPHERE


def test_sphere2500_far_pairs(api):
    s = sphere(api)
    g = s["g"]
    print(f"sphere2500: {g.stats()}")
    assert g.stats()["n_big_fronts"] > 0
    nodes, a, b = far_pairs(g.num_nodes)
    k = len(nodes)
    vals, off = g.covariance_blocks(a, b)
    want, floor = s["gate"].ref.blocks(a, b)
    got = split(vals, off, want)
    t = g.covariances_times()
    print(f"sphere2500 after 5 iterations: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, products + gather {t[2]:.3f} ms")
    check_blocks("sphere2500 after 5 iterations, far pairs", got, want, floor)
    for i in range(k):
        for j in range(i + 1):
            assert np.array_equal(got[j * k + i], got[i * k + j].T), (nodes[i], nodes[j])


def test_sphere2500_gate_edges(api):
    s = sphere(api)
    g, ref, cand = s["g"], s["gate"], s["cand"]
    print(ref.summary("sphere2500"))
    d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
    check("sphere2500", "d2", d2, ref.d2, ref.floor_d2, ref.tol_d2, FLOOR_MAX)
    check("sphere2500", "chi2", chi2, ref.chi2, ref.floor_chi2, ref.tol_chi2, FLOOR_MAX)
    check("sphere2500", "S", S, ref.S, ref.floor_S, ref.tol_S, FLOOR_MAX)
    for M in S:
        assert np.array_equal(M, M.T) and np.all(np.linalg.eigvalsh(M) > 0)
    keep = ~ref.undecided
    assert np.sum(~keep) <= 1
    assert np.array_equal((d2 <= thresholds(cand[0]))[keep], ref.accept[keep])
