"""rr_pgo_marginals on trees with fronts beyond LDS, under rr_pgo_set_marginals_big_fronts: the cases, pins
and trees of tests/test_big_front_queries_gpu.py (its docstring says what each tree reaches), and sphere2500.

The rule of the dataset tests: a GPU value passes at marginals_reference.tolerance(floor) = max(1e-12, 100 x floor), the
floor from the reference alone and at most FLOOR_MAX = 1e-6; every comparison prints its worst figure, the floor and the
tolerance before it asserts.  Without the switch every test here fails at its first use of the setter."""
import ctypes as C

import numpy as np
import pytest

from big_front_cases import LATTICES, STATES, at_state, query_case
from conftest import g2o_path
from covariances_cases import FLOOR_MAX
from marginals_big_cases import fixed_case, landmark_blocks, lattice_blocks
from marginals_reference import rel_diff, tolerance
from test_big_front_queries_gpu import MIN_BIG, PIN, check_blocks, create, node_kinds, refusal, sphere, split, the_five

pytestmark = pytest.mark.gpu

CASES = [(name, which) for name in LATTICES for which in STATES]
IDS = [f"{name}-{which}" for name, which in CASES]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


_HANDLES = {}


def fresh(api, name, which, monkeypatch):
    """a fresh handle of the case at the state under the case's pin, rr_pgo_set_marginals_big_fronts on (and only that switch)"""
    g = create(api, name, which, monkeypatch, switch=False)
    g.marginals_big_fronts = True
    return g


def handle(api, name, which, monkeypatch):
    if (name, which) not in _HANDLES:
        g = fresh(api, name, which, monkeypatch)
        s = g.stats()
        print(f"{name} {which}: {s}")
        assert s["n_big_fronts"] >= MIN_BIG[name]
        if name in ("lattice6", "lattice7"):   # a front beyond LDS with rows below its pivot block
            assert s["max_front"] > s["max_pivot_cols"]
        _HANDLES[(name, which)] = g
    return _HANDLES[(name, which)]


def all_blocks(label, g, want):
    """every diagonal block (node_a == NULL) and both orientations of every edge's cross block against `want`
    (marginals_big_cases), with the bitwise symmetries and a second call"""
    diag = g.marginals()
    t = g.marginals_times()
    print(f"{label}: all nodes: linearise + factor {t[0]:.3f} ms, selected inverse {t[1]:.3f} ms, gather {t[2]:.3f} ms")
    check_blocks(f"{label} every diagonal block", diag, want["diag"], want["floor_diag"])
    for v, blk in enumerate(diag):
        assert np.array_equal(blk, blk.T), v
    a, b = want["a"], want["b"]
    vals, off = g.marginal_blocks(a, b)
    cross = split(vals, off, want["cross"])
    check_blocks(f"{label} every edge's cross block", cross, want["cross"], want["floor_cross"])
    vals_t, off_t = g.marginal_blocks(b, a)
    for q, w in enumerate(cross):
        assert np.array_equal(vals_t[off_t[q]:off_t[q + 1]].reshape(w.shape[1], w.shape[0]), w.T), (a[q], b[q])
    again = g.marginals()
    assert all(np.array_equal(x, y) for x, y in zip(diag, again))
    vals2, off2 = g.marginal_blocks(a, b)
    assert np.array_equal(off, off2) and np.array_equal(vals, vals2)
    return diag, cross


# ---- 1. the switch -----------------------------------------------------------------------------------------------------------

def test_the_switch_is_off_by_default_and_travels_with_the_handle(api, monkeypatch):
    """n = 5 under the pin (one front beyond LDS, the root), kept set for the whole test so that rr_pgo_extend and
    rr_pgo_remove_edges, which read the environment again, build such a tree too"""
    from rustrobotics_amd import _lib
    L = _lib.load()
    for k, v in PIN.items():
        monkeypatch.setenv(k, v)
    c = query_case("lattice5", "initial")
    arrays, cand, sets = c["arrays"], c["cand"], c["sets"]
    g = api[0].from_arrays(*arrays)
    assert g.stats()["n_big_fronts"] >= 1
    assert g.marginals_big_fronts is False and g.query_big_fronts is False

    def refused_as_today():
        code, msg = refusal(lambda: g.marginals([0]))
        assert code == _lib.EUNSUPPORTED and msg.startswith("rr_pgo_marginals:") and "beyond LDS" in msg, msg
        assert "use rr_pgo_covariances with rr_pgo_set_query_big_fronts" in msg, msg
    refused_as_today()
    g.query_big_fronts = True            # the other switch alone does not enable it
    assert g.marginals_big_fronts is False
    refused_as_today()
    g.query_big_fronts = False
    g.marginals_big_fronts = True        # ... and this one does not enable the five tree-solve queries
    assert g.marginals_big_fronts is True and g.query_big_fronts is False
    for who, call in the_five(g, cand, sets).items():
        code, msg = refusal(call)
        assert code == _lib.EUNSUPPORTED and msg.startswith(who + ":") and "beyond LDS" in msg, (who, code, msg)
    assert len(g.marginals([0])) == 1
    g.marginals_big_fronts = False
    refused_as_today()
    g.marginals_big_fronts = True
    # ---- one new pose, hung on node 0 by a copy of the first edge's measurement: the grown handle answers without being asked again
    n, ml, il = g.num_nodes, 7, 21
    g.extend([2], [0], [n], arrays[5][:ml], arrays[6][:il], node_kind=[2])
    assert g.num_nodes == n + 1 and g.stats()["n_big_fronts"] >= 1 and g.marginals_big_fronts is True and g.query_big_fronts is False
    vals, _ = g.marginal_blocks([n, 0], [n, n])
    assert np.all(np.isfinite(vals)) and len(vals) == 72
    # ---- a loop edge goes (every lattice node keeps three or more edges)
    g.remove_edges([7])
    assert g.stats()["n_big_fronts"] >= 1 and g.marginals_big_fronts is True
    assert len(g.marginals()) == n + 1
    # ---- off travels too
    g.marginals_big_fronts = False
    g.remove_edges([9])
    assert g.marginals_big_fronts is False
    refused_as_today()
    # ---- the setter is RR_PGO_OK on handles that refuse for their own reasons, and those reasons come first
    for precision, word in (("f32", "F32"), ("mixed", "MIXED")):
        h = api[0].from_arrays(*arrays, precision=precision)
        h.marginals_big_fronts = True
        code, msg = refusal(lambda: h.marginals([0]))
        assert code == _lib.EUNSUPPORTED and word in msg and "beyond LDS" not in msg, msg
    assert L.rr_pgo_get_marginals_big_fronts(None) == 0 and L.rr_pgo_set_marginals_big_fronts(None, 1) == _lib.EINVAL


# ---- 2. no effect without fronts beyond LDS ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["simulation-pose-pose", "intel", "parking-garage"])
def test_the_switch_changes_no_bit_and_no_launch_on_a_tree_without_fronts_beyond_lds(api, name):
    off, on = api[0].new(g2o_path(name)), api[0].new(g2o_path(name))
    on.marginals_big_fronts = True
    assert off.stats()["n_big_fronts"] == 0
    v0, o0 = off.marginal_blocks()
    v1, o1 = on.marginal_blocks()
    assert np.array_equal(o0, o1) and np.array_equal(v0, v1)
    counts = ("n_launches_per_iter", "n_plain_iterations", "n_graph_replays", "n_loop_items", "n_graph_captures")
    s0, s1 = off.stats(), on.stats()
    assert [s0[k] for k in counts] == [s1[k] for k in counts]


# ---- 3. every node and every edge ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,which", CASES, ids=IDS)
def test_all_diagonal_blocks_and_all_edge_blocks(api, name, which, monkeypatch):
    all_blocks(f"{name} {which}", handle(api, name, which, monkeypatch), lattice_blocks(name, which))


# ---- 4. fronts by kind, against the tree solve -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(LATTICES))
def test_nodes_by_the_kind_of_their_front_against_rr_pgo_covariances(api, name, monkeypatch, capfd):
    """a node in the root front, one in a non-root front beyond LDS, one in an LDS front without children whose parent is
    beyond LDS: each block asked for on its own, and against rr_pgo_covariances under rr_pgo_set_query_big_fronts, which
    gets it by a forward solve over the tree -- another path through other kernels"""
    which = "initial"
    k = node_kinds(api, name, which, monkeypatch, capfd)
    fronts, front_of = k["fronts"], k["front_of"]
    n = len(front_of)

    def first(pred):
        return next((v for v in range(n) if pred(fronts[front_of[v]])), None)
    picks = dict(root=k["root"], big=k["big"],
                 leaf=first(lambda f: not f["big"] and f["children"] == 0 and f["parent"] >= 0 and fronts[f["parent"]]["big"]))
    print(f"{name}: query nodes {picks}")
    assert picks["root"] is not None and picks["leaf"] is not None and fronts[front_of[picks["root"]]]["big"]
    assert (picks["big"] is not None) == (name != "lattice5")
    g = handle(api, name, which, monkeypatch)
    other = create(api, name, which, monkeypatch)   # rr_pgo_set_query_big_fronts on, this file's switch off
    every = g.marginals()
    for kind, v in picks.items():
        if v is None:
            continue
        want, floor = lattice_blocks(name, which)["diag"][v], lattice_blocks(name, which)["floor_diag"]
        alone = g.marginals([v])[0]
        assert np.array_equal(alone, every[v]), (kind, v)
        cv, _ = other.covariance_blocks([v], [v])
        check_blocks(f"{name} node {v} ({kind}) against the reference", [alone], [want], floor)
        check_blocks(f"{name} node {v} ({kind}) against rr_pgo_covariances", [alone], [cv.reshape(6, 6)], floor)


# ---- 5. a pair that shares no front ----------------------------------------------------------------------------------------------

def test_a_pair_that_shares_no_front_is_refused_and_writes_nothing(api, monkeypatch):
    from rustrobotics_amd import _lib
    L = _lib.load()
    g = handle(api, "lattice7", "initial", monkeypatch)
    n = g.num_nodes
    rng = np.random.default_rng(11)
    refused = 0
    ip = C.POINTER(C.c_int32)
    for _ in range(40):
        a, b = (int(v) for v in rng.choice(n, 2, replace=False))
        na, nb = np.array([0, a], np.int32), np.array([0, b], np.int32)
        out = np.full(72, -777.0)
        nv = C.c_int64()
        rc = L.rr_pgo_marginals(g._h, 2, na.ctypes.data_as(ip), nb.ctypes.data_as(ip), out.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(nv))
        if rc == _lib.EINVAL:
            refused += 1
            msg = L.rr_pgo_last_error().decode()
            assert f"nodes {a} and {b}" in msg and "share no front" in msg, msg
            assert np.all(out == -777.0)
        else:
            assert rc == 0, (rc, L.rr_pgo_last_error())
    print(f"lattice7: {refused} of 40 seeded pairs refused")
    assert refused > 0


# ---- 6. fixed nodes and priors ----------------------------------------------------------------------------------------------------

def test_fixed_nodes_and_priors(api, monkeypatch, capfd):
    """20 seeded poses fixed, two of them in the root front, five priors on free poses, keep_anchor = 0: Sigma is
    conditional on the fixed poses, so their blocks are exact zeros"""
    name, which = "lattice6", "initial"
    k = node_kinds(api, name, which, monkeypatch, capfd)
    n = len(k["front_of"])
    in_root = [v for v in range(n) if k["fronts"][k["front_of"][v]]["parent"] < 0][:2]
    c = fixed_case(in_root)
    F = c["F"]
    assert all(v in F for v in in_root) and len(F) == 20
    g = fresh(api, name, which, monkeypatch)
    g.set_priors(*c["priors"])
    g.set_fixed(F, keep_anchor=False)
    diag = g.marginals()
    a, b = c["a"], c["b"]
    vals, off = g.marginal_blocks(a, b)
    cross = split(vals, off, c["cross"])
    live_d = [v for v in range(n) if v not in F]
    live_c = [q for q in range(len(a)) if a[q] not in F and b[q] not in F]
    print(f"lattice6 fixed {F}, priors on {c['prior_nodes']}: {len(a) - len(live_c)} of {len(a)} edge blocks with a fixed node")
    assert 0 < len(live_c) < len(a)
    check_blocks("lattice6 with 20 fixed poses and 5 priors, diagonal blocks", [diag[v] for v in live_d], [c["diag"][v] for v in live_d], c["floor"])
    check_blocks("lattice6 with 20 fixed poses and 5 priors, edge blocks", [cross[q] for q in live_c], [c["cross"][q] for q in live_c], c["floor"])
    for v in F:
        assert not np.any(diag[v]) and not np.any(c["diag"][v]), v
    for q in range(len(a)):
        if q not in live_c:
            assert not np.any(cross[q]) and not np.any(c["cross"][q]), (a[q], b[q])


# ---- 7. point landmarks: 3-scalar nodes inside fronts beyond LDS -----------------------------------------------------------------

@pytest.mark.parametrize("which", STATES)
def test_landmark_case(api, which, monkeypatch):
    name = "landmarks6"
    want = landmark_blocks(which)
    diag, cross = all_blocks(f"{name} {which}", handle(api, name, which, monkeypatch), want)
    nk = at_state(name, which)[0][0]
    assert [d.shape[0] for d in diag] == [6 if kind == 2 else 3 for kind in nk]
    assert {x.shape for x in cross} == {(6, 6), (6, 3)}


# ---- 8. the state is untouched ---------------------------------------------------------------------------------------------------

def test_optimize_after_marginals_gives_the_same_bits(api, monkeypatch):
    a, b = fresh(api, "lattice6", "initial", monkeypatch), fresh(api, "lattice6", "initial", monkeypatch)
    a.marginals()
    ea, na = a.optimize(3, return_norms=True)
    eb, nb = b.optimize(3, return_norms=True)
    assert np.array_equal(np.array(ea), np.array(eb)) and np.array_equal(np.array(na), np.array(nb))
    assert np.array_equal(a.state(), b.state())
    a.marginals([0, 1])   # ... and between two optimize calls
    assert np.array_equal(np.array(a.optimize(3)), np.array(b.optimize(3)))
    assert np.array_equal(a.state(), b.state())


# ---- 9. sphere2500 ---------------------------------------------------------------------------------------------------------------

def test_sphere2500_after_five_iterations(api):
    """300 seeded nodes, the anchor and the last node, and 60 seeded edges against the sparse reference; the same nodes
    against rr_pgo_covariances.  The handle and its reference are those of tests/test_big_front_queries_gpu.py (built once);
    neither call changes the state."""
    s = sphere(api)
    g, ref = s["g"], s["gate"].ref
    g.marginals_big_fronts = True
    assert g.stats()["n_big_fronts"] > 0
    n = g.num_nodes
    rng = np.random.default_rng(20240607)
    nodes = sorted(set(int(v) for v in rng.choice(n, 300, replace=False)) | {n - 1, g.anchor_node})
    got = g.marginals(nodes)
    t = g.marginals_times()
    print(f"sphere2500 after 5 iterations: linearise + factor {t[0]:.3f} ms, selected inverse {t[1]:.3f} ms, gather {t[2]:.3f} ms")
    want, floor = ref.blocks(nodes)
    check_blocks(f"sphere2500 after 5 iterations, {len(nodes)} diagonal blocks", got, want, floor)
    every = g.marginals()
    for q, v in enumerate(nodes):
        assert np.array_equal(got[q], every[v]) and np.array_equal(got[q], got[q].T), v
    _, _, _, ef, et, _, _ = g.graph_arrays()
    idx = np.random.default_rng(7).choice(len(ef), 60, replace=False)
    a, b = ef[idx].astype(np.int32), et[idx].astype(np.int32)
    vals, off = g.marginal_blocks(a, b)
    wc, fc = ref.blocks(a, b)
    cross = split(vals, off, wc)
    check_blocks("sphere2500 after 5 iterations, 60 seeded edges", cross, wc, fc)
    vals_t, off_t = g.marginal_blocks(b, a)
    for q, w in enumerate(cross):
        assert np.array_equal(vals_t[off_t[q]:off_t[q + 1]].reshape(6, 6), w.T)
    cv, co = g.covariance_blocks(nodes, nodes)
    tc = g.covariances_times()
    print(f"sphere2500: rr_pgo_covariances of the same {len(nodes)} nodes: tree solve {tc[1]:.3f} ms")
    check_blocks("sphere2500 after 5 iterations, against rr_pgo_covariances", got, split(cv, co, want), floor)
