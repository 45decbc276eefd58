"""rr_pgo_marginals on the MI355X against the CPU reference (tests/marginals_reference.py).

A GPU block passes when its relative difference to the reference (max|A - B| / max|B|) is at most
max(1e-12, 100 x noise floor), the floor being the worst difference between the reference's two independent f64
computations of the same blocks at the same state.  Every comparison prints its worst figure before it asserts."""
import ctypes as C

import numpy as np
import pytest

from conftest import g2o_path
from marginals_reference import MarginalsReference, graph_at_state, rel_diff, tolerance

pytestmark = pytest.mark.gpu

SMALL = ["simulation-pose-landmark", "simulation-pose-pose", "intel"]   # dim <= 5184: every node
LARGE = ["dlr", "input_M3500_g2o", "parking-garage"]                    # 300 seeded nodes + the anchor + the last node (parking-garage: SE(3))


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


_REFS = {}


def reference_for(g, key=None):
    """MarginalsReference at the handle's current state (cached by `key`)"""
    if key is not None and key in _REFS:
        return _REFS[key]
    ref = MarginalsReference(graph_at_state(g.graph_arrays(), g.state()))
    if key is not None:
        _REFS[key] = ref
    return ref


def check_blocks(label, got, want, floor):
    tol = tolerance(floor)
    worst = max(rel_diff(a, b) for a, b in zip(got, want))
    print(f"{label}: {len(want)} blocks, worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert len(got) == len(want)
    assert worst <= tol, (label, worst, tol)
    return worst


def query_nodes(g, name):
    n = g.num_nodes
    if name in SMALL:
        return list(range(n))
    rng = np.random.default_rng(20240607)
    picked = set(int(v) for v in rng.choice(n, 300, replace=False))
    return sorted(picked | {n - 1} | ({g.anchor_node} if g.anchor_node >= 0 else set()))


@pytest.mark.parametrize("state", ["initial", "optimized"])
@pytest.mark.parametrize("name", SMALL + LARGE)
def test_diagonal_blocks_match_the_reference(api, name, state):
    g = api[0].new(g2o_path(name))
    if state == "optimized":
        g.optimize(10)
    nodes = query_nodes(g, name)
    got = g.marginals(None if name in SMALL else nodes)
    want, floor = reference_for(g, (name, state)).blocks(nodes)
    check_blocks(f"{name} {state} diagonal", got, want, floor)
    for b in got:
        assert np.array_equal(b, b.T)
    print(f"{name} {state}: linearise + factor {g.marginals_times()[0]:.3f} ms, selected inverse {g.marginals_times()[1]:.3f} ms, "
          f"gather {g.marginals_times()[2]:.3f} ms")


@pytest.mark.parametrize("name,count", [("simulation-pose-landmark", None), ("intel", 500)])
def test_cross_blocks_of_edges_match_the_reference(api, name, count):
    g = api[0].new(g2o_path(name))
    _, _, _, ef, et, _, _ = g.graph_arrays()
    idx = np.arange(len(ef)) if count is None else np.random.default_rng(7).choice(len(ef), count, replace=False)
    a, b = ef[idx].astype(np.int32), et[idx].astype(np.int32)
    vals, off = g.marginal_blocks(a, b)
    ref = reference_for(g, (name, "initial"))
    want, floor = ref.blocks(a, b)
    got = [vals[off[q]:off[q + 1]].reshape(w.shape) for q, w in enumerate(want)]
    check_blocks(f"{name} cross blocks", got, want, floor)
    # the other orientation is the transpose
    vals_t, off_t = g.marginal_blocks(b, a)
    for q, w in enumerate(got):
        assert np.array_equal(vals_t[off_t[q]:off_t[q + 1]].reshape(w.shape[1], w.shape[0]), w.T)
    for q in range(0, len(idx), max(1, len(idx) // 25)):
        J = g.joint_marginal(int(a[q]), int(b[q]))
        Jr, fl = ref.joint(int(a[q]), int(b[q]))
        assert np.array_equal(J, J.T)
        assert np.all(np.linalg.eigvalsh(J) > 0), (a[q], b[q])
        assert rel_diff(J, Jr) <= tolerance(fl)


def test_a_pair_that_shares_no_front_is_refused_and_writes_nothing(api):
    from rustrobotics_amd import _lib
    L = _lib.load()
    g = api[0].new(g2o_path("input_M3500_g2o"))
    n = g.num_nodes
    rng = np.random.default_rng(11)
    refused, answered = 0, []
    for _ in range(200):
        a, b = (int(v) for v in rng.choice(n, 2, replace=False))
        na, nb = np.array([a], np.int32), np.array([b], np.int32)
        out = np.full(9, -777.0)
        nv = C.c_int64()
        rc = L.rr_pgo_marginals(g._h, 1, na.ctypes.data_as(C.POINTER(C.c_int32)), nb.ctypes.data_as(C.POINTER(C.c_int32)),
                                out.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(nv))
        if rc == _lib.EINVAL:
            refused += 1
            msg = L.rr_pgo_last_error().decode()
            assert str(a) in msg and str(b) in msg, msg
            assert np.all(out == -777.0)
        else:
            assert rc == 0, (rc, L.rr_pgo_last_error())
            answered.append((a, b, out.reshape(3, 3).copy()))
    print(f"M3500: {refused} of 200 seeded pairs refused, {len(answered)} answered")
    assert refused > 0
    if answered:
        want, floor = reference_for(g, ("input_M3500_g2o", "initial")).blocks([p[0] for p in answered], [p[1] for p in answered])
        check_blocks("M3500 answered far pairs", [p[2] for p in answered], want, floor)


@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
def test_optimize_after_marginals_gives_the_same_bits(api, solver):
    PoseGraph, Solver = api
    a = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    b = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    a.marginals()
    ea, na = a.optimize(10, return_norms=True)
    eb, nb = b.optimize(10, return_norms=True)
    assert np.array_equal(np.array(ea), np.array(eb)) and np.array_equal(np.array(na), np.array(nb))
    assert np.array_equal(a.state(), b.state())
    a.marginals([0, 1])   # ... and between two optimize calls
    assert np.array_equal(np.array(a.optimize(3)), np.array(b.optimize(3)))
    assert np.array_equal(a.state(), b.state())


def test_replayed_graph_iterations_after_marginals_give_the_same_bits(api, monkeypatch):
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    a = api[0].new(g2o_path("intel"))
    b = api[0].new(g2o_path("intel"))
    monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    a.iterate_async(2)
    b.iterate_async(2)
    a.sync()
    b.sync()
    a.marginals()
    a.iterate_async(8)
    b.iterate_async(8)
    a.sync()
    b.sync()
    assert np.array_equal(a.state(), b.state())
    for g in (a, b):   # every one of the ten iterations was a replay of the one captured graph
        st = g.stats()
        assert (st["n_graph_replays"], st["n_graph_captures"], st["n_plain_iterations"]) == (10, 1, 0)


@pytest.mark.parametrize("env,value", [("RR_PGO_SOLVE_KFORM", "0"), ("RR_PGO_SOLVE_KFORM", "1"),
                                       ("RR_PGO_LDS_FLOW", "0"), ("RR_PGO_LDS_FLOW", "1")])
def test_every_schedule_and_solve_form_gives_the_reference(api, env, value, monkeypatch):
    monkeypatch.setenv(env, value)
    g = api[0].new(g2o_path("intel"))
    monkeypatch.delenv(env)
    want, floor = reference_for(g, ("intel", "initial")).blocks(range(g.num_nodes))
    check_blocks(f"intel {env}={value}", g.marginals(), want, floor)


def test_cauchy_weights_are_part_of_the_inverted_matrix(api):
    from robust_reference import RobustReference
    g = api[0].new(g2o_path("intel"))
    plain = g.marginals()
    g.set_robust_kernel("cauchy", 1.0)
    got = g.marginals()
    gw, w = RobustReference(g.graph_arrays(), "cauchy", 1.0).weighted_graph()
    assert np.min(w) < 0.5   # the weights matter at the initial state
    want, floor = MarginalsReference(gw).blocks(range(g.num_nodes))
    check_blocks("intel cauchy delta 1", got, want, floor)
    assert max(rel_diff(a, b) for a, b in zip(plain, got)) > 1e-3


def test_unsupported_handles_say_why(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]
    handles = {
        "sharded": PoseGraph.from_arrays(*PoseGraph.new(g2o_path("intel")).graph_arrays(), sharded=True),
        "mixed": PoseGraph.new(g2o_path("intel"), precision="mixed"),
        "f32": PoseGraph.new(g2o_path("intel"), precision="f32"),
        "sphere2500": PoseGraph.new(g2o_path("sphere2500")),
    }
    for what, h in handles.items():
        with pytest.raises(PoseGraphError) as ei:
            h.marginals([0])
        assert ei.value.code == _lib.EUNSUPPORTED, (what, ei.value)
        assert len(_lib.load().rr_pgo_last_error()) > 0
        print(what, "->", ei.value)


def test_size_query_defaults_and_bad_node_ids(api):
    from rustrobotics_amd import _lib
    L = _lib.load()
    g = api[0].new(g2o_path("simulation-pose-landmark"))
    n = g.num_nodes
    nk = g.graph_arrays()[0]
    dims = np.where(nk == 0, 3, 2)
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    # size query, all nodes
    nv, off = C.c_int64(), np.zeros(n + 1, np.int64)
    assert L.rr_pgo_marginals(g._h, n, None, None, None, off.ctypes.data_as(lp), C.byref(nv)) == 0
    assert nv.value == int(np.sum(dims * dims)) and np.array_equal(np.diff(off), dims * dims)
    # node_a == NULL needs n_query == num_nodes
    assert L.rr_pgo_marginals(g._h, n - 1, None, None, None, None, C.byref(nv)) == _lib.EINVAL
    # node_b == NULL: diagonal blocks of node_a, equal to the same blocks of the all-nodes call and to (a, a) queries
    every = g.marginals()
    pick = np.array([n - 1, 0, 5], np.int32)
    some = g.marginals(pick)
    vals, off2 = g.marginal_blocks(pick, pick)
    for q, v in enumerate(pick):
        assert np.array_equal(some[q], every[v])
        assert np.array_equal(vals[off2[q]:off2[q + 1]].reshape(some[q].shape), every[v])
    # out-of-range ids
    for bad in (-1, n):
        na = np.array([0, bad], np.int32)
        out = np.full(18, -777.0)
        assert L.rr_pgo_marginals(g._h, 2, na.ctypes.data_as(ip), None, out.ctypes.data_as(dp), None, C.byref(nv)) == _lib.EINVAL
        assert np.all(out == -777.0)
        assert L.rr_pgo_marginals(g._h, 2, na[::-1].copy().ctypes.data_as(ip), na.ctypes.data_as(ip), out.ctypes.data_as(dp), None,
                                  C.byref(nv)) == _lib.EINVAL
    # node_b without node_a
    assert L.rr_pgo_marginals(g._h, 1, None, pick.ctypes.data_as(ip), None, None, C.byref(nv)) == _lib.EINVAL
