"""rr_pgo_covariances on the MI355X against the CPU reference (tests/marginals_reference.py).

The rule of tests/test_marginals_gpu.py: a GPU block passes when its relative difference to the reference (max|A - B| /
max|B|) is at most max(1e-12, 100 x noise floor), the floor being the worst difference between the reference's two
independent f64 computations of the same blocks at the same state; here the floor itself must also be at most 1e-6.
Every comparison prints its worst figure, the floor and the tolerance before it asserts."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import g2o_path
from covariances_cases import FAR_GRAPHS, FLOOR_MAX, far_pairs, joint_from_blocks
from marginals_reference import MarginalsReference, graph_at_state, rel_diff, tolerance

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("state", ["initial", "optimized"])
@pytest.mark.parametrize("name", FAR_GRAPHS)
def test_far_pairs_match_the_reference(api, name, state):
    g = api[0].new(g2o_path(name))
    if state == "optimized":
        g.optimize(10)
    nodes, a, b = far_pairs(g.num_nodes)
    k = len(nodes)
    vals, off = g.covariance_blocks(a, b)
    ref = reference_for(g, (name, state))
    want, floor = ref.blocks(a, b)
    got = split(vals, off, want)
    check_blocks(f"{name} {state} far pairs", got, want, floor)
    t = g.covariances_times()
    print(f"{name} {state}: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, products + gather {t[2]:.3f} ms")
    # ---- structure: Sigma(b, a) = Sigma(a, b)^T and diagonal blocks symmetric, bit for bit
    for i in range(k):
        assert np.array_equal(got[i * k + i], got[i * k + i].T)
        for j in range(k):
            assert np.array_equal(got[j * k + i], got[i * k + j].T), (nodes[i], nodes[j])
    # ---- the dense joint matrix of the set
    J = g.covariance(nodes)
    Jr = joint_from_blocks(want, k)
    worst = rel_diff(J, Jr)
    print(f"{name} {state} joint {J.shape[0]} x {J.shape[0]}: relative difference {worst:.3g}, tolerance {tolerance(floor):.3g}, "
          f"smallest eigenvalue {np.min(np.linalg.eigvalsh(J)):.3g}")
    assert J.shape == Jr.shape
    assert np.array_equal(J, J.T)
    assert np.array_equal(J, joint_from_blocks(got, k))
    assert np.all(np.linalg.eigvalsh(J) > 0)
    assert worst <= tolerance(floor)


@pytest.mark.parametrize("name", ["intel", "simulation-pose-landmark"])
def test_the_anchor_sits_on_its_prior(api, name):
    g = api[0].new(g2o_path(name))
    assert g.anchor_node >= 0
    vals, _ = g.covariance_blocks([g.anchor_node], [g.anchor_node])
    d = int(round(np.sqrt(len(vals))))
    print(f"{name}: anchor block diagonal {np.diag(vals.reshape(d, d))}")
    np.testing.assert_allclose(np.diag(vals.reshape(d, d)), 1e-7, rtol=1e-3)


def test_the_pairs_the_selected_inverse_refuses_are_answered(api):
    """the loop of test_marginals_gpu's refusal test (M3500, seed 11, 200 pairs), through rr_pgo_covariances"""
    g = api[0].new(g2o_path("input_M3500_g2o"))
    n = g.num_nodes
    rng = np.random.default_rng(11)
    pairs = [tuple(int(v) for v in rng.choice(n, 2, replace=False)) for _ in range(200)]
    a, b = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    vals, off = g.covariance_blocks(a, b)
    assert len(off) == 201 and off[-1] == 9 * 200
    want, floor = reference_for(g, ("input_M3500_g2o", "initial")).blocks(a, b)
    check_blocks("M3500 the 200 seeded pairs", split(vals, off, want), want, floor)


def test_agreement_with_the_selected_inverse(api):
    g = api[0].new(g2o_path("intel"))
    n = g.num_nodes
    _, _, _, ef, et, _, _ = g.graph_arrays()
    idx = np.random.default_rng(7).choice(len(ef), 500, replace=False)
    a = np.concatenate([np.arange(n), ef[idx]]).astype(np.int32)
    b = np.concatenate([np.arange(n), et[idx]]).astype(np.int32)
    sel, off_s = g.marginal_blocks(a, b)
    cov, off_c = g.covariance_blocks(a, b)
    assert np.array_equal(off_s, off_c)
    want, floor = reference_for(g, ("intel", "initial")).blocks(a, b)
    check_blocks("intel diagonal + 500 edge pairs, against the reference", split(cov, off_c, want), want, floor)
    check_blocks("intel diagonal + 500 edge pairs, against the selected inverse", split(cov, off_c, want), split(sel, off_s, want), floor)


def test_a_query_of_many_chunks_and_its_pairs_one_at_a_time(api):
    g = api[0].new(g2o_path("dlr"))
    n = g.num_nodes
    rng = np.random.default_rng(5)
    nodes = rng.choice(n, 400, replace=False).astype(np.int32)
    a, b = nodes, rng.permutation(nodes).astype(np.int32)
    vals, off = g.covariance_blocks(a, b)
    t = g.covariances_times()
    print(f"dlr 400 nodes: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, products + gather {t[2]:.3f} ms")
    want, floor = reference_for(g, ("dlr", "initial")).blocks(a, b)
    got = split(vals, off, want)
    check_blocks("dlr 400 seeded nodes paired at random", got, want, floor)
    # the same call twice: the same bits
    vals2, _ = g.covariance_blocks(a, b)
    assert np.array_equal(vals, vals2)
    # a block's bits do not depend on what else is asked for
    for q in range(0, 400, 20):
        one, _ = g.covariance_blocks(a[q:q + 1], b[q:q + 1])
        assert np.array_equal(one.reshape(got[q].shape), got[q]), (q, a[q], b[q])


def test_a_plan_cut_by_the_workspace_bound_gives_the_same_bits(api, monkeypatch):
    """24 pairs of 48 distinct seeded nodes of intel: 144 columns, at least 5 chunks.  A handle whose workspace bound
    (RR_PGO_TS_WS_BYTES) is the largest need of a single pair must cut the list: a pair alone puts both nodes in one chunk
    and needs the union of their two root paths; the list needs the sum over its chunks of each chunk's union, which holds
    those two paths and at least the root front of a third chunk.  The cut changes no bit."""
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]

    def handle(bound=None):
        if bound is None:
            return PoseGraph.new(g2o_path("intel"))
        monkeypatch.setenv("RR_PGO_TS_WS_BYTES", str(bound))
        g = PoseGraph.new(g2o_path("intel"))
        monkeypatch.delenv("RR_PGO_TS_WS_BYTES")
        return g

    def refused(g, q):
        """the bytes the refusal of pair q alone names"""
        with pytest.raises(PoseGraphError) as ei:
            g.covariance_blocks(a[q:q + 1], b[q:q + 1])
        assert ei.value.code == _lib.ENOMEM, ei.value
        msg = _lib.load().rr_pgo_last_error().decode()
        m = re.fullmatch(r"rr_pgo_covariances: one pair needs (\d+) bytes of workspace", msg)
        assert m, msg
        return int(m.group(1))

    A = handle()
    nodes = np.random.default_rng(17).choice(A.num_nodes, 48, replace=False).astype(np.int32)
    a, b = nodes[:24], nodes[24:]
    vals_A, off = A.covariance_blocks(a, b)
    assert off[-1] == 24 * 9
    B = handle(1)
    need = [refused(B, q) for q in range(24)]
    print(f"intel, 24 pairs alone: workspace needs {min(need)} .. {max(need)} bytes")
    C_ = handle(max(need))
    vals_C, off_C = C_.covariance_blocks(a, b)
    assert np.array_equal(off_C, off)
    assert np.array_equal(vals_C, vals_A)
    for q in range(24):
        one, _ = C_.covariance_blocks(a[q:q + 1], b[q:q + 1])
        assert np.array_equal(one, vals_A[off[q]:off[q + 1]]), (q, a[q], b[q])
    D = handle(max(need) - 1)
    assert refused(D, int(np.argmax(need))) == max(need)


@pytest.mark.parametrize("env,value", [(None, None), ("RR_PGO_SOLVE_KFORM", "0"), ("RR_PGO_LDS_FLOW", "0")])
@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
def test_optimize_after_covariances_gives_the_same_bits(api, solver, env, value, monkeypatch):
    PoseGraph, Solver = api
    if env:
        monkeypatch.setenv(env, value)
    a = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    b = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    if env:
        monkeypatch.delenv(env)
    _, qa, qb = far_pairs(a.num_nodes)
    vals, off = a.covariance_blocks(qa, qb)
    if env:   # the blocks do not depend on the schedule or the solve form
        want, floor = reference_for(a, ("intel", "initial")).blocks(qa, qb)
        check_blocks(f"intel {env}={value}", split(vals, off, want), want, floor)
    ea, na = a.optimize(10, return_norms=True)
    eb, nb = b.optimize(10, return_norms=True)
    assert np.array_equal(np.array(ea), np.array(eb)) and np.array_equal(np.array(na), np.array(nb))
    assert np.array_equal(a.state(), b.state())
    a.covariance([0, a.num_nodes - 1])   # ... and between two optimize calls
    assert np.array_equal(np.array(a.optimize(3)), np.array(b.optimize(3)))
    assert np.array_equal(a.state(), b.state())


def test_replayed_graph_iterations_after_covariances_give_the_same_bits(api, monkeypatch):
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    a = api[0].new(g2o_path("intel"))
    b = api[0].new(g2o_path("intel"))
    monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    a.iterate_async(2)
    b.iterate_async(2)
    a.sync()
    b.sync()
    a.covariance([3, 900])
    a.iterate_async(8)
    b.iterate_async(8)
    a.sync()
    b.sync()
    assert np.array_equal(a.state(), b.state())
    for g in (a, b):   # every one of the ten iterations was a replay of the one captured graph
        st = g.stats()
        assert (st["n_graph_replays"], st["n_graph_captures"], st["n_plain_iterations"]) == (10, 1, 0)


def test_cauchy_weights_are_part_of_the_inverted_matrix(api):
    from robust_reference import RobustReference
    g = api[0].new(g2o_path("intel"))
    _, a, b = far_pairs(g.num_nodes)
    plain, off = g.covariance_blocks(a, b)
    g.set_robust_kernel("cauchy", 1.0)
    vals, off = g.covariance_blocks(a, b)
    gw, w = RobustReference(g.graph_arrays(), "cauchy", 1.0).weighted_graph()
    assert np.min(w) < 0.5   # the weights matter at the initial state
    want, floor = MarginalsReference(gw).blocks(a, b)
    got = split(vals, off, want)
    check_blocks("intel cauchy delta 1 far pairs", got, want, floor)
    assert max(rel_diff(p, q) for p, q in zip(split(plain, off, want), got)) > 1e-3


def test_unsupported_handles_say_why(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]
    handles = {
        "sharded": (PoseGraph.from_arrays(*PoseGraph.new(g2o_path("intel")).graph_arrays(), sharded=True), "sharded"),
        "mixed": (PoseGraph.new(g2o_path("intel"), precision="mixed"), "MIXED"),
        "f32": (PoseGraph.new(g2o_path("intel"), precision="f32"), "F32"),
        "sphere2500": (PoseGraph.new(g2o_path("sphere2500")), "beyond LDS"),
    }
    for what, (h, word) in handles.items():
        with pytest.raises(PoseGraphError) as ei:
            h.covariance_blocks([0], [1])
        assert ei.value.code == _lib.EUNSUPPORTED, (what, ei.value)
        msg = _lib.load().rr_pgo_last_error().decode()
        print(what, "->", msg)
        assert "rr_pgo_covariances" in msg and word in msg, (what, msg)


def test_size_query_and_bad_node_ids(api):
    from rustrobotics_amd import _lib
    L = _lib.load()
    g = api[0].new(g2o_path("simulation-pose-landmark"))
    n = g.num_nodes
    nk = g.graph_arrays()[0]
    dims = np.where(nk == 0, 3, 2)
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    # size query: every node against the last one
    a, b = np.arange(n, dtype=np.int32), np.full(n, n - 1, np.int32)
    nv, off = C.c_int64(), np.zeros(n + 1, np.int64)
    assert L.rr_pgo_covariances(g._h, n, a.ctypes.data_as(ip), b.ctypes.data_as(ip), None, off.ctypes.data_as(lp), C.byref(nv)) == 0
    assert nv.value == int(np.sum(dims * dims[n - 1])) and np.array_equal(np.diff(off), dims * dims[n - 1])
    # ... and the call itself, without out_offset
    out = np.zeros(nv.value)
    assert L.rr_pgo_covariances(g._h, n, a.ctypes.data_as(ip), b.ctypes.data_as(ip), out.ctypes.data_as(dp), None, None) == 0
    want, floor = reference_for(g).blocks(a, b)
    check_blocks("simulation-pose-landmark every node against the last", split(out, off, want), want, floor)
    # node_a and node_b are both required; n_query >= 0; an empty query is fine
    assert L.rr_pgo_covariances(g._h, 1, a.ctypes.data_as(ip), None, None, None, C.byref(nv)) == _lib.EINVAL
    assert L.rr_pgo_covariances(g._h, 1, None, a.ctypes.data_as(ip), None, None, C.byref(nv)) == _lib.EINVAL
    assert L.rr_pgo_covariances(g._h, -1, a.ctypes.data_as(ip), b.ctypes.data_as(ip), None, None, C.byref(nv)) == _lib.EINVAL
    assert L.rr_pgo_covariances(g._h, 0, None, None, out.ctypes.data_as(dp), None, C.byref(nv)) == 0 and nv.value == 0
    # out-of-range ids: nothing is written
    for bad in (-1, n):
        na, nb = np.array([0, bad], np.int32), np.array([1, 2], np.int32)
        for x, y in ((na, nb), (nb, na)):
            sentinel = np.full(18, -777.0)
            assert L.rr_pgo_covariances(g._h, 2, x.ctypes.data_as(ip), y.ctypes.data_as(ip), sentinel.ctypes.data_as(dp), None,
                                        C.byref(nv)) == _lib.EINVAL
            assert np.all(sentinel == -777.0)
            assert "out of range" in L.rr_pgo_last_error().decode()
