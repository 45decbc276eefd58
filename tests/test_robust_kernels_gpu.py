"""Robust kernels on the GPU (run with -m gpu on an MI355X): rr_pgo_set_robust_kernel / rr_pgo_edge_errors through the
Python mirror, against a plain handle built with Omega scaled by the weights, against the CPU reference on the unchanged
oracle (tests/robust_reference.py), and against the plain path it must leave alone."""
import numpy as np
import pytest

from conftest import g2o_path
from robust_reference import (INFO_LEN, RobustReference, intel_with_outliers, oracle_arrays, position_error, rho,
                              weight)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

SE2_FILES = ["simulation-pose-landmark", "simulation-pose-pose", "intel", "input_M3500_g2o", "dlr"]
# delta of the trajectory tests: every run ends by the stop rule well inside 100 iterations (dlr at delta = 1 does not)
TRAJ_DELTA = {"intel": 1.0, "input_M3500_g2o": 1.0, "dlr": 30.0, "sphere2500": 1.0}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver, PoseGraphError
    return PoseGraph, PoseGraphSolver, PoseGraphError


@pytest.fixture(scope="module")
def oracle_arrays_of():
    from oracle.oracle import OracleGraph
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle_arrays(OracleGraph.load(g2o_path(name)))
        return cache[name]
    return get


def _scaled_arrays(arrays, w):
    a = list(arrays)
    rep = np.repeat(np.arange(len(a[2])), [INFO_LEN[int(k)] for k in a[2]])
    a[6] = np.asarray(a[6], np.float64) * w[rep]
    return a


def _assert_same_system(g, ref, lm):
    lam = 0.37 if lm else 0.0
    br, bc, bo, vals, b = g.assemble(lam, lm)
    br2, bc2, bo2, vals2, b2 = ref.assemble(lam, lm)
    assert np.array_equal(br, br2) and np.array_equal(bc, bc2) and np.array_equal(bo, bo2)
    scale = np.abs(vals2).max()
    assert np.abs(vals - vals2).max() <= 1e-12 * scale
    # the weights of `ref` come from k_edge_errors, whose e carries its own rounding: near a consistent state (M3500's
    # start, sphere2500 after two steps) e is a difference of nearly equal poses and b a sum of cancelling terms, so b is
    # compared against the scale of the system as well as its own
    assert np.abs(b - b2).max() <= 1e-11 * max(np.abs(b2).max(), 1e-3 * np.sqrt(scale))
    assert vals.max() > 1e7   # the anchor prior is there, unweighted


# ---- 1. the assembled system --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SE2_FILES + ["sphere2500"])
@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_assembled_system_equals_the_plain_system_with_weighted_information(api, name, kind):
    """assemble() with a kernel (with and without LM's lambda, at the file's state and after two steps) equals assemble()
    of a plain handle whose Omega is scaled by w(s) of every edge: the weight reaches the diagonal blocks, the right-hand
    side and the off-diagonal blocks, and not the prior or lambda."""
    PoseGraph = api[0]
    g = PoseGraph.new(g2o_path(name))
    arrays = g.graph_arrays()
    g.set_robust_kernel(kind, 1.0)
    # the file's state, then two robust Gauss-Newton steps further.  M3500 starts at its odometry, where every edge's s is
    # rounding noise (1e-11): the weights recomputed by k_edge_errors would differ from the linearisation's in the 7th digit
    for steps in ((0, 2) if name != "input_M3500_g2o" else (2,)):
        for _ in range(steps):
            g.update_nodes(g.linearize_and_solve())
        s0, _ = g.edge_errors()
        delta = float(np.sqrt(np.median(s0[s0 > 0])))   # a mix of edges on both sides of delta^2
        g.set_robust_kernel(kind, delta)
        s, w = g.edge_errors()
        np.testing.assert_allclose(w, weight(kind, s, delta), rtol=1e-14)
        assert (w < 1).any()
        ref = PoseGraph.from_arrays(*_scaled_arrays(arrays, w))
        st = g.state()
        g.set_state(st)     # the same bits of (x, y, cos, sin) in both handles
        ref.set_state(st)
        for lm in (False, True):
            _assert_same_system(g, ref, lm)


# ---- 2. cost and per-edge values ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SE2_FILES + ["sphere2500"])
def test_chi2_and_edge_errors_match_the_cpu_reference(api, oracle_arrays_of, name):
    g = api[0].new(g2o_path(name))
    ref = RobustReference(oracle_arrays_of(name), None)
    so = ref.edge_s()
    s, w = g.edge_errors()
    np.testing.assert_allclose(s, so, rtol=1e-12, atol=1e-12 * so.mean())
    assert np.all(w == 1.0)
    chi = g.global_error()
    assert abs(s.sum() - chi) <= 1e-12 * chi
    for kind, delta in (("huber", 1.0), ("cauchy", 1.0), ("cauchy", 25.0)):
        g.set_robust_kernel(kind, delta)
        expect = float(np.sum(rho(kind, so, delta)))
        assert abs(g.global_error() - expect) <= 1e-12 * expect
        s2, w2 = g.edge_errors()
        np.testing.assert_array_equal(s2, s)
        np.testing.assert_allclose(w2, weight(kind, so, delta), rtol=1e-11)


# ---- 3. trajectories ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["intel", "input_M3500_g2o", "dlr", "sphere2500"])
@pytest.mark.parametrize("kind", ["cauchy", "huber"])
def test_gauss_newton_trajectory_matches_the_cpu_reference(api, oracle_arrays_of, name, kind):
    delta = TRAJ_DELTA[name]
    g = api[0].new(g2o_path(name))
    g.set_robust_kernel(kind, delta)
    eg, ng = g.optimize(100, return_norms=True)
    ref = RobustReference(oracle_arrays_of(name), kind, delta)
    eo, no = ref.optimize(100)
    assert len(eg) == len(eo) and len(eg) < 101
    np.testing.assert_allclose(eg, eo, rtol=1e-7)
    np.testing.assert_allclose(ng, no, rtol=1e-4, atol=1e-8)
    if name == "sphere2500":
        a, b = g.state().reshape(-1, 7), ref.state().reshape(-1, 7)
        dq = np.minimum(np.abs(a[:, 3:] - b[:, 3:]).max(1), np.abs(a[:, 3:] + b[:, 3:]).max(1)).max()
        assert max(np.abs(a[:, :3] - b[:, :3]).max(), dq) <= 1e-8
    else:
        assert np.abs(g.state() - ref.state()).max() <= 1e-8


@pytest.mark.parametrize("kind", ["cauchy", "huber"])
def test_levenberg_marquardt_trajectory_matches_the_cpu_reference(api, oracle_arrays_of, kind):
    g = api[0].new(g2o_path("intel"), api[1].LevenbergMarquardt)
    g.set_robust_kernel(kind, 1.0)
    eg = g.optimize(100)
    ref = RobustReference(oracle_arrays_of("intel"), kind, 1.0)
    eo, _ = ref.optimize(100, lm=True)
    assert len(eg) == len(eo)
    np.testing.assert_allclose(eg, eo, rtol=1e-8)
    assert np.abs(g.state() - ref.state()).max() <= 1e-6


def test_mixed_precision_reaches_the_robust_f64_answer(api, oracle_arrays_of):
    gm = api[0].new(g2o_path("intel"), precision="mixed")
    gm.set_robust_kernel("cauchy", 1.0)
    em = gm.optimize(30)
    ref = RobustReference(oracle_arrays_of("intel"), "cauchy", 1.0)
    eo, _ = ref.optimize(30)
    assert len(em) - 1 <= len(eo) - 1 + 3
    assert abs(em[-1] - eo[-1]) <= 1e-10 * eo[-1]
    assert np.abs(gm.state() - ref.state()).max() <= 1e-5


def test_single_precision_robust_handle_gets_through_the_gauge_transfer(api, oracle_arrays_of):
    g32 = api[0].new(g2o_path("intel"), precision="f32")
    g32.set_robust_kernel("cauchy", 1.0)
    e32 = g32.optimize(30)
    ref = RobustReference(oracle_arrays_of("intel"), "cauchy", 1.0)
    eo, _ = ref.optimize(30)
    assert abs(e32[0] - eo[0]) <= 1e-5 * eo[0]
    assert abs(e32[-1] - eo[-1]) <= 1e-4 * eo[-1]


# ---- 4. outliers --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def outliers():
    from oracle.oracle import OracleGraph
    clean, outl = intel_with_outliers(g2o_path("intel"))
    oc = OracleGraph.from_arrays(*clean)
    oc.optimize(100)
    return clean, outl, oc.state()


def test_false_loop_closures_are_switched_off_on_the_gpu(api, outliers):
    clean, outl, clean_opt = outliers
    g = api[0].from_arrays(*outl)
    g.set_robust_kernel("cauchy", 1.0)
    eg, ng = g.optimize(100, return_norms=True)
    assert len(eg) - 1 <= 20 and ng[-1] < 1e-4
    assert position_error(g.state(), clean_opt, clean[0]) <= 0.15
    _, w = g.edge_errors()
    m = len(clean[2])
    assert w[m:].max() < 0.01
    ref = RobustReference(outl, "cauchy", 1.0)
    eo, _ = ref.optimize(100)
    assert len(eg) == len(eo)
    np.testing.assert_allclose(eg, eo, rtol=1e-7)
    assert np.abs(g.state() - ref.state()).max() <= 1e-8


# ---- 5. masks -----------------------------------------------------------------------------------------------------

def test_mask_of_the_added_edges_matches_the_cpu_reference(api, outliers):
    clean, outl, clean_opt = outliers
    m = len(clean[2])
    mask = np.zeros(len(outl[2]), np.int32)
    mask[m:] = 1
    g = api[0].from_arrays(*outl)
    g.set_robust_kernel("cauchy", 1.0, mask)
    eg = g.optimize(100)
    _, w = g.edge_errors()
    assert np.all(w[:m] == 1.0) and w[m:].max() < 0.01
    ref = RobustReference(outl, "cauchy", 1.0, mask)
    eo, _ = ref.optimize(100)
    assert len(eg) == len(eo)
    np.testing.assert_allclose(eg, eo, rtol=1e-7)
    assert np.abs(g.state() - ref.state()).max() <= 1e-8
    assert position_error(g.state(), clean_opt, clean[0]) <= 0.15


@pytest.mark.parametrize("name", ["intel", "sphere2500"])
def test_all_zero_mask_is_plain_least_squares(api, name):
    g0, gz = api[0].new(g2o_path(name)), api[0].new(g2o_path(name))
    gz.set_robust_kernel("cauchy", 1.0, np.zeros(gz.num_edges, np.int32))
    e0, ez = np.array(g0.optimize(100)), np.array(gz.optimize(100))
    assert len(e0) == len(ez)
    np.testing.assert_allclose(ez, e0, rtol=1e-13, atol=0)
    np.testing.assert_allclose(gz.state(), g0.state(), rtol=1e-13, atol=1e-13)


# ---- 6. nothing changes without a kernel ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,solver", [("intel", "GaussNewton"), ("intel", "LevenbergMarquardt"), ("sphere2500", "GaussNewton")])
def test_kernel_set_then_cleared_is_bit_identical_to_a_plain_handle(api, name, solver):
    PoseGraph, S = api[0], api[1]
    fresh = PoseGraph.new(g2o_path(name), S[solver])
    g = PoseGraph.new(g2o_path(name), S[solver])
    g.set_robust_kernel("cauchy", 1.0)
    g.global_error()
    g.assemble()
    g.set_robust_kernel(None)
    e1, e0 = np.array(g.optimize(100)), np.array(fresh.optimize(100))
    assert e1.tobytes() == e0.tobytes()
    assert g.state().tobytes() == fresh.state().tobytes()


@pytest.mark.parametrize("name", ["intel", "sphere2500"])
def test_handle_after_a_robust_handle_is_bit_identical_to_a_fresh_one(api, name):
    """the stream / memory pools and the analysis cache hand a robust handle's resources to the next handle: it starts
    with no kernel"""
    PoseGraph = api[0]
    before = PoseGraph.new(g2o_path(name))
    e_before = np.array(before.optimize(100))
    s_before = before.state()
    del before
    r = PoseGraph.new(g2o_path(name))
    r.set_robust_kernel("huber", 0.5)
    r.optimize(3)
    del r
    after = PoseGraph.new(g2o_path(name))
    assert np.array(after.optimize(100)).tobytes() == e_before.tobytes()
    assert after.state().tobytes() == s_before.tobytes()


# ---- 7. captured graphs -------------------------------------------------------------------------------------------

def test_kernel_set_after_a_captured_iteration_reaches_the_replays(api, monkeypatch):
    """RR_PGO_FORCE_GRAPH=1: iterate_async replays a captured hipGraph.  A kernel set after the capture must throw the
    captured graph away (it holds the plain kernel and its arguments)."""
    PoseGraph = api[0]
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    g = PoseGraph.new(g2o_path("intel"))
    monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    g.iterate_async(1)   # captures the plain iteration
    g.sync()
    plain = PoseGraph.new(g2o_path("intel"))
    plain.set_robust_kernel("cauchy", 1.0)
    plain.set_state(g.state())
    g.set_robust_kernel("cauchy", 1.0)
    g.iterate_async(3)
    g.sync()
    plain.iterate_async(3)
    plain.sync()
    assert np.abs(g.state() - plain.state()).max() <= 1e-12
    assert abs(g.global_error() - plain.global_error()) <= 1e-12 * plain.global_error()
    # four replays of two captured graphs (the one with the kernel was captured anew) against three plain iterations
    st, sp = g.stats(), plain.stats()
    assert (st["n_graph_replays"], st["n_graph_captures"], st["n_plain_iterations"]) == (4, 2, 0)
    assert (sp["n_graph_replays"], sp["n_graph_captures"], sp["n_plain_iterations"]) == (0, 0, 3)


# ---- 8. sharded handles -------------------------------------------------------------------------------------------

def test_one_rank_sharded_handle_with_a_kernel_matches_the_unsharded_handle(api):
    from rustrobotics_amd import sharding, synthetic_grid_arrays
    PoseGraph, _, PoseGraphError = api
    arrays = synthetic_grid_arrays(60, 40)
    shards, coll = sharding.emulate(arrays, 1, "f64")
    shards[0].set_robust_kernel("cauchy", 1.0)
    es, ns = sharding.gauss_newton(shards, 20, coll)
    g = PoseGraph.from_arrays(*arrays)
    g.set_robust_kernel("cauchy", 1.0)
    eg, ng = g.optimize(20, return_norms=True)
    assert len(es) == len(eg)
    np.testing.assert_allclose(es, eg, rtol=1e-7)
    assert np.abs(shards[0].state() - g.state()).max() <= 1e-8
    with pytest.raises(PoseGraphError) as err:
        shards[0].edge_errors()
    assert err.value.code == -7


# ---- 9. bad arguments ---------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_leave_the_handle_alone(api):
    from rustrobotics_amd import _lib
    g = api[0].new(g2o_path("simulation-pose-landmark"))
    g.set_robust_kernel("huber", 2.0)
    chi = g.global_error()
    L = _lib.load()
    for kind, delta in ((3, 1.0), (-1, 1.0), (1, 0.0), (2, -1.0), (2, float("nan")), (1, float("inf"))):
        assert L.rr_pgo_set_robust_kernel(g._h, kind, delta, None) == _lib.EINVAL
        assert g.global_error() == chi
    assert L.rr_pgo_set_robust_kernel(g._h, _lib.ROBUST_NONE, float("nan"), None) == _lib.OK   # NONE ignores delta
    assert L.rr_pgo_edge_errors(g._h, None, None) == _lib.EINVAL
    with pytest.raises(ValueError):
        g.set_robust_kernel("tukey", 1.0)
    with pytest.raises(ValueError):
        g.set_robust_kernel("cauchy", 1.0, np.ones(3, np.int32))
