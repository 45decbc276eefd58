"""Pivot columns in arrival order and children added mid-panel (symbolic.cpp step 5, kernels.hip.h panel_factor /
process_front) on the device: the graphs and tree pins of arrival_order_cases.GPU_CASES, which
tests/test_arrival_order_cpu.py proves to contain a child due in a middle block, one due in a partial last block, two due
at the same block, a front with three or more distinct due values and a front whose children are all due at 0 -- and
intel once.

f64 against the oracle, at the tolerances of tests/test_gpu_parity.py for the same quantities (quoted where they are used),
with the arrival order (the default) AND with RR_PGO_ARRIVAL_ORDER=0 -- the two are never compared with each other; between
launch forms of one handle (the level schedule RR_PGO_LDS_FLOW=0, one workgroup drawing every ticket RR_PGO_LDS_FLOW_GRID=1)
byte for byte; the factor queries against marginals_reference at its own tolerance.  f32 and mixed handles keep the
elimination order whatever the switch says: that is what is asserted of them.  One oracle run per graph serves every test."""
import numpy as np
import pytest

from arrival_order_cases import GPU_CASES, INTEL, TREES, arrays_of, case_id, is_file
from conftest import g2o_path
from marginals_reference import MarginalsReference, rel_diff, tolerance
from covariances_cases import FLOOR_MAX

pytestmark = pytest.mark.gpu

ORDERS = [{}, {"RR_PGO_ARRIVAL_ORDER": "0"}]
ORDER_IDS = ["arrival", "elimination"]
FILE_ITERS = 100      # test_gauss_newton_trajectory_matches_oracle
RANDOM_ITERS = 5      # test_random_ragged_graphs_match_the_oracle (SE(3): 4, test_random_se3_graphs_match_the_oracle)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


def make(api, monkeypatch, case, env=None, **kw):
    """a handle of the case's graph, created under the case's pins and `env`"""
    graph, pins = case
    every = {**pins, **(env or {})}
    for k, v in every.items():
        monkeypatch.setenv(k, v)
    try:
        if is_file(graph):
            return api[0].new(g2o_path(graph), **kw)
        return api[0].from_arrays(*arrays_of(graph), **kw)
    finally:
        for k in every:
            monkeypatch.delenv(k)


def se3(graph):
    return (not is_file(graph)) and bool(np.any(np.asarray(arrays_of(graph)[0]) == 2))


def iters(graph):
    return FILE_ITERS if is_file(graph) else 4 if se3(graph) else RANDOM_ITERS


_ORACLE = {}


def oracle_of(graph):
    """first step, Gauss-Newton trajectory (errors, norms, final state) and marginals reference of the graph: computed once"""
    if graph not in _ORACLE:
        from oracle.oracle import OracleGraph
        fresh = (lambda: OracleGraph.load(g2o_path(graph))) if is_file(graph) else (lambda: OracleGraph.from_arrays(*arrays_of(graph)))
        o = fresh()
        dx = o.linearize_and_solve()
        errors, norms = o.optimize(iters(graph), return_norms=True)
        _ORACLE[graph] = dict(system=fresh(), dx=dx, errors=np.array(errors), norms=np.array(norms), state=np.array(o.state()),
                              marg=None, fresh=fresh)
    return _ORACLE[graph]


def marginals_of(graph):
    d = oracle_of(graph)
    if d["marg"] is None:
        d["marg"] = MarginalsReference(d["fresh"]())
    return d["marg"]


def check_f64_against_the_oracle(g, graph, label):
    d = oracle_of(graph)
    if not se3(graph):
        # H and b: 1e-12 / 1e-11 relative (test_assembled_system_matches_oracle)
        from test_gpu_parity import _assert_system_matches_oracle
        for lm in (False, True):
            _assert_system_matches_oracle(g, d["system"], graph, lm, 1e-12, 1e-11)
    dx = g.linearize_and_solve()
    step = np.abs(dx - d["dx"]).max() / max(1.0, np.abs(d["dx"]).max())
    eg, ng = g.optimize(iters(graph), return_norms=True)
    eg, ng = np.array(eg), np.array(ng)
    assert len(eg) == len(d["errors"]), (label, len(eg), len(d["errors"]))
    traj = np.max(np.abs(eg - d["errors"]) / np.abs(d["errors"]))
    pose = np.abs(np.array(g.state()) - d["state"]).max()
    print(f"{label}: first step {step:.3g}, chi2 trajectory {traj:.3g} relative over {len(eg) - 1} iterations, final poses {pose:.3g}")
    if se3(graph):          # test_random_se3_graphs_match_the_oracle
        assert step <= 1e-7
        np.testing.assert_allclose(eg, d["errors"], rtol=1e-7)
    elif is_file(graph):    # test_first_step_matches_oracle, test_gauss_newton_trajectory_matches_oracle
        assert step <= 1e-8
        np.testing.assert_allclose(eg, d["errors"], rtol=1e-7)
        assert abs(eg[-1] - d["errors"][-1]) <= 1e-9 * d["errors"][-1]
        np.testing.assert_allclose(ng, d["norms"], rtol=1e-4, atol=1e-8)
        assert pose <= 1e-8
    else:                   # test_random_ragged_graphs_match_the_oracle
        assert step <= 1e-8
        np.testing.assert_allclose(eg, d["errors"], rtol=1e-8)
        assert pose <= 1e-7


@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_f64_system_first_step_and_trajectory_match_the_oracle(api, monkeypatch, case, order):
    g = make(api, monkeypatch, case, order)
    assert g.stats()["n_big_fronts"] == 0
    check_f64_against_the_oracle(g, case[0], f"{case_id(case)} {order or 'default'}")


@pytest.mark.parametrize("precision", ["mixed", "f32"])
@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_an_fp32_factor_keeps_the_elimination_order(api, monkeypatch, case, precision):
    """f32 and mixed handles never get the new order (pgo_api.hip, analyze_handle; the fp32 kernels have no mid-panel add): with
    the switch at 1 and at 0 errors, norms and state agree byte for byte -- their results are those of the parent commit, which
    the existing fp32 tests hold against the oracle.  Both handles take the same path today: this is a guard against someone
    enabling the new order for fp32 factors later, not a check of the code this file is about."""
    runs = []
    for v in ("1", "0"):
        g = make(api, monkeypatch, case, {"RR_PGO_ARRIVAL_ORDER": v}, precision=precision)
        e, n = g.optimize(6, return_norms=True)
        runs.append((np.array(e), np.array(n), np.array(g.state())))
    for x, y in zip(*runs):
        assert np.array_equal(x, y), (case_id(case), precision)


@pytest.mark.parametrize("case", GPU_CASES + [INTEL], ids=case_id)
def test_launch_forms_agree_byte_for_byte(api, monkeypatch, case):
    """the dataflow launch against the level schedule (the same due blocks, no waits) and against one workgroup drawing every
    ticket: errors, norms and state; and the handle's tree is the one tests/test_arrival_order_cpu.py inspected"""
    ref = make(api, monkeypatch, case)
    st = ref.stats()
    assert (st["n_supernodes"], st["max_front"], st["max_pivot_cols"]) == TREES[case_id(case)], case_id(case)
    eref, nref = ref.optimize(4, return_norms=True)
    sref = np.array(ref.state())
    for env in ({"RR_PGO_LDS_FLOW": "0"}, {"RR_PGO_LDS_FLOW_GRID": "1"}):
        alt = make(api, monkeypatch, case, env)
        e, n = alt.optimize(4, return_norms=True)
        assert np.array_equal(np.array(e), np.array(eref)), (case_id(case), env)
        assert np.array_equal(np.array(n), np.array(nref)), (case_id(case), env)
        assert np.array_equal(np.array(alt.state()), sref), (case_id(case), env)
    lvl = make(api, monkeypatch, case, {"RR_PGO_LDS_FLOW": "0"}).stats()
    assert lvl["n_launches_per_iter"] > st["n_launches_per_iter"]   # (the level schedule really is another launch form)


@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_factor_queries_read_the_reordered_factor(api, monkeypatch, case, order):
    """rr_pgo_marginals and rr_pgo_covariances of a handful of nodes and pairs at the initial state, against
    marginals_reference at max(1e-12, 100 x its noise floor)"""
    graph = case[0]
    ref = marginals_of(graph)
    g = make(api, monkeypatch, case, order)
    n = g.num_nodes
    nodes = sorted(int(v) for v in np.random.default_rng(11).choice(n, min(n, 6), replace=False))
    a, b = np.repeat(nodes, len(nodes)).astype(np.int32), np.tile(nodes, len(nodes)).astype(np.int32)
    label = f"{case_id(case)} {order or 'default'}"
    got = g.marginals(np.array(nodes, np.int32))
    want, floor = ref.blocks(nodes)
    worst = max(rel_diff(x, y) for x, y in zip(got, want))
    print(f"{label} marginals of {len(nodes)} nodes: worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tolerance(floor):.3g}")
    assert floor <= FLOOR_MAX and worst <= tolerance(floor)
    vals, off = g.covariance_blocks(a, b)
    want, floor = ref.blocks(a, b)
    got = [vals[off[q]:off[q + 1]].reshape(w.shape) for q, w in enumerate(want)]
    worst = max(rel_diff(x, y) for x, y in zip(got, want))
    print(f"{label} covariances of {len(a)} pairs: worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tolerance(floor):.3g}")
    assert floor <= FLOOR_MAX and worst <= tolerance(floor)


@pytest.mark.parametrize("order", ORDERS, ids=ORDER_IDS)
def test_intel_once(api, monkeypatch, order):
    g = make(api, monkeypatch, INTEL, order)
    assert g.stats()["n_big_fronts"] == 0
    check_f64_against_the_oracle(g, INTEL[0], f"{case_id(INTEL)} {order or 'default'}")
