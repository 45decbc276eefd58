"""rr_pgo_extend without a GPU: the exports are declared everywhere they have to be; the graphs of tests/extend_cases.py
are usable (connected, anchored, the oracle optimises them); the CPU reference of the initial guess
(tests/extend_reference.py) is validated with the unchanged oracle; the step planner; the --extend and --gate --accept
parsers of the command line."""
import os
import re

import numpy as np
import pytest

import extend_reference as ref
from conftest import ROOT
from extend_cases import K_EDGES, M_NODES, SOURCES, case, closures_only, connected, source_arrays
from oracle.oracle import OracleGraph


def test_extend_exports_are_declared_in_header_mirror_and_integration_guide():
    from rustrobotics_amd import PoseGraph, _lib
    header = open(os.path.join(ROOT, "include", "rr_pgo.h")).read()
    assert re.search(r"\bint\s+rr_pgo_extend\s*\(\s*rr_pgo\s*\*h\s*,\s*int32_t\s+n_new_nodes", header)
    assert re.search(r"\bint\s+rr_pgo_extend_times\s*\(\s*const\s+rr_pgo\s*\*h", header)
    assert "#define RR_PGO_ABI_VERSION 4" in header   # new exports only
    assert "rr_pgo_extend" in _lib.EXPORTS and "rr_pgo_extend_times" in _lib.EXPORTS
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn rr_pgo_extend(" in integration and "fn rr_pgo_extend_times(" in integration and "pub fn extend(" in integration
    assert callable(PoseGraph.extend) and callable(PoseGraph.extend_times)


# ---- the cases
@pytest.mark.parametrize("name", SOURCES)
def test_base_graph_is_connected_anchored_and_both_graphs_optimise(name):
    c = case(name)
    n = len(c.grown[0])
    # the last six nodes go, and with them the nodes only they hold in the graph (landmarks of the pose-landmark file alone)
    assert c.n_base == n - len(c.addition[5]) and len(c.addition[5]) >= M_NODES
    assert len(c.addition[5]) == M_NODES or name == "simulation-pose-landmark"
    assert np.array_equal(c.grown[0][-M_NODES:], source_arrays(name)[0][-M_NODES:]) and np.all(c.addition[5][:-M_NODES] == 1)
    touching = int(np.sum((c.grown[3] >= c.n_base) | (c.grown[4] >= c.n_base)))
    assert len(c.addition[0]) == touching + K_EDGES and c.e_base + len(c.addition[0]) == len(c.grown[2])
    # what was removed is what is added: the closures between old nodes, then / among them every edge of a removed node
    ek, ef, et = c.addition[:3]
    old_old = (ef < c.n_base) & (et < c.n_base)
    assert int(np.sum(old_old)) == K_EDGES and np.all(np.abs(ef[old_old] - et[old_old]) > 1)
    assert connected(c.base) and connected(c.grown)
    assert np.any(c.base[2] != 1)   # a pose-pose edge: the base graph has its anchor
    for arrays in (c.base, c.grown):
        errors = OracleGraph.from_arrays(*arrays).optimize(10)   # (raises on a failed factorisation)
        assert len(errors) >= 2 and np.all(np.isfinite(errors)) and errors[-1] <= errors[0]


def test_closures_only_case_of_the_graph_with_fronts_beyond_lds():
    c = closures_only("sphere2500", 3)
    assert c.n_base == len(c.grown[0]) and len(c.addition[0]) == 3 and len(c.addition[5]) == 0
    assert connected(c.base)


# ---- the reference of the guess, validated with the oracle: a node guessed from one edge leaves the edge without error
NODE_OF = {0: (0, 0), 1: (0, 1), 2: (2, 2)}   # edge kind -> kinds of (from, to)
IDENT = {0: [0.0, 0.0, 0.0], 1: [0.0, 0.0], 2: [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]}


def random_case(kind, rng):
    """(state of from, state of to [to be replaced], measurement, packed information)"""
    def pose(k):
        if k == 0:
            return np.concatenate([rng.uniform(-50, 50, 2), [rng.uniform(-3.1, 3.1)]])
        if k == 1:
            return rng.uniform(-50, 50, 2)
        q = rng.standard_normal(4)
        return np.concatenate([rng.uniform(-50, 50, 3), q / np.linalg.norm(q)])
    d = {0: 3, 1: 2, 2: 6}[kind]
    A = rng.standard_normal((d, d))
    W = A @ A.T + d * np.eye(d)
    W *= 10.0 ** rng.uniform(0, 4)
    z = pose({0: 0, 1: 1, 2: 2}[kind])
    if kind != 1:
        z[:len(z) - (1 if kind == 0 else 4)] *= 0.1   # a step of a few metres
    return pose(NODE_OF[kind][0]), pose(NODE_OF[kind][1]), z, W[np.triu_indices(d)]


@pytest.mark.parametrize("kind,inverse", [(0, False), (0, True), (1, False), (2, False), (2, True)])
def test_compose_leaves_the_edge_without_error(kind, inverse):
    """chi2 of the two-node, one-edge graph <= 1e-20 * max|Omega|: rounding gives e ~ 1e-14 at most, so e^T Omega e ~ 1e-28
    |Omega|; the bound leaves eight orders of margin.  (A landmark edge has one direction only.)"""
    rng = np.random.default_rng(100 + 10 * kind + int(inverse))
    worst = 0.0
    for _ in range(50):
        a, b, z, w = random_case(kind, rng)
        if inverse:
            a = ref.compose(kind, b, z, inverse=True)
        else:
            b = ref.compose(kind, a, z)
        o = OracleGraph.from_arrays(list(NODE_OF[kind]), np.concatenate([a, b]), [kind], [0], [1], z, w)
        chi2 = o.global_error()
        worst = max(worst, chi2 / np.max(np.abs(w)))
        assert chi2 <= 1e-20 * np.max(np.abs(w)), (kind, inverse, chi2, np.max(np.abs(w)))
    print(f"kind {kind} inverse {inverse}: worst chi2 / max|Omega| {worst:.3g}")


def test_compose_refuses_a_pose_from_a_landmark():
    with pytest.raises(ValueError):
        ref.compose(1, [1.0, 2.0], [0.5, 0.5], inverse=True)


# ---- the planner
def test_plan_chain_in_list_order():
    # old nodes 0..2; new 3, 4, 5 chained 2 -> 3 -> 4 -> 5, edges given out of order: two scans
    steps, lost = ref.plan(3, 3, [0, 0, 0], [4, 2, 3], [5, 3, 4])
    assert lost == [] and steps == [(1, 2, 3, False), (2, 3, 4, False), (0, 4, 5, False)]


def test_plan_backwards_step():
    # the edge goes FROM the new pose 3 TO the old pose 1
    steps, lost = ref.plan(3, 1, [0], [3], [1])
    assert lost == [] and steps == [(0, 1, 3, True)]
    steps, lost = ref.plan(3, 1, [2], [3], [1])
    assert lost == [] and steps == [(0, 1, 3, True)]


def test_plan_landmark_from_a_new_pose():
    # new pose 3 by odometry from 2, new landmark 4 seen from 3 (listed first: it waits for the second scan)
    steps, lost = ref.plan(3, 2, [1, 0], [3, 2], [4, 3])
    assert lost == [] and steps == [(1, 2, 3, False), (0, 3, 4, False)]


def test_plan_unreachable_node():
    # new nodes 3 and 4 joined to each other only
    steps, lost = ref.plan(3, 2, [0], [3], [4])
    assert steps == [] and lost == [3, 4]
    # an edge between two old nodes is no step
    steps, lost = ref.plan(3, 1, [0, 0], [0, 2], [2, 3])
    assert steps == [(1, 2, 3, False)] and lost == []


def test_plan_pose_that_only_a_landmark_edge_reaches_is_unreachable():
    # old landmark 1 (node kinds do not matter to the planner: the edge kind does), new pose 3 sees it
    steps, lost = ref.plan(3, 1, [1], [3], [1])
    assert steps == [] and lost == [3]


def test_guess_follows_the_plan():
    old_kind, old_state = [0, 0], [0.0, 0.0, 0.0, 1.0, 0.0, np.pi / 2]
    got = ref.guess(old_kind, old_state, [0, 1, 0], [0, 1, 0], [1, 2, 4], [2, 3, 0], [1.0, 0.0, 0.5, 2.0, 0.0, 1.0, 1.0, 0.25])
    np.testing.assert_allclose(got[0], [1.0, 1.0, np.pi / 2 + 0.5], atol=1e-15)
    np.testing.assert_allclose(got[1], got[0][:2] + ref.rot2(got[0][2]) @ [2.0, 0.0], atol=1e-15)
    # node 4 is the FROM of an edge to node 0 with z = (1, 1, 0.25): X_4 = X_0 Z^-1
    np.testing.assert_allclose(got[2], [-(np.cos(0.25) + np.sin(0.25)), np.sin(0.25) - np.cos(0.25), -0.25], atol=1e-15)


# ---- the command line's parsers
EXTEND_FILE = """# two poses, a landmark, odometry and a closure
VERTEX_SE2 100 1.0 2.0 0.5
EDGE_SE2 7 100 1.5 -0.25 0.125 44.7 0 0 44.7 0 30.9
EDGE_SE2 101 3 0.5 0.5 0.1 10 0 0 10 0 5
VERTEX_SE2 101 2.0 3.0 0.75
VERTEX_XY 102 4.0 5.0
EDGE_SE2_XY 101 102 0.5 2.0 10 1 20
EDGE_SE2 3 12 1 2 3 4 5 6 7 8 9
"""


def test_extend_file_parser(tmp_path):
    from rustrobotics_amd.__main__ import parse_extend_file
    index = {3: 0, 7: 1, 12: 2}
    p = tmp_path / "more.g2o"
    p.write_text(EXTEND_FILE)
    nkind, nid, nstate, kind, a, b, meas, info = parse_extend_file(str(p), index)
    assert nkind == [0, 0, 1] and nid == [100, 101, 102]
    assert nstate == [1.0, 2.0, 0.5, 2.0, 3.0, 0.75, 4.0, 5.0]
    assert kind == [0, 0, 1, 0] and a == [1, 4, 4, 0] and b == [3, 0, 5, 2]   # (an edge may precede its vertex line)
    assert meas == [1.5, -0.25, 0.125, 0.5, 0.5, 0.1, 0.5, 2.0, 1, 2, 3]
    assert info == [44.7, 0, 0, 44.7, 0, 30.9, 10, 0, 0, 10, 0, 5, 10, 1, 20, 4, 5, 6, 7, 8, 9]
    # a 3-D file
    q = tmp_path / "more3d.g2o"
    q.write_text("VERTEX_SE3:QUAT 50 1 2 3 0 0 0 1\nEDGE_SE3:QUAT 12 50 1 2 3 0 0 0 1 " + " ".join(str(float(v)) for v in range(1, 22)) + "\n")
    nkind, nid, nstate, kind, a, b, meas, info = parse_extend_file(str(q), index)
    assert nkind == [2] and nid == [50] and kind == [2] and a == [2] and b == [3] and len(meas) == 7 and len(info) == 21
    # an unknown tag, a duplicate id (of the graph, of the file), a short line, an unknown vertex: SystemExit naming the line
    for text, line, word in ((EXTEND_FILE.replace("VERTEX_XY", "VERTEX_XYZ"), 6, "VERTEX_XYZ"),
                             (EXTEND_FILE.replace("VERTEX_SE2 101", "VERTEX_SE2 7"), 5, "id 7"),
                             (EXTEND_FILE.replace("VERTEX_XY 102", "VERTEX_XY 100"), 6, "id 100"),
                             (EXTEND_FILE.replace("VERTEX_SE2 100 1.0 2.0 0.5", "VERTEX_SE2 100 1.0 2.0"), 2, "3 values"),
                             (EXTEND_FILE.replace("EDGE_SE2_XY 101 102 0.5 2.0 10 1 20", "EDGE_SE2_XY 101 102 0.5 2.0 10 1"), 7, "5 values"),
                             (EXTEND_FILE + "EDGE_SE2 3 99 0 0 0 1 0 0 1 0 1\n", 9, "99")):
        p.write_text(text)
        with pytest.raises(SystemExit) as ei:
            parse_extend_file(str(p), index)
        assert f"{p}:{line}:" in str(ei.value) and word in str(ei.value), str(ei.value)


def test_gate_accept_uses_the_gate_file_parser(tmp_path):
    """--gate FILE --accept reads FILE with parse_gate_file: good files parse, bad lines are named (the flag is --gate)"""
    from rustrobotics_amd.__main__ import main, parse_gate_file
    index = {3: 0, 7: 1, 12: 2}
    p = tmp_path / "cand.txt"
    good = "EDGE_SE2 3 7 1.5 -0.25 0.125 44.7 0 0 44.7 0 30.9\nEDGE_SE2_XY 7 12 0.5 2.0 10 1 20\n"
    p.write_text(good)
    kind, a, b, meas, info, ids = parse_gate_file(str(p), index)
    assert kind == [0, 1] and ids == [(3, 7), (7, 12)]
    for text, line, word in ((good.replace("EDGE_SE2_XY", "VERTEX_XY"), 2, "VERTEX_XY"),
                             (good + "EDGE_SE2 3 7 0 0 0 1 0 0 1 0\n", 3, "9 values"),
                             (good + "EDGE_SE2 3 99 0 0 0 1 0 0 1 0 1\n", 3, "99")):
        p.write_text(text)
        with pytest.raises(SystemExit) as ei:
            parse_gate_file(str(p), index)
        assert f"--gate: {p}:{line}:" in str(ei.value) and word in str(ei.value), str(ei.value)
    # the new flags need their partners (decided by the argument parser, before any device is touched)
    for argv in (["x.g2o", "--accept"], ["x.g2o", "--guess"]):
        with pytest.raises(SystemExit):
            main(argv)
