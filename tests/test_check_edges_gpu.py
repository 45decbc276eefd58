"""rr_pgo_check_edges on the MI355X against the CPU reference (tests/check_edges_reference.py) on the fixtures of
tests/check_edges_cases.py.

A GPU value passes when its difference to the reference is at most max(1e-12, 100 x noise floor), the floor being the worst
difference between the reference's two independent computations of the same quantity (relative for d2, R and chi2, absolute
for the redundancy r); every floor must be at most FLOOR_MAX = 1e-6.  d2, R and chi2 are compared on every queried edge whose
reference redundancy is at least 0.01, r on every edge.  The one exception is d2 of an edge whose smallest directional redundancy
is zero within the reference's own tolerance (R singular to rounding in a direction: only the PARTIAL fixtures have such edges).
Every comparison prints its worst figures before it asserts."""
import ctypes as C
import re

import numpy as np
import pytest

from check_edges_cases import BRIDGE_ONLY, DATASET_EDGES, PARTIAL, ROBUST, SMALL, at_state, reference, robust_mask, seeded_edges
from check_edges_reference import MIN_REDUNDANCY, CheckReference
from conftest import g2o_path
from covariances_cases import FLOOR_MAX
from gate_cases import GATE_GRAPHS, INFO_LEN, MEAS_LEN, info_matrix, split_packed
from gate_reference import GateReference
from marginals_reference import rel_diff
from query_small_cases import STATES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


_CASES = {}


def same(x, y):
    """two results of check_edges(return_residual=True), bit for bit (NaN equals NaN)"""
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in ("d2", "redundancy", "chi2")) and len(x["R"]) == len(y["R"]) and \
        all(np.array_equal(a, b) for a, b in zip(x["R"], y["R"]))


def pick(res, idx):
    return {"d2": res["d2"][idx], "redundancy": res["redundancy"][idx], "chi2": res["chi2"][idx], "R": [res["R"][i] for i in idx]}


def dataset(api, name):
    """the handle at the state of GATE_GRAPHS, the queried edges and one full call (made once per graph)"""
    if name not in _CASES:
        g = api[0].new(g2o_path(name))
        if GATE_GRAPHS[name]:
            g.optimize(GATE_GRAPHS[name])
        arrays, state = g.graph_arrays(), g.state()
        edges = seeded_edges(arrays, DATASET_EDGES.get(name, 64))
        got = g.check_edges(edges, return_residual=True)
        t = g.check_edges_times()
        print(f"{name}: {len(got['d2'])} edges: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, kernel + copy {t[2]:.3f} ms")
        _CASES[name] = dict(g=g, arrays=arrays, state=state, edges=edges, got=got)
    return _CASES[name]


# ---- 1. against the reference
@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("name", SMALL)
def test_small_graphs_match_the_reference(api, name, which):
    arrays, state = at_state(name, which)
    g = api[0].from_arrays(*arrays)
    got = g.check_edges(return_residual=True)
    ref = reference((name, which), arrays, state)
    print(ref.summary(f"{name} {which}"))
    ref.check(f"{name} {which}", got)
    assert all(np.array_equal(R, R.T) for R in got["R"])
    assert np.array_equal(got["chi2"], g.edge_errors()[0])   # every edge, bridges included
    if name in BRIDGE_ONLY:
        assert np.all(np.abs(got["redundancy"]) <= ref.tol_r)
    # edges=None is the explicit full list; without R and without the optional outputs the same bits
    full = g.check_edges(np.arange(g.num_edges), return_residual=True)
    assert same(full, got)
    plain = g.check_edges()
    assert all(np.array_equal(plain[k], got[k], equal_nan=True) for k in ("d2", "redundancy", "chi2"))


@pytest.mark.parametrize("name", list(DATASET_EDGES))
def test_datasets_match_the_reference(api, name):
    c = dataset(api, name)
    ref = reference((name, "gpu state"), c["arrays"], c["state"], c["edges"])
    print(ref.summary(name))
    ref.check(name, c["got"])
    assert 2 * int(np.sum(ref.compared)) >= ref.n
    assert all(np.array_equal(R, R.T) for R in c["got"]["R"])
    s = c["g"].edge_errors()[0]
    assert np.array_equal(c["got"]["chi2"], s if c["edges"] is None else s[c["edges"]])


# ---- 2. bits
@pytest.mark.parametrize("name", ["intel", "parking-garage", "simulation-pose-landmark"])
def test_bits_do_not_depend_on_the_rest_of_the_call(api, name):
    c = dataset(api, name)
    g, got = c["g"], c["got"]
    edges = np.arange(g.num_edges, dtype=np.int32) if c["edges"] is None else c["edges"]
    assert same(g.check_edges(edges, return_residual=True), got)          # the same call twice; None is the full list
    step = 1 if c["edges"] is not None else 9   # every edge of the 64- and 32-edge lists; every 9th of all 297 edges
    for q in range(0, len(edges), step):                                    # one at a time
        assert same(g.check_edges(edges[q:q + 1], return_residual=True), pick(got, [q])), q
    rng = np.random.default_rng(3)
    idx = np.concatenate([rng.permutation(len(edges)), rng.integers(0, len(edges), 9), [0, 0]])   # permuted, with repeats
    assert same(g.check_edges(edges[idx], return_residual=True), pick(got, idx))


def test_a_plan_cut_by_the_workspace_bound_gives_the_same_bits(api, monkeypatch):
    """24 edges of intel with distinct `to` nodes (at least 3 chunks of columns).  A handle whose workspace bound
    (RR_PGO_TS_WS_BYTES) is the largest need of a single edge must cut the list; the cut changes no bit."""
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]
    et = dataset(api, "intel")["arrays"][4]
    edges, seen = [], set()
    for k in np.random.default_rng(5).permutation(len(et)):
        if int(et[k]) not in seen and len(edges) < 24:
            seen.add(int(et[k]))
            edges.append(int(k))
    edges = np.array(edges, np.int32)

    def handle(bound=None):
        if bound is None:
            return PoseGraph.new(g2o_path("intel"))
        monkeypatch.setenv("RR_PGO_TS_WS_BYTES", str(bound))
        g = PoseGraph.new(g2o_path("intel"))
        monkeypatch.delenv("RR_PGO_TS_WS_BYTES")
        return g

    def refused(g, q):
        with pytest.raises(PoseGraphError) as ei:
            g.check_edges(edges[q:q + 1], return_residual=True)
        assert ei.value.code == _lib.ENOMEM, ei.value
        m = re.fullmatch(r"rr_pgo_check_edges: one edge needs (\d+) bytes of workspace", _lib.load().rr_pgo_last_error().decode())
        assert m
        return int(m.group(1))

    want = handle().check_edges(edges, return_residual=True)
    B = handle(1)
    need = [refused(B, q) for q in range(24)]
    print(f"intel, 24 edges alone: workspace needs {min(need)} .. {max(need)} bytes")
    C_ = handle(max(need))
    assert same(C_.check_edges(edges, return_residual=True), want)
    D = handle(max(need) - 1)
    assert refused(D, int(np.argmax(need))) == max(need)


# ---- 3. settings
@pytest.mark.parametrize("name", ROBUST)
def test_cauchy_weight_enters_the_residual_covariance_and_chi2_stays_unweighted(api, name):
    """Cauchy, delta 1, on two edges of three, at the moved state (no error at rounding level there).  The floors are those of
    the reference's two Sigmas alone, as everywhere."""
    arrays, state = at_state(name, "moved")
    g = api[0].from_arrays(*arrays)
    plain = g.check_edges(return_residual=True)
    mask = robust_mask(g.num_edges)
    g.set_robust_kernel("cauchy", 1.0, mask)
    got = g.check_edges(return_residual=True)
    s, w = g.edge_errors()
    assert np.min(w) < 0.5 and np.all(w[mask == 0] == 1.0)
    ref = reference((name, "moved", "cauchy"), arrays, state, kind="cauchy", delta=1.0, mask=mask)
    print(ref.summary(f"{name} moved, cauchy delta 1, masked"))
    ref.check(f"{name} moved, cauchy delta 1, masked", got)
    assert np.array_equal(got["chi2"], s) and np.array_equal(got["chi2"], plain["chi2"])
    c = np.flatnonzero(ref.compared)
    change = float(np.nanmax(np.abs(got["d2"][c] - plain["d2"][c]) / np.abs(plain["d2"][c])))
    print(f"d2 differs from the unweighted call by up to {change:.3g} relative")
    assert change > 1e-3
    # the weight is what the reference says: R of a masked-in edge against R of the unweighted call differs, w Omega scales r
    q = int(np.argmin(w))
    assert not np.array_equal(got["R"][q], plain["R"][q])


@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("name", PARTIAL)
def test_partial_redundancy_is_reported_and_never_a_suspect(api, name, which):
    """Graphs with edges at r = 0.05 .. 0.41 whose R is singular to rounding in one direction.  r, R and the smallest
    directional redundancy follow the reference on every compared edge; d2 is compared on the edges the reference does not flag
    as singular and may be finite or NaN on exactly the flagged ones; suspect_edges names none of them."""
    arrays, state = at_state(name, which)
    g = api[0].from_arrays(*arrays)
    got = g.check_edges(return_residual=True)
    ref = reference((name, which), arrays, state)
    print(ref.summary(f"{name} {which}"))
    assert np.any(ref.singular)
    ref.check(f"{name} {which}", got)
    flagged = np.flatnonzero(ref.singular)
    print(f"{name} {which}: singular edges {flagged.tolist()}: r {np.round(got['redundancy'][flagged], 3).tolist()}, "
          f"smallest directional redundancy {got['redundancy_min'][flagged].tolist()}, d2 {got['d2'][flagged].tolist()}")
    assert np.all(np.abs(got["redundancy_min"][flagged]) <= ref.tol_rmin) and np.all(got["redundancy"][flagged] >= MIN_REDUNDANCY)
    assert np.all(np.isfinite(got["d2"][ref.compared & ~ref.singular]))
    assert np.array_equal(got["chi2"], g.edge_errors()[0])
    suspects = g.suspect_edges()
    assert not set(suspects.tolist()) & set(flagged.tolist())
    # with the caller's parameters below 0 they come back wherever rounding left a finite d2 (1e13 and up): the default keeps them out
    loose = g.suspect_edges(min_redundancy=-1.0, min_directional=-1.0)
    huge = flagged[np.isfinite(got["d2"][flagged]) & (got["d2"][flagged] > 7.815)]
    assert set(huge.tolist()) <= set(loose.tolist()) and set(suspects.tolist()) <= set(loose.tolist())


@pytest.mark.parametrize("keep_anchor", [True, False])
def test_priors_and_the_dropped_anchor_are_part_of_the_inverted_matrix(api, keep_anchor):
    from priors_reference import PriorsReference, random_priors
    arrays, state = at_state("mid-se2", "moved")
    g = api[0].from_arrays(*arrays)
    node, meas, info = random_priors(np.random.default_rng(8), arrays, [0, 17, 250, 430])
    g.set_priors(node, meas, info, keep_anchor=keep_anchor)
    got = g.check_edges(return_residual=True)
    sig = PriorsReference(arrays, node, meas, info, keep_anchor=keep_anchor).sigma_pair()
    ref = CheckReference(arrays, state, sig=sig)
    ref.check(f"mid-se2 with 4 priors, keep_anchor {keep_anchor}", got)
    before = reference(("mid-se2", "moved"), arrays, state)
    assert float(np.max(np.abs(ref.r - before.r))) > 1e-3    # the priors matter


def test_fixed_endpoints_drop_out(api):
    from fixed_reference import FixedReference
    arrays, state = at_state("se2-5", "moved")
    ek, ef, et = arrays[2], arrays[3], arrays[4]
    pose_edges = np.flatnonzero(ek == 0)
    one, both = int(pose_edges[1]), int(pose_edges[len(pose_edges) // 2])
    fixed = sorted({int(ef[one]), int(ef[both]), int(et[both])})
    g = api[0].from_arrays(*arrays)
    g.set_fixed(fixed)
    got = g.check_edges(return_residual=True)
    ref = CheckReference(arrays, state, sig=FixedReference(arrays, fixed).sigma_pair())
    ref.check(f"se2-5 with fixed nodes {fixed}", got)
    # both endpoints fixed: P = 0, r = 1 and d2 = e^T Omega e (no kernel: w = 1)
    W = info_matrix(0, split_packed(ek, arrays[6], INFO_LEN)[both])
    print(f"edge {both}, both endpoints fixed: r - 1 = {got['redundancy'][both] - 1.0:.3g}, d2 / chi2 - 1 = {got['d2'][both] / got['chi2'][both] - 1.0:.3g}")
    assert abs(got["redundancy"][both] - 1.0) <= 1e-12 and abs(got["d2"][both] / got["chi2"][both] - 1.0) <= 1e-12
    assert rel_diff(got["R"][both], np.linalg.inv(W)) <= 1e-12


# ---- 4. against the gate: the identity at one linearisation point
def test_leave_one_out_distance_is_the_gate_of_the_graph_without_the_edge(api):
    """For eight edges of simulation-pose-pose, none the first pose-pose edge: a handle on the graph without the edge
    (remove_edges), at the same state, gates the edge as a candidate.  S_without = Omega^-1 R^-1 Omega^-1 (Woodbury), so
    Omega^-1 S^-1 Omega^-1 is R and e^T Omega S Omega e is d2, at the larger of the two references' tolerances."""
    name = "simulation-pose-pose"
    c = dataset(api, name)
    arrays, state, edges = c["arrays"], c["state"], c["edges"]
    g = api[0].from_arrays(*arrays)
    g.set_state(state)   # (as the handles below: all of them hold the same bits)
    got = g.check_edges(edges, return_residual=True)
    ref = reference((name, "gpu state"), arrays, state, edges)
    nk, _, ek, ef, et, em, ei = arrays
    meas, info = split_packed(ek, em, MEAS_LEN), split_packed(ek, ei, INFO_LEN)
    first = int(np.flatnonzero(ek != 1)[0])
    qs = [q for q in range(len(edges)) if ref.compared[q] and int(edges[q]) != first][:8]
    assert len(qs) == 8
    for q in qs:
        k = int(edges[q])
        h = api[0].from_arrays(*arrays)
        h.set_state(state)
        h.remove_edges([k])
        assert h.num_edges == len(ek) - 1 and np.array_equal(h.state(), g.state())
        cand = (ek[k:k + 1], ef[k:k + 1], et[k:k + 1], meas[k], info[k])
        d2g, _, S = h.gate_edges(*cand, return_innovation=True)
        gref = GateReference(h.graph_arrays(), state, cand)
        assert gref.floor <= FLOOR_MAX
        Wi = np.linalg.inv(ref.omega[q])
        e = ref.lin[q][2]
        R_gate = Wi @ np.linalg.inv(S[0]) @ Wi
        d2_gate = float(e @ ref.omega[q] @ S[0] @ ref.omega[q] @ e)
        tol_R, tol_d2 = max(ref.tol_R, gref.tol_S), max(ref.tol_d2, gref.tol_d2)
        dR, dd = rel_diff(R_gate, got["R"][q]), abs(d2_gate - got["d2"][q]) / got["d2"][q]
        print(f"edge {k}: r {got['redundancy'][q]:.3g}, d2 {got['d2'][q]:.6g}; R from the gate differs by {dR:.3g} (tolerance {tol_R:.3g}), "
              f"d2 by {dd:.3g} (tolerance {tol_d2:.3g})")
        assert dR <= tol_R and dd <= tol_d2, k


def test_an_accepted_false_closure_is_the_first_suspect_and_can_be_taken_out(api):
    """simulation-pose-pose with one false closure (the measurement of nowhere, between two far poses), optimised: the
    optimiser smears it over its neighbours, suspect_edges names it first, and without it the cost is the clean graph's."""
    g = api[0].new(g2o_path("simulation-pose-pose"))
    clean = g.optimize(10)[-1]
    arrays = g.graph_arrays()
    w = split_packed(arrays[2], arrays[6], INFO_LEN)[0]
    n, e = g.num_nodes, g.num_edges
    g.extend([0], [10], [n // 2], [25.0, -25.0, 2.0], w)
    bad = g.optimize(10)[-1]
    suspects = g.suspect_edges()
    c = g.check_edges()
    print(f"chi2 clean {clean:.6g}, with the false closure {bad:.6g}; {len(suspects)} suspects, the first is edge {suspects[0]} "
          f"(d2 {c['d2'][suspects[0]]:.6g}, r {c['redundancy'][suspects[0]]:.3g}, chi2 {c['chi2'][suspects[0]]:.6g})")
    cr = g.check_edges([e], return_residual=True)
    print(f"the false closure: smallest directional redundancy {cr['redundancy_min'][0]:.3g}")
    assert bad > clean and suspects[0] == e and c["redundancy"][e] >= 0.01 and c["d2"][e] > c["chi2"][e]
    assert np.all(np.diff(c["d2"][suspects]) <= 0)
    assert list(g.suspect_edges(edges=[e, 0, 1]))[0] == e and g.suspect_edges(threshold=1e300).size == 0
    g.remove_edges([e])
    after = g.optimize(10)[-1]
    print(f"chi2 after the removal and ten iterations {after:.6g}")
    assert g.num_edges == e and after < bad and abs(after - clean) <= 1e-3 * clean   # (the stop rule |dx| < 1e-4 leaves chi2 far inside)


# ---- 5. untouched
@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
def test_optimize_after_the_check_gives_the_same_bits(api, solver):
    PoseGraph, Solver = api
    edges = dataset(api, "intel")["edges"]
    a = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    b = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    s0 = a.state()
    got = a.check_edges(edges, return_residual=True)
    assert same(got, dataset(api, "intel")["got"])   # (the solver of the handle plays no part)
    assert np.array_equal(a.state(), s0)
    ea, na = a.optimize(10, return_norms=True)
    eb, nb = b.optimize(10, return_norms=True)
    assert np.array_equal(np.array(ea), np.array(eb)) and np.array_equal(np.array(na), np.array(nb))
    a.check_edges(edges[:5])   # ... and between two optimize calls (Levenberg-Marquardt: lambda is carried)
    assert np.array_equal(a.state(), b.state())
    assert np.array_equal(np.array(a.optimize(3)), np.array(b.optimize(3)))
    assert np.array_equal(a.state(), b.state())


def test_replayed_graph_iterations_after_the_check_give_the_same_bits(api, monkeypatch):
    edges = dataset(api, "intel")["edges"]
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    a = api[0].new(g2o_path("intel"))
    b = api[0].new(g2o_path("intel"))
    monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    a.iterate_async(2)
    b.iterate_async(2)
    a.sync()
    b.sync()
    a.check_edges(edges[:3])
    a.iterate_async(8)
    b.iterate_async(8)
    a.sync()
    b.sync()
    assert np.array_equal(a.state(), b.state())
    for g in (a, b):   # every one of the ten iterations was a replay of the one captured graph
        st = g.stats()
        assert (st["n_graph_replays"], st["n_graph_captures"], st["n_plain_iterations"]) == (10, 1, 0)


# ---- 6. refusals
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
            h.check_edges([0, 1])
        assert ei.value.code == _lib.EUNSUPPORTED, (what, ei.value)
        msg = _lib.load().rr_pgo_last_error().decode()
        print(what, "->", msg)
        assert "rr_pgo_check_edges" in msg and word in msg, (what, msg)


def test_bad_arguments_are_refused_before_anything_is_written(api):
    from rustrobotics_amd import _lib
    L = _lib.load()
    c = dataset(api, "simulation-pose-landmark")
    g, E = c["g"], c["g"].num_edges
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def call(n, edge, d2=True):
        out = [np.full(max(E, 4), -777.0) for _ in range(3)]
        resid, off = np.full(36 * max(E, 4), -777.0), np.full(max(E, 4) + 1, -777, np.int64)
        e = None if edge is None else np.array(edge, np.int32)
        rc = L.rr_pgo_check_edges(g._h, n, None if e is None else e.ctypes.data_as(ip), out[0].ctypes.data_as(dp) if d2 else None,
                                  out[1].ctypes.data_as(dp), out[2].ctypes.data_as(dp), resid.ctypes.data_as(dp), off.ctypes.data_as(lp))
        msg = L.rr_pgo_last_error().decode()
        if rc != 0:   # a refusal writes nothing
            assert all(np.all(o == -777.0) for o in out) and np.all(resid == -777.0) and np.all(off == -777)
        return rc, msg

    bad = {"n_query < 0": (-1, [0]), "null d2_out": (2, [0, 1], False), "edge NULL with another count": (E - 1, None),
           "index below range": (2, [0, -1]), "index beyond range": (2, [0, E])}
    for what, args in bad.items():
        rc, msg = call(*args)
        print(what, "->", msg)
        assert rc == _lib.EINVAL and "rr_pgo_check_edges" in msg, (what, rc, msg)
    assert call(0, None)[0] == 0 and call(0, [0])[0] == 0     # n_query == 0 is fine, with or without a list
    assert L.rr_pgo_check_edges(g._h, 0, None, None, None, None, None, None) == 0
    # ... and the handle still answers: d2 alone
    d2 = np.zeros(E)
    assert L.rr_pgo_check_edges(g._h, E, None, d2.ctypes.data_as(dp), None, None, None, None) == 0
    assert np.array_equal(d2, c["got"]["d2"], equal_nan=True)
