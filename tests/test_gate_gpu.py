"""rr_pgo_gate_edges on the MI355X against the CPU reference (tests/gate_reference.py) on the candidates of
tests/gate_cases.py.

A GPU value passes when its relative difference to the reference is at most max(1e-12, 100 x noise floor), the floor being
the worst relative difference between the reference's two independent computations of the same quantity; the floor itself
must be at most FLOOR_MAX = 1e-6.  Every comparison prints its worst figure, the floor and the tolerance before it asserts."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import g2o_path
from covariances_cases import FLOOR_MAX
from gate_cases import EDGE_DIM, GATE_GRAPHS, candidates, reverse, select, thresholds
from gate_reference import GateReference, check
from marginals_reference import rel_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


_CASES, _REFS = {}, {}


def case(api, name):
    """the handle at the state of GATE_GRAPHS, its candidates and one full call (made once per graph)"""
    if name not in _CASES:
        g = api[0].new(g2o_path(name))
        if GATE_GRAPHS[name]:
            g.optimize(GATE_GRAPHS[name])
        arrays, state = g.graph_arrays(), g.state()
        cand = candidates(arrays, state)
        d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
        t = g.gate_times()
        print(f"{name}: {len(d2)} candidates: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, gate kernel + copy {t[2]:.3f} ms")
        _CASES[name] = dict(g=g, arrays=arrays, state=state, cand=cand, d2=d2, chi2=chi2, S=S)
    return _CASES[name]


def reference(api, name):
    if name not in _REFS:
        c = case(api, name)
        _REFS[name] = GateReference(c["arrays"], c["state"], c["cand"])
        print(_REFS[name].summary(name))
    return _REFS[name]


def check_all(label, ref, d2, chi2, S):
    check(label, "d2", d2, ref.d2, ref.floor_d2, ref.tol_d2, FLOOR_MAX)
    check(label, "chi2", chi2, ref.chi2, ref.floor_chi2, ref.tol_chi2, FLOOR_MAX)
    check(label, "S", S, ref.S, ref.floor_S, ref.tol_S, FLOOR_MAX)


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_gate_matches_the_reference(api, name):
    c, ref = case(api, name), reference(api, name)
    check_all(name, ref, c["d2"], c["chi2"], c["S"])
    # ---- decisions at the default threshold; a candidate whose reference d2 lies within the tolerance of the threshold
    # is left out (at most one per graph; with these seeds the reference has none: tests/test_gate_cpu.py)
    g, cand = c["g"], c["cand"]
    mask = g.gate(*cand)
    assert mask.dtype == bool and np.array_equal(mask, c["d2"] <= thresholds(cand[0]))
    keep = ~ref.undecided
    print(f"{name}: {int(np.sum(mask))} accepted, {int(np.sum(~mask))} rejected, {int(np.sum(~keep))} left out of the comparison")
    assert np.sum(~keep) <= 1
    assert np.array_equal(mask[keep], ref.accept[keep])
    assert np.sum(mask) >= 5 and np.sum(~mask) >= 5
    # a scalar and a per-kind threshold
    assert np.array_equal(g.gate(*cand, threshold=1.0), c["d2"] <= 1.0)
    assert np.array_equal(g.gate(*cand, threshold={0: 1.0, 1: 2.0, 2: 3.0}), c["d2"] <= np.array([{0: 1.0, 1: 2.0, 2: 3.0}[int(k)] for k in cand[0]]))


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_innovation_covariances_are_symmetric_and_positive(api, name):
    c, ref = case(api, name), reference(api, name)
    worst_min, worst_p = np.inf, 0.0
    for k, S, W in zip(c["cand"][0], c["S"], ref.omega):
        assert S.shape == (EDGE_DIM[int(k)],) * 2
        assert np.array_equal(S, S.T)
        lo = float(np.min(np.linalg.eigvalsh(S)))
        p = float(np.min(np.linalg.eigvalsh(S - np.linalg.inv(W))) / np.max(np.abs(S)))
        worst_min, worst_p = min(worst_min, lo), min(worst_p, p)
    print(f"{name}: smallest eigenvalue of an S {worst_min:.3g}; most negative eigenvalue of an S - Omega^-1, relative to max|S| "
          f"{worst_p:.3g}, tolerance {ref.tol_S:.3g}")
    assert worst_min > 0
    assert worst_p >= -ref.tol_S


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_agreement_with_the_covariance_blocks(api, name):
    """S built on the host from rr_pgo_covariances' blocks and the reference Jacobians: a column map or a coordinate order
    mistaken in the same way on both sides of the parity test would show here"""
    c, ref = case(api, name), reference(api, name)
    _, a, b, _, _ = c["cand"]
    n = len(a)
    vals, off = c["g"].covariance_blocks(np.concatenate([a, a, b]), np.concatenate([a, b, b]))
    dims = ref.ref.dims
    host = []
    for q in range(n):
        da, db = int(dims[a[q]]), int(dims[b[q]])
        saa = vals[off[q]:off[q + 1]].reshape(da, da)
        sab = vals[off[n + q]:off[n + q + 1]].reshape(da, db)
        sbb = vals[off[2 * n + q]:off[2 * n + q + 1]].reshape(db, db)
        host.append(ref.innovation_from_blocks(q, saa, sab, sbb))
    check(name, "S against S from covariance blocks", c["S"], host, ref.floor_S, ref.tol_S, FLOOR_MAX)


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_bits_do_not_depend_on_the_rest_of_the_call(api, name):
    c = case(api, name)
    g, cand, n = c["g"], c["cand"], len(c["d2"])
    # the same call twice
    d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
    assert np.array_equal(d2, c["d2"]) and np.array_equal(chi2, c["chi2"])
    assert all(np.array_equal(x, y) for x, y in zip(S, c["S"]))
    # without the innovation covariances
    d2, chi2 = g.gate_edges(*cand)
    assert np.array_equal(d2, c["d2"]) and np.array_equal(chi2, c["chi2"])
    # every 10th candidate alone
    for q in range(0, n, 10):
        d2, chi2, S = g.gate_edges(*select(cand, [q]), return_innovation=True)
        assert d2[0] == c["d2"][q] and chi2[0] == c["chi2"][q] and np.array_equal(S[0], c["S"][q]), q
    # the list reversed
    d2, chi2, S = g.gate_edges(*reverse(cand), return_innovation=True)
    assert np.array_equal(d2[::-1], c["d2"]) and np.array_equal(chi2[::-1], c["chi2"])
    assert all(np.array_equal(x, y) for x, y in zip(S[::-1], c["S"]))


def test_a_plan_cut_by_the_workspace_bound_gives_the_same_bits(api, monkeypatch):
    """24 candidates of intel with distinct end nodes: at least 72 columns, at least 3 chunks.  A handle whose workspace bound
    (RR_PGO_TS_WS_BYTES) is the largest need of a single candidate must cut the list (the reasoning of the test of this
    name in tests/test_covariances_gpu.py).  The cut changes no bit of d2, chi2 and S."""
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]
    full = case(api, "intel")["cand"]
    idx, seen = [], set()
    for c, to in enumerate(full[2]):
        if int(to) not in seen and len(idx) < 24:
            seen.add(int(to))
            idx.append(c)
    assert len(idx) == 24
    cand = select(full, idx)

    def handle(bound=None):
        if bound is None:
            return PoseGraph.new(g2o_path("intel"))
        monkeypatch.setenv("RR_PGO_TS_WS_BYTES", str(bound))
        g = PoseGraph.new(g2o_path("intel"))
        monkeypatch.delenv("RR_PGO_TS_WS_BYTES")
        return g

    def refused(g, q):
        """the bytes the refusal of candidate q alone names"""
        with pytest.raises(PoseGraphError) as ei:
            g.gate_edges(*select(cand, [q]), return_innovation=True)
        assert ei.value.code == _lib.ENOMEM, ei.value
        msg = _lib.load().rr_pgo_last_error().decode()
        m = re.fullmatch(r"rr_pgo_gate_edges: one candidate needs (\d+) bytes of workspace", msg)
        assert m, msg
        return int(m.group(1))

    def same(got, want):
        return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and len(got[2]) == len(want[2]) and \
            all(np.array_equal(x, y) for x, y in zip(got[2], want[2]))

    want = handle().gate_edges(*cand, return_innovation=True)
    B = handle(1)
    need = [refused(B, q) for q in range(24)]
    print(f"intel, 24 candidates alone: workspace needs {min(need)} .. {max(need)} bytes")
    C_ = handle(max(need))
    assert same(C_.gate_edges(*cand, return_innovation=True), want)
    for q in range(24):
        one = C_.gate_edges(*select(cand, [q]), return_innovation=True)
        assert same(one, (want[0][q:q + 1], want[1][q:q + 1], want[2][q:q + 1])), q
    D = handle(max(need) - 1)
    assert refused(D, int(np.argmax(need))) == max(need)


@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
def test_optimize_after_the_gate_gives_the_same_bits(api, solver):
    PoseGraph, Solver = api
    cand = case(api, "intel")["cand"]
    a = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    b = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    d2, _ = a.gate_edges(*cand)
    assert np.array_equal(d2, case(api, "intel")["d2"])   # (the solver of the handle plays no part)
    ea, na = a.optimize(10, return_norms=True)
    eb, nb = b.optimize(10, return_norms=True)
    assert np.array_equal(np.array(ea), np.array(eb)) and np.array_equal(np.array(na), np.array(nb))
    assert np.array_equal(a.state(), b.state())
    a.gate_edges(*select(cand, [0, 5]))   # ... and between two optimize calls
    assert np.array_equal(a.state(), b.state())
    assert np.array_equal(np.array(a.optimize(3)), np.array(b.optimize(3)))
    assert np.array_equal(a.state(), b.state())


def test_replayed_graph_iterations_after_the_gate_give_the_same_bits(api, monkeypatch):
    cand = case(api, "intel")["cand"]
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    a = api[0].new(g2o_path("intel"))
    b = api[0].new(g2o_path("intel"))
    monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    a.iterate_async(2)
    b.iterate_async(2)
    a.sync()
    b.sync()
    a.gate_edges(*select(cand, [1, 2, 3]))
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
    c = case(api, "intel")
    g = api[0].new(g2o_path("intel"))
    cand = c["cand"]
    g.set_robust_kernel("cauchy", 1.0)
    d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
    gw, w = RobustReference(g.graph_arrays(), "cauchy", 1.0).weighted_graph()
    assert np.min(w) < 0.5   # the weights matter at the initial state
    ref = GateReference(c["arrays"], c["state"], cand, h_graph=gw)
    print(ref.summary("intel cauchy delta 1"))
    check_all("intel cauchy delta 1", ref, d2, chi2, S)
    assert np.array_equal(chi2, c["chi2"])   # the candidate's own term is never weighted
    change = float(np.max(np.abs(d2 - c["d2"]) / np.abs(c["d2"])))
    print(f"intel cauchy delta 1: d2 differs from the unweighted call by up to {change:.3g} relative")
    assert change > 1e-3


def test_unsupported_handles_say_why(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]
    cand2 = select(case(api, "intel")["cand"], [0])
    sphere = PoseGraph.new(g2o_path("sphere2500"))
    w3 = sphere.graph_arrays()[6][:21]
    cand3 = (np.array([2], np.int32), np.array([0], np.int32), np.array([5], np.int32), np.array([0, 0, 0, 0, 0, 0, 1.0]), w3)
    handles = {
        "sharded": (PoseGraph.from_arrays(*PoseGraph.new(g2o_path("intel")).graph_arrays(), sharded=True), "sharded", cand2),
        "mixed": (PoseGraph.new(g2o_path("intel"), precision="mixed"), "MIXED", cand2),
        "f32": (PoseGraph.new(g2o_path("intel"), precision="f32"), "F32", cand2),
        "sphere2500": (sphere, "beyond LDS", cand3),
    }
    for what, (h, word, cand) in handles.items():
        with pytest.raises(PoseGraphError) as ei:
            h.gate_edges(*cand)
        assert ei.value.code == _lib.EUNSUPPORTED, (what, ei.value)
        msg = _lib.load().rr_pgo_last_error().decode()
        print(what, "->", msg)
        assert "rr_pgo_gate_edges" in msg and word in msg, (what, msg)


def _raw(L, g, n, kind, a, b, meas, info, d2, chi2=None, innov=None, off=None):
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def p(x, t):
        return None if x is None else x.ctypes.data_as(t)
    return L.rr_pgo_gate_edges(g._h, n, p(kind, ip), p(a, ip), p(b, ip), p(meas, dp), p(info, dp), p(d2, dp), p(chi2, dp),
                               p(innov, dp), p(off, lp))


def test_bad_candidates_are_refused_before_anything_is_written(api):
    from rustrobotics_amd import _lib
    L = _lib.load()
    c = case(api, "simulation-pose-landmark")
    g, nk = c["g"], c["arrays"][0]
    n_nodes = len(nk)
    p0, p1 = (int(v) for v in np.flatnonzero(nk == 0)[:2])
    l0, l1 = (int(v) for v in np.flatnonzero(nk == 1)[:2])
    g3 = case(api, "parking-garage")["g"]
    good_w = [10.0, 1.0, 2.0, 10.0, 3.0, 10.0]
    w21 = list(np.eye(6)[np.triu_indices(6)])
    z7 = [0.0, 0, 0, 0, 0, 0, 1]

    def call(h, second, keep_null=None, n=2):
        """a valid SE2 candidate (p0 -> p1) followed by `second` = (kind, from, to, meas, info)"""
        first = (2, 0, 1, z7, w21) if h is g3 else (0, p0, p1, [0.1, 0.2, 0.3], good_w)
        kind = np.array([first[0], second[0]], np.int32)
        a = np.array([first[1], second[1]], np.int32)
        b = np.array([first[2], second[2]], np.int32)
        meas = np.array(list(first[3]) + list(second[3]) + [0.0] * 8, np.float64)
        info = np.array(list(first[4]) + list(second[4]) + [0.0] * 21, np.float64)
        d2, chi2, innov = np.full(2, -777.0), np.full(2, -777.0), np.full(72, -777.0)
        off = np.full(3, -777, np.int64)
        args = dict(kind=kind, a=a, b=b, meas=meas, info=info, d2=d2, chi2=chi2, innov=innov, off=off)
        if keep_null:
            args[keep_null] = None
        rc = _raw(L, h, n, **args)
        msg = L.rr_pgo_last_error().decode()
        if rc != 0:   # a refusal writes nothing
            assert np.all(d2 == -777.0) and np.all(chi2 == -777.0) and np.all(innov == -777.0) and np.all(off == -777)
        return rc, msg

    se2 = lambda a, b, z=(0.1, 0.2, 0.3), w=good_w: (0, a, b, list(z), list(w))   # noqa: E731
    bad = {
        "node below range": se2(-1, p1), "node beyond range": se2(p0, n_nodes), "to beyond range": se2(n_nodes, p0),
        "from == to": se2(p1, p1),
        "unknown kind 3": (3, p0, p1, [0.1, 0.2, 0.3], good_w), "unknown kind -1": (-1, p0, p1, [0.1, 0.2, 0.3], good_w),
        "SE2 edge into a landmark": se2(p0, l0), "SE2 edge out of a landmark": se2(l0, p0),
        "SE2_XY edge into a pose": (1, p0, p1, [0.1, 0.2], [1.0, 0, 1]), "SE2_XY edge out of a landmark": (1, l0, l1, [0.1, 0.2], [1.0, 0, 1]),
        "SE3 edge on 2-D nodes": (2, p0, p1, z7, w21),
        "indefinite Omega": se2(p0, p1, w=[1.0, 0, 0, -1.0, 0, 1.0]), "zero Omega": se2(p0, p1, w=[0.0] * 6),
        "singular Omega": se2(p0, p1, w=[1.0, 1.0, 0, 1.0, 0, 1.0]),
        "indefinite 2 x 2 Omega": (1, p0, l0, [0.1, 0.2], [1.0, 2.0, 1.0]),
        "NaN measurement": se2(p0, p1, z=(0.1, float("nan"), 0.3)), "infinite measurement": se2(p0, p1, z=(float("inf"), 0.2, 0.3)),
    }
    for what, second in bad.items():
        rc, msg = call(g, second)
        print(what, "->", msg)
        assert rc == _lib.EINVAL, (what, rc, msg)
        assert "rr_pgo_gate_edges" in msg and "candidate 1" in msg, (what, msg)
    for what, second in {"SE2 edge on SE3 nodes": (0, 0, 1, [0.1, 0.2, 0.3], good_w), "SE2_XY edge on SE3 nodes": (1, 0, 1, [0.1, 0.2], [1.0, 0, 1]),
                         "indefinite 6 x 6 Omega": (2, 0, 1, z7, list((np.eye(6) - 2 * np.eye(6)[5][:, None] * np.eye(6)[5])[np.triu_indices(6)]))}.items():
        rc, msg = call(g3, second)
        print(what, "->", msg)
        assert rc == _lib.EINVAL and "candidate 1" in msg, (what, rc, msg)
    # a null required pointer; n_cand < 0
    for name in ("kind", "a", "b", "meas", "info", "d2"):
        rc, msg = call(g, se2(p1, p0), keep_null=name)
        assert rc == _lib.EINVAL and "rr_pgo_gate_edges" in msg, (name, rc, msg)
    rc, msg = call(g, se2(p1, p0), n=-1)
    assert rc == _lib.EINVAL and "rr_pgo_gate_edges" in msg
    # n_cand == 0 is fine, with or without arrays
    assert _raw(L, g, 0, None, None, None, None, None, None) == 0
    rc, _ = call(g, se2(p1, p0), n=0)
    assert rc == 0
    # ... and the handle still answers: innov_out without innov_offset and without chi2_out
    cand = c["cand"]
    n = len(cand[0])
    d2, innov = np.zeros(n), np.zeros(sum(EDGE_DIM[int(k)] ** 2 for k in cand[0]))
    assert _raw(L, g, n, cand[0], cand[1], cand[2], cand[3], cand[4], d2, None, innov, None) == 0
    assert np.array_equal(d2, c["d2"])
    assert np.array_equal(innov, np.concatenate([S.ravel() for S in c["S"]]))
    assert rel_diff(d2, c["d2"]) == 0.0
