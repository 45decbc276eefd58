"""rr_pgo_gate_joint on the MI355X against the CPU reference (tests/gate_joint_reference.py) on the sets of
tests/gate_joint_cases.py, and the properties the interface promises bit for bit.

A GPU value passes when its relative difference to the reference is at most max(1e-12, 100 x noise floor), the floor being
the worst relative difference between the reference's two independent computations of the same quantity; the floor itself
must be at most FLOOR_MAX = 1e-6.  Every comparison prints its worst figure, the floor and the tolerance before it asserts."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import g2o_path
from covariances_cases import FLOOR_MAX
from gate_cases import EDGE_DIM, GATE_GRAPHS, candidates, select
from gate_joint_cases import block_starts, joint_sets, set_dims
from gate_joint_reference import JointReference, check_each
from gate_reference import check
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
    """the handle at the state of GATE_GRAPHS, its candidates and sets and one full call (made once per graph)"""
    if name not in _CASES:
        g = api[0].new(g2o_path(name))
        if GATE_GRAPHS[name]:
            g.optimize(GATE_GRAPHS[name])
        arrays, state = g.graph_arrays(), g.state()
        cand = candidates(arrays, state)
        sets = joint_sets(len(cand[0]))
        d2, prefix, S = g.gate_joint(*cand, sets, return_prefix=True, return_innovation=True)
        t = g.gate_joint_times()
        print(f"{name}: {len(sets)} sets: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, joint kernel + copy {t[2]:.3f} ms")
        _CASES[name] = dict(g=g, arrays=arrays, state=state, cand=cand, sets=sets, d2=d2, prefix=prefix, S=S)
    return _CASES[name]


def reference(api, name):
    if name not in _REFS:
        c = case(api, name)
        _REFS[name] = JointReference(c["arrays"], c["state"], c["cand"], c["sets"])
        print(_REFS[name].summary(name))
    return _REFS[name]


def check_all(label, ref, d2, prefix, S):
    check(label, "d2", d2, ref.d2, ref.floor_d2, ref.tol_d2, FLOOR_MAX)
    check_each(label, "prefixes", prefix, ref.prefix, ref.floor_prefix, ref.tol_prefix, FLOOR_MAX)
    check(label, "S", S, ref.S, ref.floor_S, ref.tol_S, FLOOR_MAX)


def same(got, want):
    """(d2, prefixes, S) bit for bit"""
    return np.array_equal(got[0], want[0]) and len(got[1]) == len(want[1]) and len(got[2]) == len(want[2]) and \
        all(np.array_equal(x, y) for x, y in zip(got[1], want[1])) and all(np.array_equal(x, y) for x, y in zip(got[2], want[2]))


def full(g, cand, sets):
    return g.gate_joint(*cand, sets, return_prefix=True, return_innovation=True)


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_gate_joint_matches_the_reference(api, name):
    c, ref = case(api, name), reference(api, name)
    assert [S.shape[0] for S in c["S"]] == set_dims(c["cand"][0], c["sets"])
    check_all(name, ref, c["d2"], c["prefix"], c["S"])
    # ---- decisions at the default threshold; a set whose reference d2 lies within the tolerance of the threshold is left
    # out (at most one per graph; the reference has none: tests/test_gate_joint_cpu.py)
    g, cand, sets = c["g"], c["cand"], c["sets"]
    mask = g.gate_joint_accept(*cand, sets)
    assert mask.dtype == bool and np.array_equal(mask, c["d2"] <= ref.threshold)
    keep = ~ref.undecided
    print(f"{name}: {int(np.sum(mask))} accepted, {int(np.sum(~mask))} rejected, {int(np.sum(~keep))} left out of the comparison")
    assert np.sum(~keep) <= 1
    assert np.array_equal(mask[keep], ref.accept[keep])
    assert np.array_equal(g.gate_joint_accept(*cand, sets, threshold=30.0), c["d2"] <= 30.0)
    # without the optional outputs: the same d2
    assert np.array_equal(g.gate_joint(*cand, sets), c["d2"])


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_bitwise_symmetry_and_the_last_prefix(api, name):
    c = case(api, name)
    for S, pre, d2 in zip(c["S"], c["prefix"], c["d2"]):
        assert np.array_equal(S, S.T)
        assert pre[-1] == d2 and np.all(np.diff(pre) >= 0)


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_a_block_depends_on_its_two_candidates_alone(api, name):
    """every block (c, d), c != d, of sets of 8 against the set [d, c] alone -- among other pair sets -- and every diagonal
    block against the set [c] alone, bit for bit"""
    c = case(api, name)
    g, cand, kind = c["g"], c["cand"], c["cand"][0]
    small, where = [], []
    for s, members in enumerate(c["sets"]):
        if len(members) != 8 or s % 4 != 0:
            continue
        o = block_starts(kind, members)
        for i in range(len(members)):
            for j in range(i + 1):
                small.append([members[j], members[i]] if j < i else [members[i]])
                where.append((s, o[i], o[i + 1], o[j], o[j + 1]))
    assert len(small) >= 5 * 36
    _, _, S2 = full(g, cand, small)
    for (s, i0, i1, j0, j1), P in zip(where, S2):
        if i0 == j0:
            assert np.array_equal(P, c["S"][s][i0:i1, i0:i1]), (s, i0)
            continue
        dj = j1 - j0
        assert np.array_equal(P[dj:, :dj], c["S"][s][i0:i1, j0:j1]), (s, i0, j0)
        assert np.array_equal(P[:dj, :dj], c["S"][s][j0:j1, j0:j1]), (s, j0)
        assert np.array_equal(P[dj:, dj:], c["S"][s][i0:i1, i0:i1]), (s, i0)


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_a_prefix_is_the_distance_of_the_truncated_set(api, name):
    c = case(api, name)
    cut, where = [], []
    for s, members in enumerate(c["sets"]):
        for k in range(len(members)):
            cut.append(members[:k + 1])
            where.append((s, k))
    d2, prefix, S = full(c["g"], c["cand"], cut)
    o = [block_starts(c["cand"][0], m) for m in c["sets"]]
    for q, (s, k) in enumerate(where):
        assert d2[q] == c["prefix"][s][k], (s, k)
        assert np.array_equal(prefix[q], c["prefix"][s][:k + 1]), (s, k)
        assert np.array_equal(S[q], c["S"][s][:o[s][k + 1], :o[s][k + 1]]), (s, k)


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_bits_do_not_depend_on_the_rest_of_the_call(api, name):
    c = case(api, name)
    g, cand, sets = c["g"], c["cand"], c["sets"]
    want = (c["d2"], c["prefix"], c["S"])
    assert same(full(g, cand, sets), want)                                   # the same call twice
    got = full(g, cand, sets[::-1])                                          # the sets in reverse order
    assert same((got[0][::-1], got[1][::-1], got[2][::-1]), want)
    for s in range(0, len(sets), 3):                                         # a set alone
        assert same(full(g, cand, [sets[s]]), (want[0][s:s + 1], want[1][s:s + 1], want[2][s:s + 1])), s
    # ... and with only the candidates of the set in the call
    s = 16
    assert same(full(g, select(cand, sets[s]), [list(range(len(sets[s])))]), (want[0][s:s + 1], want[1][s:s + 1], want[2][s:s + 1]))


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_a_permuted_set_gives_the_permuted_blocks(api, name):
    c, ref = case(api, name), reference(api, name)
    kind = c["cand"][0]
    rng = np.random.default_rng(5)
    worst = 0.0
    for s in (0, 16, 17):
        members = c["sets"][s]
        perm = [int(p) for p in rng.permutation(len(members))]
        d2, _, S = full(c["g"], c["cand"], [[members[p] for p in perm]])
        o, op = block_starts(kind, members), block_starts(kind, [members[p] for p in perm])
        for i, pi in enumerate(perm):
            for j, pj in enumerate(perm):
                assert np.array_equal(S[0][op[i]:op[i + 1], op[j]:op[j + 1]], c["S"][s][o[pi]:o[pi + 1], o[pj]:o[pj + 1]]), (s, i, j)
        worst = max(worst, abs(d2[0] - c["d2"][s]) / c["d2"][s])
    print(f"{name}: d2 of a permuted set differs by up to {worst:.3g} relative, tolerance {ref.tol_d2:.3g}")
    assert worst <= ref.tol_d2


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_joint_innovation_covariances_are_positive(api, name):
    c, ref = case(api, name), reference(api, name)
    worst_min, worst_p = np.inf, 0.0
    for s, S in enumerate(c["S"]):
        worst_min = min(worst_min, float(np.min(np.linalg.eigvalsh(S))))
        worst_p = min(worst_p, float(np.min(np.linalg.eigvalsh(S - ref.blockdiag_cov(s))) / np.max(np.abs(S))))
    print(f"{name}: smallest eigenvalue of an S {worst_min:.3g}; most negative eigenvalue of an S - blockdiag(Omega^-1), relative "
          f"to max|S| {worst_p:.3g}, tolerance {ref.tol_S:.3g}")
    assert worst_min > 0
    assert worst_p >= -ref.tol_S


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_agreement_with_the_covariance_blocks(api, name):
    """S_s built on the host from PoseGraph.covariance of the set's nodes and the reference Jacobians: a column map mistaken
    in the same way on both sides of the parity test would show here"""
    c, ref = case(api, name), reference(api, name)
    host = []
    for s in range(len(c["sets"])):
        _, nodes = ref.jacobian(s)
        host.append(ref.innovation_from_covariance(s, c["g"].covariance(nodes)))
    check(name, "S against S from the covariance of the set's nodes", c["S"], host, ref.floor_S, ref.tol_S, FLOOR_MAX)


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_one_candidate_sets_agree_with_gate_edges(api, name):
    c, ref = case(api, name), reference(api, name)
    g, cand = c["g"], c["cand"]
    n = len(cand[0])
    d2e, _, Se = g.gate_edges(*cand, return_innovation=True)
    d2, prefix, S = full(g, cand, [[q] for q in range(n)])
    assert all(np.array_equal(p, d2[q:q + 1]) for q, p in enumerate(prefix))
    wd = float(np.max(np.abs(d2 - d2e) / np.abs(d2e)))
    ws = max(rel_diff(x, y) for x, y in zip(S, Se))
    print(f"{name}: {n} one-candidate sets against gate_edges: d2 {wd:.3g} (tolerance {ref.gate.tol_d2:.3g}), S {ws:.3g} (tolerance {ref.gate.tol_S:.3g})")
    assert wd <= ref.gate.tol_d2 and ws <= ref.gate.tol_S


def test_a_plan_cut_by_the_workspace_bound_gives_the_same_bits(api, monkeypatch):
    """24 candidates of intel with distinct `to` nodes in 6 sets of 4: a set alone has at most 8 nodes, 24 columns, one chunk,
    and needs the union of its nodes' root paths; the list has at least 72 columns, 3 chunks, and needs the sum over its
    chunks of each chunk's union, which holds every one of those paths and the root front twice more.  A handle whose
    workspace bound (RR_PGO_TS_WS_BYTES) is the largest need of a single set must cut the list -- between sets, a set is
    never split -- and the cut changes no bit."""
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]
    cand = case(api, "intel")["cand"]
    idx, seen = [], set()
    for q, to in enumerate(cand[2]):
        if int(to) not in seen and len(idx) < 24:
            seen.add(int(to))
            idx.append(q)
    assert len(idx) == 24
    sets = [idx[4 * s:4 * s + 4] for s in range(6)]

    def handle(bound=None):
        if bound is None:
            return PoseGraph.new(g2o_path("intel"))
        monkeypatch.setenv("RR_PGO_TS_WS_BYTES", str(bound))
        g = PoseGraph.new(g2o_path("intel"))
        monkeypatch.delenv("RR_PGO_TS_WS_BYTES")
        return g

    def refused(g, s):
        """the bytes the refusal of set s alone names"""
        with pytest.raises(PoseGraphError) as ei:
            full(g, cand, [sets[s]])
        assert ei.value.code == _lib.ENOMEM, ei.value
        msg = _lib.load().rr_pgo_last_error().decode()
        m = re.fullmatch(r"rr_pgo_gate_joint: one set needs (\d+) bytes of workspace", msg)
        assert m, msg
        return int(m.group(1))

    want = full(handle(), cand, sets)
    B = handle(1)
    need = [refused(B, s) for s in range(6)]
    print(f"intel, 6 sets of 4 alone: workspace needs {min(need)} .. {max(need)} bytes")
    C_ = handle(max(need))
    assert same(full(C_, cand, sets), want)
    for s in range(6):
        assert same(full(C_, cand, [sets[s]]), (want[0][s:s + 1], want[1][s:s + 1], want[2][s:s + 1])), s
    D = handle(max(need) - 1)
    assert refused(D, int(np.argmax(need))) == max(need)


@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
def test_optimize_after_the_joint_gate_gives_the_same_bits(api, solver):
    PoseGraph, Solver = api
    c = case(api, "intel")
    cand, sets = c["cand"], c["sets"]
    a = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    b = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    assert np.array_equal(a.gate_joint(*cand, sets), c["d2"])   # (the solver of the handle plays no part)
    assert np.array_equal(a.state(), b.state())
    ea, na = a.optimize(10, return_norms=True)
    eb, nb = b.optimize(10, return_norms=True)
    assert np.array_equal(np.array(ea), np.array(eb)) and np.array_equal(np.array(na), np.array(nb))
    assert np.array_equal(a.state(), b.state())
    a.gate_joint(*cand, sets[:3])   # ... and between two optimize calls
    assert np.array_equal(a.state(), b.state())
    assert np.array_equal(np.array(a.optimize(3)), np.array(b.optimize(3)))
    assert np.array_equal(a.state(), b.state())


def test_replayed_graph_iterations_around_the_joint_gate_give_the_same_bits(api, monkeypatch):
    c = case(api, "intel")
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    a = api[0].new(g2o_path("intel"))
    b = api[0].new(g2o_path("intel"))
    monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    a.iterate_async(2)
    b.iterate_async(2)
    a.sync()
    b.sync()
    a.gate_joint(*c["cand"], c["sets"][16:19])
    a.iterate_async(8)
    b.iterate_async(8)
    a.sync()
    b.sync()
    assert np.array_equal(a.state(), b.state())
    for g in (a, b):   # every one of the ten iterations was a replay of the one captured graph
        st = g.stats()
        assert (st["n_graph_replays"], st["n_graph_captures"], st["n_plain_iterations"]) == (10, 1, 0)


def test_cauchy_weights_are_part_of_the_inverted_matrix_and_stay_set(api):
    from robust_reference import RobustReference
    name = "simulation-pose-pose"
    a = api[0].new(g2o_path(name))
    b = api[0].new(g2o_path(name))
    arrays, state = a.graph_arrays(), a.state()
    cand = candidates(arrays, state)
    sets = joint_sets(len(cand[0]))
    plain = a.gate_joint(*cand, sets)
    a.set_robust_kernel("cauchy", 1.0)
    b.set_robust_kernel("cauchy", 1.0)
    d2, prefix, S = full(a, cand, sets)
    gw, w = RobustReference(arrays, "cauchy", 1.0).weighted_graph()
    print(f"{name} cauchy delta 1: weights in [{float(np.min(w)):.3g}, {float(np.max(w)):.3g}]")
    assert np.min(w) < 1.0
    ref = JointReference(arrays, state, cand, sets, h_graph=gw)
    print(ref.summary(name + " cauchy delta 1"))
    check_all(name + " cauchy delta 1", ref, d2, prefix, S)
    change = float(np.max(np.abs(d2 - plain) / np.abs(plain)))
    print(f"{name} cauchy delta 1: d2 differs from the unweighted call by up to {change:.3g} relative")
    assert change > 100 * ref.tol_d2
    # the robust setting is still the handle's
    assert np.array_equal(np.array(a.optimize(3)), np.array(b.optimize(3)))
    assert np.array_equal(a.state(), b.state())


def test_unsupported_handles_say_why(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]
    cand2 = select(case(api, "intel")["cand"], [0, 1])
    sphere = PoseGraph.new(g2o_path("sphere2500"))
    w3 = sphere.graph_arrays()[6][:21]
    cand3 = (np.array([2], np.int32), np.array([0], np.int32), np.array([5], np.int32), np.array([0, 0, 0, 0, 0, 0, 1.0]), w3)
    handles = {
        "sharded": (PoseGraph.from_arrays(*PoseGraph.new(g2o_path("intel")).graph_arrays(), sharded=True), "sharded", cand2, [[0, 1]]),
        "f32": (PoseGraph.new(g2o_path("intel"), precision="f32"), "F32", cand2, [[0, 1]]),
        "sphere2500": (sphere, "beyond LDS", cand3, [[0]]),
    }
    for what, (h, word, cand, sets) in handles.items():
        with pytest.raises(PoseGraphError) as ei:
            h.gate_joint(*cand, sets)
        assert ei.value.code == _lib.EUNSUPPORTED, (what, ei.value)
        msg = _lib.load().rr_pgo_last_error().decode()
        print(what, "->", msg)
        assert "rr_pgo_gate_joint" in msg and word in msg, (what, msg)


def test_bad_arguments_are_refused_before_anything_is_written(api):
    from rustrobotics_amd import _lib
    L = _lib.load()
    c = case(api, "simulation-pose-landmark")
    g, nk = c["g"], c["arrays"][0]
    p = [int(v) for v in np.flatnonzero(nk == 0)[:4]]
    l0 = int(np.flatnonzero(nk == 1)[0])
    good_w = [10.0, 1.0, 2.0, 10.0, 3.0, 10.0]
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def ptr(x, t):
        return None if x is None else x.ctypes.data_as(t)

    def call(cands, set_ptr, set_cand, null=(), n_cand=None, n_sets=None, h=None):
        """cands: (kind, from, to, meas, info) per candidate; returns (rc, message) and checks that a refusal wrote nothing"""
        args = dict(kind=np.array([q[0] for q in cands], np.int32), a=np.array([q[1] for q in cands], np.int32),
                    b=np.array([q[2] for q in cands], np.int32),
                    meas=np.array([v for q in cands for v in q[3]] + [0.0] * 8, np.float64),
                    info=np.array([v for q in cands for v in q[4]] + [0.0] * 21, np.float64),
                    set_ptr=np.array(set_ptr, np.int32), set_cand=np.array(list(set_cand) + [0], np.int32),
                    d2=np.full(8, -777.0), prefix=np.full(64, -777.0), innov=np.full(8 * 48 * 48, -777.0), off=np.full(9, -777, np.int64))
        for k in null:
            args[k] = None
        rc = L.rr_pgo_gate_joint((h or g)._h, len(cands) if n_cand is None else n_cand, ptr(args["kind"], ip), ptr(args["a"], ip),
                                 ptr(args["b"], ip), ptr(args["meas"], dp), ptr(args["info"], dp),
                                 len(set_ptr) - 1 if n_sets is None else n_sets, ptr(args["set_ptr"], ip), ptr(args["set_cand"], ip),
                                 ptr(args["d2"], dp), ptr(args["prefix"], dp), ptr(args["innov"], dp), ptr(args["off"], lp))
        msg = L.rr_pgo_last_error().decode()
        if rc != 0:
            for k in ("d2", "prefix", "innov", "off"):
                assert args[k] is None or np.all(args[k] == -777), (k, msg)
        return rc, msg, args

    se2 = lambda a, b, z=(0.1, 0.2, 0.3), w=good_w: (0, a, b, list(z), list(w))   # noqa: E731
    xy = (1, p[0], l0, [0.1, 0.2], [1.0, 0.0, 1.0])
    two = [se2(p[0], p[1]), se2(p[2], p[3])]
    rc, msg, out = call(two, [0, 2, 3], [0, 1, 1])
    assert rc == 0, msg
    assert np.all(out["d2"][:2] > 0) and np.all(out["d2"][2:] == -777) and out["prefix"][1] == out["d2"][0] and out["prefix"][2] == out["d2"][1]
    assert list(out["off"][:3]) == [0, 36, 45] and np.all(out["innov"][:45] != -777) and np.all(out["innov"][45:] == -777)
    # ---- every candidate check of rr_pgo_gate_edges, through the shared code: the message names the candidate
    bad_cand = {
        "node out of range": se2(p[0], len(nk)), "from == to": se2(p[1], p[1]), "unknown kind": (3, p[0], p[1], [0.1, 0.2, 0.3], good_w),
        "SE2 edge into a landmark": se2(p[0], l0), "SE2_XY edge into a pose": (1, p[0], p[1], [0.1, 0.2], [1.0, 0, 1]),
        "SE3 edge on 2-D nodes": (2, p[0], p[1], [0.0, 0, 0, 0, 0, 0, 1], list(np.eye(6)[np.triu_indices(6)])),
        "indefinite Omega": se2(p[0], p[1], w=[1.0, 0, 0, -1.0, 0, 1.0]), "NaN measurement": se2(p[0], p[1], z=(0.1, float("nan"), 0.3)),
    }
    for what, second in bad_cand.items():
        rc, msg, _ = call([two[0], second], [0, 1], [0])   # (refused although no set names the candidate)
        print(what, "->", msg)
        assert rc == _lib.EINVAL and "rr_pgo_gate_joint" in msg and "candidate 1" in msg, (what, rc, msg)
    # ---- the sets: the message names the set
    seventeen = [se2(p[0], p[1])] * 17
    bad_sets = {
        "set_ptr[0] != 0": (two, [1, 2], [0, 1], "set_ptr[0]"),
        "set_ptr decreases": (two, [0, 2, 1], [0, 1], "set 1"),
        "an empty set": (two, [0, 1, 1, 2], [0, 1], "set 1"),
        "set_cand beyond range": (two, [0, 1, 2], [0, 2], "set 1"),
        "set_cand below range": (two, [0, 2], [0, -1], "set 0"),
        "17 candidates": ([xy] * 17, [0, 1, 18], [0] + list(range(17)), "set 1"),
        "17 candidates of D_s = 51": (seventeen, [0, 17], list(range(17)), "set 0"),
    }
    for what, (cands, sp, sc, word) in bad_sets.items():
        rc, msg, _ = call(cands, sp, sc)
        print(what, "->", msg)
        assert rc == _lib.EINVAL and "rr_pgo_gate_joint" in msg and word in msg, (what, rc, msg)
    se3 = (2, 0, 1, [0.0, 0, 0, 0, 0, 0, 1], list(np.eye(6)[np.triu_indices(6)]))
    g3 = case(api, "parking-garage")["g"]
    rc, msg, _ = call([se3] * 9, [0, 1, 10], [0] + list(range(9)), h=g3)   # 9 SE3 candidates: D_s = 54
    print("D_s = 54 ->", msg)
    assert rc == _lib.EINVAL and "set 1" in msg and "RR_PGO_GATE_JOINT_MAX_DIM" in msg, (rc, msg)
    rc, msg, _ = call([se3] * 8, [0, 8], list(range(8)), h=g3)
    assert rc == 0, msg
    rc, msg, _ = call(seventeen[:16], [0, 16], list(range(16)))       # 16 candidates, D_s = 48: the caps themselves
    assert rc == 0, msg
    rc, msg, _ = call(seventeen, [0, 17], list(range(17)))            # 17 SE2 candidates: the count is named first
    assert rc == _lib.EINVAL and "RR_PGO_GATE_JOINT_MAX_CAND" in msg
    rc, msg, _ = call([se2(p[0], p[1])] * 15 + [xy, xy], [0, 16], [15] + list(range(15)))   # 16 candidates of D_s = 47
    assert rc == 0, msg
    # a null required pointer; n_sets < 0; n_cand < 0
    for name in ("kind", "a", "b", "meas", "info", "set_ptr", "set_cand", "d2"):
        rc, msg, _ = call(two, [0, 2], [0, 1], null=(name,))
        assert rc == _lib.EINVAL and "rr_pgo_gate_joint" in msg, (name, rc, msg)
    for kw in (dict(n_sets=-1), dict(n_cand=-1)):
        rc, msg, _ = call(two, [0, 2], [0, 1], **kw)
        assert rc == _lib.EINVAL and "rr_pgo_gate_joint" in msg, (kw, rc, msg)
    # n_sets == 0 is fine, with or without arrays, and writes nothing
    rc, msg, out = call(two, [0], [], n_sets=0)
    assert rc == 0 and np.all(out["d2"] == -777) and out["off"][0] == 0 and np.all(out["off"][1:] == -777), msg
    assert L.rr_pgo_gate_joint(g._h, 0, None, None, None, None, None, 0, None, None, None, None, None, None) == 0
    # ... and the handle still answers, without the optional outputs
    rc, msg, out = call(two, [0, 2], [0, 1], null=("prefix", "innov", "off"))
    assert rc == 0 and out["d2"][0] > 0, msg
    assert np.array_equal(g.gate_joint(*c["cand"], c["sets"]), c["d2"])
