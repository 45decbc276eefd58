"""rr_pgo_extend on the MI355X: the extended handle against a fresh handle on the grown graph (bit for bit), against the CPU
oracle, and its initial guess against the numpy reference of tests/extend_reference.py.  Graphs: tests/extend_cases.py."""
import ctypes as C

import numpy as np
import pytest

import extend_reference as ref
from covariances_cases import FLOOR_MAX, far_pairs
from extend_cases import case, closures_only, source_arrays
from gate_cases import INFO_LEN, MEAS_LEN, split_packed
from marginals_reference import MarginalsReference, graph_at_state, rel_diff, tolerance

pytestmark = pytest.mark.gpu

STATS = ("nnz_l_scalars", "n_supernodes", "factor_flops", "n_big_fronts", "n_launches_per_iter")
STATE_LEN = {0: 3, 1: 2, 2: 7}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


def extended(api, c, **kw):
    """the base handle of case c with the addition appended (node_state given)"""
    g = api[0].from_arrays(*c.base, **kw)
    edges, nodes = c.extend_args()
    first = g.extend(*edges, **(nodes if len(c.addition[5]) else {}))
    assert first == (c.n_base, c.e_base)
    return g


def same_graph(a, b):
    assert (a.num_nodes, a.num_edges, a.len, a.anchor_node) == (b.num_nodes, b.num_edges, b.len, b.anchor_node)
    for x, y in zip(a.graph_arrays(), b.graph_arrays()):
        assert np.array_equal(x, y)
    sa, sb = a.stats(), b.stats()
    assert {k: sa[k] for k in STATS} == {k: sb[k] for k in STATS}


def state_offsets(node_kind):
    return np.concatenate([[0], np.cumsum([STATE_LEN[int(k)] for k in node_kind])]).astype(int)


# ---- 1. equals a fresh handle, bit for bit
@pytest.mark.parametrize("name,solver,precision", [
    ("intel", "GaussNewton", "f64"), ("intel", "LevenbergMarquardt", "f64"), ("intel", "GaussNewton", "mixed"),
    ("simulation-pose-landmark", "GaussNewton", "f64"), ("simulation-pose-landmark", "LevenbergMarquardt", "f64"),
    ("parking-garage", "GaussNewton", "f64"), ("parking-garage", "LevenbergMarquardt", "f64"),
    ("sphere2500", "GaussNewton", "f64")])
def test_extended_handle_equals_a_fresh_handle_bit_for_bit(api, name, solver, precision):
    c = closures_only(name, 3) if name == "sphere2500" else case(name)
    kw = dict(solver=api[1][solver], precision=precision)
    a = extended(api, c, **kw)
    b = api[0].from_arrays(*c.grown, **kw)
    same_graph(a, b)
    if name == "sphere2500":
        assert a.stats()["n_big_fronts"] > 0   # fronts beyond LDS: what this case is for
    t = a.extend_times()
    print(f"{name} {solver} {precision}: analysis {t[0]:.3f} ms, engine {t[1]:.3f} ms, state carry {t[2]:.3f} ms")
    assert a.global_error() == b.global_error()
    ea, na = a.optimize(10, return_norms=True)
    eb, nb = b.optimize(10, return_norms=True)
    assert np.array_equal(ea, eb) and np.array_equal(na, nb)
    assert np.array_equal(a.state(), b.state())


# ---- 2. the estimate is carried, not rebuilt
@pytest.mark.parametrize("name", ["intel", "simulation-pose-landmark", "parking-garage"])
def test_estimate_of_the_old_nodes_is_carried_bit_for_bit(api, name):
    c = case(name)
    a = api[0].from_arrays(*c.base)
    a.optimize(5)
    s0 = a.state()
    edges, nodes = c.extend_args()
    a.extend(*edges, **nodes)
    s1 = a.state()
    assert np.array_equal(s1[:len(s0)], s0)
    # the oracle on the grown graph at that state: chi2 and five Gauss-Newton iterations (the tolerances of tests/test_gpu_parity.py)
    o = graph_at_state(a.graph_arrays(), s1)
    chi_gpu, chi_cpu = a.global_error(), o.global_error()
    print(f"{name}: chi2 after extend {chi_gpu:.12g} (oracle {chi_cpu:.12g})")
    np.testing.assert_allclose(chi_gpu, chi_cpu, rtol=1e-9)
    e_gpu, e_cpu = np.array(a.optimize(5)), o.optimize(5)
    print(f"{name}: {e_gpu} against {e_cpu}")
    assert len(e_gpu) == len(e_cpu)
    np.testing.assert_allclose(e_gpu, e_cpu, rtol=1e-7)


# ---- 3. initial guess
def guess_addition(arrays, seed=5):
    """A chain of 5 new poses by odometry from the last old pose (edges listed last link first: five scans), one new pose
    attached by an edge FROM it TO an old pose, and on a 2-D graph a new landmark seen from the third pose of the chain."""
    nk, _, ek, _, _, em, ei = arrays
    n = len(nk)
    rng = np.random.default_rng(seed)
    is3d = bool(np.any(nk == 2))
    pk, pe = (2, 2) if is3d else (0, 0)
    poses = np.flatnonzero(nk == pk)
    w_pose = split_packed(ek, ei, INFO_LEN)[int(np.flatnonzero(ek == pe)[0])]

    def motion():
        if not is3d:
            return np.array([rng.uniform(0.2, 1.0), rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 0.5)])
        q = np.concatenate([0.2 * rng.standard_normal(3), [1.0]])
        return np.concatenate([rng.uniform(-1.0, 1.0, 3), q / np.linalg.norm(q)])
    new_kind = [pk] * 6
    chain = [int(poses[-1])] + [n + i for i in range(5)]
    links = [(pe, chain[i], chain[i + 1], motion(), w_pose) for i in range(5)][::-1]
    links.append((pe, n + 5, int(poses[len(poses) // 2]), motion(), w_pose))
    if not is3d:
        new_kind.append(1)
        w_lm = split_packed(ek, ei, INFO_LEN)[int(np.flatnonzero(ek == 1)[0])]
        links.insert(2, (1, n + 2, n + 6, rng.uniform(-3.0, 3.0, 2), w_lm))
    return (np.array(new_kind, np.int32), np.array([l[0] for l in links], np.int32), np.array([l[1] for l in links], np.int32),
            np.array([l[2] for l in links], np.int32), np.concatenate([l[3] for l in links]), np.concatenate([l[4] for l in links]))


def check_guess(label, new_kind, got_state, want):
    off = state_offsets(new_kind)
    worst_p = worst_a = 0.0
    for i, k in enumerate(new_kind):
        g, w = got_state[off[i]:off[i + 1]], want[i]
        npos = 3 if k == 2 else 2
        worst_p = max(worst_p, float(np.max(np.abs(g[:npos] - w[:npos]) / np.maximum(1.0, np.abs(w[:npos])))))
        if k == 0:
            d = g[2] - w[2]
            worst_a = max(worst_a, abs(np.arctan2(np.sin(d), np.cos(d))))
        elif k == 2:
            assert abs(np.linalg.norm(g[3:]) - 1.0) <= 1e-12
            worst_a = max(worst_a, float(min(np.max(np.abs(g[3:] - w[3:])), np.max(np.abs(g[3:] + w[3:])))))
    print(f"{label}: worst position difference {worst_p:.3g} (relative to max(1, |coordinate|)), worst angle / quaternion difference {worst_a:.3g}; bound 1e-12")
    assert worst_p <= 1e-12 and worst_a <= 1e-12


@pytest.mark.parametrize("name", ["simulation-pose-landmark", "parking-garage"])
def test_initial_guess_follows_the_reference(api, name):
    """f64 chains of at most 6 compositions: about 1e-14 of rounding, bound 1e-12"""
    arrays = source_arrays(name)
    new_kind, ek, ef, et, em, ei = guess_addition(arrays)
    n, n_new = len(arrays[0]), len(new_kind)
    for iterations in (0, 3):   # at the initial state, and at an estimate that only the device holds
        a = api[0].from_arrays(*arrays)
        if iterations:
            a.optimize(iterations)
        s0 = a.state()
        assert a.extend(ek, ef, et, em, ei, node_kind=new_kind) == (n, len(arrays[2]))
        t = a.extend_times()
        print(f"{name}: analysis {t[0]:.3f} ms, engine {t[1]:.3f} ms, state carry + guess {t[2]:.3f} ms")
        s1 = a.state()
        assert a.num_nodes == n + n_new and np.array_equal(s1[:len(s0)], s0)
        want = ref.guess(arrays[0], s0, new_kind, ek, ef, et, em)
        check_guess(f"{name} after {iterations} iterations", new_kind, s1[len(s0):], want)
        ga = a.graph_arrays()
        assert np.array_equal(ga[1][len(s0):], s1[len(s0):])      # the host graph shows what the device holds
        assert np.array_equal(ga[1][:len(s0)], arrays[1])         # ... and keeps the old nodes' initial values
        if not iterations:
            b = api[0].from_arrays(*ga)
            np.testing.assert_allclose(a.global_error(), b.global_error(), rtol=1e-12)
            assert {k: a.stats()[k] for k in STATS} == {k: b.stats()[k] for k in STATS}
        a.optimize(3)   # the grown handle works


def test_unreachable_node_in_guess_mode_is_named(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    arrays = source_arrays("simulation-pose-landmark")
    n = len(arrays[0])
    a = api[0].from_arrays(*arrays)
    w = split_packed(arrays[2], arrays[6], INFO_LEN)[int(np.flatnonzero(arrays[2] == 0)[0])]
    pose = int(np.flatnonzero(arrays[0] == 0)[0])
    # node n is reached, nodes n + 1 and n + 2 hang on each other only
    with pytest.raises(PoseGraphError) as ei:
        a.extend([0, 0], [pose, n + 1], [n, n + 2], [1.0, 0, 0, 1.0, 0, 0], np.concatenate([w, w]), node_kind=[0, 0, 0])
    assert ei.value.code == _lib.EINVAL and f"node {n + 1}" in str(ei.value), str(ei.value)
    # a pose that only a landmark edge reaches
    lm = int(np.flatnonzero(arrays[0] == 1)[0])
    wl = split_packed(arrays[2], arrays[6], INFO_LEN)[int(np.flatnonzero(arrays[2] == 1)[0])]
    with pytest.raises(PoseGraphError) as ei:
        a.extend([1], [n], [lm], [1.0, 0.0], wl, node_kind=[0])
    assert ei.value.code == _lib.EINVAL and f"node {n}" in str(ei.value), str(ei.value)
    assert a.num_nodes == n


# ---- 4. failure leaves the handle alone
def test_a_refused_call_leaves_the_handle_as_it_was(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    arrays = source_arrays("simulation-pose-landmark")
    nk, _, ek, _, _, _, ei_ = arrays
    n, m = len(nk), len(ek)
    a, twin = api[0].from_arrays(*arrays), api[0].from_arrays(*arrays)
    a.optimize(2)
    twin.optimize(2)
    s0 = a.state()
    w = split_packed(ek, ei_, INFO_LEN)[int(np.flatnonzero(ek == 0)[0])]
    wl = split_packed(ek, ei_, INFO_LEN)[int(np.flatnonzero(ek == 1)[0])]
    p0, p1 = (int(v) for v in np.flatnonzero(nk == 0)[:2])
    lm = int(np.flatnonzero(nk == 1)[0])
    z = [1.0, 0.0, 0.1]
    bad = {   # label -> (arguments of extend, a word of the message)
        "bad edge kind": (([7], [p0], [p1], z, w), {}, "edge 0"),
        "bad node kind": (([0], [p0], [n], z, w), dict(node_kind=[5], node_state=[0.0, 0.0, 0.0]), "node 0"),
        "kind does not fit its endpoints": (([0], [p0], [lm], z, w), {}, "edge 0"),
        "landmark edge between two poses": (([1], [p0], [p1], z[:2], wl), {}, "edge 0"),
        "self loop": (([0, 0], [p0, p1], [p1, p1], z + z, np.concatenate([w, w])), {}, "edge 1"),
        "unknown vertex": (([0], [p0], [n + 1], z, w), dict(node_kind=[0], node_state=[0.0, 0.0, 0.0]), "edge 0"),
        "negative vertex": (([0], [-1], [p1], z, w), {}, "edge 0"),
        "mixed 2-D / 3-D": (([], [], [], [], []), dict(node_kind=[2], node_state=[0, 0, 0, 0, 0, 0, 1.0]), "3D"),
        "duplicate id of the graph": (([0], [p0], [n], z, w), dict(node_kind=[0], node_state=[0.0, 0.0, 0.0], node_id=[p1]), f"id {p1}"),
        "duplicate id among the new nodes": (([0, 0], [p0, p0], [n, n + 1], z + z, np.concatenate([w, w])),
                                             dict(node_kind=[0, 0], node_state=[0.0] * 6, node_id=[5000, 5000]), "id 5000"),
        "unreachable node": (([], [], [], [], []), dict(node_kind=[0]), f"node {n}"),
    }
    for label, (edges, nodes, word) in bad.items():
        with pytest.raises(PoseGraphError) as ei:
            a.extend(*edges, **nodes)
        assert ei.value.code == _lib.EINVAL and word in str(ei.value), (label, str(ei.value))
        assert (a.num_nodes, a.num_edges) == (n, m), label
        assert np.array_equal(a.state(), s0), label
    # what the mirror cannot express: negative counts, null pointers
    L = _lib.load()
    one = np.zeros(1, np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    zz, ww = np.array(z), np.ascontiguousarray(w)
    for label, args in {
            "negative node count": (-1, None, None, None, 0, None, None, None, None, None),
            "negative edge count": (0, None, None, None, -1, None, None, None, None, None),
            "null node kinds": (1, None, None, None, 0, None, None, None, None, None),
            "null edge arrays": (0, None, None, None, 1, one.ctypes.data_as(ip), None, None, zz.ctypes.data_as(dp), ww.ctypes.data_as(dp))}.items():
        assert L.rr_pgo_extend(a._h, *args) == _lib.EINVAL, label
        assert L.rr_pgo_last_error(), label
        assert (a.num_nodes, a.num_edges) == (n, m) and np.array_equal(a.state(), s0), label
    ea, na = a.optimize(5, return_norms=True)
    et, nt = twin.optimize(5, return_norms=True)
    assert np.array_equal(ea, et) and np.array_equal(na, nt) and np.array_equal(a.state(), twin.state())


# ---- 5. the robust setting is carried
@pytest.mark.parametrize("masked", [False, True])
def test_robust_setting_is_carried_and_new_edges_are_robustified(api, masked):
    c = case("intel")
    ek, ef, et, em, ei, nk, ns = c.addition
    # ... plus a deliberately false closure: the measurement of another one, between two far old poses
    w = split_packed(ek, ei, INFO_LEN)[0]
    ek2, ef2, et2 = np.concatenate([ek, [0]]), np.concatenate([ef, [10]]), np.concatenate([et, [c.n_base // 2]])
    em2, ei2 = np.concatenate([em, [25.0, -25.0, 2.0]]), np.concatenate([ei, w])
    mask = None
    if masked:
        mask = (np.arange(c.e_base) % 3 != 0).astype(np.int32)
    a = api[0].from_arrays(*c.base)
    a.set_robust_kernel("cauchy", 1.0, mask)
    a.extend(ek2, ef2, et2, em2, ei2, node_kind=nk, node_state=ns)
    grown = c.grown[:2] + (np.concatenate([c.grown[2], [0]]), np.concatenate([c.grown[3], [10]]), np.concatenate([c.grown[4], [c.n_base // 2]]),
                           np.concatenate([c.grown[5], [25.0, -25.0, 2.0]]), np.concatenate([c.grown[6], w]))
    b = api[0].from_arrays(*grown)
    b.set_robust_kernel("cauchy", 1.0, None if mask is None else np.concatenate([mask, np.ones(len(ek2), np.int32)]))
    sa, wa = a.edge_errors()
    sb, wb = b.edge_errors()
    assert np.array_equal(sa, sb) and np.array_equal(wa, wb)
    print(f"masked {masked}: the false closure has s = {sa[-1]:.6g}, weight {wa[-1]:.3g}")
    assert wa[-1] < 0.5
    if masked:
        assert np.all(wa[:c.e_base][mask == 0] == 1.0) and np.any(wa[:c.e_base][mask == 1] < 1.0)
    assert a.global_error() == b.global_error()
    assert np.array_equal(a.optimize(3), b.optimize(3))


# ---- 6. queries see the new graph
def test_queries_after_extend_see_the_new_graph(api):
    name = "simulation-pose-landmark"
    c = case(name)
    a = api[0].from_arrays(*c.base)
    a.optimize(5)
    ek, ef, et, em, ei, nk, ns = c.addition
    old_old = int(np.flatnonzero((ef < c.n_base) & (et < c.n_base))[0])
    m, w = split_packed(ek, em, MEAS_LEN), split_packed(ek, ei, INFO_LEN)
    cand = ([ek[old_old]], [ef[old_old]], [et[old_old]], m[old_old], w[old_old])
    d2_before, _ = a.gate_edges(*cand)           # (builds the tree tables of the base graph's factor)
    a.extend(ek, ef, et, em, ei, node_kind=nk, node_state=ns)
    d2_after, _ = a.gate_edges(*cand)            # the candidate is now an edge of the graph: its information counts twice
    print(f"{name}: d2 of an added closure before {d2_before[0]:.9g}, after {d2_after[0]:.9g}")
    assert np.isfinite(d2_after[0]) and d2_after[0] != d2_before[0]
    nodes, qa, qb = far_pairs(a.num_nodes)
    vals, off = a.covariance_blocks(qa, qb)
    want, floor = MarginalsReference(graph_at_state(a.graph_arrays(), a.state())).blocks(qa, qb)
    got = [vals[off[q]:off[q + 1]].reshape(wq.shape) for q, wq in enumerate(want)]
    worst, tol = max(rel_diff(g, wq) for g, wq in zip(got, want)), tolerance(floor)
    print(f"{name} after extend: {len(want)} blocks, worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert len(got) == len(want) and floor <= FLOOR_MAX and worst <= tol


# ---- 7. captured graphs
def test_replayed_graph_iterations_around_extend(api, monkeypatch):
    """RR_PGO_FORCE_GRAPH=1 across creation AND extend: the graph captured before the call must not be replayed after it.
    Both handles then start from one state given through set_state (so that both hold the same bits) and replay eight
    iterations."""
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    try:
        c = case("intel")
        a = api[0].from_arrays(*c.base)
        a.iterate_async(2)
        a.sync()
        edges, nodes = c.extend_args()
        a.extend(*edges, **nodes)
        b = api[0].from_arrays(*c.grown)
        b.iterate_async(2)
        b.sync()
    finally:
        monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    same_graph(a, b)
    s = a.state()
    a.set_state(s)
    b.set_state(s)
    assert np.array_equal(a.state(), b.state())
    a.iterate_async(8)
    b.iterate_async(8)
    a.sync()
    b.sync()
    sa, sb = a.state(), b.state()
    assert np.array_equal(sa, sb) and not np.array_equal(sa, s)
    assert a.global_error() == b.global_error()
    # replays of a graph captured on the grown graph's engine (rr_pgo_extend builds a new one: its counters start again)
    sta, stb = a.stats(), b.stats()
    assert (sta["n_graph_replays"], sta["n_graph_captures"], sta["n_plain_iterations"]) == (8, 1, 0)
    assert (stb["n_graph_replays"], stb["n_graph_captures"], stb["n_plain_iterations"]) == (10, 1, 0)


# ---- 8. refusal
def test_sharded_handle_is_refused_and_the_empty_call_changes_nothing(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    c = case("simulation-pose-landmark")
    edges, nodes = c.extend_args()
    sh = api[0].from_arrays(*c.base, sharded=True)
    with pytest.raises(PoseGraphError) as ei:
        sh.extend(*edges, **nodes)
    assert ei.value.code == _lib.EUNSUPPORTED and "sharded" in str(ei.value)
    assert (sh.num_nodes, sh.num_edges) == (c.n_base, c.e_base)
    a = api[0].from_arrays(*c.base)
    a.optimize(2)
    s0, t0, stream = a.state(), a.extend_times(), a.stream_ptr()
    assert a.extend([], [], [], [], []) == (c.n_base, c.e_base)
    assert _lib.load().rr_pgo_extend(a._h, 0, None, None, None, 0, None, None, None, None, None) == _lib.OK
    assert (a.num_nodes, a.num_edges) == (c.n_base, c.e_base) and np.array_equal(a.state(), s0)
    assert a.extend_times() == t0 and a.stream_ptr() == stream   # nothing was rebuilt
