"""rr_pgo_remove_edges on the MI355X: extend-then-remove is the handle before the extend, bit for bit; a handle after a removal
against a fresh handle on the remaining arrays; what is carried; the anchor; refusals.  Graphs: tests/extend_cases.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import g2o_path
from extend_cases import K_EDGES, SOURCES, connected, select_edges, source_arrays, split_case

pytestmark = pytest.mark.gpu

# what of stats() describes the handle: the analysis and the launches.  The rest -- the counters of iterations run, replayed and
# captured, and the times -- belongs to the engine, and a rebuilt engine starts them again (as after rr_pgo_extend).
STATS = ("nnz_l_scalars", "n_supernodes", "factor_flops", "n_big_fronts", "n_launches_per_iter")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


def remaining(arrays, removed):
    """(arrays without the edges `removed`, the indices kept)"""
    keep = np.array([k for k in range(len(arrays[2])) if k not in set(int(r) for r in removed)])
    return tuple(arrays[:2]) + select_edges(arrays, keep), keep


def seeded_removal(arrays, count=K_EDGES, seed=9, skip_first=True):
    """`count` seeded non-consecutive edges whose removal leaves the graph connected and every node with an edge"""
    ek, ef, et = np.asarray(arrays[2]), np.asarray(arrays[3], np.int64), np.asarray(arrays[4], np.int64)
    pool = np.flatnonzero(np.abs(ef - et) > 1)
    if skip_first:
        pool = pool[pool != np.flatnonzero(ek != 1)[0]]
    picked = np.sort(np.random.default_rng(seed).choice(pool, count, replace=False)).astype(np.int32)
    rest, _ = remaining(arrays, picked)
    assert connected(rest)
    return picked, rest


def same_graph(a, b):
    assert (a.num_nodes, a.num_edges, a.len, a.anchor_node) == (b.num_nodes, b.num_edges, b.len, b.anchor_node)
    for x, y in zip(a.graph_arrays(), b.graph_arrays()):
        assert np.array_equal(x, y)
    sa, sb = a.stats(), b.stats()
    assert {k: sa[k] for k in STATS} == {k: sb[k] for k in STATS}


# ---- 1. round trip
@pytest.mark.parametrize("name", SOURCES)
def test_extend_then_remove_is_the_handle_before_the_extend_bit_for_bit(api, name):
    c = split_case(source_arrays(name), m_nodes=0, k_edges=K_EDGES)
    a, twin = api[0].from_arrays(*c.base), api[0].from_arrays(*c.base)
    a.optimize(2)
    twin.optimize(2)
    ek, ef, et, em, ei, _, _ = c.addition
    assert len(ek) == K_EDGES and a.extend(ek, ef, et, em, ei) == (c.n_base, c.e_base)
    assert a.num_edges == c.e_base + K_EDGES
    a.remove_edges(np.arange(c.e_base, c.e_base + K_EDGES))
    t = a.remove_edges_times()
    print(f"{name}: analysis {t[0]:.3f} ms, engine {t[1]:.3f} ms, state carry {t[2]:.3f} ms")
    same_graph(a, twin)
    assert np.array_equal(a.state(), twin.state())
    assert a.global_error() == twin.global_error()
    ea, na = a.optimize(3, return_norms=True)
    eb, nb = twin.optimize(3, return_norms=True)
    assert np.array_equal(ea, eb) and np.array_equal(na, nb) and np.array_equal(a.state(), twin.state())


# ---- 2. against a fresh handle on the remaining arrays
@pytest.mark.parametrize("name", SOURCES)
def test_removal_equals_a_fresh_handle_on_the_remaining_graph(api, name):
    arrays = source_arrays(name)
    picked, rest = seeded_removal(arrays)
    a = api[0].from_arrays(*arrays)
    a.optimize(3)
    s = a.state()
    a.set_state(s)            # both handles get the SAME array through set_state, so that both hold the same bits
    before = a.state()
    a.remove_edges(np.concatenate([picked, picked[:2]]))   # a duplicate counts once
    assert np.array_equal(a.state(), before)               # across the call, bit for bit
    b = api[0].from_arrays(*rest)
    b.set_state(s)
    same_graph(a, b)
    ca, cb = a.global_error(), b.global_error()
    print(f"{name}: chi2 after the removal {ca:.12g}, fresh handle {cb:.12g}")
    np.testing.assert_allclose(ca, cb, rtol=1e-12)   # (the tolerance tests/test_extend_gpu.py gives a fresh handle at the same state)
    (ra, cola, oa, va, ba), (rb, colb, ob, vb, bb) = a.assemble(), b.assemble()
    assert np.array_equal(ra, rb) and np.array_equal(cola, colb) and np.array_equal(oa, ob)
    np.testing.assert_allclose(va, vb, rtol=1e-12, atol=1e-12 * float(np.max(np.abs(vb))))
    np.testing.assert_allclose(ba, bb, rtol=1e-12, atol=1e-12 * float(np.max(np.abs(bb))))
    a.optimize(3)   # the handle works


# ---- 3. what is carried
def test_robust_mask_priors_fixed_set_and_solver_are_carried(api):
    from priors_reference import random_priors
    PoseGraph, Solver = api
    arrays = source_arrays("intel")
    E = len(arrays[2])
    picked, rest = seeded_removal(arrays)
    keep = remaining(arrays, picked)[1]
    mask = (np.arange(E) % 3 != 0).astype(np.int32)
    node, meas, info = random_priors(np.random.default_rng(4), arrays, [5, 300, 900])
    fixed = [40, 41, 700]

    def dress(g, m):
        g.set_robust_kernel("cauchy", 1.0, m)
        g.set_priors(node, meas, info, robust=[1, 0, 1], keep_anchor=False)
        g.set_fixed(fixed, keep_anchor=False)

    a = PoseGraph.from_arrays(*arrays, solver=Solver.LevenbergMarquardt)
    dress(a, mask)
    s0, w0 = a.edge_errors()
    p0 = a.prior_errors()
    a.remove_edges(picked)
    s1, w1 = a.edge_errors()
    assert np.array_equal(s1, s0[keep]) and np.array_equal(w1, w0[keep])     # the survivors keep their weights: the mask was compacted
    assert np.all(w1[mask[keep] == 0] == 1.0) and np.any(w1[mask[keep] == 1] < 1.0)
    assert a.num_priors == 3 and all(np.array_equal(x, y) for x, y in zip(a.prior_errors(), p0))
    assert list(a.fixed_nodes()) == fixed
    b = PoseGraph.from_arrays(*rest, solver=Solver.LevenbergMarquardt)
    dress(b, mask[keep])
    assert a.global_error() == b.global_error()      # robust kernel, priors and both keep_anchor settings
    ea, na = a.optimize(4, return_norms=True)
    eb, nb = b.optimize(4, return_norms=True)
    assert np.array_equal(ea, eb) and np.array_equal(na, nb) and np.array_equal(a.state(), b.state())   # ... and Levenberg-Marquardt
    # an unmasked kernel stays unmasked
    c = PoseGraph.from_arrays(*arrays)
    c.set_robust_kernel("huber", 2.0)
    _, wc0 = c.edge_errors()
    c.remove_edges(picked)
    assert np.array_equal(c.edge_errors()[1], wc0[keep]) and np.any(wc0[keep] < 1.0)


def test_every_setting_at_once_through_extend_then_remove(api):
    """A handle dressed with every setting there is -- a masked kernel, priors with robust flags and keep_anchor off, a fixed
    set with keep_anchor off, both big-front switches -- goes through extend and then remove_edges of exactly the added edges.
    After the extend it is a fresh handle on the grown graph dressed alike, the mask extended by ones; after the removal it
    is the twin that was never rebuilt: every comparison is of bits.  A second pass reads the getters alone under truncated
    least squares, so that mu is seen to survive (delta as in tests/test_gnc_gpu.py's carry test; mu there is the last stage
    of a run, mu0 * 1.4^k: any such value does, the getter must return its bits)."""
    from extend_cases import closures_only
    from priors_reference import random_priors
    PoseGraph = api[0]
    c = closures_only("simulation-pose-landmark", K_EDGES)
    ek, ef, et, em, ei, _, _ = c.addition
    nk = np.asarray(c.base[0])
    poses, lms = np.flatnonzero(nk == 0), np.flatnonzero(nk == 1)
    node, meas, info = random_priors(np.random.default_rng(5), c.base, [int(poses[3]), int(poses[len(poses) // 2]), int(lms[0])])
    fixed = sorted(int(v) for v in (poses[10], poses[11], lms[-1]))
    mask = (np.arange(c.e_base) % 3 != 0).astype(np.int32)
    grown_mask = np.concatenate([mask, np.ones(K_EDGES, np.int32)])
    added = np.arange(c.e_base, c.e_base + K_EDGES)

    def dress(g, m, tls=None):
        if tls:
            g.set_robust_tls(*tls, m)
        else:
            g.set_robust_kernel("cauchy", 1.0, m)
        g.set_priors(node, meas, info, robust=[1, 0, 1], keep_anchor=False)
        g.set_fixed(fixed, keep_anchor=False)
        g.query_big_fronts = True
        g.marginals_big_fronts = True

    def told(g):
        """what the getters say, and what the settings do to the errors at the current state"""
        return (g.global_error(), *g.edge_errors(), *g.prior_errors(), np.array(g.robust_setting), g.num_priors, g.fixed_nodes(),
                g.query_big_fronts, g.marginals_big_fronts)

    def same(x, y):
        assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))

    a, twin, fresh = PoseGraph.from_arrays(*c.base), PoseGraph.from_arrays(*c.base), PoseGraph.from_arrays(*c.grown)
    dress(a, mask)
    dress(twin, mask)
    dress(fresh, grown_mask)
    a.optimize(2)
    s = a.state()
    for g in (a, twin, fresh):    # all three get the SAME array through set_state, so that all hold the same bits
        g.set_state(s)
    assert a.extend(ek, ef, et, em, ei) == (c.n_base, c.e_base)
    same_graph(a, fresh)
    ta = told(a)
    assert ta[5].tolist() == [2, 1.0, 0.0] and ta[6] == 3 and list(ta[7]) == fixed and ta[8] is True and ta[9] is True
    assert np.all(ta[2][:c.e_base][mask == 0] == 1.0) and np.any(ta[2] < 1.0) and np.any(ta[4] < 1.0) and ta[4][1] == 1.0
    same(ta, told(fresh))
    a.remove_edges(added)
    same_graph(a, twin)
    same(told(a), told(twin))
    ea, na = a.optimize(3, return_norms=True)
    eb, nb = twin.optimize(3, return_norms=True)
    assert np.array_equal(ea, eb) and np.array_equal(na, nb) and np.array_equal(a.state(), twin.state())
    assert np.all(np.isfinite(ea))
    # the getters and the errors alone (no iteration) under truncated least squares
    tls = (3.3682, 1.4 ** 9)
    t, t_twin, t_fresh = PoseGraph.from_arrays(*c.base), PoseGraph.from_arrays(*c.base), PoseGraph.from_arrays(*c.grown)
    dress(t, mask, tls)
    dress(t_twin, mask, tls)
    dress(t_fresh, grown_mask, tls)
    t.extend(ek, ef, et, em, ei)
    assert t.robust_setting == (3, *tls)
    same(told(t), told(t_fresh))
    t.remove_edges(added)
    assert t.robust_setting == (3, *tls)
    same(told(t), told(t_twin))


# ---- 4. the anchor
@pytest.mark.parametrize("name", ["triangle", "clique5", "landmarks-1-3"])
def test_anchor_moves_when_the_first_pose_pose_edge_goes(api, name):
    from check_edges_cases import arrays_of
    arrays = arrays_of(name)
    ek, ef = arrays[2], arrays[3]
    first = int(np.flatnonzero(ek != 1)[0])
    a = api[0].from_arrays(*arrays)
    assert a.anchor_node == int(ef[first])
    a.optimize(2)
    s = a.state()
    a.set_state(s)            # (the fresh handle below gets the same array: the same bits)
    before = a.state()
    rest, _ = remaining(arrays, [first])
    second = int(rest[3][np.flatnonzero(rest[2] != 1)[0]])
    assert second != int(ef[first]) and connected(rest)      # the rule gives another node, and the graph stays one component
    a.remove_edges([first])
    assert a.anchor_node == second and a.num_edges == len(ek) - 1
    assert np.array_equal(a.state(), before)
    b = api[0].from_arrays(*rest)
    b.set_state(s)
    same_graph(a, b)
    ea, eb = a.optimize(3), b.optimize(3)     # the 1e7 term sits on the new anchor in both
    assert np.array_equal(ea, eb) and np.array_equal(a.state(), b.state())


# ---- 5. refusals leave the handle alone
def test_a_refused_call_leaves_the_handle_as_it_was(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    L = _lib.load()
    arrays = source_arrays("simulation-pose-landmark")
    nk, ek, ef, et = arrays[0], arrays[2], arrays[3], arrays[4]
    E = len(ek)
    a, twin = api[0].from_arrays(*arrays), api[0].from_arrays(*arrays)
    a.optimize(2)
    twin.optimize(2)
    s0, chi0, st0, stream = a.state(), a.global_error(), a.stats(), a.stream_ptr()
    counts = lambda g: tuple(g.stats()[k] for k in ("n_graph_replays", "n_graph_captures", "n_plain_iterations"))   # noqa: E731
    c0 = counts(a)
    # a landmark seen once: removing its one sighting leaves it without any edge
    deg = np.bincount(np.concatenate([ef, et]), minlength=len(nk))
    lonely = [int(v) for v in np.flatnonzero((nk == 1) & (deg == 1))]
    if lonely:
        orphan_case = ([int(np.flatnonzero(et == lonely[0])[0])], f"node {lonely[0]}")
    else:   # every sighting of the least-seen landmark
        v = int(np.flatnonzero(nk == 1)[np.argmin(deg[nk == 1])])
        orphan_case = ([int(k) for k in np.flatnonzero(et == v)], f"node {v}")
    bad = {"index below range": ([0, -1], "entry 1"), "index beyond range": ([E], "entry 0"), "a node left without any edge": orphan_case}
    for label, (edges, word) in bad.items():
        with pytest.raises(PoseGraphError) as ei:
            a.remove_edges(edges)
        assert ei.value.code == _lib.EINVAL and "rr_pgo_remove_edges" in str(ei.value) and word in str(ei.value), (label, str(ei.value))
        assert a.num_edges == E and np.array_equal(a.state(), s0) and a.global_error() == chi0 and counts(a) == c0, label
    one = np.zeros(1, np.int32)
    for label, args in {"negative count": (-1, one.ctypes.data_as(C.POINTER(C.c_int32))), "null list": (1, None)}.items():
        assert L.rr_pgo_remove_edges(a._h, *args) == _lib.EINVAL and b"rr_pgo_remove_edges" in L.rr_pgo_last_error(), label
        assert a.num_edges == E and np.array_equal(a.state(), s0) and a.global_error() == chi0 and counts(a) == c0, label
    # the empty call changes nothing and rebuilds nothing
    t0 = a.remove_edges_times()
    a.remove_edges([])
    assert L.rr_pgo_remove_edges(a._h, 0, None) == _lib.OK
    assert a.num_edges == E and a.remove_edges_times() == t0 and a.stream_ptr() == stream and np.array_equal(a.state(), s0)
    assert {k: a.stats()[k] for k in STATS} == {k: st0[k] for k in STATS}
    ea, na = a.optimize(5, return_norms=True)
    eb, nb = twin.optimize(5, return_norms=True)
    assert np.array_equal(ea, eb) and np.array_equal(na, nb) and np.array_equal(a.state(), twin.state())


def test_sharded_handle_is_refused(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    arrays = source_arrays("simulation-pose-landmark")
    sh = api[0].from_arrays(*arrays, sharded=True)
    with pytest.raises(PoseGraphError) as ei:
        sh.remove_edges(seeded_removal(arrays)[0])
    assert ei.value.code == _lib.EUNSUPPORTED and "rr_pgo_remove_edges" in str(ei.value) and "sharded" in str(ei.value)
    assert sh.num_edges == len(arrays[2])


# ---- 6. single precision, and fronts beyond LDS
def test_f32_handle_and_sphere2500_remove_and_still_optimise(api):
    PoseGraph = api[0]
    arrays = source_arrays("intel")
    picked, rest = seeded_removal(arrays)
    a = PoseGraph.from_arrays(*arrays, precision="f32")
    a.optimize(2)
    s = a.state()
    a.remove_edges(picked)
    assert np.array_equal(a.state(), s)
    same_graph(a, PoseGraph.from_arrays(*rest, precision="f32"))
    e = a.optimize(3)
    assert np.all(np.isfinite(e)) and e[-1] <= e[0]
    g = PoseGraph.new(g2o_path("sphere2500"))
    assert g.stats()["n_big_fronts"] > 0   # fronts beyond LDS: what this case is for
    sph = g.graph_arrays()
    picked, rest = seeded_removal(sph, count=3)
    g.optimize(2)
    s = g.state()
    g.remove_edges(picked)
    assert np.array_equal(g.state(), s) and g.num_edges == len(sph[2]) - 3
    same_graph(g, PoseGraph.from_arrays(*rest))
    e = g.optimize(3)
    assert np.all(np.isfinite(e)) and e[-1] <= e[0]
