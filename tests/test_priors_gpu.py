"""rr_pgo_set_priors on the GPU against tests/priors_reference.py (the unchanged oracle on the graph augmented by a fixed
identity node): the assembled system, the cost, Gauss-Newton and Levenberg-Marquardt trajectories, the factor queries, and
the lifecycle of the prior list (replace, clear, refuse, extend, repeat)."""
import ctypes as C

import numpy as np
import pytest

from conftest import g2o_path
from covariances_cases import FLOOR_MAX
from oracle.oracle import OracleGraph
from priors_reference import PriorsReference, random_priors, rel_diff, tolerance
from random_graphs import random_graph
from robust_reference import oracle_arrays

pytestmark = pytest.mark.gpu

INFO_LEN = {0: 6, 1: 3, 2: 21}
NODE_DIM = {0: 3, 1: 2, 2: 6}
# The assembled system.  f64: the figures of the robust-kernel tests (1e-12 of max|vals| for the blocks, 1e-11 for b).
# mixed: the same arithmetic in f64 and ONE rounding to f32 where a value is stored (half an ulp, 2^-24, of the value).
# f32: every operation of the f64 bound rounds at 2^-24 instead of 2^-53, so the f64 figures scale by 2^29.
EPS32 = 2.0 ** -24
SYSTEM_TOL = {"f64": (1e-12, 1e-11), "mixed": (1e-12 + EPS32, 1e-11 + EPS32), "f32": (1e-12 * 2.0 ** 29, 1e-11 * 2.0 ** 29)}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver, PoseGraphError
    return PoseGraph, PoseGraphSolver, PoseGraphError


def small_graph(dim):
    if dim == "se2":
        return random_graph(np.random.default_rng(21), n_pose=14, n_lm=5, n_extra=10)
    return random_graph(np.random.default_rng(22), n_pose=12, n_lm=0, n_extra=8, se3=True)


def query_graph(dim):
    """28 / 26 nodes: gate_cases.candidates draws 24 seeded nodes"""
    if dim == "se2":
        return random_graph(np.random.default_rng(23), n_pose=22, n_lm=6, n_extra=14)
    return random_graph(np.random.default_rng(24), n_pose=26, n_lm=0, n_extra=14, se3=True)


def anchor_of(arrays):
    return int(arrays[3][np.flatnonzero(arrays[2] != 1)[0]])


def shape_nodes(shape, arrays):
    n = len(arrays[0])
    anchor = anchor_of(arrays)
    return {"pose": [7 if anchor != 7 else 6], "landmark": [n - 1], "anchor": [anchor], "every": list(range(n)),
            "nine": [3] * 9}[shape]   # nine: one more than LIN_GROUP, the strided loop wraps


SHAPES = [("se2", s, k) for s in ("pose", "landmark", "anchor", "every", "nine") for k in (1, 0) if not (s == "landmark" and k == 0)] + \
         [("se3", s, k) for s in ("pose", "anchor", "every", "nine") for k in (1, 0)]   # (a landmark prior alone fixes no gauge)


def assert_same_system(label, g, ref, lm, precision, keep_anchor):
    """the rule of the robust-kernel tests' system comparison, restated: blocks at tb * max|vals|, b against its own scale and
    the system's"""
    tb, tr = SYSTEM_TOL[precision]
    lam = 0.37 if lm else 0.0
    br, bc, bo, vals, b = g.assemble(lam, lm)
    H, b2 = ref.system(lam, lm)
    scale = np.abs(H).max()
    # dense from the block list (parallel edges have a block each: they add), compared entry by entry; every entry of the
    # reference outside the stored blocks must be zero: the pattern did not change
    G = np.zeros_like(H)
    for r, c, o in zip(br, bc, bo):
        blk = vals[o:o + ref.dims[r] * ref.dims[c]].reshape(ref.dims[r], ref.dims[c])
        G[np.ix_(ref.scalars(r), ref.scalars(c))] += blk
        if r != c:
            G[np.ix_(ref.scalars(c), ref.scalars(r))] += blk.T
    worst = float(np.abs(G - H).max())
    bscale = max(np.abs(b2).max(), 1e-3 * np.sqrt(scale))
    print(f"{label} lm={lm}: blocks worst {worst:.3g} (bound {tb * scale:.3g}), b worst {np.abs(b - b2).max():.3g} (bound {tr * bscale:.3g}), max|vals| {vals.max():.3g}")
    assert worst <= tb * scale
    assert np.abs(b - b2).max() <= tr * bscale
    if keep_anchor:
        assert vals.max() > 1e7      # the anchor term is there
    else:
        assert vals.max() < 1e7      # ... and here it is not


# ---- 1. the assembled system ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,shape,keep", SHAPES)
def test_assembled_system_equals_the_reference_system(api, dim, shape, keep):
    arrays = small_graph(dim)
    node, meas, info = random_priors(np.random.default_rng(5), arrays, shape_nodes(shape, arrays))
    ref = PriorsReference(arrays, node, meas, info, keep_anchor=keep)
    for precision in ("f64", "mixed", "f32"):
        g = api[0].from_arrays(*arrays, precision=precision)
        g.set_priors(node, meas, info, keep_anchor=bool(keep))
        assert g.num_priors == len(node)
        for lm in (False, True):
            assert_same_system(f"{dim} {shape} keep_anchor={keep} {precision}", g, ref, lm, precision, keep)


@pytest.mark.parametrize("dim", ["se2", "se3"])
@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_assembled_system_with_a_kernel_and_a_mix_of_robust_flags(api, dim, kind):
    arrays = small_graph(dim)
    n = len(arrays[0])
    node, meas, info = random_priors(np.random.default_rng(6), arrays, list(range(n)) + [3, 3], noise=0.4)
    flags = (np.arange(len(node)) % 2).astype(np.int32)
    ref = PriorsReference(arrays, node, meas, info, robust=flags, kind=kind, delta=1.0)
    g = api[0].from_arrays(*arrays)
    g.set_robust_kernel(kind, 1.0)
    g.set_priors(node, meas, info, robust=flags)
    for lm in (False, True):
        assert_same_system(f"{dim} {kind}", g, ref, lm, "f64", 1)


# ---- 2. the cost ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", ["se2", "se3"])
@pytest.mark.parametrize("kind", [None, "huber", "cauchy"])
def test_cost_and_prior_errors(api, dim, kind):
    arrays = small_graph(dim)
    n = len(arrays[0])
    node, meas, info = random_priors(np.random.default_rng(7), arrays, list(range(n)) + [3] * 9, noise=0.4)
    flags = (np.arange(len(node)) % 2).astype(np.int32)
    ref = PriorsReference(arrays, node, meas, info, robust=flags, kind=kind, delta=1.0)
    g = api[0].from_arrays(*arrays)
    if kind:
        g.set_robust_kernel(kind, 1.0)
    g.set_priors(node, meas, info, robust=flags)
    s, w = g.prior_errors()
    s2, w2 = ref.prior_errors()
    chi, chi2 = g.global_error(), ref.cost()
    print(f"{dim} {kind}: chi2 {chi:.15g} against {chi2:.15g}; s worst {np.abs(s / s2 - 1).max():.3g}, w worst {np.abs(w / w2 - 1).max():.3g}")
    np.testing.assert_allclose(chi, chi2, rtol=1e-12)
    np.testing.assert_allclose(s, s2, rtol=1e-12)
    np.testing.assert_allclose(w, w2, rtol=1e-12)
    assert np.all(w[flags == 0] == 1.0)           # unflagged priors keep w = 1
    if kind:
        assert np.any(w[flags == 1] < 1.0)
    else:
        assert np.all(w == 1.0)
    # the edges' list stays edges-only
    assert len(g.edge_errors()[0]) == g.num_edges
    # optimize()'s last entry is a chi2-only launch: it counts the priors too
    errors = g.optimize(1)
    np.testing.assert_allclose(errors[0], chi2, rtol=1e-12)
    np.testing.assert_allclose(errors[-1], g.global_error(), rtol=1e-13)


# ---- 3. trajectories --------------------------------------------------------------------------------------------------

def assert_same_trajectory(label, g, ref, iters, lm):
    eg = np.array(g.optimize(iters))
    eo, _ = ref.optimize(iters, lm)
    sg, so = g.state(), ref.state()
    print(f"{label}: {eg} against {eo}; state worst {np.abs(sg - so).max():.3g}")
    assert len(eg) == len(eo)
    np.testing.assert_allclose(eg, eo, rtol=1e-7)
    np.testing.assert_allclose(sg, so, rtol=0, atol=1e-6)   # (the figure of the parity tests' trajectory states)


@pytest.mark.parametrize("dim", ["se2", "se3"])
@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
@pytest.mark.parametrize("keep", [1, 0])
def test_small_graph_trajectories(api, dim, solver, keep):
    arrays = small_graph(dim)
    n = len(arrays[0])
    node, meas, info = random_priors(np.random.default_rng(8), arrays, [2, 9, 9, n - 1], noise=0.3)
    g = api[0].from_arrays(*arrays, solver=api[1][solver])
    g.set_priors(node, meas, info, keep_anchor=bool(keep))
    ref = PriorsReference(arrays, node, meas, info, keep_anchor=keep)
    assert_same_trajectory(f"{dim} {solver} keep_anchor={keep}", g, ref, 8, solver == "LevenbergMarquardt")


def test_small_graph_trajectory_with_huber_and_flagged_priors(api):
    arrays = small_graph("se2")
    node, meas, info = random_priors(np.random.default_rng(9), arrays, [2, 9, 9, 5], noise=0.5)
    flags = [1, 0, 1, 1]
    g = api[0].from_arrays(*arrays)
    g.set_robust_kernel("huber", 1.0)
    g.set_priors(node, meas, info, robust=flags, keep_anchor=False)
    ref = PriorsReference(arrays, node, meas, info, robust=flags, keep_anchor=False, kind="huber", delta=1.0)
    assert_same_trajectory("se2 huber", g, ref, 8, False)


def gps_priors(arrays, count, seed, sigma=0.1):
    """`count` seeded pose nodes of a file: z = the position of the oracle's optimum + N(0, sigma) and its heading,
    Omega = diag(100, 100, 1) (SE(3): diag(100 x 3, 1 x 3))"""
    o = OracleGraph.from_arrays(*arrays)
    o.optimize(10)
    opt = list(arrays)
    opt[1] = o.state()
    rng = np.random.default_rng(seed)
    poses = np.flatnonzero(np.asarray(arrays[0]) != 1)
    nodes = sorted(int(v) for v in rng.choice(poses, count, replace=False))
    node, meas, _ = random_priors(rng, opt, nodes, at_state=True)
    se3 = arrays[0][nodes[0]] == 2
    per = 7 if se3 else 3
    meas = meas.reshape(-1, per)
    meas[:, :3 if se3 else 2] += rng.normal(scale=sigma, size=(count, 3 if se3 else 2))
    W = np.diag([100.0] * 3 + [1.0] * 3) if se3 else np.diag([100.0, 100.0, 1.0])
    d = 6 if se3 else 3
    return node, meas.ravel(), np.tile(W[np.triu_indices(d)], count)


def test_intel_with_forty_gps_priors_and_no_anchor(api):
    arrays = oracle_arrays(OracleGraph.load(g2o_path("intel")))
    node, meas, info = gps_priors(arrays, 40, 41)
    g = api[0].from_arrays(*arrays)
    g.set_priors(node, meas, info, keep_anchor=False)
    ref = PriorsReference(arrays, node, meas, info, keep_anchor=False)
    assert_same_trajectory("intel 40 priors", g, ref, 4, False)


def test_parking_garage_with_ten_priors(api):
    arrays = oracle_arrays(OracleGraph.load(g2o_path("parking-garage")))
    node, meas, info = gps_priors(arrays, 10, 42)
    g = api[0].from_arrays(*arrays)
    g.set_priors(node, meas, info)
    ref = PriorsReference(arrays, node, meas, info)
    assert_same_trajectory("parking-garage 10 priors", g, ref, 3, False)


def f32_against_f64(label, api, arrays, node, meas, info, keep, iters, tol_min):
    """the rule of the parity tests for single-precision trajectories: the first error to 1e-5, the minimum to tol_min"""
    g32 = api[0].from_arrays(*arrays, precision="f32")
    g64 = api[0].from_arrays(*arrays)
    for g in (g32, g64):
        g.set_priors(node, meas, info, keep_anchor=keep)
    assert g32.stats()["n_big_fronts"] > 0
    e32, e64 = g32.optimize(iters), g64.optimize(iters)
    print(f"{label}: f32 {e32} f64 {e64}")
    assert abs(e32[0] - e64[0]) <= 1e-5 * e64[0]
    assert abs(min(e32) - e64[-1]) <= tol_min * e64[-1]
    return g32, g64


def test_sphere2500_f32_with_five_priors(api):
    """fronts beyond LDS in single precision, five priors, no anchor term"""
    PoseGraph = api[0]
    arrays = PoseGraph.new(g2o_path("sphere2500")).graph_arrays()
    h = PoseGraph.from_arrays(*arrays)
    h.optimize(8)
    opt = list(arrays)
    opt[1] = h.state()
    rng = np.random.default_rng(43)
    nodes = sorted(int(v) for v in rng.choice(len(arrays[0]), 5, replace=False))
    node, meas, _ = random_priors(rng, opt, nodes, noise=0.01)
    info = np.tile((100.0 * np.eye(6))[np.triu_indices(6)], 5)
    f32_against_f64("sphere2500", api, arrays, node, meas, info, False, 8, 1e-5)


@pytest.mark.parametrize("keep", [1, 0])
def test_lattice_f32_gauge_transfer_is_off_with_priors(api, keep):
    """An SE(2) graph whose single-precision Gauss-Newton steps use the gauge transfer (a big root front): with priors the
    system is the one with the priors (and with the 1e7 term under keep_anchor), not the gauge term's.  keep_anchor = 1 puts
    1e7 into a single-precision factor: the minimum is asked to 1e-4, the figure of the parity test that does the same."""
    from rustrobotics_amd import synthetic_grid_arrays
    arrays = synthetic_grid_arrays(60, 40)
    h = api[0].from_arrays(*arrays)
    h.optimize(6)
    opt = list(arrays)
    opt[1] = h.state()
    rng = np.random.default_rng(44)
    nodes = sorted(int(v) for v in rng.choice(len(arrays[0]), 5, replace=False))
    node, meas, _ = random_priors(rng, opt, nodes, noise=0.05)
    info = np.tile(np.diag([100.0, 100.0, 1.0])[np.triu_indices(3)], 5)
    g32, g64 = f32_against_f64(f"lattice60x40 keep_anchor={keep}", api, arrays, node, meas, info, bool(keep), 6, 1e-4 if keep else 1e-5)
    # the assembled single-precision system is the reference's (assemble() never uses the gauge term; the trajectory above does
    # not either, or the priors' pull on the gauge would be counted twice and the minimum missed)
    s32, s64 = g32.prior_errors()[0], g64.prior_errors()[0]
    print(f"prior errors f32 {s32} f64 {s64}")
    assert np.abs(s32 - s64).max() <= 1e-3 * max(s64.max(), 1.0)


# ---- 4. the queries see the priors -----------------------------------------------------------------------------------------

def check(label, what, got, want, floor):
    worst = max(rel_diff(g, w) for g, w in zip(got, want))
    tol = tolerance(floor)
    print(f"{label} {what}: {len(want)} values, worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert len(got) == len(want)
    assert floor <= FLOOR_MAX, (label, what, floor)
    assert worst <= tol, (label, what, worst, tol)


@pytest.mark.parametrize("dim", ["se2", "se3"])
@pytest.mark.parametrize("keep", [1, 0])
def test_marginals_covariances_and_gate_with_priors(api, dim, keep):
    from gate_cases import candidates
    arrays = query_graph(dim)
    n = len(arrays[0])
    node, meas, info = random_priors(np.random.default_rng(10), arrays, [4, 11, 11, n - 1, 17], noise=0.2)
    g = api[0].from_arrays(*arrays)
    g.optimize(3)
    plain = g.marginals()
    g.set_priors(node, meas, info, keep_anchor=bool(keep))
    st = g.state()
    ref = PriorsReference(arrays, node, meas, info, keep_anchor=keep)
    ref.set_state(st)
    sig = ref.sigma_pair()
    label = f"{dim} keep_anchor={keep}"
    want, floor = ref.blocks(list(range(n)), sig=sig)
    got = g.marginals()
    check(label, "marginals", got, want, floor)
    assert max(rel_diff(a, b) for a, b in zip(got, plain)) > 1e-3      # the priors are part of the inverted matrix
    rng = np.random.default_rng(11)
    a, b = rng.integers(0, n, 30).astype(np.int32), rng.integers(0, n, 30).astype(np.int32)
    vals, off = g.covariance_blocks(a, b)
    want, floor = ref.blocks(a, b, sig=sig)
    got = [vals[off[q]:off[q + 1]].reshape(w.shape) for q, w in enumerate(want)]
    check(label, "covariance blocks", got, want, floor)
    cand = candidates(arrays, st)
    S, d2, chi2, fS, fd = ref.gate(cand, sig=sig)
    gd2, gchi2, gS = g.gate_edges(*cand, return_innovation=True)
    check(label, "gate d2", [np.array([v]) for v in gd2], [np.array([v]) for v in d2], fd)
    check(label, "gate S", gS, S, fS)
    np.testing.assert_allclose(gchi2, chi2, rtol=1e-9)


@pytest.mark.parametrize("dim", ["se2", "se3"])
def test_strong_prior_on_a_far_pose_shrinks_its_marginal(api, dim):
    arrays = query_graph(dim)
    g = api[0].from_arrays(*arrays)
    g.optimize(3)
    before = g.marginals()
    poses = np.flatnonzero(np.asarray(arrays[0]) != 1)
    far = int(poses[np.argmax([np.trace(before[v]) for v in poses])])
    opt = list(arrays)
    opt[1] = g.state()
    node, meas, _ = random_priors(np.random.default_rng(12), opt, [far], at_state=True)
    d = NODE_DIM[int(arrays[0][far])]
    g.set_priors(node, meas, (1e6 * np.eye(d))[np.triu_indices(d)])
    after = g.marginals()
    print(f"{dim}: node {far}, trace of its marginal {np.trace(before[far]):.3g} -> {np.trace(after[far]):.3g}")
    assert np.trace(after[far]) < np.trace(before[far])
    assert np.all(np.diag(after[far]) < np.diag(before[far]))


# ---- 5. lifecycle ---------------------------------------------------------------------------------------------------------

def same_bits(a, b, iters=0):
    assert a.global_error() == b.global_error()
    for x, y in zip(a.assemble(), b.assemble()):
        assert np.array_equal(x, y)
    if iters:
        assert np.array_equal(np.array(a.optimize(iters)), np.array(b.optimize(iters)))
    assert np.array_equal(a.state(), b.state())


@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
def test_set_then_clear_is_a_handle_that_never_had_priors(api, solver, monkeypatch):
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    a = api[0].new(g2o_path("simulation-pose-landmark"), api[1][solver])
    b = api[0].new(g2o_path("simulation-pose-landmark"), api[1][solver])
    monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    for g in (a, b):
        g.iterate_async(2)
        g.sync()
        assert g.stats()["n_graph_replays"] == 2 and g.stats()["n_plain_iterations"] == 0   # the captured graph really ran
    arrays = a.graph_arrays()
    node, meas, info = random_priors(np.random.default_rng(13), arrays, [0, 5, 5, len(arrays[0]) - 1], noise=0.3)
    a.set_priors(node, meas, info, robust=[1, 0, 1, 0], keep_anchor=False)
    assert a.num_priors == 4 and a.global_error() != b.global_error()
    a.linearize_and_solve()
    a.clear_priors()
    assert a.num_priors == 0 and len(a.prior_errors()[0]) == 0
    assert a.stats()["bytes_linearize"] == b.stats()["bytes_linearize"]
    same_bits(a, b, 10)


def test_second_call_replaces_the_first(api):
    arrays = small_graph("se2")
    a, b = api[0].from_arrays(*arrays), api[0].from_arrays(*arrays)
    first = random_priors(np.random.default_rng(14), arrays, list(range(len(arrays[0]))), noise=0.3)
    second = random_priors(np.random.default_rng(15), arrays, [1, 8], noise=0.3)
    a.set_priors(*first, keep_anchor=False)
    a.set_priors(*second)
    b.set_priors(*second)
    assert a.num_priors == b.num_priors == 2
    assert np.array_equal(a.prior_errors()[0], b.prior_errors()[0])
    assert a.stats()["bytes_linearize"] == b.stats()["bytes_linearize"] > api[0].from_arrays(*arrays).stats()["bytes_linearize"]
    same_bits(a, b, 5)


@pytest.mark.parametrize("dim", ["se2", "se3"])
def test_every_refusal_names_the_prior_and_changes_nothing(api, dim):
    from rustrobotics_amd import _lib
    arrays = small_graph(dim)
    n = len(arrays[0])
    a, b = api[0].from_arrays(*arrays), api[0].from_arrays(*arrays)
    good = random_priors(np.random.default_rng(16), arrays, [2, 6], noise=0.3)
    for g in (a, b):
        g.set_priors(*good, keep_anchor=False)
    node, meas, info = random_priors(np.random.default_rng(17), arrays, [1, 4, 7], noise=0.3)
    per_m, per_i = (7, 21) if dim == "se3" else (3, 6)

    def broken(what):
        nd, m, w = node.copy(), meas.copy(), info.copy()
        if what == "node":
            nd[1] = n
        elif what == "negative node":
            nd[1] = -1
        elif what == "nan":
            m[per_m + 1] = np.nan
        elif what == "inf":
            w[per_i + 2] = np.inf
        elif what == "indefinite":
            w[per_i:2 * per_i] *= -1.0
        elif what == "quaternion":
            m[per_m + 3:per_m + 7] = 0.0
        return nd, m, w

    cases = ["node", "negative node", "nan", "inf", "indefinite"] + (["quaternion"] if dim == "se3" else [])
    for what in cases:
        with pytest.raises(api[2]) as ei:
            a.set_priors(*broken(what))
        print(what, "->", ei.value)
        assert ei.value.code == _lib.EINVAL and "prior 1" in str(ei.value), (what, ei.value)
        assert a.num_priors == 2
    L = _lib.load()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    pn, pm, pw = node.ctypes.data_as(ip), meas.ctypes.data_as(dp), info.ctypes.data_as(dp)
    assert L.rr_pgo_set_priors(a._h, -1, pn, pm, pw, None, 1) == _lib.EINVAL
    for args in ((None, pm, pw), (pn, None, pw), (pn, pm, None)):
        assert L.rr_pgo_set_priors(a._h, 3, *args, None, 1) == _lib.EINVAL
    assert a.num_priors == 2
    assert np.array_equal(a.prior_errors()[0], b.prior_errors()[0])
    same_bits(a, b, 5)


def test_sharded_and_edge_parallel_handles_are_unsupported(api, monkeypatch):
    from rustrobotics_amd import _lib
    PoseGraph = api[0]
    arrays = small_graph("se2")
    monkeypatch.setenv("RR_PGO_EDGE_LINEARIZE", "1")
    edge_form = PoseGraph.from_arrays(*arrays)
    monkeypatch.delenv("RR_PGO_EDGE_LINEARIZE")
    twin = PoseGraph.from_arrays(*arrays)
    handles = {"sharded": PoseGraph.from_arrays(*arrays, sharded=True), "RR_PGO_EDGE_LINEARIZE=1": edge_form}
    prior = random_priors(np.random.default_rng(18), arrays, [2])
    for what, h in handles.items():
        with pytest.raises(api[2]) as ei:
            h.set_priors(*prior)
        print(what, "->", ei.value)
        assert ei.value.code == _lib.EUNSUPPORTED, (what, ei.value)
        assert h.num_priors == 0
    np.testing.assert_allclose(edge_form.global_error(), twin.global_error(), rtol=1e-12)


def test_extend_carries_priors_flags_and_keep_anchor(api):
    from extend_cases import case
    c = case("simulation-pose-landmark")
    rng = np.random.default_rng(19)
    nodes = [int(v) for v in rng.choice(c.n_base, 6, replace=False)] + [3, 3]
    node, meas, info = random_priors(rng, c.base, nodes, noise=0.3)
    flags = (np.arange(len(node)) % 2).astype(np.int32)
    a = api[0].from_arrays(*c.base)
    a.set_robust_kernel("huber", 1.0)
    a.set_priors(node, meas, info, robust=flags, keep_anchor=False)
    a.optimize(2)
    edges, new_nodes = c.extend_args()
    a.extend(*edges, **new_nodes)
    b = api[0].from_arrays(*c.grown)
    b.set_robust_kernel("huber", 1.0)
    b.set_priors(node, meas, info, robust=flags, keep_anchor=False)
    assert a.num_priors == b.num_priors == len(node)
    assert a.stats()["bytes_linearize"] == b.stats()["bytes_linearize"]
    st = a.state()
    a.set_state(st)
    b.set_state(st)
    sa, wa = a.prior_errors()
    sb, wb = b.prior_errors()
    assert np.array_equal(sa, sb) and np.array_equal(wa, wb) and np.all(wa[flags == 0] == 1.0)
    br, bc, bo, vals, _ = a.assemble()
    assert vals.max() < 1e7          # keep_anchor = 0 came along
    same_bits(a, b, 5)


@pytest.mark.parametrize("dim", ["se2", "se3"])
def test_two_runs_give_identical_bits(api, dim):
    arrays = small_graph(dim)
    n = len(arrays[0])
    node, meas, info = random_priors(np.random.default_rng(20), arrays, list(range(n)) + [3] * 9, noise=0.3)
    a, b = api[0].from_arrays(*arrays), api[0].from_arrays(*arrays)
    for g in (a, b):
        g.set_priors(node, meas, info, keep_anchor=False)
    same_bits(a, b, 6)
    assert np.array_equal(a.prior_errors()[0], b.prior_errors()[0])
