"""rr_pgo_set_fixed on the GPU against tests/fixed_reference.py (the unchanged oracle's system with the rows and columns of the
fixed nodes deleted) and against an identical handle without a fixed set: the assembled system bit for bit, the step, Gauss-
Newton and Levenberg-Marquardt trajectories, a frozen map, single-precision handles with fronts beyond LDS, the factor
queries (conditional on the fixed nodes), the launch forms, and the lifecycle of the set."""
import ctypes as C

import numpy as np
import pytest

from conftest import g2o_path
from covariances_cases import FLOOR_MAX
from fixed_reference import FixedReference, rel_diff, tolerance
from oracle.oracle import OracleGraph
from priors_reference import random_priors
from random_graphs import random_graph
from robust_reference import oracle_arrays

pytestmark = pytest.mark.gpu

NODE_DIM = {0: 3, 1: 2, 2: 6}
STATE_LEN = {0: 3, 1: 2, 2: 7}
# The assembled system against the reference: SYSTEM_TOL and the rule of assert_same_system in tests/test_priors_gpu.py,
# restated.  f64: 1e-12 of max|vals| for the blocks, 1e-11 for b.  mixed: the same arithmetic in f64 and ONE rounding to f32
# where a value is stored (half an ulp, 2^-24).  f32: every operation rounds at 2^-24 instead of 2^-53: the figures scale by 2^29.
EPS32 = 2.0 ** -24
SYSTEM_TOL = {"f64": (1e-12, 1e-11), "mixed": (1e-12 + EPS32, 1e-11 + EPS32), "f32": (1e-12 * 2.0 ** 29, 1e-11 * 2.0 ** 29)}
# The first step against the reference's reduced solve: the figures test_gpu_parity.py holds random_graph graphs to
# (test_random_ragged_graphs_match_the_oracle: 1e-8 of max(1, |dx|); test_random_se3_graphs_match_the_oracle: 1e-7).  The
# robust-kernel and priors GPU tests state no bound of their own for dx; their graphs are of this family.
DX_TOL = {"se2": 1e-8, "se3": 1e-7}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver, PoseGraphError
    return PoseGraph, PoseGraphSolver, PoseGraphError


def small_graph(dim):
    """the small graphs of tests/test_priors_gpu.py"""
    if dim == "se2":
        return random_graph(np.random.default_rng(21), n_pose=14, n_lm=5, n_extra=10)
    return random_graph(np.random.default_rng(22), n_pose=12, n_lm=0, n_extra=8, se3=True)


def query_graph(dim):
    """the query graphs of tests/test_priors_gpu.py: 28 / 26 nodes"""
    if dim == "se2":
        return random_graph(np.random.default_rng(23), n_pose=22, n_lm=6, n_extra=14)
    return random_graph(np.random.default_rng(24), n_pose=26, n_lm=0, n_extra=14, se3=True)


def hub_graph(dim):
    """7 poses and 18 loop closures: node 2 has 12 (SE(2)) and 10 (SE(3)) incidences, more than the 8 lanes of its group"""
    return random_graph(np.random.default_rng(31 if dim == "se2" else 32), n_pose=7, n_lm=2 if dim == "se2" else 0, n_extra=18, se3=dim == "se3")


def anchor_of(arrays):
    return int(arrays[3][np.flatnonzero(arrays[2] != 1)[0]])


def degrees(arrays):
    return np.bincount(np.concatenate([arrays[3], arrays[4]]), minlength=len(arrays[0]))


def state_offsets(arrays):
    return np.concatenate([[0], np.cumsum([STATE_LEN[int(k)] for k in arrays[0]])]).astype(int)


def state_of(arrays, state, nodes):
    so = state_offsets(arrays)
    return np.concatenate([state[so[v]:so[v + 1]] for v in nodes]) if len(nodes) else np.zeros(0)


def scalars_of(arrays, nodes):
    off = np.concatenate([[0], np.cumsum([NODE_DIM[int(k)] for k in arrays[0]])]).astype(int)
    return np.concatenate([np.arange(off[v], off[v + 1]) for v in nodes]).astype(int) if len(nodes) else np.zeros(0, int)


# ---- 1. the system, bit for bit -----------------------------------------------------------------------------------------

# shape -> (graph, F, keep_anchor).  keep_anchor = 0 only where F holds the from-node of a pose-pose edge (the reference)
def shape_case(dim, shape):
    arrays = hub_graph(dim) if shape == "hub" else small_graph(dim)
    n = len(arrays[0])
    anchor = anchor_of(arrays)
    k = int(np.flatnonzero((arrays[2] != 1) & (arrays[3] != anchor) & (arrays[4] != anchor))[2])    # a pose-pose edge off the anchor
    edge = [int(arrays[3][k]), int(arrays[4][k])]
    F, keep = {"pose": ([7 if anchor != 7 else 6], 1), "landmark": ([n - 1], 1), "anchor": ([anchor], 1), "anchor, term dropped": ([anchor], 0),
               "edge": (edge, 1), "edge, term dropped": (edge, 0), "hub": ([2], 1),
               "all but one": ([v for v in range(n) if v != 5], 1), "every": (list(range(n)), 0)}[shape]
    return arrays, F, keep


SE3_SHAPES = ("pose", "anchor", "anchor, term dropped", "edge", "edge, term dropped", "hub", "all but one", "every")
SHAPES = [("se2", s) for s in SE3_SHAPES + ("landmark",)] + [("se3", s) for s in SE3_SHAPES]


def overwritten(asm, arrays, F, take=None):
    """assemble() of the unfixed handle with the entries rr_pgo_set_fixed defines overwritten: diagonal blocks of F -> I,
    blocks touching F -> 0, b at F -> 0.  take = (node, asm of the fixed handle): that node's diagonal block is taken from
    the fixed handle (the anchor's, where the two handles differ by the 1e7 term)"""
    br, bc, bo, vals, b = [np.array(x) for x in asm]
    dims = [NODE_DIM[int(k)] for k in arrays[0]]
    Fs = set(F)
    for r, c, o in zip(br, bc, bo):
        if r in Fs or c in Fs:
            vals[o:o + dims[r] * dims[c]] = np.eye(dims[r]).ravel() if r == c else 0.0
        elif take is not None and r == c == take[0]:
            vals[o:o + dims[r] * dims[c]] = take[1][3][o:o + dims[r] * dims[c]]
    b[scalars_of(arrays, sorted(Fs))] = 0.0
    return br, bc, bo, vals, b


def assert_same_system(label, asm, ref, lam, lm, precision):
    """the rule of tests/test_priors_gpu.py: the blocks summed into a dense matrix (parallel edges have a block each),
    compared entry by entry at tb * max|H|; b against its own scale and the system's"""
    tb, tr = SYSTEM_TOL[precision]
    br, bc, bo, vals, b = asm
    H, b2 = ref.expected_system(lam, lm)
    scale = np.abs(H).max()
    G = np.zeros_like(H)
    for r, c, o in zip(br, bc, bo):
        blk = vals[o:o + ref.dims[r] * ref.dims[c]].reshape(ref.dims[r], ref.dims[c])
        G[np.ix_(ref.scalars(r), ref.scalars(c))] += blk
        if r != c:
            G[np.ix_(ref.scalars(c), ref.scalars(r))] += blk.T
    worst = float(np.abs(G - H).max())
    bscale = max(np.abs(b2).max(), 1e-3 * np.sqrt(scale))
    print(f"{label}: blocks worst {worst:.3g} (bound {tb * scale:.3g}), b worst {np.abs(b - b2).max():.3g} (bound {tr * bscale:.3g})")
    assert worst <= tb * scale
    assert np.abs(b - b2).max() <= tr * bscale


@pytest.mark.parametrize("dim,shape", SHAPES)
def test_assembled_system_is_the_unfixed_one_with_identity_rows(api, dim, shape):
    """f64 / mixed / f32, lambda 0 and 0.37, plain and under a Cauchy kernel, without priors and with a list that holds two
    priors on a fixed node: the fixed handle's assemble() equals, bit for bit, that of an identical unfixed handle at the same
    state with the entries of F overwritten; and the same system against the reference."""
    arrays, F, keep = shape_case(dim, shape)
    n = len(arrays[0])
    anchor = anchor_of(arrays)
    if shape == "hub":
        assert degrees(arrays)[2] > 8
    prior_nodes = [F[0], F[0], 4 if 4 not in F else 5, n - 1]
    priors = random_priors(np.random.default_rng(50), arrays, prior_nodes, noise=0.3)
    variants = {"plain": (None, None), "cauchy": ("cauchy", None), "priors": (None, priors), "cauchy + priors": ("cauchy", priors)}
    refs = {v: FixedReference(arrays, F, keep_anchor=keep, priors=p, kind=k, delta=1.0) for v, (k, p) in variants.items()}
    # under keep_anchor = 0 with a free anchor the two handles differ in the anchor's own block by the 1e7 term
    differs = anchor if (not keep and anchor not in F) else None
    for precision in ("f64", "mixed", "f32"):
        for variant, (kind, pr) in variants.items():
            g, u = api[0].from_arrays(*arrays, precision=precision), api[0].from_arrays(*arrays, precision=precision)
            for h in (g, u):
                if kind:
                    h.set_robust_kernel(kind, 1.0)
                if pr is not None:
                    h.set_priors(*pr)
            g.set_fixed(F, keep_anchor=bool(keep))
            assert g.num_fixed == len(set(F)) and g.fixed_nodes().tolist() == sorted(set(F))
            assert g.global_error() == u.global_error()     # chi2 is unchanged: every edge and every prior counts
            if pr is not None:
                assert np.array_equal(g.prior_errors()[0], u.prior_errors()[0])
            for lm in (False, True):
                lam = 0.37 if lm else 0.0
                label = f"{dim} {shape} {precision} {variant} lm={lm}"
                got = g.assemble(lam, lm)
                want = overwritten(u.assemble(lam, lm), arrays, F, None if differs is None else (differs, got))
                for name, x, y in zip(("rows", "cols", "offsets", "vals", "b"), got, want):
                    assert np.array_equal(x, y), (label, name, float(np.abs(np.asarray(x, float) - np.asarray(y, float)).max()),
                                                  np.flatnonzero(np.asarray(x) != np.asarray(y))[:12].tolist(), F)
                if anchor in F or not keep:
                    assert got[3].max() < 1e7, label
                else:
                    assert got[3].max() > 1e7, label
                assert_same_system(label, got, refs[variant], lam, lm, precision)


# ---- 2. the step ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", ["se2", "se3"])
@pytest.mark.parametrize("shape", ["pose", "edge, term dropped", "hub", "all but one", "every"])
def test_step_is_zero_at_the_fixed_nodes_and_the_reduced_solve_elsewhere(api, dim, shape):
    arrays, F, keep = shape_case(dim, shape)
    ref = FixedReference(arrays, F, keep_anchor=keep)
    fs, free = scalars_of(arrays, sorted(F)), ref.free
    for precision in ("f64", "mixed", "f32"):
        g, u = api[0].from_arrays(*arrays, precision=precision), api[0].from_arrays(*arrays, precision=precision)
        g.set_fixed(F, keep_anchor=bool(keep))
        dx = g.linearize_and_solve()
        assert np.all(dx[fs] == 0.0), (dim, shape, precision)
        if precision == "f64":
            want = ref.step()
            worst = np.abs(dx - want).max() if len(free) else 0.0
            print(f"{dim} {shape}: step worst {worst:.3g} of {np.abs(want).max():.3g} (bound {DX_TOL[dim] * max(1.0, np.abs(want).max()):.3g})")
            assert worst <= DX_TOL[dim] * max(1.0, np.abs(want).max())
        # update_nodes: the entries of F are ignored, the free nodes move as on an unfixed handle, bit for bit
        s0 = g.state()
        step = np.random.default_rng(52).normal(scale=0.1, size=len(dx))
        g.update_nodes(step)
        u.update_nodes(step)
        sg, su = g.state(), u.state()
        others = [v for v in range(len(arrays[0])) if v not in F]
        assert np.array_equal(state_of(arrays, sg, sorted(F)), state_of(arrays, s0, sorted(F))), (dim, shape, precision)
        assert np.array_equal(state_of(arrays, sg, others), state_of(arrays, su, others)), (dim, shape, precision)
        if others:
            assert not np.array_equal(state_of(arrays, sg, others), state_of(arrays, s0, others))
        g.update_nodes(step, -1.0)
        assert np.array_equal(state_of(arrays, g.state(), sorted(F)), state_of(arrays, s0, sorted(F)))


# ---- 3. trajectories ------------------------------------------------------------------------------------------------------

TRAJ_F = {"se2": [1, 9, 18], "se3": [1, 7]}    # poses that are from-nodes of pose-pose edges (keep_anchor = 0), a landmark


def assert_same_trajectory(label, g, ref, arrays, F, iters, lm):
    """the figures of assert_same_trajectory in tests/test_priors_gpu.py: errors rtol 1e-7, state atol 1e-6, the same number
    of iterations; the norms to 1e-6 (a step is the difference of two states that agree to 1e-6); the state at F bit-equal"""
    s0 = g.state()
    eg, ng = g.optimize(iters, return_norms=True)
    eo, no, rejected = ref.optimize(iters, lm)
    sg, so = g.state(), ref.state()
    print(f"{label}: {np.array(eg)} against {eo}; norms {np.array(ng)} against {no}; state worst {np.abs(sg - so).max():.3g}; rejected {rejected}")
    assert len(eg) == len(eo) and len(ng) == len(no)
    np.testing.assert_allclose(eg, eo, rtol=1e-7)
    np.testing.assert_allclose(sg, so, rtol=0, atol=1e-6)
    np.testing.assert_allclose(ng, no, rtol=1e-6, atol=1e-6)
    assert np.array_equal(state_of(arrays, sg, F), state_of(arrays, s0, F))
    assert not np.array_equal(sg, s0)
    return rejected


@pytest.mark.parametrize("dim", ["se2", "se3"])
@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
@pytest.mark.parametrize("keep", [1, 0])
def test_small_graph_trajectories(api, dim, solver, keep):
    arrays = small_graph(dim)
    F = TRAJ_F[dim]
    g = api[0].from_arrays(*arrays, solver=api[1][solver])
    g.set_fixed(F, keep_anchor=bool(keep))
    ref = FixedReference(arrays, F, keep_anchor=keep)
    assert_same_trajectory(f"{dim} {solver} keep_anchor={keep}", g, ref, arrays, F, 8, solver == "LevenbergMarquardt")


@pytest.mark.parametrize("dim", ["se2", "se3"])
def test_fixed_nodes_stay_across_a_levenberg_marquardt_rejection(api, dim):
    """The free nodes start 4 units off (seed 103): the reference run rejects a step (SE(2): the second, SE(3): the seventh),
    and the undo leaves F alone as the step did."""
    arrays = list(small_graph(dim))
    F = TRAJ_F[dim]
    rng = np.random.default_rng(103)
    ns = np.array(arrays[1], np.float64)
    so = state_offsets(arrays)
    for v in range(len(arrays[0])):
        if v in F:
            continue
        k = int(arrays[0][v])
        m = 3 if k == 2 else 2
        ns[so[v]:so[v] + m] += rng.normal(scale=4.0, size=m)
        if k == 0:
            ns[so[v] + 2] += rng.normal(scale=0.3 * 4.0)
    arrays[1] = ns
    g = api[0].from_arrays(*arrays, solver=api[1].LevenbergMarquardt)
    g.set_fixed(F)
    rejected = assert_same_trajectory(f"{dim} LM with a rejection", g, FixedReference(arrays, F), arrays, F, 8, True)
    assert rejected >= 1


# ---- 4. a frozen map --------------------------------------------------------------------------------------------------------

def frozen_map(api, name, n_fixed, iters, seed, noise):
    """The WHOLE graph is optimised for ten iterations (not the first n_fixed poses alone: a map built that way and a map cut
    out of the optimum are the same thing to the code under test, fixed poses at some state); the first n_fixed poses are
    fixed at that state, the positions of the others displaced by N(0, noise), and `iters` iterations are held against the
    reference"""
    arrays = list(oracle_arrays(OracleGraph.load(g2o_path(name))))
    h = api[0].from_arrays(*arrays)
    h.optimize(10)
    st = h.state()
    F = list(range(n_fixed))
    so = state_offsets(arrays)
    rng = np.random.default_rng(seed)
    for v in range(n_fixed, len(arrays[0])):
        m = 3 if arrays[0][v] == 2 else 2
        st[so[v]:so[v] + m] += rng.normal(scale=noise, size=m)
    arrays[1] = st
    g = api[0].from_arrays(*arrays)
    g.set_fixed(F)
    ref = FixedReference(arrays, F)
    assert_same_trajectory(f"{name}, the first {n_fixed} poses fixed", g, ref, arrays, F, iters, False)


def test_intel_frozen_map_of_a_thousand_poses(api):
    """the first 1000 poses at the whole graph's optimum and fixed, the rest perturbed by 0.1 (frozen_map): four iterations
    against the reference (SciPy's sparse LU of the reduced matrix where SciPy is there, as PriorsReference.step has it)"""
    frozen_map(api, "intel", 1000, 4, 61, 0.1)


def test_parking_garage_with_the_first_half_fixed(api):
    """SE(3): the first half of the poses at the whole graph's optimum and fixed, the rest perturbed by 0.05, three iterations"""
    n = OracleGraph.load(g2o_path("parking-garage")).num_nodes
    frozen_map(api, "parking-garage", n // 2, 3, 62, 0.05)


# ---- 5. fronts beyond LDS, single precision -------------------------------------------------------------------------------

def f32_against_f64(label, api, arrays, F, keep, iters, tol_min):
    """the rule of f32_against_f64 in tests/test_priors_gpu.py (the parity tests' rule for single-precision trajectories):
    the first error to 1e-5, the minimum to tol_min; and the fixed states bit-equal"""
    g32 = api[0].from_arrays(*arrays, precision="f32")
    g64 = api[0].from_arrays(*arrays)
    before = {}
    for g in (g32, g64):
        g.set_fixed(F, keep_anchor=keep)
        before[g] = state_of(arrays, g.state(), F)
    assert g32.stats()["n_big_fronts"] > 0
    e32, e64 = g32.optimize(iters), g64.optimize(iters)
    print(f"{label}: f32 {e32} f64 {e64}")
    assert abs(e32[0] - e64[0]) <= 1e-5 * e64[0]
    assert abs(min(e32) - e64[-1]) <= tol_min * e64[-1]
    assert e64[-1] < e64[0]
    for g in (g32, g64):
        assert np.array_equal(state_of(arrays, g.state(), F), before[g])
    return g32, g64


def perturbed_optimum(api, arrays, F, iters, seed, noise):
    """the graph at its optimum, the nodes outside F displaced by N(0, noise)"""
    arrays = list(arrays)
    h = api[0].from_arrays(*arrays)
    h.optimize(iters)
    st = h.state()
    so = state_offsets(arrays)
    rng = np.random.default_rng(seed)
    Fs = set(F)
    for v in range(len(arrays[0])):
        if v not in Fs:
            m = 3 if arrays[0][v] == 2 else 2
            st[so[v]:so[v] + m] += rng.normal(scale=noise, size=m)
    arrays[1] = st
    return arrays


def test_sphere2500_f32_with_two_hundred_fixed_poses_and_no_anchor_term(api):
    arrays = api[0].new(g2o_path("sphere2500")).graph_arrays()
    F = sorted(int(v) for v in np.random.default_rng(63).choice(len(arrays[0]), 200, replace=False))
    arrays = perturbed_optimum(api, arrays, F, 8, 64, 0.05)
    f32_against_f64("sphere2500, 200 fixed", api, arrays, F, False, 8, 1e-5)


@pytest.mark.parametrize("keep", [1, 0])
def test_lattice_f32_gauge_transfer_is_off_with_fixed_nodes(api, keep):
    """An SE(2) graph whose single-precision Gauss-Newton steps use the gauge transfer (a big root front): with fixed nodes the
    system is the one with their identity rows (and with the 1e7 term under keep_anchor), not the gauge term's.  keep_anchor = 1
    puts 1e7 into a single-precision factor: the minimum is asked to 1e-4, as tests/test_priors_gpu.py argues for its lattice."""
    from rustrobotics_amd import synthetic_grid_arrays
    arrays = synthetic_grid_arrays(60, 40)
    anchor = anchor_of(arrays)
    pool = [v for v in range(len(arrays[0])) if v != anchor]
    F = sorted(int(v) for v in np.random.default_rng(65).choice(pool, 5, replace=False))
    arrays = perturbed_optimum(api, arrays, F, 6, 66, 0.05)
    g32, _ = f32_against_f64(f"lattice60x40 keep_anchor={keep}", api, arrays, F, bool(keep), 6, 1e-4 if keep else 1e-5)
    vals = g32.assemble()[3]
    assert (vals.max() > 1e7) == bool(keep)


# ---- 6. the queries are conditional on the fixed nodes ----------------------------------------------------------------------

QUERY_F = {"se2": [3, 8, 15, 19, 25], "se3": [3, 8, 15, 19, 24]}     # se2: 25 is a landmark


def check(label, what, got, want, floor):
    worst = max(rel_diff(g, w) for g, w in zip(got, want))
    tol = tolerance(floor)
    print(f"{label} {what}: {len(want)} values, worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert len(got) == len(want)
    assert floor <= FLOOR_MAX, (label, what, floor)
    assert worst <= tol, (label, what, worst, tol)


@pytest.mark.parametrize("dim", ["se2", "se3"])
def test_marginals_covariances_and_gates_are_conditional_on_the_fixed_nodes(api, dim):
    """Noise floors of the reference (LU inverse against Cholesky solve of the reduced H) at the oracle's state after three
    iterations, computed on the CPU for these graphs and this F: se2 -- marginals 4.9e-15, covariance blocks 2.2e-14, gate S
    5.0e-15, gate d2 2.1e-15, joint d2 9.2e-16; se3 -- 5.9e-14, 1.5e-13, 6.5e-14, 1.0e-14, 2.6e-15.  FLOOR_MAX is 1e-6."""
    from gate_cases import INFO_LEN, MEAS_LEN, candidates, split_packed
    from gate_joint_cases import joint_sets
    arrays = query_graph(dim)
    n = len(arrays[0])
    F = QUERY_F[dim]
    if dim == "se2":
        assert arrays[0][25] == 1
    g = api[0].from_arrays(*arrays)
    g.optimize(3)
    plain = g.marginals()
    st = g.state()
    g.set_fixed(F)
    assert np.array_equal(g.state(), st)
    ref = FixedReference(arrays, F)
    ref.set_state(st)
    sig = ref.sigma_pair()
    free = [v for v in range(n) if v not in F]
    # ---- marginals
    want, floor = ref.blocks(list(range(n)), sig=sig)
    got = g.marginals()
    for v in F:
        assert got[v].shape == want[v].shape and np.all(got[v] == 0.0), v
    check(dim, "marginals", [got[v] for v in free], [want[v] for v in free], floor)
    ef, et = np.asarray(arrays[3]), np.asarray(arrays[4])
    adjacent = sorted({int(b) for a, b in zip(ef, et) if a in F and b not in F} | {int(a) for a, b in zip(ef, et) if b in F and a not in F})
    assert adjacent
    for v in adjacent:     # conditioning on a neighbour shrinks the marginal
        assert np.trace(got[v]) < np.trace(plain[v]), (v, np.trace(got[v]), np.trace(plain[v]))
    # ---- marginal blocks of edges with a fixed end, and covariance blocks of 30 random pairs
    k = next(int(k) for k in range(len(ef)) if (ef[k] in F) != (et[k] in F))
    vals, off = g.marginal_blocks([int(ef[k])], [int(et[k])])
    assert len(vals) == off[-1] > 0 and np.all(vals == 0.0)
    rng = np.random.default_rng(11)
    a = np.concatenate([rng.integers(0, n, 30), [F[0], F[1], F[4]]]).astype(np.int32)
    b = np.concatenate([rng.integers(0, n, 30), [F[0], F[2], free[0]]]).astype(np.int32)
    vals, off = g.covariance_blocks(a, b)
    want, floor = ref.blocks(a, b, sig=sig)
    got = [vals[off[q]:off[q + 1]].reshape(w.shape) for q, w in enumerate(want)]
    with_f = [q for q in range(len(a)) if a[q] in F or b[q] in F]
    assert len(with_f) >= 3
    for q in with_f:
        assert np.all(got[q] == 0.0), (a[q], b[q])
    # two free nodes that only fixed nodes join are conditionally independent: the reference's block is exactly zero, and the
    # handle's is held to the tolerance times the scale Cauchy-Schwarz gives a covariance block, sqrt(|Sigma_aa| |Sigma_bb|)
    marg = g.marginals()
    apart = [q for q in range(len(a)) if q not in with_f and not np.any(want[q] != 0.0)]
    for q in apart:
        scale = np.sqrt(np.abs(marg[a[q]]).max() * np.abs(marg[b[q]]).max())
        print(f"{dim}: nodes {a[q]} and {b[q]} are conditionally independent: worst {np.abs(got[q]).max():.3g} of {scale:.3g}")
        assert np.abs(got[q]).max() <= tolerance(floor) * scale
    rest = [q for q in range(len(a)) if q not in with_f and q not in apart]
    check(dim, "covariance blocks", [got[q] for q in rest], [want[q] for q in rest], floor)
    # ---- the gates: the candidates of gate_cases, two more with one fixed endpoint and one with both
    kind, ca, cb, meas, info = candidates(arrays, st)
    pk = int(kind[0])
    m0, w0 = split_packed(kind, meas, MEAS_LEN)[0], split_packed(kind, info, INFO_LEN)[0]
    extra = [(F[0], free[1]), (free[2], F[1]), (F[0], F[2])]
    cand = (np.concatenate([kind, [pk] * 3]).astype(np.int32), np.concatenate([ca, [e[0] for e in extra]]).astype(np.int32),
            np.concatenate([cb, [e[1] for e in extra]]).astype(np.int32), np.concatenate([meas, m0, m0, m0]), np.concatenate([info, w0, w0, w0]))
    nc = len(cand[0])
    S, d2, chi2, fS, fd = ref.gate(cand, sig=sig)
    gd2, gchi2, gS = g.gate_edges(*cand, return_innovation=True)
    check(dim, "gate d2", [np.array([v]) for v in gd2], [np.array([v]) for v in d2], fd)
    check(dim, "gate S", gS, S, fS)
    np.testing.assert_allclose(gchi2, chi2, rtol=1e-9)
    omega = np.zeros((len(w0) and NODE_DIM[0 if pk == 0 else 2],) * 2)
    omega[np.triu_indices(len(omega))] = w0
    omega = omega + np.triu(omega, 1).T
    both = np.linalg.inv(omega)
    print(f"{dim}: S of the candidate between two fixed nodes against Omega^-1: {np.abs(gS[nc - 1] - both).max():.3g} of {np.abs(both).max():.3g}")
    assert np.abs(gS[nc - 1] - both).max() <= 1e-12 * np.abs(both).max()
    sets = joint_sets(len(kind)) + [[nc - 3, nc - 2], [nc - 1, 0], [nc - 3, nc - 1, 1]]
    jd2, fj = ref.gate_joint(cand, sets, sig=sig)
    check(dim, "joint d2", [np.array([v]) for v in g.gate_joint(*cand, sets)], [np.array([v]) for v in jd2], fj)


# ---- 7. launch forms ---------------------------------------------------------------------------------------------------------

FORM_CASES = [("se2", "f64"), ("se3", "mixed"), ("lattice", "f32")]
_form_ref = {}


def form_fixed(graph, n):
    return {"se2": [2, 7, n - 1], "se3": [1, 5]}.get(graph) or sorted(int(v) for v in np.random.default_rng(67).choice(np.arange(1, n), 5, replace=False))


@pytest.mark.parametrize("graph,precision", FORM_CASES)
@pytest.mark.parametrize("form", ["a", "b", "c", "d"])
def test_every_launch_form_sees_the_fixed_set(api, graph, precision, form, monkeypatch):
    import launch_forms as lf
    n = len(lf.arrays_of(graph)[0])
    F = form_fixed(graph, n)

    def run(frm):
        h = lf.Handle(api, graph, frm, monkeypatch, precision)
        launches = h.stats()["n_launches_per_iter"]
        s0 = h.state()
        h.set_fixed(F)
        assert h.stats()["n_launches_per_iter"] == launches      # no launch more per iteration
        return h, s0, lf.s1(h, s0)

    key = (graph, precision)
    if key not in _form_ref:
        h, s0, trace = run("ref")
        c = h.counts()
        assert c[lf.PLAIN] > 0 and c[lf.REPLAY] == 0 and c[lf.ITEM] == 0 and c[lf.CAPTURE] == 0
        t = dict(trace)
        assert t["chi2"] < t["errors"][0] and not np.array_equal(t["state"], s0)
        arrays = lf.arrays_of(graph)
        assert np.array_equal(state_of(arrays, t["state"], F), state_of(arrays, s0, F))
        _form_ref[key] = trace
    h, s0, got = run(form)
    assert lf.same(got, _form_ref[key]) is None, (graph, precision, form, lf.same(got, _form_ref[key]))
    # A change of the set drops the captured graph: the next replay captures again.  Per form (launch_forms.py): under
    # RR_PGO_FORCE_GRAPH (b, c) iterate_async replays, so s1 has replayed one capture and the iteration behind the second
    # set_fixed is a replay of a second capture; forms a and d (these graphs stay below 48 launches per iteration, d sets
    # RR_PGO_NO_GRAPH) never replay and never capture, and that iteration is a plain launch
    c = h.counts()
    h.g.set_fixed(F[:-1])
    h.g.iterate_async(1)
    h.g.sync()
    c2 = h.counts()
    if form in ("b", "c"):
        assert c[lf.REPLAY] > 0 and c[lf.CAPTURE] == 1
        assert c2[lf.REPLAY] == c[lf.REPLAY] + 1 and c2[lf.CAPTURE] == 2 and c2[lf.PLAIN] == c[lf.PLAIN]
    else:
        assert c[lf.REPLAY] == 0 and c[lf.CAPTURE] == 0
        assert c2[lf.PLAIN] == c[lf.PLAIN] + 1 and c2[lf.REPLAY] == 0 and c2[lf.CAPTURE] == 0


# ---- 8. lifecycle ---------------------------------------------------------------------------------------------------------------

def same_bits(a, b, iters=0):
    """the same_bits rule of tests/test_priors_gpu.py"""
    assert a.global_error() == b.global_error()
    for x, y in zip(a.assemble(), b.assemble()):
        assert np.array_equal(x, y)
    if iters:
        assert np.array_equal(np.array(a.optimize(iters)), np.array(b.optimize(iters)))
    assert np.array_equal(a.state(), b.state())


def launch_counts(g):
    st = g.stats()
    return np.array([st[k] for k in ("n_plain_iterations", "n_graph_replays", "n_loop_items", "n_graph_captures")])


@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
def test_set_then_clear_is_a_handle_that_never_had_a_fixed_set(api, solver, monkeypatch):
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    a = api[0].new(g2o_path("simulation-pose-landmark"), api[1][solver])
    b = api[0].new(g2o_path("simulation-pose-landmark"), api[1][solver])
    monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    for g in (a, b):
        g.iterate_async(2)
        g.sync()
        assert g.stats()["n_graph_replays"] == 2 and g.stats()["n_plain_iterations"] == 0   # the captured graph really ran
    n = a.num_nodes
    a.set_fixed([0, 5, 5, n - 1], keep_anchor=False)
    assert a.num_fixed == 3
    dx = a.linearize_and_solve()
    assert np.count_nonzero(dx) < len(dx) and np.any(dx != b.linearize_and_solve())
    a.clear_fixed()
    assert a.num_fixed == 0 and len(a.fixed_nodes()) == 0
    assert a.assemble()[3].max() > 1e7      # keep_anchor is back at 1
    assert a.stats()["n_launches_per_iter"] == b.stats()["n_launches_per_iter"]
    ca, cb = launch_counts(a), launch_counts(b)
    same_bits(a, b, 5)
    a.iterate_async(1)
    b.iterate_async(1)
    a.sync()
    b.sync()
    da, db = launch_counts(a) - ca, launch_counts(b) - cb
    assert da[:3].tolist() == db[:3].tolist()           # the same launches in the same forms ...
    assert da[3] == db[3] + 1 == 1                      # ... and the one capture more that the two changes of the set cost
    assert np.array_equal(a.state(), b.state())


def test_second_call_replaces_the_first_and_duplicates_count_once(api):
    arrays = small_graph("se2")
    n = len(arrays[0])
    a, b = api[0].from_arrays(*arrays), api[0].from_arrays(*arrays)
    a.set_fixed(list(range(n)), keep_anchor=False)
    a.set_fixed([9, 1, 9, n - 1, 1])
    b.set_fixed([1, 9, n - 1])
    assert a.num_fixed == b.num_fixed == 3
    assert a.fixed_nodes().tolist() == b.fixed_nodes().tolist() == [1, 9, n - 1]
    assert a.assemble()[3].max() > 1e7      # the second call's keep_anchor
    same_bits(a, b, 5)


@pytest.mark.parametrize("dim", ["se2", "se3"])
def test_every_refusal_names_the_entry_and_changes_nothing(api, dim):
    from rustrobotics_amd import _lib
    arrays = small_graph(dim)
    n = len(arrays[0])
    a, b = api[0].from_arrays(*arrays), api[0].from_arrays(*arrays)
    for g in (a, b):
        g.set_fixed([2, 6], keep_anchor=False)
    for what, nodes in (("node", [1, n, 3]), ("negative node", [1, -1, 3])):
        with pytest.raises(api[2]) as ei:
            a.set_fixed(nodes)
        print(what, "->", ei.value)
        assert ei.value.code == _lib.EINVAL and "entry 1" in str(ei.value), (what, ei.value)
        assert a.fixed_nodes().tolist() == [2, 6]
    L = _lib.load()
    node = np.array([1, 4], np.int32)
    pn = node.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.rr_pgo_set_fixed(a._h, -1, pn, 1) == _lib.EINVAL and b"n_fixed" in L.rr_pgo_last_error()
    assert L.rr_pgo_set_fixed(a._h, 2, None, 1) == _lib.EINVAL and b"node" in L.rr_pgo_last_error()
    assert a.fixed_nodes().tolist() == [2, 6]
    assert a.assemble()[3].max() < 1e7      # keep_anchor = 0 is still in force
    same_bits(a, b, 5)


def test_sharded_and_edge_parallel_handles_are_unsupported(api, monkeypatch):
    from rustrobotics_amd import _lib
    PoseGraph = api[0]
    arrays = small_graph("se2")
    monkeypatch.setenv("RR_PGO_EDGE_LINEARIZE", "1")
    edge_form = PoseGraph.from_arrays(*arrays)
    monkeypatch.delenv("RR_PGO_EDGE_LINEARIZE")
    twin = PoseGraph.from_arrays(*arrays)
    handles = {"sharded": PoseGraph.from_arrays(*arrays, sharded=True), "RR_PGO_EDGE_LINEARIZE": edge_form}
    for what, h in handles.items():
        with pytest.raises(api[2]) as ei:
            h.set_fixed([2])
        print(what, "->", ei.value)
        assert ei.value.code == _lib.EUNSUPPORTED and what in str(ei.value), (what, ei.value)
        assert h.num_fixed == 0
    np.testing.assert_allclose(edge_form.global_error(), twin.global_error(), rtol=1e-12)


def test_extend_carries_the_set_and_keep_anchor_and_new_nodes_are_free(api):
    from extend_cases import case
    c = case("simulation-pose-landmark")
    rng = np.random.default_rng(68)
    F = sorted(int(v) for v in rng.choice(c.n_base, 6, replace=False))
    a = api[0].from_arrays(*c.base)
    a.set_fixed(F, keep_anchor=False)
    a.optimize(2)
    edges, new_nodes = c.extend_args()
    a.extend(*edges, **new_nodes)
    b = api[0].from_arrays(*c.grown)
    b.set_fixed(F, keep_anchor=False)
    assert a.num_nodes == b.num_nodes > c.n_base
    assert a.fixed_nodes().tolist() == b.fixed_nodes().tolist() == F
    st = a.state()
    a.set_state(st)
    b.set_state(st)
    assert a.assemble()[3].max() < 1e7          # keep_anchor = 0 came along
    dx = a.linearize_and_solve()
    assert np.all(dx[scalars_of(c.grown, F)] == 0.0)
    new = scalars_of(c.grown, list(range(c.n_base, a.num_nodes)))
    assert np.all(dx[new] != 0.0)               # the new nodes are free
    same_bits(a, b, 5)
    assert np.array_equal(state_of(c.grown, a.state(), F), state_of(c.grown, st, F))


@pytest.mark.parametrize("dim", ["se2", "se3"])
def test_two_runs_give_identical_bits(api, dim):
    arrays = small_graph(dim)
    a, b = api[0].from_arrays(*arrays), api[0].from_arrays(*arrays)
    for g in (a, b):
        g.set_fixed(TRAJ_F[dim], keep_anchor=False)
    same_bits(a, b, 6)
    assert np.array_equal(a.linearize_and_solve(), b.linearize_and_solve())
