"""Bearing-only and range-only landmark edges (RR_PGO_EDGE_SE2_BEARING = 4, RR_PGO_EDGE_SE2_RANGE = 6) on the GPU, through
the C ABI via the mirror, against tests/bearing_range_reference.py (numpy f64; tests/test_bearing_range_cpu.py holds it to
the oracle and to 50-digit differences and checks the fixtures of tests/bearing_range_cases.py).  Every test here fails on a
build without the kinds, where kind 4 is a bad edge kind at rr_pgo_create."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import g2o_path
from bearing_range_cases import CASES, case, mixed_marks
from bearing_range_reference import (BEARING, EDGE_DIM, FLOOR_MAX, INFO_LEN, META_LEN, RANGE, SE2, SE2_XY, BearingRangeReference, rel_diff,
                                     tolerance)
from test_priors_gpu import assert_same_system   # the frame's arithmetic is the same: its comparison and SYSTEM_TOL, imported

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -7
PRECISIONS = ("f64", "mixed", "f32")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver, PoseGraphError
    return PoseGraph, PoseGraphSolver, PoseGraphError


_CONVERGED = {}


def converged(name):
    """the fixture at the reference's converged state (computed once, not modified)"""
    if name not in _CONVERGED:
        ref = BearingRangeReference(case(name))
        ref.optimize(20)
        a = list(case(name))
        a[1] = ref.state()
        _CONVERGED[name] = tuple(a)
    return _CONVERGED[name]


def landmarks(arrays):
    return [int(v) for v in np.flatnonzero(arrays[0] == 1)]


def some_priors(arrays, nodes, seed=5, noise=0.1):
    """(node, meas, info) of priors near the nodes' states: a pose 3 | 6 values, a landmark 2 | 3"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum([3 if k == 0 else 2 for k in arrays[0]])])
    meas, info = [], []
    for v in nodes:
        d = int(off[v + 1] - off[v])
        meas.append(arrays[1][off[v]:off[v + 1]] + rng.normal(scale=noise, size=d))
        a = rng.normal(size=(d, d))
        info.append((a @ a.T + d * np.eye(d))[np.triu_indices(d)] * 20.0)
    return np.array(nodes, np.int32), np.concatenate(meas), np.concatenate(info)


# ---- 1. the assembled system ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_assembled_system_plain(api, name):
    """rr_pgo_assemble against the reference entry by entry (every entry of the reference outside the stored blocks is zero;
    parallel edges have a block each, which add), in f64, mixed and f32, plain and with lambda"""
    arrays = case(name)
    ref = BearingRangeReference(arrays)
    for precision in PRECISIONS:
        g = api[0].from_arrays(*arrays, precision=precision)
        for lm in (False, True):
            assert_same_system(f"{name} {precision}", g, ref, lm, precision, 1)


def test_parallel_edges_have_a_block_each(api):
    arrays = case("mixed")
    a, b = mixed_marks()["parallel"]
    pair = {int(arrays[3][a]), int(arrays[4][a])}
    br, bc, _, _, _ = api[0].from_arrays(*arrays).assemble()
    assert sum(1 for r, c in zip(br, bc) if {int(r), int(c)} == pair) == 2


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_assembled_system_with_a_kernel_and_a_mask(api, kind):
    """delta = 1 at the initial state of `mixed`, where most errors are several sigma: edges on both sides of the threshold"""
    arrays = case("mixed")
    mask = (np.arange(len(arrays[2])) % 3 != 0).astype(np.int32)
    ref = BearingRangeReference(arrays, kind=kind, delta=1.0, edge_mask=mask)
    s, w = ref.edge_errors()
    br = np.isin(arrays[2], (BEARING, RANGE))
    assert np.any(w[br] < 1.0) and np.any(w[~br] < 1.0)      # the kernel bites on edges of the new kinds and of the old
    for precision in PRECISIONS:
        g = api[0].from_arrays(*arrays, precision=precision)
        g.set_robust_kernel(kind, 1.0, mask)
        for lm in (False, True):
            assert_same_system(f"mixed {kind} {precision}", g, ref, lm, precision, 1)


@pytest.mark.parametrize("keep", [1, 0])
def test_assembled_system_with_priors_on_a_landmark_and_a_pose(api, keep):
    """a prior stays the edge of the node's own kind: on a landmark that only bearings and ranges see, and on a pose (nine on
    one landmark: the strided prior loop wraps); both keep_anchor values"""
    arrays = case("mixed")
    lm_nodes = landmarks(arrays)
    node, meas, info = some_priors(arrays, [lm_nodes[4]] * 9 + [lm_nodes[1], 5, 0])
    ref = BearingRangeReference(arrays, priors=(node, meas, info), keep_anchor=bool(keep))
    for precision in PRECISIONS:
        g = api[0].from_arrays(*arrays, precision=precision)
        g.set_priors(node, meas, info, keep_anchor=bool(keep))
        for lm in (False, True):
            assert_same_system(f"mixed priors keep_anchor={keep} {precision}", g, ref, lm, precision, keep)
    g = api[0].from_arrays(*arrays)
    g.set_priors(node, meas, info, keep_anchor=bool(keep))
    s, w = g.prior_errors()
    s2, w2 = ref.prior_errors()
    np.testing.assert_allclose(s, s2, rtol=1e-12)
    np.testing.assert_allclose(w, w2, rtol=1e-12)
    np.testing.assert_allclose(g.global_error(), ref.cost(), rtol=1e-12)


def fixed_sets(arrays):
    k = mixed_marks()["cut"]
    lm_nodes = landmarks(arrays)
    return {"pose": [6], "landmark": [lm_nodes[2]], "both ends": [int(arrays[3][k]), int(arrays[4][k])]}


@pytest.mark.parametrize("which", ["pose", "landmark", "both ends"])
def test_assembled_system_with_fixed_nodes_and_its_unfixed_twin(api, which):
    """against the reference, and -- in all three precisions -- entry by entry against the handle without the fixed set: the same
    bits on free rows, identity blocks, zero off-diagonal blocks and b = 0 on fixed ones"""
    arrays = case("mixed")
    fixed = fixed_sets(arrays)[which]
    ref = BearingRangeReference(arrays, fixed=fixed)
    for precision in PRECISIONS:
        g, twin = api[0].from_arrays(*arrays, precision=precision), api[0].from_arrays(*arrays, precision=precision)
        g.set_fixed(fixed)
        for lm in (False, True):
            assert_same_system(f"mixed fixed {which} {precision}", g, ref, lm, precision, 1)
            lam = 0.37 if lm else 0.0
            br, bc, bo, vals, b = g.assemble(lam, lm)
            br2, bc2, bo2, vals2, b2 = twin.assemble(lam, lm)
            assert np.array_equal(br, br2) and np.array_equal(bc, bc2) and np.array_equal(bo, bo2)
            for r, c, o in zip(br, bc, bo):
                n = ref.dims[r] * ref.dims[c]
                blk, blk2 = vals[o:o + n], vals2[o:o + n]
                if r in fixed or c in fixed:
                    want = np.eye(ref.dims[r]).ravel() if r == c else np.zeros(n)
                    assert np.array_equal(blk, want), (precision, r, c)
                else:
                    assert np.array_equal(blk, blk2), (precision, r, c)
            for v in range(len(arrays[0])):
                iv = ref.scalars(v)
                assert np.array_equal(b[iv], np.zeros(len(iv)) if v in fixed else b2[iv]), (precision, v)


# ---- 2. the cost and the error lists ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("kind", [None, "huber", "cauchy"])
def test_cost_and_edge_errors(api, name, kind):
    """chi2 at rtol 1e-12; the per-edge terms by the floor rule max(1e-12, 100 x floor), floor = the reference's f64 against
    50 digits over these edges (a small error is a difference of large coordinates: a plain 1e-12 does not hold for it, as
    tests/test_landmarks3d_gpu.py notes beside its check_edges test); the weights follow s"""
    arrays = case(name)
    ref = BearingRangeReference(arrays, kind=kind, delta=1.0)
    g = api[0].from_arrays(*arrays)
    if kind:
        g.set_robust_kernel(kind, 1.0)
    s, w = g.edge_errors()
    s2, w2 = ref.edge_errors()
    s_mp = ref.edge_s_mp()
    floor = float(np.max(np.abs(s2 - s_mp) / s_mp))
    worst = float(np.max(np.abs(s - s_mp) / s_mp))
    print(f"{name} {kind}: chi2 {g.global_error():.15g} against {ref.cost():.15g}; s worst {worst:.3g}, floor {floor:.3g}, tolerance {tolerance(floor):.3g}")
    assert floor <= FLOOR_MAX
    np.testing.assert_allclose(g.global_error(), ref.cost(), rtol=1e-12)
    assert worst <= tolerance(floor)
    np.testing.assert_allclose(w, w2, rtol=max(1e-12, tolerance(floor)))


@pytest.mark.parametrize("name", ["mixed", "corridor"])
def test_check_edges_chi2_is_edge_errors_bit_for_bit(api, name):
    for arrays in (case(name), converged(name)):
        g = api[0].from_arrays(*arrays)
        s, _ = g.edge_errors()
        out = g.check_edges()
        assert np.array_equal(out["chi2"], s), np.flatnonzero(out["chi2"] != s)


# ---- 3. one solved step and its update --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_linearize_solve_and_update(api, name):
    arrays = case(name)
    ref = BearingRangeReference(arrays)
    g = api[0].from_arrays(*arrays)
    for lam, lm in ((0.0, False), (0.37, True)):
        dx = g.linearize_and_solve(lam, lm)
        dx2 = ref.step(lam, lm)
        H, b = ref.system(lam, lm)
        dx3 = np.linalg.solve(H, b)                       # a second route: the reference's own noise floor
        floor = rel_diff(dx3, dx2)
        print(f"{name} lm={lm}: dx rel {rel_diff(dx, dx2):.3g}, floor {floor:.3g}")
        assert floor <= FLOOR_MAX and rel_diff(dx, dx2) <= tolerance(floor)
    dx = g.linearize_and_solve(0.0, False)
    before = g.state()
    g.update_nodes(dx)
    ref.set_state(before)
    ref.update(dx)
    after, want = g.state(), ref.state()
    for v, k in enumerate(arrays[0]):
        sl = ref.scalars(v)
        if k == 1:   # l + dl, one f64 addition per coordinate: the same bits
            assert np.array_equal(after[sl], before[sl] + dx[sl]), v
        else:
            np.testing.assert_allclose(after[sl], want[sl], rtol=0, atol=1e-12)


# ---- 4. trajectories ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["beacons", "mixed", "corridor"])
@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
def test_trajectories_f64(api, name, solver):
    """errors at rtol 1e-7 and states at atol 1e-6 against the reference loop, the figures of test_priors_gpu.py and
    test_landmarks3d_gpu.py; two runs give the same bits"""
    arrays = case(name)
    lm = solver == "LevenbergMarquardt"
    g = api[0].from_arrays(*arrays, solver=api[1][solver])
    ref = BearingRangeReference(arrays)
    eg = np.array(g.optimize(10))
    eo, _ = ref.optimize(10, lm)
    sg, so = g.state(), ref.state()
    print(f"{name} {solver}: {eg} against {eo}; state worst {np.abs(sg - so).max():.3g}")
    assert len(eg) == len(eo)
    np.testing.assert_allclose(eg, eo, rtol=1e-7)
    np.testing.assert_allclose(sg, so, rtol=0, atol=1e-6)
    g2 = api[0].from_arrays(*arrays, solver=api[1][solver])
    eg2 = np.array(g2.optimize(10))
    assert np.array_equal(eg, eg2) and np.array_equal(sg, g2.state())


def test_trajectory_with_the_beacons_fixed(api):
    """the landmarks of `beacons` held through set_fixed, which then fixes the gauge (keep_anchor = 0): they never move"""
    arrays = case("beacons")
    fixed = landmarks(arrays)
    g = api[0].from_arrays(*arrays)
    g.set_fixed(fixed, keep_anchor=False)
    ref = BearingRangeReference(arrays, fixed=fixed, fixed_keep_anchor=False)
    before = g.state()
    eg = np.array(g.optimize(10))
    eo, _ = ref.optimize(10)
    assert len(eg) == len(eo)
    np.testing.assert_allclose(eg, eo, rtol=1e-7)
    np.testing.assert_allclose(g.state(), ref.state(), rtol=0, atol=1e-6)
    for v in fixed:
        assert np.array_equal(g.state()[ref.scalars(v)], before[ref.scalars(v)])


@pytest.mark.parametrize("name", ["mixed", "corridor"])
@pytest.mark.parametrize("precision", ["f32", "mixed"])
def test_trajectories_single_precision(api, name, precision):
    """the project's single-precision rule (tests/test_landmarks3d_gpu.py): the first error to 1e-5, the minimum to 1e-5 of the
    reference's f64 minimum; two runs give the same bits"""
    arrays = case(name)
    g = api[0].from_arrays(*arrays, precision=precision)
    eg = np.array(g.optimize(10))
    eo, _ = BearingRangeReference(arrays).optimize(10, False)
    print(f"{name} {precision}: {eg} against {eo}")
    np.testing.assert_allclose(eg[0], eo[0], rtol=1e-5)
    np.testing.assert_allclose(eg.min(), eo.min(), rtol=1e-5)
    g2 = api[0].from_arrays(*arrays, precision=precision)
    assert np.array_equal(eg, np.array(g2.optimize(10))) and np.array_equal(g.state(), g2.state())


# ---- 5. queries -------------------------------------------------------------------------------------------------------------

def prediction(ref, kind, a, b):
    """the measurement of kind `kind` from node a to node b that the state of `ref` predicts (e = 0)"""
    x1, x2 = ref.x[a], ref.x[b]
    d = x2[:2] - x1[:2]
    p = np.array([x1[2] * d[0] + x1[3] * d[1], -x1[3] * d[0] + x1[2] * d[1]])
    if kind == SE2:
        return np.array([p[0], p[1], np.arctan2(x2[3], x2[2]) - np.arctan2(x1[3], x1[2])])
    return {SE2_XY: p, BEARING: np.array([np.arctan2(p[1], p[0])]), RANGE: np.array([np.hypot(*p)])}[kind]


KINDS = (BEARING, RANGE, SE2_XY, SE2, RANGE, BEARING)


def candidates(arrays, seed, n=16, kinds=KINDS, distinct=False):
    """seeded candidates of the kinds of `kinds` (cycled; default: all four 2-D kinds in one list), a few sigma off the state's
    prediction; distinct: no node is named twice, so n candidates name at least 5 n scalar columns of the tree solve"""
    rng = np.random.default_rng(seed)
    ref = BearingRangeReference(arrays)
    poses, lms = np.flatnonzero(arrays[0] == 0), np.flatnonzero(arrays[0] == 1)
    free_poses, free_lms = [int(v) for v in rng.permutation(poses)], [int(v) for v in rng.permutation(lms)]
    kind, a, b, meas, info = [], [], [], [], []
    for c in range(n):
        k = kinds[c % len(kinds)]
        if distinct:
            pa = free_poses.pop()
            pb = free_poses.pop() if k == SE2 else free_lms.pop()
        else:
            pa = int(rng.choice(poses))
            pb = int(rng.choice(poses[poses != pa])) if k == SE2 else int(rng.choice(lms))
        d = EDGE_DIM[k]
        sig = {SE2: [0.05, 0.05, 0.02], SE2_XY: [0.05, 0.05], BEARING: [0.02], RANGE: [0.05]}[k]
        m = rng.normal(size=(d, d))
        om = (m @ m.T + d * np.eye(d)) / d * (1.0 / np.mean(sig) ** 2)
        kind.append(k); a.append(pa); b.append(pb)
        meas.append(prediction(ref, k, pa, pb) + rng.normal(size=d) * sig * 1.5)
        info.append(om[np.triu_indices(d)])
    return (np.array(kind, np.int32), np.array(a, np.int32), np.array(b, np.int32), np.concatenate(meas), np.concatenate(info))


def sub(cand, idx):
    kind, a, b, meas, info = cand
    mo = np.concatenate([[0], np.cumsum([META_LEN[int(k)] for k in kind])])
    io = np.concatenate([[0], np.cumsum([INFO_LEN[int(k)] for k in kind])])
    return (kind[idx], a[idx], b[idx], np.concatenate([meas[mo[q]:mo[q + 1]] for q in idx]), np.concatenate([info[io[q]:io[q + 1]] for q in idx]))


@pytest.mark.parametrize("name", ["tri", "beacons", "mixed", "corridor"])
@pytest.mark.parametrize("state", ["initial", "converged"])
def test_marginals_and_covariances(api, name, state):
    """marginals, covariance_blocks and cross_covariance of poses and landmarks against dense Sigma, by the floor rule; on
    `beacons` also conditional on the fixed landmarks"""
    arrays = case(name) if state == "initial" else converged(name)
    for fixed in ([], landmarks(arrays)) if name == "beacons" else ([],):
        ref = BearingRangeReference(arrays, fixed=fixed, fixed_keep_anchor=not fixed)
        g = api[0].from_arrays(*arrays)
        if fixed:
            g.set_fixed(fixed, keep_anchor=False)
        sig = ref.sigma_pair()
        N = len(arrays[0])
        rng = np.random.default_rng(33)
        nodes = list(range(N)) if N <= 30 else sorted(int(v) for v in rng.choice(N, 24, replace=False))
        want, floor = ref.blocks(nodes, nodes, sig)
        got = g.marginals(nodes)
        worst = max(rel_diff(x, y) for x, y, v in zip(got, want, nodes) if v not in fixed)
        print(f"{name} {state} fixed={len(fixed)}: marginals worst {worst:.3g}, floor {floor:.3g}")
        assert floor <= FLOOR_MAX and worst <= tolerance(floor)
        for x, v in zip(got, nodes):
            assert x.shape == (ref.dims[v], ref.dims[v])
            if v in fixed:
                assert not np.any(x)
        pa = [int(v) for v in rng.choice(nodes, 12)]
        pb = [int(v) for v in rng.choice(nodes, 12)]
        want, floor = ref.blocks(pa, pb, sig)
        vals, off = g.covariance_blocks(pa, pb)
        scale = max(np.abs(x).max() for x in want)
        worst = max(np.abs(vals[off[q]:off[q + 1]].reshape(want[q].shape) - want[q]).max() for q in range(12)) / scale
        fl = max(np.abs(sig[0] - sig[1]).max() / scale, floor)
        print(f"{name} {state}: covariance blocks worst {worst:.3g} of the largest block, floor {fl:.3g}")
        assert fl <= FLOOR_MAX and worst <= tolerance(fl)
        rows, cols = pa[:5], pb[:4]
        X = g.cross_covariance(rows, cols)
        ri, ci = np.concatenate([ref.scalars(v) for v in rows]), np.concatenate([ref.scalars(v) for v in cols])
        worst = np.abs(X - sig[0][np.ix_(ri, ci)]).max() / scale
        assert worst <= tolerance(fl), worst
        # independent of list order and of repeats, bit for bit
        perm = [3, 0, 2, 1, 0]
        X2 = g.cross_covariance([rows[q] for q in perm], cols)
        rr = np.concatenate([[0], np.cumsum([ref.dims[v] for v in rows])])
        assert np.array_equal(X2, np.vstack([X[rr[q]:rr[q + 1]] for q in perm]))


@pytest.mark.parametrize("name", ["mixed", "corridor"])
@pytest.mark.parametrize("state", ["initial", "converged"])
def test_gate_edges(api, name, state):
    """bearing, range, XY and SE2 candidates in ONE call: S (1 x 1 for the new kinds, at the offsets sum of d_e^2), d2 and chi2
    by the floor rule (chi2: the reference's f64 against 50 digits); outputs independent of list order, of repeats and of cutting
    the list into two calls (a plan cut by the workspace bound: test_a_plan_cut_by_the_workspace_bound_gives_the_same_bits)"""
    arrays = case(name) if state == "initial" else converged(name)
    g = api[0].from_arrays(*arrays)
    ref = BearingRangeReference(arrays)
    cand = candidates(arrays, 71)
    d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
    S2, d22, chi22, fS, fd = ref.gate(cand, ref.sigma_pair())
    worst_S = max(rel_diff(x, y) for x, y in zip(S, S2))
    worst_d = float(np.max(np.abs(d2 / d22 - 1)))
    s_mp = ref.cand_s_mp(cand)
    fc, worst_c = float(np.max(np.abs(chi22 - s_mp) / s_mp)), float(np.max(np.abs(chi2 - s_mp) / s_mp))
    print(f"{name} {state}: S worst {worst_S:.3g} (floor {fS:.3g}), d2 worst {worst_d:.3g} (floor {fd:.3g}), chi2 worst {worst_c:.3g} (floor {fc:.3g})")
    assert max(fS, fd, fc) <= FLOOR_MAX
    for c, k in enumerate(cand[0]):
        assert S[c].shape == (EDGE_DIM[int(k)],) * 2
    assert worst_S <= tolerance(fS) and worst_d <= tolerance(fd)
    assert worst_c <= tolerance(fc)
    # the raw call: offsets are the running sum of d_e^2
    from rustrobotics_amd import _lib
    L = _lib.load()
    dp, ip = (lambda x: x.ctypes.data_as(C.POINTER(C.c_double))), (lambda x: x.ctypes.data_as(C.POINTER(C.c_int32)))
    n = len(cand[0])
    out, off = np.zeros(9 * n), np.zeros(n + 1, np.int64)
    raw = [np.ascontiguousarray(x) for x in cand]
    d2r, chi2r = np.zeros(n), np.zeros(n)
    assert L.rr_pgo_gate_edges(g._h, n, ip(raw[0]), ip(raw[1]), ip(raw[2]), dp(raw[3]), dp(raw[4]), dp(d2r), dp(chi2r), dp(out),
                               off.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([EDGE_DIM[int(k)] ** 2 for k in cand[0]])]))
    assert np.array_equal(d2r, d2)
    # order, repeats, the list in two calls: the same bits per candidate
    perm = np.array([5, 0, 11, 3, 3, 8, 1, 0, 15, 6])
    d2p, chi2p, Sp = g.gate_edges(*sub(cand, perm), return_innovation=True)
    assert np.array_equal(d2p, d2[perm]) and np.array_equal(chi2p, chi2[perm])
    assert all(np.array_equal(Sp[q], S[c]) for q, c in enumerate(perm))
    d2a, _ = g.gate_edges(*sub(cand, np.arange(7)))
    d2b, _ = g.gate_edges(*sub(cand, np.arange(7, n)))
    assert np.array_equal(np.concatenate([d2a, d2b]), d2)
    # a call without a candidate of the new kinds on the same handle answers with the same bits for its candidates
    old = np.flatnonzero(np.isin(cand[0], (SE2, SE2_XY)))
    d2o, _ = g.gate_edges(*sub(cand, old))
    assert np.array_equal(d2o, d2[old])
    thr = g.gate(*cand)
    from rustrobotics_amd.mapping import CHI2_95
    want = d2 <= np.array([CHI2_95[EDGE_DIM[int(k)]] for k in cand[0]])
    assert np.array_equal(thr, want)


@pytest.mark.parametrize("name", ["mixed", "corridor"])
def test_gate_joint(api, name):
    """sets that mix the dimensions 1, 1, 2, 3: d2 by the floor rule, the prefix property bit for bit (prefix k = d2 of the set
    cut after candidate k), and block (c, d) of S independent of the rest of the set"""
    arrays = converged(name)
    g = api[0].from_arrays(*arrays)
    ref = BearingRangeReference(arrays)
    cand = candidates(arrays, 72)           # kinds cycle 4, 6, 1, 0, 6, 4
    sets = [[0, 1, 2, 3], [3, 2, 1, 0], [4], [5, 9, 10], [0, 1, 2, 3, 4, 5, 6, 7], [7, 6, 1]]
    d2, prefix, S = g.gate_joint(*cand, sets, return_prefix=True, return_innovation=True)
    d22, floor = ref.gate_joint(cand, sets, ref.sigma_pair())
    worst = float(np.max(np.abs(d2 / d22 - 1)))
    print(f"{name}: joint d2 worst {worst:.3g}, floor {floor:.3g}")
    assert floor <= FLOOR_MAX and worst <= tolerance(floor)
    dims = [sum(EDGE_DIM[int(cand[0][c])] for c in s) for s in sets]
    assert dims[:3] == [7, 7, 1] and [x.shape[0] for x in S] == dims
    for s, members in enumerate(sets):
        assert prefix[s][-1] == d2[s]
        for k in range(len(members)):
            cut = g.gate_joint(*cand, [members[:k + 1]])
            assert cut[0] == prefix[s][k], (s, k)
    # a set of one candidate is the single gate, and its S the gate's
    d2s, _, Ss = g.gate_edges(*cand, return_innovation=True)
    assert np.allclose(d2[2], d2s[4], rtol=1e-10) and S[2].shape == (1, 1)
    # block independence: the blocks of candidates (0, 1) in set 0 and in set 4 have the same bits
    assert np.array_equal(S[0][:2, :2], S[4][:2, :2])
    # ... and set 1 is set 0 reversed: the same blocks, transposed into place
    o0, o1 = np.concatenate([[0], np.cumsum([EDGE_DIM[int(cand[0][c])] for c in sets[0]])]), np.concatenate([[0], np.cumsum([EDGE_DIM[int(cand[0][c])] for c in sets[1]])])
    for i, ci in enumerate(sets[0]):
        for j, cj in enumerate(sets[0]):
            i1, j1 = sets[1].index(ci), sets[1].index(cj)
            assert np.array_equal(S[0][o0[i]:o0[i + 1], o0[j]:o0[j + 1]], S[1][o1[i1]:o1[i1 + 1], o1[j1]:o1[j1 + 1]])


@pytest.mark.parametrize("name", ["mixed", "corridor"])
@pytest.mark.parametrize("state", ["initial", "converged"])
def test_check_edges(api, name, state):
    """every edge: r absolute, R and d2 relative, by the floor rule of tests/check_edges_reference.py (d2 and R where r >=
    0.01, d2 only where no direction of the residual is a bridge); independent of order, repeats and a shorter list"""
    arrays = case(name) if state == "initial" else converged(name)
    g = api[0].from_arrays(*arrays)
    ref = BearingRangeReference(arrays)
    E = len(arrays[2])
    chk = ref.check(range(E), ref.sigma_pair())
    out = g.check_edges(return_residual=True)
    cR, c = np.flatnonzero(chk["compared"]), np.flatnonzero(chk["compared"] & ~chk["singular"])
    worst_r = float(np.max(np.abs(out["redundancy"] - chk["r"])))
    worst_R = max(rel_diff(out["R"][q], chk["R"][q]) for q in cR)
    worst_d = float(np.max(np.abs(out["d2"][c] / chk["d2"][c] - 1)))
    br = np.flatnonzero(np.isin(arrays[2], (BEARING, RANGE)))
    print(f"{name} {state}: {E} edges ({len(br)} bearing / range), {len(cR)} compared in R, {len(c)} in d2: r worst {worst_r:.3g} (floor "
          f"{chk['floor_r']:.3g}), R {worst_R:.3g} (floor {chk['floor_R']:.3g}), d2 {worst_d:.3g} (floor {chk['floor_d2']:.3g})")
    assert max(chk["floor_r"], chk["floor_R"], chk["floor_d2"]) <= FLOOR_MAX
    assert set(br) <= set(c)                         # every edge of the new kinds is compared in full
    for q in br:
        assert out["R"][q].shape == (1, 1)
    assert worst_r <= tolerance(chk["floor_r"]) and worst_R <= tolerance(chk["floor_R"])
    assert np.all(np.isfinite(out["d2"][c])) and worst_d <= tolerance(chk["floor_d2"])
    perm = np.array([int(br[0]), 0, int(br[5]), int(br[0]), E - 1, 3])
    sub_out = g.check_edges(perm, return_residual=True)
    for key in ("d2", "redundancy", "chi2"):
        assert np.array_equal(sub_out[key], out[key][perm], equal_nan=True), key
    assert all(np.array_equal(sub_out["R"][q], out["R"][k]) for q, k in enumerate(perm))
    suspects = g.suspect_edges()
    assert all(out["d2"][k] > {1: 3.841, 2: 5.991, 3: 7.815}[EDGE_DIM[int(arrays[2][k])]] for k in suspects)


def test_check_edges_sees_the_two_bridges_of_tri2(api):
    arrays = converged("tri2")
    g = api[0].from_arrays(*arrays)
    out = g.check_edges()
    br = np.flatnonzero(arrays[2] == BEARING)
    print(f"tri2: redundancy {out['redundancy']}")
    assert len(br) == 2 and np.all(np.abs(out["redundancy"][br]) <= 1e-6)
    three = api[0].from_arrays(*converged("tri")).check_edges()
    assert np.all(three["redundancy"][np.flatnonzero(case("tri")[2] == BEARING)] > 0.01)


def bounded_handle(api, monkeypatch, make, bound=None):
    """make() under the workspace bound RR_PGO_TS_WS_BYTES = bound (read when the handle is built); None: the default"""
    if bound is None:
        return make()
    monkeypatch.setenv("RR_PGO_TS_WS_BYTES", str(bound))
    g = make()
    monkeypatch.delenv("RR_PGO_TS_WS_BYTES")
    return g


def needed_bytes(api, call, what):
    """the bytes the refusal of a one-item call names on a handle whose bound is 1"""
    import re
    from rustrobotics_amd import _lib
    with pytest.raises(api[2]) as e:
        call()
    assert e.value.code == _lib.ENOMEM, e.value
    msg = _lib.load().rr_pgo_last_error().decode()
    m = re.fullmatch(rf"rr_pgo_\w+: one {what} needs (\d+) bytes of workspace", msg)
    assert m, msg
    return int(m.group(1))


def same_lists(got, want):
    return len(got) == len(want) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, want))


def test_a_plan_cut_by_the_workspace_bound_gives_the_same_bits(api, monkeypatch):
    """`corridor`: 24 candidates that name 48 distinct nodes (at least 120 scalar columns, four chunks of 32), 24 edges with
    distinct `to` nodes and 6 sets of 4 of the candidates.  A handle whose workspace bound is the largest need of a single item
    must cut each plan (the reasoning of the test of this name in tests/test_gate_gpu.py); the instantiation is chosen by the
    whole call, so every piece runs the same code: the cut changes no bit of d2, chi2, S, r, R and the prefixes."""
    arrays = converged("corridor")
    make = lambda: api[0].from_arrays(*arrays)
    cand = candidates(arrays, 74, n=24, distinct=True)
    assert len(set(cand[1]) | set(cand[2])) == 48 and {int(k) for k in cand[0]} == {SE2, SE2_XY, BEARING, RANGE}
    edges, seen = [], set()
    for k in np.random.default_rng(75).permutation(len(arrays[2])):
        if int(arrays[4][k]) not in seen and int(arrays[3][k]) not in seen and len(edges) < 24:
            seen.update((int(arrays[3][k]), int(arrays[4][k])))
            edges.append(int(k))
    edges = np.array(edges, np.int32)
    assert len(edges) == 24 and np.any(np.isin(arrays[2][edges], (BEARING, RANGE))) and np.any(arrays[2][edges] == SE2)
    sets = [list(range(4 * s, 4 * s + 4)) for s in range(6)]
    full, tiny = make(), bounded_handle(api, monkeypatch, make, 1)
    calls = {
        "candidate": (lambda g, q: g.gate_edges(*(cand if q is None else sub(cand, np.array([q]))), return_innovation=True), 24),
        "edge": (lambda g, q: [v for _, v in sorted(g.check_edges(edges if q is None else edges[q:q + 1], return_residual=True).items())], 24),
        "set": (lambda g, q: g.gate_joint(*cand, sets if q is None else [sets[q]], return_prefix=True, return_innovation=True), 6),
    }
    for what, (call, n) in calls.items():
        want = call(full, None)
        need = [needed_bytes(api, lambda q=q: call(tiny, q), what) for q in range(n)]
        g = bounded_handle(api, monkeypatch, make, max(need))
        got = call(g, None)
        print(f"corridor, {n} {what}s alone: workspace needs {min(need)} .. {max(need)} bytes")
        for x, y in zip(got, want):
            assert same_lists(x, y) if isinstance(x, list) else np.array_equal(x, y, equal_nan=True), what


def test_a_cut_plan_on_a_handle_without_the_kinds_with_one_bearing_candidate(api, monkeypatch):
    """simulation-pose-landmark, which has no edge of the kinds: 12 candidates on 24 distinct nodes (at least 60 columns, two
    chunks), ONE of them a bearing.  Under the bound of a single candidate the plan is cut, and the pieces without the bearing
    run the instantiation the whole call chose: the same bits as on the handle that does not cut."""
    make = lambda: api[0].new(g2o_path("simulation-pose-landmark"))
    full = make()
    arrays = full.graph_arrays()
    kinds = [SE2_XY, SE2, SE2, SE2_XY, SE2, SE2_XY, SE2, BEARING, SE2_XY, SE2, SE2_XY, SE2]
    cand = candidates(arrays, 76, n=12, kinds=kinds, distinct=True)
    assert int(np.sum(np.isin(cand[0], (BEARING, RANGE)))) == 1 and len(set(cand[1]) | set(cand[2])) == 24
    want = full.gate_edges(*cand, return_innovation=True)
    tiny = bounded_handle(api, monkeypatch, make, 1)
    need = [needed_bytes(api, lambda q=q: tiny.gate_edges(*sub(cand, np.array([q])), return_innovation=True), "candidate") for q in range(12)]
    got = bounded_handle(api, monkeypatch, make, max(need)).gate_edges(*cand, return_innovation=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_lists(got[2], want[2])


# ---- 6. the live handle -------------------------------------------------------------------------------------------------------

def grown(arrays, with_xy):
    """a new landmark behind `mixed`, seen by a bearing from pose 3 and a range from pose 5 (and, with_xy, an SE2_XY from pose 4)"""
    n = len(arrays[0])
    ref = BearingRangeReference(arrays)
    ref.x.append(np.array([6.0, 4.0, 0.0, 0.0]))
    kind = [BEARING, RANGE] + ([SE2_XY] if with_xy else [])
    frm = [3, 5] + ([4] if with_xy else [])
    meas = np.concatenate([prediction(ref, k, a, n) + 0.01 for k, a in zip(kind, frm)])
    info = np.concatenate([[2500.0], [400.0]] + ([[900.0, 100.0, 1200.0]] if with_xy else []))
    return (np.array(kind, np.int32), np.array(frm, np.int32), np.full(len(kind), n, np.int32), meas, info), ref.x[n][:2] + 0.05


def test_extend_with_node_state_keeps_the_old_bits_and_equals_a_fresh_handle(api):
    arrays = case("mixed")
    g = api[0].from_arrays(*arrays)
    g.optimize(2)
    before = g.state()
    edges, l_state = grown(arrays, False)
    first = g.extend(*edges, node_kind=[1], node_state=l_state)
    assert first == (len(arrays[0]), len(arrays[2]))
    st = g.state()
    assert np.array_equal(st[:len(before)], before) and np.array_equal(st[len(before):], l_state)
    full = [np.concatenate([arrays[0], [1]]).astype(np.int32), st] + [np.concatenate([arrays[2 + i], edges[i]]) for i in range(5)]
    fresh = api[0].from_arrays(*full)
    ref = BearingRangeReference(full)
    np.testing.assert_allclose(g.global_error(), ref.cost(), rtol=1e-12)
    np.testing.assert_allclose(g.global_error(), fresh.global_error(), rtol=1e-12)   # (a fresh handle takes cos / sin of the read-back angle)
    eg, ef = np.array(g.optimize(5)), np.array(fresh.optimize(5))
    eo, _ = ref.optimize(5)
    assert len(eg) == len(eo) == len(ef)
    np.testing.assert_allclose(eg, eo, rtol=1e-7)
    np.testing.assert_allclose(ef, eo, rtol=1e-7)
    np.testing.assert_allclose(g.state(), ref.state(), rtol=0, atol=1e-6)
    # get_graph round trip: the grown graph in the packing of the header, one value each for the new kinds
    nk, ns, ek, a, b, em, ei = g.graph_arrays()
    assert np.array_equal(ek, full[2]) and np.array_equal(a, full[3]) and np.array_equal(b, full[4])
    assert np.array_equal(em, full[5]) and np.array_equal(ei, full[6]) and np.array_equal(nk, full[0])


def test_extend_guess_mode(api):
    """a bearing or range edge yields no guess step: a new landmark that only such edges reach is refused, the node named, the
    handle untouched; with an SE2_XY edge from a ready pose it is guessed from that edge, l = t + R z"""
    arrays = case("mixed")
    g = api[0].from_arrays(*arrays)
    n = len(arrays[0])
    before, chi = g.state(), g.global_error()
    edges, _ = grown(arrays, False)
    with pytest.raises(api[2]) as e:
        g.extend(*edges, node_kind=[1])
    assert e.value.code == EINVAL and f"(node {n})" in str(e.value) and "no initial value" in str(e.value), str(e.value)
    assert g.num_nodes == n and g.num_edges == len(arrays[2]) and np.array_equal(g.state(), before) and g.global_error() == chi
    edges, _ = grown(arrays, True)
    g.extend(*edges, node_kind=[1])
    assert g.num_nodes == n + 1 and g.num_edges == len(arrays[2]) + 3
    st = g.state()
    ref = BearingRangeReference(arrays)
    x, z = ref.x[4], edges[3][2:4]
    want = x[:2] + np.array([x[2] * z[0] - x[3] * z[1], x[3] * z[0] + x[2] * z[1]])
    np.testing.assert_allclose(st[-2:], want, rtol=0, atol=1e-12)
    assert np.array_equal(st[:-2], before)
    full = [np.concatenate([arrays[0], [1]]).astype(np.int32), st] + [np.concatenate([arrays[2 + i], edges[i]]) for i in range(5)]
    np.testing.assert_allclose(g.global_error(), BearingRangeReference(full).cost(), rtol=1e-12)


def test_remove_a_bearing_edge_out_of_a_parallel_pair(api):
    arrays = converged("mixed")
    g = api[0].from_arrays(*arrays)
    k = mixed_marks()["parallel"][0]
    assert arrays[2][k] == BEARING
    g.remove_edges([k])
    keep = np.arange(len(arrays[2])) != k
    mo = np.concatenate([[0], np.cumsum([META_LEN[int(x)] for x in arrays[2]])])
    io = np.concatenate([[0], np.cumsum([INFO_LEN[int(x)] for x in arrays[2]])])
    rest = [arrays[0], arrays[1], arrays[2][keep], arrays[3][keep], arrays[4][keep],
            np.concatenate([arrays[5][mo[q]:mo[q + 1]] for q in np.flatnonzero(keep)]),
            np.concatenate([arrays[6][io[q]:io[q + 1]] for q in np.flatnonzero(keep)])]
    fresh = api[0].from_arrays(*rest)
    assert g.num_edges == len(arrays[2]) - 1 and g.global_error() == fresh.global_error()
    np.testing.assert_allclose(g.global_error(), BearingRangeReference(rest).cost(), rtol=1e-12)
    assert np.array_equal(np.array(g.optimize(4)), np.array(fresh.optimize(4))) and np.array_equal(g.state(), fresh.state())
    got = g.graph_arrays()
    assert all(np.array_equal(x, y) for x, y in zip(got[2:], rest[2:]))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals(api):
    arrays = case("mixed")
    nk, ns, ek, ef, et, em, ei = arrays
    poses, lms = np.flatnonzero(nk == 0).astype(np.int32), np.flatnonzero(nk == 1).astype(np.int32)

    def with_edge(kind, a, b, meas=0.3, info=100.0):
        return (nk, ns, np.concatenate([ek, [kind]]).astype(np.int32), np.concatenate([ef, [a]]).astype(np.int32),
                np.concatenate([et, [b]]).astype(np.int32), np.concatenate([em, [meas]]), np.concatenate([ei, [info]]))

    # rr_pgo_create: wrong endpoints, a non-positive information value, the reserved kinds
    for kind in (BEARING, RANGE):
        for a, b in ((poses[0], poses[1]), (lms[0], lms[1]), (lms[0], poses[0])):
            with pytest.raises(api[2]) as e:
                api[0].from_arrays(*with_edge(kind, a, b))
            assert e.value.code == EINVAL and "endpoint kinds do not match the edge kind" in str(e.value), str(e.value)
        for info in (0.0, -1.0):
            with pytest.raises(api[2]) as e:
                api[0].from_arrays(*with_edge(kind, poses[0], lms[0], info=info))
            assert e.value.code == EINVAL and "must be positive" in str(e.value), str(e.value)
    for kind in (5, 7):
        with pytest.raises(api[2]) as e:
            api[0].from_arrays(*with_edge(kind, poses[0], lms[0]))
        assert e.value.code == EINVAL and "bad edge kind" in str(e.value), str(e.value)
    # a sharded handle
    with pytest.raises(api[2]) as e:
        api[0].from_arrays(*arrays, sharded=True)
    assert e.value.code == EUNSUPPORTED and "bearing" in str(e.value), str(e.value)
    # rr_pgo_extend: wrong endpoints and reserved kinds, the handle untouched
    g = api[0].from_arrays(*arrays)
    before = g.state()
    for kind, a, b, what in ((BEARING, poses[0], poses[1], "endpoint kinds"), (RANGE, lms[0], poses[1], "endpoint kinds"),
                             (5, poses[0], lms[0], "bad edge kind 5"), (7, poses[0], lms[0], "bad edge kind 7")):
        with pytest.raises(api[2]) as e:
            g.extend([kind], [a], [b], [0.3], [100.0])
        assert e.value.code == EINVAL and what in str(e.value), str(e.value)
    with pytest.raises(api[2]) as e:
        g.extend([BEARING], [poses[0]], [lms[0]], [0.3], [0.0])
    assert e.value.code == EINVAL and "must be positive" in str(e.value), str(e.value)
    assert g.num_edges == len(ek) and np.array_equal(g.state(), before)
    # the gate: wrong endpoints per entry point, nothing written (the call itself, on marked buffers)
    from rustrobotics_amd import _lib
    L = _lib.load()
    dp, ip = (lambda x: x.ctypes.data_as(C.POINTER(C.c_double))), (lambda x: x.ctypes.data_as(C.POINTER(C.c_int32)))
    bad = {"an SE2_BEARING edge goes from an SE2 pose to an XY landmark": (BEARING, poses[1], poses[2]),
           "an SE2_RANGE edge goes from an SE2 pose to an XY landmark": (RANGE, lms[0], poses[2])}
    for what, (kind, a, b) in bad.items():
        cand = (np.array([BEARING, kind], np.int32), np.array([poses[0], a], np.int32), np.array([lms[0], b], np.int32),
                np.array([0.3, 0.4]), np.array([100.0, 100.0]))
        with pytest.raises(api[2]) as e:
            g.gate_edges(*cand)
        assert e.value.code == EINVAL and "candidate 1" in str(e.value) and what in str(e.value), str(e.value)
        with pytest.raises(api[2]) as e:
            g.gate_joint(*cand, [[0, 1]])
        assert e.value.code == EINVAL and "candidate 1" in str(e.value) and what in str(e.value), str(e.value)
        d2, chi2, sout, off = np.full(2, -7.0), np.full(2, -7.0), np.full(18, -7.0), np.full(3, -7, np.int64)
        rc = L.rr_pgo_gate_edges(g._h, 2, ip(cand[0]), ip(cand[1]), ip(cand[2]), dp(cand[3]), dp(cand[4]), dp(d2), dp(chi2), dp(sout),
                                 off.ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == EINVAL
        assert np.all(d2 == -7.0) and np.all(chi2 == -7.0) and np.all(sout == -7.0) and np.all(off == -7)
        # rr_pgo_gate_joint, one set of both: d2, the prefixes, S and the offsets stay marked
        ptr, members = np.array([0, 2], np.int32), np.array([0, 1], np.int32)
        jd2, jpre, jout, joff = np.full(1, -7.0), np.full(2, -7.0), np.full(48 * 48, -7.0), np.full(2, -7, np.int64)
        rc = L.rr_pgo_gate_joint(g._h, 2, ip(cand[0]), ip(cand[1]), ip(cand[2]), dp(cand[3]), dp(cand[4]), 1, ip(ptr), ip(members),
                                 dp(jd2), dp(jpre), dp(jout), joff.ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == EINVAL and np.all(jd2 == -7.0) and np.all(jpre == -7.0) and np.all(jout == -7.0) and np.all(joff == -7)
        # rr_pgo_extend with the same two edges: nothing of the handle changes, and the graph it shows is the old one
        rc = L.rr_pgo_extend(g._h, 0, None, None, None, 2, ip(cand[0]), ip(cand[1]), ip(cand[2]), dp(cand[3]), dp(cand[4]))
        assert rc == EINVAL and g.num_edges == len(ek) and np.array_equal(g.state(), before)
        assert all(np.array_equal(x, y) for x, y in zip(g.graph_arrays()[2:], arrays[2:]))
    with pytest.raises(api[2]) as e:
        g.gate_edges([BEARING], [poses[0]], [lms[0]], [0.3], [-2.0])
    assert e.value.code == EINVAL and "not positive definite" in str(e.value), str(e.value)
    for kind in (5, 7):
        with pytest.raises(api[2]) as e:
            g.gate_edges(np.array([kind], np.int32), poses[:1], lms[:1], [0.3], [100.0])
        assert e.value.code == EINVAL and f"unknown edge kind {kind}" in str(e.value), str(e.value)
    # a 3-D node next to the graph of a bearing: mixed, as ever
    with pytest.raises(api[2]) as e:
        api[0].from_arrays(np.array([0, 1, 3], np.int32), np.zeros(8), np.array([BEARING], np.int32), np.array([0], np.int32),
                           np.array([1], np.int32), np.array([0.3]), np.array([100.0]))
    assert e.value.code == EINVAL and "mixed 2D / 3D" in str(e.value)


@pytest.mark.parametrize("form", ["1", "2"])
def test_edge_parallel_forms_refuse_the_kinds(api, monkeypatch, form):
    """RR_PGO_EDGE_LINEARIZE is read when a handle is built: a graph with one of the kinds is refused there, as rr_pgo_set_fixed
    and rr_pgo_set_priors refuse such handles; a graph without them is built as ever"""
    monkeypatch.setenv("RR_PGO_EDGE_LINEARIZE", form)
    with pytest.raises(api[2]) as e:
        api[0].from_arrays(*case("tri"))
    assert e.value.code == EUNSUPPORTED and "RR_PGO_EDGE_LINEARIZE" in str(e.value), str(e.value)
    arrays = case("tri")
    keep = np.flatnonzero(arrays[2] == SE2)
    g = api[0].from_arrays(arrays[0][:3], arrays[1][:9], arrays[2][keep], arrays[3][keep], arrays[4][keep], arrays[5][:6], arrays[6][:12])
    assert np.isfinite(g.global_error())
    with pytest.raises(api[2]) as e:
        g.extend([BEARING], [0], [3], [0.3], [100.0], node_kind=[1], node_state=[2.0, 3.0])
    assert e.value.code == EUNSUPPORTED and g.num_nodes == 3


def test_a_handle_without_the_kinds_gates_candidates_of_the_kinds(api):
    """candidates are not part of the graph: a handle on simulation-pose-landmark gates bearing and range candidates by the floor
    rule.  Its SE2 / SE2_XY candidates agree with a call without a candidate of the kinds to ROUNDING (1e-12), not bit for bit:
    such a call runs k_gate_pairs<double, 3, false>, the mixed one <double, 3, true>, and two instantiations promise no common
    bits -- the one exception to "a candidate's bits do not depend on what else the call asks for", stated in the header"""
    g = api[0].new(g2o_path("simulation-pose-landmark"))
    arrays = g.graph_arrays()
    ref = BearingRangeReference(arrays)
    cand = candidates(arrays, 73, n=12)
    d2, chi2, S = g.gate_edges(*cand, return_innovation=True)
    S2, d22, chi22, fS, fd = ref.gate(cand, ref.sigma_pair())
    assert max(fS, fd) <= FLOOR_MAX
    assert max(rel_diff(x, y) for x, y in zip(S, S2)) <= tolerance(fS) and float(np.max(np.abs(d2 / d22 - 1))) <= tolerance(fd)
    old = np.flatnonzero(np.isin(cand[0], (SE2, SE2_XY)))
    d2o, _ = g.gate_edges(*sub(cand, old))
    np.testing.assert_allclose(d2o, d2[old], rtol=1e-12)


# ---- 8. handles without the kinds are untouched -----------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "bearing_range_untouched.json")
KERNELS = os.path.join(os.path.dirname(__file__), "golden", "landmarks3d_pure_se3.json")


def test_handles_without_the_kinds_report_what_they_did(api):
    """a handle on simulation-pose-landmark and one on dlr report the statistics and the launch counts of the commit before the
    kinds (taken there, on the GPU), the library still exports every kernel name of tests/golden/landmarks3d_pure_se3.json, and
    the new instantiations are there under their own names"""
    from rustrobotics_amd import _lib
    names = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in json.load(open(KERNELS))["kernel_names"]:
        assert name in names, name
    assert "k_linearize_br<" in names
    fx = json.load(open(GOLDEN))
    for graph, want in fx["stats"].items():
        g = api[0].new(g2o_path(graph))
        g.optimize(3)
        st = g.stats()
        for key, value in want.items():
            assert st[key] == value, (graph, key, st[key], value)
