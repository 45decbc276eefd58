"""rr_pgo_check_edges without a GPU: the identity the leave-one-out distance rests on, the Python mirror, and the condition
on the fixtures of tests/test_check_edges_gpu.py, asserted on the reference alone."""
import os

import numpy as np
import pytest

from check_edges_cases import BRIDGE_ONLY, DATASET_EDGES, PARTIAL, ROBUST, SMALL, at_state, reference, robust_mask, seeded_edges
from check_edges_reference import MIN_REDUNDANCY, pose_cycle_edges, residual
from conftest import g2o_path
from gate_cases import GATE_GRAPHS
from query_small_cases import STATES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_leave_one_out_distance_is_the_gate_of_the_graph_without_the_edge():
    """A linear problem: minimise sum_k |J_k x - z_k|^2_Omega_k.  For edge c: e and R at the optimum of the whole problem;
    e_without and S_without = Omega^-1 + J Sigma_without J^T at the optimum of the problem without c.  The two distances
    agree to rounding (Woodbury), and so does S_without = Omega^-1 R^-1 Omega^-1."""
    rng = np.random.default_rng(11)
    n, m, d = 12, 9, 3
    J = [rng.normal(size=(d, n)) for _ in range(m)]
    z = [rng.normal(size=d) for _ in range(m)]
    W = []
    for _ in range(m):
        a = rng.normal(size=(d, d))
        W.append(a @ a.T + d * np.eye(d))

    def optimum(keep):
        H = sum(J[k].T @ W[k] @ J[k] for k in keep)
        x = np.linalg.solve(H, sum(J[k].T @ W[k] @ z[k] for k in keep))
        return x, np.linalg.inv(H)

    x, sigma = optimum(range(m))
    worst = 0.0
    for c in range(m):
        e = J[c] @ x - z[c]
        R = np.linalg.inv(W[c]) - J[c] @ sigma @ J[c].T
        d2 = float(e @ np.linalg.solve(R, e))
        xw, sw = optimum([k for k in range(m) if k != c])
        ew = J[c] @ xw - z[c]
        S = np.linalg.inv(W[c]) + J[c] @ sw @ J[c].T
        d2w = float(ew @ np.linalg.solve(S, ew))
        Wi = np.linalg.inv(W[c])
        worst = max(worst, abs(d2 - d2w) / d2w, float(np.max(np.abs(Wi @ np.linalg.inv(R) @ Wi - S)) / np.max(np.abs(S))))
        r = np.trace(R @ W[c]) / d
        assert 0.0 < r < 1.0
    print(f"worst relative difference of the two distances and of S_without: {worst:.3g}")
    assert worst <= 1e-10


def test_residual_of_a_bridge_and_of_a_fixed_pair():
    rng = np.random.default_rng(12)
    a = rng.normal(size=(3, 3))
    W = a @ a.T + 3 * np.eye(3)
    A, B, e = rng.normal(size=(3, 3)), rng.normal(size=(3, 3)), rng.normal(size=3)
    # both endpoints fixed: Sigma = 0, R = Omega_w^-1, r = 1, d2 = e^T Omega_w e
    R, d2, r, r_min = residual(e, A, B, W, 0.25, np.zeros((6, 6)))
    assert abs(r - 1.0) <= 1e-14 and abs(r_min - 1.0) <= 1e-14 and abs(d2 - 0.25 * float(e @ W @ e)) <= 1e-12 * d2
    # a bridge on a free node: H_bb = B^T Omega_w B alone, so P = Omega_w^-1 and R = 0 up to rounding
    sig = np.zeros((6, 6))
    sig[3:, 3:] = np.linalg.inv(B.T @ (0.25 * W) @ B)
    R, _, r, r_min = residual(e, A, B, W, 0.25, sig)
    assert abs(r) <= 1e-12 and r < MIN_REDUNDANCY and abs(r_min) <= 1e-12


def test_exports_are_declared_in_header_mirror_and_integration_guide():
    from rustrobotics_amd import _lib
    header = open(os.path.join(ROOT, "include", "rr_pgo.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("rr_pgo_check_edges", "rr_pgo_check_edges_times", "rr_pgo_remove_edges", "rr_pgo_remove_edges_times"):
        assert name in _lib.EXPORTS and f"int {name}(" in header and f"pub fn {name}(" in guide, name
    assert _lib.ABI_VERSION == 4


def test_select_suspects_by_redundancy_direction_and_threshold_sorted_by_falling_distance():
    from rustrobotics_amd.mapping import select_suspects
    #            SE2    SE2    XY     SE2   SE2 (bridge)  XY     SE2 (NaN)  SE2 (one direction a bridge)
    kind = [0, 0, 1, 0, 0, 1, 0, 0]
    d2 = [9.0, 7.0, 6.5, 100.0, 1e9, 5.0, float("nan"), 1e14]
    red = [0.5, 0.9, 0.02, 0.3, 0.001, 0.8, 0.0, 0.395]
    rmin = [0.4, 0.8, 0.015, 0.2, 0.0, 0.7, 0.0, 1e-16]

    def suspect(**kw):
        return list(select_suspects(kind, d2, red, rmin, **kw))
    assert suspect() == [3, 0, 2]                               # 7.815 / 5.991; the bridge, the NaN and the partial bridge stay out
    assert suspect(threshold=6.0) == [3, 0, 1, 2]
    assert suspect(threshold={0: 50.0, 1: 1.0}) == [3, 2, 5]
    assert suspect(min_redundancy=0.35) == [0]
    assert suspect(min_redundancy=0.0, threshold=8.0) == [3, 0]           # the bridge's R is rounding in every direction
    assert suspect(min_redundancy=0.0, min_directional=-1.0, threshold=8.0) == [7, 4, 3, 0]   # the caller's parameters let them all in
    assert suspect(threshold=1e300) == []


def test_directional_redundancy_recovers_the_smallest_eigenvalue_without_the_weight():
    """the mirror sees R, the UNWEIGHTED Omega and r; the reference knows w"""
    from rustrobotics_amd.mapping import directional_redundancy
    rng = np.random.default_rng(13)
    for d, w in ((3, 1.0), (2, 0.3), (6, 0.02)):
        a = rng.normal(size=(d, d))
        W = a @ a.T + d * np.eye(d)
        L = np.linalg.cholesky(w * W)
        lam = np.sort(rng.uniform(0.0, 1.0, d))
        lam[0] = 0.0 if d == 3 else lam[0]                     # one direction a bridge
        q, _ = np.linalg.qr(rng.normal(size=(d, d)))
        R = np.linalg.inv(L.T) @ (q * lam) @ q.T @ np.linalg.inv(L)
        got = directional_redundancy(R, W, float(np.mean(lam)))
        assert abs(got - lam[0]) <= 1e-12, (d, got, lam[0])


def test_pose_cycle_edges_on_a_known_graph():
    # chain 0-1-2-3, closure 3-1, two parallel edges 4-5, bridge 3-4, a landmark (node 6) seen from 0 and 1
    nk = np.array([0, 0, 0, 0, 0, 0, 1])
    ek = np.array([0, 0, 0, 0, 1, 0, 0, 0, 1])
    ef = np.array([0, 1, 2, 3, 0, 4, 5, 3, 1])
    et = np.array([1, 2, 3, 1, 6, 5, 4, 4, 6])
    assert pose_cycle_edges((nk, None, ek, ef, et)) == [1, 2, 3, 5, 6]


def test_host_part_of_remove_edges_in_a_stand_alone_program(tmp_path):
    """tests/native/remove_edges_check.cpp: the orphan check, the compaction and the anchor rule, under the host sanitizers"""
    import subprocess
    csrc = os.path.join(ROOT, "rustrobotics_amd", "csrc")
    exe = tmp_path / "remove_edges_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "remove_edges_check.cpp"), os.path.join(csrc, "g2o_loader.cpp"),
                           "-pthread", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def condition(label, ref, arrays):
    """what the GPU tests rely on: at least half of the queried edges are compared, among them every queried edge on a cycle
    of pose-pose edges, and the floors stay within FLOOR_MAX"""
    print(ref.summary(label))
    assert ref.floors_ok(), label
    on_cycle = set(pose_cycle_edges(arrays))
    missed = [int(k) for k, c in zip(ref.edges, ref.compared) if int(k) in on_cycle and not c]
    assert not missed, (label, "edges on a pose-pose cycle below the redundancy level", missed)
    assert not np.any(ref.singular), (label, "edges with r >= 0.01 and a singular direction", ref.edges[ref.singular])
    assert np.all(np.isfinite(ref.d2[ref.compared]))
    return int(np.sum(ref.compared)), ref.n


@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("name", SMALL)
def test_small_fixtures_meet_the_condition(name, which):
    arrays, state = at_state(name, which)
    ref = reference((name, which), arrays, state)
    compared, queried = condition(f"{name} {which}", ref, arrays)
    if name in BRIDGE_ONLY:   # nothing to compare by construction: every edge is a bridge, and the reference says so
        assert not pose_cycle_edges(arrays) and compared == 0
        assert np.all(np.abs(ref.r) <= ref.tol_r)
    else:
        assert 2 * compared >= queried, (name, which, compared, queried)
    assert np.all((ref.r >= -ref.tol_r) & (ref.r <= 1.0 + ref.tol_r))


@pytest.mark.parametrize("name", ROBUST)
def test_robust_fixtures_meet_the_condition(name):
    """the moved state, every edge, Cauchy with delta 1 on two edges of three: the floors are those of the two Sigmas alone"""
    from check_edges_reference import CheckReference
    arrays, state = at_state(name, "moved")
    mask = robust_mask(len(arrays[2]))
    ref = reference((name, "moved", "cauchy"), arrays, state, kind="cauchy", delta=1.0, mask=mask)
    compared, queried = condition(f"{name} moved, cauchy", ref, arrays)
    assert 2 * compared >= queried and np.min(ref.w) < 0.5 and np.all(ref.w[mask == 0] == 1.0)
    assert isinstance(ref, CheckReference)


@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("name", PARTIAL)
def test_partial_redundancy_fixtures_have_singular_edges_and_quiet_floors(name, which):
    """what these graphs are kept for: edges at r >= 0.01 whose R is singular in one direction.  r, R and r_min have quiet
    floors there; d2 is compared on the other edges, whose floors hold."""
    arrays, state = at_state(name, which)
    ref = reference((name, which), arrays, state)
    print(ref.summary(f"{name} {which}"), "; singular:", [(int(k), round(float(r), 3), float(m)) for k, r, m in
                                                           zip(ref.edges[ref.singular], ref.r[ref.singular], ref.r_min[ref.singular])])
    assert np.any(ref.singular) and ref.floors_ok() and ref.floor_rmin <= 1e-6
    assert np.all(np.abs(ref.r_min[ref.singular]) <= ref.tol_rmin)      # singular to rounding, not merely weak
    assert np.all(ref.r[ref.singular] >= MIN_REDUNDANCY) and np.max(ref.r[ref.singular]) > 0.25
    assert 2 * int(np.sum(ref.compared & ~ref.singular)) >= ref.n


@pytest.mark.parametrize("name", list(DATASET_EDGES))
def test_dataset_fixtures_meet_the_condition(name):
    from oracle.oracle import OracleGraph
    from robust_reference import oracle_arrays
    o = OracleGraph.load(g2o_path(name))
    arrays = tuple(oracle_arrays(o))
    if GATE_GRAPHS[name]:
        o.optimize(GATE_GRAPHS[name])
    state = o.state()
    edges = seeded_edges(arrays, DATASET_EDGES[name])
    if edges is not None:
        assert len(set(edges.tolist())) == DATASET_EDGES[name]
        assert 2 * int(np.sum(np.abs(arrays[3][edges] - arrays[4][edges]) > 1)) == len(edges)
    ref = reference((name, "oracle"), arrays, state, edges)
    compared, queried = condition(name, ref, arrays)
    assert 2 * compared >= queried, (name, compared, queried)
