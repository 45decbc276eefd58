"""rr_pgo_initialize on the device (include/rr_pgo.h, "initialisation from the measurements") against
tests/chordal_reference.py and against the truth of consistent measurements.  Rotations are compared as matrices."""
import functools
import re
import subprocess
import sys

import numpy as np
import pytest

from chordal_cases import (NOISE_FREE_GPU_BOUND, RING_CASES, RING_IDS, RX_PI, hub_graph, reflection_graph, ring_graph)
from chordal_reference import all_at_node0, chordal_initialize, quat_to_rot, state_diff
from conftest import ROOT, g2o_path
from oracle.oracle import OracleGraph
from random_graphs import pack_upper, random_graph, random_spd

pytestmark = pytest.mark.gpu

EINVAL, ENOTSPD, EUNSUPPORTED = -1, -5, -7
# a state against its CPU reference, f64: the bound of tests/test_gnc_gpu.py
STATE_TOL = 1e-8
# Single-precision factor on the noise-free rings: the worst error against the truth measured on the MI355X (positions of order
# 10: mixed 1.161e-5, f32 1.257e-5 over the four graphs; f64 1.4e-14), and the bound at 10 x that
NOISE_FREE_MEASURED = {"mixed": 1.161e-5, "f32": 1.257e-5}
NOISE_FREE_BOUND = {"f64": NOISE_FREE_GPU_BOUND, "mixed": 10 * NOISE_FREE_MEASURED["mixed"], "f32": 10 * NOISE_FREE_MEASURED["f32"]}
# chi2 of a mixed handle against the f64 one: the tolerance tests/test_gpu_parity.py has for that mode
MIXED_CHI2_RTOL = 1e-8


@pytest.fixture(scope="module")
def api():
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


def unique_projection(info):
    """The inputs sit at no non-unique projection: |u_i| > 1e-3 in 2-D; in 3-D the two smallest singular values of every M_i
    with det M_i < 0 differ by more than 1e-3 relative.  (Where det M_i > 0 the projection is the polar factor, unique whatever
    the gap, and the margin asked for is s2 + s3 > 1e-3 s1: a leaf with ONE edge has M_i = a rotation exactly, all three singular
    values equal, so a gap could not be asked of the hub graphs' leaves at any seed.  chordal_reference's "margin" is both.)"""
    return (not np.isfinite(info["margin"]) or info["margin"] > 1e-3) and (not np.isfinite(info["u_min"]) or info["u_min"] > 1e-3)


def node_slices(nk):
    length = {0: 3, 1: 2, 2: 7, 3: 3}
    off = np.concatenate([[0], np.cumsum([length[int(k)] for k in nk])])
    return [slice(int(off[i]), int(off[i + 1])) for i in range(len(nk))]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---- 1. noise-free graphs

@pytest.mark.parametrize("precision", ["f64", "mixed", "f32"])
@pytest.mark.parametrize("seed,se3,landmarks", RING_CASES, ids=RING_IDS)
def test_noise_free_measurements_are_recovered(api, seed, se3, landmarks, precision):
    arrays, start = ring_graph(seed, se3, landmarks)
    truth = arrays[1]
    g = api[0].from_arrays(arrays[0], start, *arrays[2:], precision=precision)
    assert g.anchor_node == 0
    g.initialize()
    err = state_diff(arrays[0], g.state(), truth)
    print(f"noise-free ring se3={se3} landmarks={landmarks} {precision}: error against the truth {err:.3e}")
    assert err <= NOISE_FREE_BOUND[precision]


# ---- 2. the reflection

def test_reflection_case_ends_at_rx_pi(api):
    arrays, t3 = reflection_graph()
    g = api[0].from_arrays(*arrays)
    g.set_fixed([0, 1, 2])
    g.initialize()
    out = np.array(g.state())
    assert np.max(np.abs(quat_to_rot(out[24:28]) - RX_PI)) <= 1e-14
    assert np.max(np.abs(out[21:24] - t3)) <= 1e-13
    assert out[27] >= 0.0                        # q_w >= 0
    assert same_bits(out[:21], arrays[1][:21])


# ---- 3. the hub

@pytest.mark.parametrize("se3", [False, True], ids=["2d", "3d"])
def test_hub_of_degree_19_matches_the_reference(api, se3):
    arrays, _ = hub_graph(211 + int(se3), se3)
    ref, info = chordal_initialize(arrays, held=[0])
    assert unique_projection(info), info
    g = api[0].from_arrays(*arrays)
    assert g.anchor_node == 0
    g.initialize()
    diff = state_diff(arrays[0], g.state(), ref)
    print(f"hub se3={se3}: state against the reference {diff:.3e}")
    assert diff <= STATE_TOL
    ms = g.initialize_times()
    assert ms[0] > 0 and ms[1] > 0 and ms[2] >= ms[0] + ms[1] - 1e-3


# ---- 4. held nodes and priors

@pytest.mark.parametrize("se3", [False, True], ids=["2d", "3d"])
def test_fixed_nodes_and_priors(api, se3):
    rng = np.random.default_rng(77 + int(se3))
    arrays = list(random_graph(rng, 12, 4, 10, se3))
    nk = arrays[0]
    sl = node_slices(nk)
    g = api[0].from_arrays(*arrays)
    anchor = g.anchor_node
    before = np.array(g.state())
    # (a) two fixed nodes, the anchor free
    g.set_fixed([3, 7], keep_anchor=False)
    ref, info = chordal_initialize(arrays, before, held=[3, 7])
    assert unique_projection(info), info
    g.initialize()
    out = np.array(g.state())
    diff = state_diff(nk, out, ref)
    print(f"fixed [3, 7] se3={se3}: state against the reference {diff:.3e}")
    assert diff <= STATE_TOL
    for v in (3, 7):
        assert same_bits(out[sl[v]], before[sl[v]])
    assert g.fixed_nodes().tolist() == [3, 7]
    # (b) priors on two poses (and, where the graph has one, a landmark), the anchor kept and held
    g.clear_fixed()
    g.set_state(before)
    nodes = [2, 5] + ([len(nk) - 1] if not se3 else [])
    meas = np.concatenate([arrays[1][sl[v]] for v in nodes])
    info_p = np.concatenate([pack_upper(d, random_spd(rng, d)) for d in [{0: 3, 1: 2, 2: 6}[int(nk[v])] for v in nodes]])
    g.set_priors(nodes, meas, info_p, keep_anchor=True)
    start = np.array(g.state())
    ref, info = chordal_initialize(arrays, start, held=[anchor], priors=(nodes, meas, info_p))
    assert unique_projection(info), info
    g.initialize()
    out = np.array(g.state())
    diff = state_diff(nk, out, ref)
    print(f"priors on {nodes} se3={se3}: state against the reference {diff:.3e}")
    assert diff <= STATE_TOL
    assert same_bits(out[sl[anchor]], start[sl[anchor]])
    assert g.num_priors == len(nodes)


# ---- 5. the datasets: sphere2500 (fronts beyond LDS) and M3500 (the dataflow launches at size)

@functools.lru_cache(maxsize=None)
def dataset_reference(name):
    """(arrays, the start "every node at node 0's pose", the reference's state from there, its chi2)"""
    from robust_reference import oracle_arrays
    arrays = oracle_arrays(OracleGraph.load(g2o_path(name)))
    anchor = int(arrays[3][np.flatnonzero((arrays[2] == 0) | (arrays[2] == 2))[0]])
    start = all_at_node0(arrays)
    ref, info = chordal_initialize(arrays, start, held=[anchor])
    a = list(arrays)
    a[1] = ref
    return arrays, start, ref, OracleGraph.from_arrays(*a).global_error(), info, anchor


@pytest.mark.parametrize("name", ["sphere2500", "input_M3500_g2o"])
def test_datasets_from_every_node_at_node_0(api, name):
    arrays, start, ref, ref_chi2, info, anchor = dataset_reference(name)
    assert unique_projection(info), info
    g = api[0].new(g2o_path(name))
    assert g.anchor_node == anchor
    assert (g.stats()["n_big_fronts"] != 0) == (name == "sphere2500")
    from_file = api[0].new(g2o_path(name)).optimize(10)[-1]
    g.set_state(start)
    g.initialize()
    diff = state_diff(arrays[0], g.state(), ref)
    chi2 = g.global_error()
    print(f"{name}: state against the reference {diff:.3e}, chi2 {chi2:.6f} (reference {ref_chi2:.6f}), times {g.initialize_times()}")
    assert diff <= STATE_TOL
    assert abs(chi2 - ref_chi2) <= 1e-6 * ref_chi2
    final = g.optimize(10)[-1]
    print(f"{name}: optimize(10) from the chordal state {final:.8f}, from the file's vertices {from_file:.8f}")
    assert abs(final - from_file) <= 1e-6 * from_file


def test_sphere2500_mixed_reaches_the_same_optimum(api):
    _, start, _, _, _, _ = dataset_reference("sphere2500")
    g64, gm = api[0].new(g2o_path("sphere2500")), api[0].new(g2o_path("sphere2500"), precision="mixed")
    out = []
    for g in (g64, gm):
        g.set_state(start)
        g.initialize()
        out.append(g.optimize(10)[-1])
    print(f"sphere2500: initialize + optimize(10), f64 {out[0]:.10f}, mixed {out[1]:.10f}")
    assert abs(out[1] - out[0]) <= MIXED_CHI2_RTOL * out[0]


# ---- 6. determinism, and what the call leaves alone

@pytest.mark.parametrize("se3", [False, True], ids=["2d", "3d"])
def test_two_handles_give_the_same_bits(api, se3):
    arrays, _ = hub_graph(311 + int(se3), se3)
    states = []
    for _ in range(2):
        g = api[0].from_arrays(*arrays)
        g.initialize()
        states.append(np.array(g.state()))
    assert same_bits(states[0], states[1])


def launch_counts(g):
    st = g.stats()
    return [st[k] for k in ("n_plain_iterations", "n_graph_replays", "n_loop_items", "n_graph_captures")]


@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
@pytest.mark.parametrize("captured", [False, True], ids=["plain", "captured"])
def test_a_handle_that_initialised_iterates_like_a_fresh_one(api, monkeypatch, captured, solver):
    path = g2o_path("simulation-pose-landmark")
    if captured:
        monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    a, b = api[0].new(path, api[1][solver]), api[0].new(path, api[1][solver])
    if captured:
        monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    s0 = np.array(b.state())
    if captured:
        a.iterate_async(1)
        a.sync()
        assert launch_counts(a)[3] == 1
        a.set_state(s0)
    counts = launch_counts(a)
    a.initialize()
    assert launch_counts(a) == counts                    # no iteration counted, no capture made or dropped
    assert not same_bits(a.state(), s0)
    a.set_state(s0)
    b.set_state(s0)
    assert np.array_equal(np.array(a.optimize(5)), np.array(b.optimize(5)))
    assert same_bits(a.state(), b.state())
    if captured:
        assert launch_counts(a)[3] == 1


def test_settings_are_untouched(api):
    rng = np.random.default_rng(5)
    arrays = list(random_graph(rng, 12, 4, 10, False))
    sl = node_slices(arrays[0])
    g = api[0].from_arrays(*arrays)
    mask = (np.arange(g.num_edges) % 2).astype(np.int32)
    g.set_robust_kernel("cauchy", 2.5, mask)
    nodes = [4, 13]
    meas = np.concatenate([arrays[1][sl[v]] for v in nodes])
    info = np.concatenate([pack_upper(3, random_spd(rng, 3)), pack_upper(2, random_spd(rng, 2))])
    g.set_priors(nodes, meas, info, robust=[1, 0], keep_anchor=True)
    g.set_fixed([6, 9])
    setting = g.robust_setting
    g.initialize()
    assert g.robust_setting == setting == (2, 2.5, 0.0)
    assert g.num_priors == 2 and g.fixed_nodes().tolist() == [6, 9]
    # the mask and the priors' flags still act: the weights of a handle given the same settings and the same state
    h = api[0].from_arrays(*arrays)
    h.set_robust_kernel("cauchy", 2.5, mask)
    h.set_priors(nodes, meas, info, robust=[1, 0], keep_anchor=True)
    h.set_fixed([6, 9])
    s = g.state()   # (through rr_pgo_get_state's angles: both handles take the same round trip)
    g.set_state(s)
    h.set_state(s)
    for x, y in zip(g.edge_errors() + g.prior_errors(), h.edge_errors() + h.prior_errors()):
        assert np.array_equal(x, y)
    assert np.array_equal(np.array(g.optimize(3)), np.array(h.optimize(3)))


# ---- 7. refusals: an error code, and the state as it was

def refused(g, code, call, *needles):
    from rustrobotics_amd.mapping import PoseGraphError
    before = np.array(g.state())
    with pytest.raises(PoseGraphError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for needle in needles:
        assert needle in str(e.value), str(e.value)
    assert same_bits(g.state(), before)


@pytest.mark.parametrize("se3", [False, True], ids=["2d", "3d"])
def test_refusals_change_nothing(api, se3):
    arrays, _ = hub_graph(411 + int(se3), se3)
    g = api[0].from_arrays(*arrays)
    refused(g, EINVAL, lambda: g.initialize(7), "unknown method")
    s = api[0].from_arrays(*hub_graph(411, False)[0], sharded=True)
    refused(s, EUNSUPPORTED, lambda: s.initialize(), "sharded")
    # nothing holds the graph: a fixed set that came and went, priors on landmarks alone with the anchor term dropped
    g.set_fixed([2])
    g.clear_fixed()
    lm = len(arrays[0]) - 1
    d = 3 if se3 else 2
    g.set_priors([lm], arrays[1][-d:], pack_upper(d, np.eye(d)), keep_anchor=False)
    refused(g, ENOTSPD, lambda: g.initialize(), "singular")
    g.clear_priors()
    g.initialize()                                         # ... and with the anchor back it runs


def test_a_landmark_seen_by_a_bearing_alone_is_named(api):
    arrays, _ = hub_graph(411, False)
    nk, ns, ek, ef, et, em, ei = arrays
    nk = np.concatenate([nk, [1]]).astype(np.int32)        # one more landmark, node 24, reached by one bearing edge
    ns = np.concatenate([ns, [1.0, 2.0]])
    ek = np.concatenate([ek, [4]]).astype(np.int32)
    ef, et = np.concatenate([ef, [6]]).astype(np.int32), np.concatenate([et, [24]]).astype(np.int32)
    em, ei = np.concatenate([em, [0.3]]), np.concatenate([ei, [10.0]])
    g = api[0].from_arrays(nk, ns, ek, ef, et, em, ei)
    refused(g, EINVAL, lambda: g.initialize(), "landmark node 24")
    # a prior places it: the bearing edge then takes no part, the rest is the reference's
    g.set_priors([24], [1.5, 2.5], pack_upper(2, np.eye(2)))
    ref, _ = chordal_initialize([nk, ns, ek, ef, et, em, ei], held=[0], priors=([24], [1.5, 2.5], pack_upper(2, np.eye(2))))
    g.initialize()
    assert state_diff(nk, g.state(), ref) <= STATE_TOL


# ---- 8. the command line

def test_cli_prints_chi2_before_and_after(api):
    path = g2o_path("parking-garage")
    out = subprocess.run([sys.executable, "-m", "rustrobotics_amd", path, "--init", "chordal", "--iterations", "1"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    m = re.search(r"chordal initialisation: chi2 before (\S+), after (\S+) ", out.stdout)
    assert m, out.stdout
    before, after = float(m.group(1).rstrip(",")), float(m.group(2).rstrip(","))
    from robust_reference import oracle_arrays
    o = OracleGraph.load(path)
    arrays = oracle_arrays(o)
    ref, _ = chordal_initialize(arrays, held=[api[0].new(path).anchor_node])
    arrays[1] = ref
    ref_after = OracleGraph.from_arrays(*arrays).global_error()
    print(f"parking-garage --init chordal: chi2 before {before}, after {after} (reference {o.global_error()}, {ref_after})")
    assert abs(before - o.global_error()) <= 1e-6 * o.global_error()
    assert abs(after - ref_after) <= 1e-6 * ref_after
