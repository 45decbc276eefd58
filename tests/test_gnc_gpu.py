"""Truncated least squares and rr_pgo_optimize_gnc on the GPU (run with -m gpu on an MI355X), through the Python mirror:
against a plain handle built with Omega scaled by the weights, against the CPU reference on the unchanged oracle
(tests/gnc_reference.py), and what the rest of the toolbox does with weights that are exactly 0."""
import ctypes as C

import numpy as np
import pytest

from conftest import g2o_path
from gnc_reference import GncReference, gnc, tls_band, tls_rho, tls_weight
from robust_reference import intel_with_outliers, position_error

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

DELTA = 3.3682   # delta^2 = 11.345: the 0.99 chi-square quantile of 3 degrees of freedom
# The assembled system: SYSTEM_TOL and the rule of test_priors_gpu.assert_same_system, restated; in f64 it is
# test_robust_kernels_gpu._assert_same_system's (1e-12 of max|vals| for the blocks, 1e-11 for b).
EPS32 = 2.0 ** -24
SYSTEM_TOL = {"f64": (1e-12, 1e-11), "mixed": (1e-12 + EPS32, 1e-11 + EPS32), "f32": (1e-12 * 2.0 ** 29, 1e-11 * 2.0 ** 29)}
EINVAL, ENOTSPD, EUNSUPPORTED = -1, -5, -7


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver, PoseGraphError
    return PoseGraph, PoseGraphSolver, PoseGraphError


def _info_rep(ek):
    from rustrobotics_amd.mapping import GATE_INFO_LEN
    return np.repeat(np.arange(len(ek)), np.take(GATE_INFO_LEN, ek))


def _scaled_arrays(arrays, w, zero=0.0):
    """the graph with Omega scaled by w.  zero: what stands for a weight of exactly 0 -- rr_pgo_create takes an SE2 / SE3 / XY / XYZ
    edge with Omega = 0, but refuses a bearing or range edge whose information value is not positive: there 1e-300 Omega, 280
    orders of magnitude below the tolerance, keeps the edge in the pattern."""
    a = list(arrays)
    a[6] = np.asarray(a[6], np.float64) * np.where(w == 0.0, zero, w)[_info_rep(a[2])]
    return a


def _assert_same_system(label, g, ref, lm, precision="f64"):
    tb, tr = SYSTEM_TOL[precision]
    lam = 0.37 if lm else 0.0
    br, bc, bo, vals, b = g.assemble(lam, lm)
    br2, bc2, bo2, vals2, b2 = ref.assemble(lam, lm)
    assert np.array_equal(br, br2) and np.array_equal(bc, bc2) and np.array_equal(bo, bo2)
    scale = np.abs(vals2).max()
    bscale = max(np.abs(b2).max(), 1e-3 * np.sqrt(scale))
    print(f"{label} {precision} lm={lm}: blocks worst {np.abs(vals - vals2).max():.3g} (bound {tb * scale:.3g}), "
          f"b worst {np.abs(b - b2).max():.3g} (bound {tr * bscale:.3g})")
    assert np.abs(vals - vals2).max() <= tb * scale
    assert np.abs(b - b2).max() <= tr * bscale


def _set_tls_at_the_median(g):
    """delta^2 = the median of the positive s, mu = 1: the band is (delta^2 / 2, 2 delta^2).  All three regimes must be there."""
    s0, _ = g.edge_errors()
    delta = float(np.sqrt(np.median(s0[s0 > 0])))
    g.set_robust_tls(delta, 1.0)
    s, w = g.edge_errors()
    assert np.any(w == 1.0) and np.any((w > 0.0) & (w < 1.0)) and np.any(w == 0.0), (np.sum(w == 1), np.sum(w == 0), len(w))
    return delta, s, w


def _check_system_against_the_scaled_plain_handle(api, label, g, arrays, precision="f64", prep=None, zero=0.0):
    delta, s, w = _set_tls_at_the_median(g)
    ref = api[0].from_arrays(*_scaled_arrays(arrays, w, zero), precision=precision)
    if prep:
        prep(ref)
    st = g.state()
    g.set_state(st)     # the same bits of the state in both handles
    ref.set_state(st)
    for lm in (False, True):
        _assert_same_system(label, g, ref, lm, precision)
    return delta, s, w


# ---- 1. the assembled system --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,steps", [("simulation-pose-landmark", 0), ("intel", 2), ("sphere2500", 2)])
def test_assembled_system_equals_the_plain_system_with_weighted_information(api, name, steps):
    g = api[0].new(g2o_path(name))
    arrays = g.graph_arrays()
    for _ in range(steps):
        g.update_nodes(g.linearize_and_solve())
    delta, s, w = _check_system_against_the_scaled_plain_handle(api, name, g, arrays)
    np.testing.assert_allclose(w, tls_weight(s, delta, 1.0), rtol=1e-11, atol=2e-11)
    assert g.robust_setting == (3, delta, 1.0)


def test_assembled_system_on_the_smallest_se3_graph(api):
    """se3-1 of tests/query_small_cases.py: three SE(3) poses, three edges, at its moved state one edge in each regime"""
    from query_small_cases import at_state
    arrays, _ = at_state("se3-1", "moved")
    g = api[0].from_arrays(*arrays)
    _check_system_against_the_scaled_plain_handle(api, "se3-1 moved", g, arrays)


@pytest.mark.parametrize("precision", ["f64", "mixed", "f32"])
@pytest.mark.parametrize("family", ["landmarks3d", "bearing_range"])
def test_assembled_system_on_landmark_graphs(api, family, precision):
    """k_linearize_lm on `room` (tests/landmarks3d_cases.py), k_linearize_br on `mixed` (tests/bearing_range_cases.py)"""
    if family == "landmarks3d":
        from landmarks3d_cases import case
        arrays = case("room")
    else:
        from bearing_range_cases import case
        arrays = [np.array(a, copy=True) for a in case("mixed")]
    g = api[0].from_arrays(*arrays, precision=precision)
    _check_system_against_the_scaled_plain_handle(api, family, g, arrays, precision, zero=0.0 if family == "landmarks3d" else 1e-300)


@pytest.mark.parametrize("precision", ["f64", "mixed", "f32"])
def test_assembled_system_with_priors_flagged_robust(api, precision):
    """nine priors on poses of simulation-pose-landmark, Omega = I, displaced so that their s are graded multiples of delta^2:
    three in each regime.  The plain handle holds the priors with Omega scaled by their weights; a prior of weight 0 is no prior
    (rr_pgo_set_priors refuses Omega = 0), so the plain handle's list leaves those out."""
    g = api[0].new(g2o_path("simulation-pose-landmark"), precision=precision)
    arrays = g.graph_arrays()
    s0, _ = g.edge_errors()
    d2 = float(np.median(s0[s0 > 0]))
    grades = np.array([0.1, 0.3, 0.45, 0.7, 1.0, 1.5, 2.5, 4.0, 10.0])
    poses = np.flatnonzero(arrays[0] == 0)[1:10]
    soff = np.concatenate([[0], np.cumsum(np.where(arrays[0] == 0, 3, 2))])
    meas = np.concatenate([arrays[1][soff[v]:soff[v] + 3] + [np.sqrt(gr * d2), 0.0, 0.0] for v, gr in zip(poses, grades)])
    info = np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], 9)
    g.set_priors(poses, meas, info, robust=np.ones(9, np.int32))
    holder = {}

    def prep(ref):
        keep = holder["w"] > 0.0
        ref.set_priors(poses[keep], meas[np.repeat(keep, 3)], (info * np.repeat(holder["w"], 6))[np.repeat(keep, 6)])

    delta, s, w = _set_tls_at_the_median(g)
    sp, wp = g.prior_errors()
    holder["w"] = wp
    print("prior s / delta^2:", sp / delta ** 2, "weights:", wp)
    assert np.sum(wp == 1.0) == 3 and np.sum(wp == 0.0) == 3 and np.sum((wp > 0) & (wp < 1)) == 3
    if precision == "f64":
        np.testing.assert_allclose(wp, tls_weight(sp, delta, 1.0), rtol=1e-11, atol=2e-11)
        expect = float(np.sum(tls_rho(s, delta, 1.0)) + np.sum(tls_rho(sp, delta, 1.0)))
        assert abs(g.global_error() - expect) <= 1e-12 * expect
    _check_system_against_the_scaled_plain_handle(api, "priors", g, arrays, precision, prep)


# ---- 2. weights and cost ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["intel", "sphere2500"])
@pytest.mark.parametrize("mu", [1e-3, 1.0, 50.0])
def test_edge_errors_and_cost_match_the_reference(api, name, mu):
    """|dw| = (w + mu) / 2 |ds| / s inside the band: rtol 1e-11 and atol 1e-11 (1 + mu) against the reference's weights at
    the GPU's own s (its s against the oracle's is test_robust_kernels_gpu's business)."""
    g = api[0].new(g2o_path(name))
    s0, _ = g.edge_errors()
    delta = float(np.sqrt(np.median(s0[s0 > 0])))
    g.set_robust_tls(delta, mu)
    s, w = g.edge_errors()
    assert np.array_equal(s, s0)
    np.testing.assert_allclose(w, tls_weight(s, delta, mu), rtol=1e-11, atol=1e-11 * (1.0 + mu))
    lo, hi = tls_band(delta, mu)
    assert np.all(w[s <= lo] == 1.0) and np.all(w[s >= hi] == 0.0)
    expect = float(np.sum(tls_rho(s, delta, mu)))
    c1, c2 = g.global_error(), g.global_error()
    print(f"{name} mu={mu}: cost {c1!r}, reference {expect!r}")
    assert abs(c1 - expect) <= 1e-12 * expect
    assert c1 == c2
    g.set_robust_mu(2.0 * mu)
    assert g.robust_setting == (3, delta, 2.0 * mu)
    np.testing.assert_allclose(g.edge_errors()[1], tls_weight(s, delta, 2.0 * mu), rtol=1e-11, atol=1e-11 * (1.0 + 2.0 * mu))


# ---- 3. the GNC run -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def outliers():
    from oracle.oracle import OracleGraph
    clean, outl = intel_with_outliers(g2o_path("intel"), K=50, seed=1)
    oc = OracleGraph.from_arrays(*clean)
    oc.optimize(100)
    mask = (np.abs(outl[3] - outl[4]) > 1).astype(np.int32)
    return clean, outl, oc.state(), mask


@pytest.fixture(scope="module")
def reference_run(outliers):
    clean, outl, clean_opt, mask = outliers
    ref = GncReference(outl, DELTA, mask=mask)
    return ref, gnc(ref)


@pytest.fixture(scope="module")
def gpu_run(api, outliers):
    """the handle after optimize_gnc and what it returned (made once; the tests that change a handle make their own)"""
    clean, outl, clean_opt, mask = outliers
    g = api[0].from_arrays(*outl)
    res = g.optimize_gnc(DELTA, mask)
    return g, res


def test_gnc_run_matches_the_reference(api, outliers, reference_run, gpu_run):
    clean, outl, clean_opt, mask = outliers
    ref, want = reference_run
    g, res = gpu_run
    m = len(clean[2])
    print("GPU:", {k: v for k, v in res.items() if not k.startswith("stage")}, "times (ms):", g.gnc_times())
    assert res["n_stages"] == want["n_stages"] == 25 and res["converged"] == 1
    np.testing.assert_allclose(res["mu0"], want["mu0"], rtol=1e-10)
    np.testing.assert_allclose(res["r2_max"], want["r2_max"], rtol=1e-10)
    np.testing.assert_allclose(res["stage_mu"], want["stage_mu"], rtol=1e-10)
    assert res["mu_last"] == res["stage_mu"][-1]
    print("stage_cost worst relative difference:", np.abs(res["stage_cost"] / want["stage_cost"] - 1.0).max(),
          "state worst difference:", np.abs(g.state() - ref.state()).max())
    np.testing.assert_allclose(res["stage_cost"], want["stage_cost"], rtol=1e-7)
    np.testing.assert_allclose(res["cost_last"], want["cost_last"], rtol=1e-7)
    assert np.abs(g.state() - ref.state()).max() <= 1e-8
    assert (res["n_rejected"], res["n_fractional"]) == (50, 0)
    assert res["final_iterations_run"] == want["final_iterations_run"]
    s, w = g.edge_errors()
    assert np.all(w[m:] == 0.0) and np.all(w[:m] == 1.0)
    assert position_error(g.state(), clean_opt, clean[0]) <= 1e-6
    assert g.robust_setting == (3, DELTA, res["mu_last"])
    # the cost the handle reports is the scan's: sum rho at mu_last
    assert abs(g.global_error() - res["cost_last"]) <= 1e-12 * res["cost_last"]


def test_gnc_with_levenberg_marquardt_rejects_the_same_set(api, outliers):
    clean, outl, clean_opt, mask = outliers
    g = api[0].from_arrays(*outl, solver=api[1].LevenbergMarquardt)
    res = g.optimize_gnc(DELTA, mask)
    ref = GncReference(outl, DELTA, mask=mask)
    want = gnc(ref, lm=True)
    m = len(clean[2])
    assert res["n_stages"] == want["n_stages"] and res["converged"] == 1
    print("LM stage_cost worst relative difference:", np.abs(res["stage_cost"] / want["stage_cost"] - 1.0).max())
    np.testing.assert_allclose(res["stage_cost"], want["stage_cost"], rtol=1e-6)
    _, w = g.edge_errors()
    assert np.array_equal(np.flatnonzero(w == 0.0), np.arange(m, m + 50)) and np.all(w[:m] == 1.0)


def test_gnc_on_a_mixed_precision_handle(api, outliers, reference_run):
    clean, outl, clean_opt, mask = outliers
    ref, want = reference_run
    g = api[0].from_arrays(*outl, precision="mixed")
    res = g.optimize_gnc(DELTA, mask)
    m = len(clean[2])
    _, w = g.edge_errors()
    assert np.array_equal(np.flatnonzero(w == 0.0), np.arange(m, m + 50)) and np.all(w[:m] == 1.0)
    print("mixed: stages", res["n_stages"], "state worst difference:", np.abs(g.state() - ref.state()).max())
    assert np.abs(g.state() - ref.state()).max() <= 1e-5


# ---- 4. captured graphs -------------------------------------------------------------------------------------------

def test_mu_set_after_a_captured_iteration_reaches_the_replays(api, monkeypatch):
    """RR_PGO_FORCE_GRAPH=1: iterate_async replays a captured hipGraph, which holds mu as a kernel argument."""
    PoseGraph = api[0]
    monkeypatch.setenv("RR_PGO_FORCE_GRAPH", "1")
    g = PoseGraph.new(g2o_path("intel"))
    monkeypatch.delenv("RR_PGO_FORCE_GRAPH")
    g.set_robust_tls(2.0, 0.05)
    g.iterate_async(1)   # captures the iteration at mu = 0.05
    g.sync()
    plain = PoseGraph.new(g2o_path("intel"))
    plain.set_robust_tls(2.0, 3.0)
    st = g.state()
    g.set_state(st)       # (the same bits of (x, y, cos, sin) in both handles: inside the band a weight w carries the rounding of
    plain.set_state(st)   # s amplified by (w + mu) / w)
    g.set_robust_mu(3.0)
    g.iterate_async(3)
    g.sync()
    plain.iterate_async(3)
    plain.sync()
    assert np.abs(g.state() - plain.state()).max() <= 1e-12
    assert abs(g.global_error() - plain.global_error()) <= 1e-12 * plain.global_error()
    st, sp = g.stats(), plain.stats()
    assert (st["n_graph_replays"], st["n_graph_captures"], st["n_plain_iterations"]) == (4, 2, 0)
    assert (sp["n_graph_replays"], sp["n_graph_captures"], sp["n_plain_iterations"]) == (0, 0, 3)
    other = PoseGraph.new(g2o_path("intel"))    # ... and mu = 0.05 would have gone elsewhere
    other.set_robust_tls(2.0, 0.05)
    other.iterate_async(4)
    other.sync()
    assert np.abs(g.state() - other.state()).max() > 1e-6


# ---- 5. extend and remove_edges carry the setting ------------------------------------------------------------------

def test_extend_and_remove_edges_carry_the_setting(api, outliers, gpu_run):
    clean, outl, clean_opt, mask = outliers
    _, res = gpu_run
    m = len(clean[2])
    g = api[0].from_arrays(*outl)
    g.set_robust_tls(DELTA, res["mu_last"], mask)
    g.set_state(gpu_run[0].state())
    # one more edge: a copy of the last file edge; it is robustified (mask entry 1)
    k = m - 1
    g.extend(outl[2][k:k + 1], outl[3][k:k + 1], outl[4][k:k + 1], outl[5][3 * k:3 * k + 3], outl[6][6 * k:6 * k + 6])
    assert g.num_edges == m + 51 and g.robust_setting == (3, DELTA, res["mu_last"])
    _, w = g.edge_errors()
    assert np.all(w[m:m + 50] == 0.0) and np.all(w[:m] == 1.0) and w[-1] == 1.0
    odo = np.flatnonzero(mask == 0)
    g.set_robust_mu(1e-9)     # the band is then nearly everything: only masked-off edges stay at exactly 1 whatever their s
    _, w9 = g.edge_errors()
    assert np.all(w9[odo] == 1.0) and np.all(w9[m:m + 50] < 1.0)
    g.set_robust_mu(res["mu_last"])
    rejected = np.flatnonzero(w == 0.0)
    g.remove_edges(np.concatenate([rejected, [m + 50]]))
    assert g.num_edges == m and g.robust_setting == (3, DELTA, res["mu_last"])
    g.set_robust_mu(1e-9)
    _, w9 = g.edge_errors()
    assert np.all(w9[odo] == 1.0)     # the compacted mask: the odometry edges keep their zeros
    g.set_robust_kernel(None)
    assert g.robust_setting == (0, 1.0, 0.0)
    g.optimize(100)
    assert np.abs(g.state() - clean_opt).max() <= 1e-7


# ---- 6. check_edges with weights that are exactly 0 -----------------------------------------------------------------

def test_check_edges_after_the_run(api, outliers, gpu_run):
    from check_edges_cases import seeded_edges
    from check_edges_reference import CheckReference
    clean, outl, clean_opt, mask = outliers
    m = len(clean[2])
    # a handle of its own at the run's final state and kernel (set_state: the same bits of (x, y, cos, sin) as in `h` below)
    st = gpu_run[0].state()
    g = api[0].from_arrays(*outl)
    g.set_robust_tls(DELTA, gpu_run[1]["mu_last"], mask)
    g.set_state(st)
    got = g.check_edges(return_residual=True)
    s, w = g.edge_errors()
    zero = w == 0.0
    assert np.array_equal(np.flatnonzero(zero), np.arange(m, m + 50))
    from rustrobotics_amd.mapping import SINGULAR_DIRECTION
    assert np.array_equal(np.isnan(got["redundancy"]), zero) and np.all(np.isnan(got["d2"][zero])) and np.all(np.isnan(got["redundancy_min"][zero]))
    # elsewhere d2 is NaN only where it always was: R singular to rounding in a direction (an odometry tail: a bridge)
    other_nan = np.isnan(got["d2"]) & ~zero
    print(f"{int(zero.sum())} edges of weight 0; {int(other_nan.sum())} other edges with a NaN d2, their smallest directional "
          f"redundancy at most {np.abs(got['redundancy_min'][other_nan]).max() if other_nan.any() else 0.0:.3g}")
    assert np.all(np.abs(got["redundancy_min"][other_nan]) <= SINGULAR_DIRECTION)
    assert all(np.all(np.isnan(got["R"][k])) for k in np.flatnonzero(zero))
    assert np.array_equal(got["chi2"], s) and np.all(np.isfinite(got["chi2"]))
    assert not set(g.suspect_edges(checked=got).tolist()) & set(np.flatnonzero(zero).tolist())
    h = api[0].from_arrays(*outl)
    h.set_state(st)
    h.remove_edges(np.flatnonzero(zero))
    assert h.num_edges == m and np.array_equal(h.state(), g.state())
    edges = seeded_edges(h.graph_arrays(), 64)
    ref = CheckReference(h.graph_arrays(), st, edges)
    print(ref.summary("intel after the run"))
    got_h = h.check_edges(edges, return_residual=True)
    got_g = g.check_edges(edges, return_residual=True)      # (the file's edges keep their indices: the outliers come last)
    ref.check("without the rejected edges", got_h)
    ref.check("with them at weight 0", got_g)


# ---- 7. sharded handles -------------------------------------------------------------------------------------------

def test_one_rank_sharded_handle_under_tls_matches_the_unsharded_handle(api):
    from rustrobotics_amd import sharding, synthetic_grid_arrays
    PoseGraph, _, PoseGraphError = api
    arrays = synthetic_grid_arrays(60, 40)
    shards, coll = sharding.emulate(arrays, 1, "f64")
    g = PoseGraph.from_arrays(*arrays)
    s0, _ = g.edge_errors()
    delta = float(np.sqrt(np.median(s0[s0 > 0])))
    mask = (np.abs(arrays[3] - arrays[4]) > 1).astype(np.int32)    # the chain of consecutive poses stays at weight 1
    shards[0].set_robust_tls(delta, 1.0, mask)
    g.set_robust_tls(delta, 1.0, mask)
    _, w = g.edge_errors()
    assert np.any(w == 0.0) and np.any((w > 0) & (w < 1))
    es, ns = sharding.gauss_newton(shards, 20, coll)
    eg, ng = g.optimize(20, return_norms=True)
    assert len(es) == len(eg) < 21
    np.testing.assert_allclose(es, eg, rtol=1e-7)
    assert np.abs(shards[0].state() - g.state()).max() <= 1e-8
    with pytest.raises(PoseGraphError) as err:
        shards[0].optimize_gnc(delta)
    assert err.value.code == EUNSUPPORTED
    assert shards[0].robust_setting == (3, delta, 1.0)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_leave_the_handle_alone(api, outliers):
    from rustrobotics_amd import _lib
    PoseGraph, _, PoseGraphError = api
    clean, outl, clean_opt, mask = outliers
    L = _lib.load()
    g = PoseGraph.new(g2o_path("simulation-pose-landmark"))
    assert L.rr_pgo_set_robust_mu(g._h, 1.0) == _lib.EINVAL          # no kernel
    g.set_robust_kernel("huber", 2.0)
    assert L.rr_pgo_set_robust_mu(g._h, 1.0) == _lib.EINVAL          # not TLS
    assert g.robust_setting == (1, 2.0, 0.0)
    chi = g.global_error()
    nan, inf = float("nan"), float("inf")
    for delta, mu in ((0.0, 1.0), (-1.0, 1.0), (nan, 1.0), (inf, 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, nan), (1.0, inf)):
        assert L.rr_pgo_set_robust_tls(g._h, delta, mu, None) == _lib.EINVAL
        assert g.global_error() == chi and g.robust_setting == (1, 2.0, 0.0)
    assert L.rr_pgo_set_robust_kernel(g._h, 3, 1.0, None) == _lib.EINVAL      # kind 3 is not taken there
    with pytest.raises(ValueError):
        g.set_robust_tls(1.0, 1.0, np.ones(3, np.int32))
    g.set_robust_tls(1.5, 0.5)
    chi_tls = g.global_error()
    for mu in (0.0, -1.0, nan, inf):
        assert L.rr_pgo_set_robust_mu(g._h, mu) == _lib.EINVAL
    res = _lib.GncResult()
    opt = _lib.GncOptions()

    def fresh(**kw):
        L.rr_pgo_default_gnc_options(C.byref(opt))
        for k, v in kw.items():
            setattr(opt, k, v)

    fresh()
    assert (opt.delta, opt.mu_factor, opt.max_stages, opt.inner_iterations, opt.final_iterations) == (1.0, 1.4, 100, 1, 20)
    assert L.rr_pgo_optimize_gnc(g._h, None, None, C.byref(res), None, None) == _lib.EINVAL
    assert L.rr_pgo_optimize_gnc(g._h, C.byref(opt), None, None, None, None) == _lib.EINVAL
    for kw in (dict(delta=0.0), dict(delta=nan), dict(mu_factor=1.0), dict(mu_factor=nan), dict(max_stages=0),
               dict(inner_iterations=0), dict(final_iterations=-1)):
        fresh(**kw)
        assert L.rr_pgo_optimize_gnc(g._h, C.byref(opt), None, C.byref(res), None, None) == _lib.EINVAL, kw
    assert g.robust_setting == (3, 1.5, 0.5) and g.global_error() == chi_tls
    g.set_robust_kernel("cauchy", 1.0)       # kinds 0..2 replace TLS
    assert g.robust_setting == (2, 1.0, 0.0)
    # the all-edges mask rejects the odometry of some node sooner or later: ENOTSPD with the state of the last completed
    # iteration, or a completed run -- either way the handle stays usable
    h = PoseGraph.from_arrays(*outl)
    before = h.state()
    try:
        h.optimize_gnc(DELTA, None, inner_iterations=3)
    except PoseGraphError as e:
        assert e.code == ENOTSPD
    st = h.state()
    assert np.all(np.isfinite(st)) and st.shape == before.shape
    assert np.array_equal(h.state(), st)
    assert h.robust_setting[0] == 3
    h.set_robust_kernel(None)
    assert np.isfinite(h.global_error())
    h.set_state(before)
    e = h.optimize(2)
    assert len(e) >= 2 and np.all(np.isfinite(e))


# ---- 9. the command line ------------------------------------------------------------------------------------------

def test_cli_gnc_prints_the_rejected_edges(api, outliers, gpu_run, tmp_path, capsys):
    from rustrobotics_amd.__main__ import main
    clean, outl, clean_opt, mask = outliers
    nk, ns, ek, ef, et, em, ei = outl
    m = len(clean[2])
    path = tmp_path / "intel_outliers.g2o"
    with open(path, "w") as f:
        for v in range(len(nk)):
            f.write("VERTEX_SE2 %d %s\n" % (v, " ".join(repr(float(x)) for x in ns[3 * v:3 * v + 3])))
        for k in range(len(ek)):
            f.write("EDGE_SE2 %d %d %s %s\n" % (ef[k], et[k], " ".join(repr(float(x)) for x in em[3 * k:3 * k + 3]),
                                                " ".join(repr(float(x)) for x in ei[6 * k:6 * k + 6])))
    assert main([str(path), "--gnc", "3.3682"]) == 0
    out = capsys.readouterr().out
    res = gpu_run[1]
    assert f"{res['n_stages']} stages (converged), mu0 {res['mu0']:.6g}, mu_last {res['mu_last']:.6g}" in out
    last = [line for line in out.splitlines() if line.startswith("50 edges rejected, 0 fractional:")]
    assert len(last) == 1 and [int(x) for x in last[0].split(":")[1].split()] == list(range(m, m + 50))
    with pytest.raises(SystemExit):
        main([str(path), "--gnc", "3.3682:some"])
    with pytest.raises(SystemExit):
        main([str(path), "--gnc", "3.3682", "--robust", "cauchy:1"])
