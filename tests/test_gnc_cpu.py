"""Truncated least squares and the graduated non-convexity loop on the CPU (no GPU): the kernel's formulas as the header
states them, and the reference loop (tests/gnc_reference.py) on intel.g2o + 50 false loop closures -- the run the GPU
tests compare rr_pgo_optimize_gnc against, and the condition that comparison rests on."""
import re

import numpy as np
import pytest

from conftest import ROOT, g2o_path
from gnc_reference import GncReference, gnc, tls_band, tls_rho, tls_weight
from robust_reference import intel_with_outliers, position_error

DELTA = 3.3682   # delta^2 = 11.345: the 0.99 chi-square quantile of 3 degrees of freedom


# ---- the kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("delta,mu", [(1.0, 1.0), (DELTA, 6.41e-5), (DELTA, 0.3), (0.5, 40.0)])
def test_weight_is_the_derivative_of_rho_in_all_three_regimes(delta, mu):
    import mpmath as mp
    mp.mp.dps = 50
    c, m = mp.mpf(delta), mp.mpf(mu)
    lo, hi = m / (m + 1) * c * c, (m + 1) / m * c * c

    def rho(s):
        if s <= lo:
            return s
        if s >= hi:
            return c * c
        return 2 * c * mp.sqrt(s * m * (m + 1)) - m * (c * c + s)

    flo, fhi = tls_band(delta, mu)
    points = [0.3 * flo, 0.999 * flo, flo + 0.001 * (fhi - flo), np.sqrt(flo * fhi), fhi - 0.001 * (fhi - flo), 1.001 * fhi, 7.0 * fhi]
    for s in points:
        x = mp.mpf(float(s))
        h = x * mp.mpf("1e-20")
        d = (rho(x + h) - rho(x - h)) / (2 * h)
        w = float(tls_weight(float(s), delta, mu))
        assert abs(w - float(d)) <= 1e-12 * (1.0 + mu), (s, w, float(d))
        assert abs(float(tls_rho(float(s), delta, mu)) - float(rho(x))) <= 1e-13 * float(rho(x))
    assert 0.0 < float(tls_weight(points[3], delta, mu)) < 1.0


@pytest.mark.parametrize("delta,mu", [(1.0, 1.0), (DELTA, 6.41e-5), (DELTA, 0.3), (0.5, 40.0)])
def test_weight_and_rho_are_continuous_and_exact_outside_the_band(delta, mu):
    lo, hi = tls_band(delta, mu)
    c2 = delta * delta
    # outside the band the constants themselves, not rounded values
    below = np.array([-5.0, -1e-300, 0.0, 0.5 * lo, np.nextafter(lo, 0.0), lo])
    above = np.array([hi, np.nextafter(hi, np.inf), 2.0 * hi, 1e300])
    assert np.all(tls_weight(below, delta, mu) == 1.0) and np.all(tls_rho(below, delta, mu) == below)   # s < 0: w = 1, rho = s
    assert np.all(tls_weight(above, delta, mu) == 0.0) and np.all(tls_rho(above, delta, mu) == c2)
    # continuity at the band's ends: one ulp inside, the values are the constants up to rounding of the formula
    s_in = np.array([np.nextafter(lo, np.inf), np.nextafter(hi, 0.0)])
    w_in, r_in = tls_weight(s_in, delta, mu), tls_rho(s_in, delta, mu)
    assert abs(w_in[0] - 1.0) <= 1e-14 * (1.0 + mu) and abs(w_in[1]) <= 1e-14 * (1.0 + mu)
    assert abs(r_in[0] - lo) <= 1e-14 * (1.0 + mu) * c2 and abs(r_in[1] - c2) <= 1e-14 * (1.0 + mu) * c2
    # the weight falls monotonically through the band
    s = np.geomspace(lo, hi, 101)
    assert np.all(np.diff(tls_weight(s, delta, mu)) <= 0.0)


def test_the_header_states_the_formulas_and_the_mirror_knows_the_entry_points():
    from rustrobotics_amd import _lib
    header = open(ROOT + "/include/rr_pgo.h").read()
    for name in ("rr_pgo_set_robust_tls", "rr_pgo_set_robust_mu", "rr_pgo_get_robust", "rr_pgo_default_gnc_options",
                 "rr_pgo_optimize_gnc", "rr_pgo_gnc_times"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"#define RR_PGO_ROBUST_TLS 3\b", header) and _lib.ROBUST_TLS == 3
    assert re.search(r"#define RR_PGO_ABI_VERSION 4\b", header)
    assert "tls" not in _lib.ROBUST_KERNELS and 3 not in _lib.ROBUST_KERNELS.values()   # rr_pgo_set_robust_kernel does not take it


# ---- the loop on intel + 50 false loop closures ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def intel_run():
    from oracle.oracle import OracleGraph
    clean, outl = intel_with_outliers(g2o_path("intel"), K=50, seed=1)
    oc = OracleGraph.from_arrays(*clean)
    oc.optimize(100)
    mask = np.abs(outl[3] - outl[4]) > 1
    ref = GncReference(outl, DELTA, mask=mask)
    res = gnc(ref)
    return clean, outl, oc.state(), mask, ref, res


def test_reference_loop_recovers_the_clean_optimum(intel_run):
    clean, outl, clean_opt, mask, ref, res = intel_run
    m = len(clean[2])
    assert res["n_stages"] == 25 and res["converged"] == 1
    assert abs(res["mu0"] - 6.41e-5) <= 0.005e-5
    assert (res["n_rejected"], res["n_fractional"]) == (50, 0)
    w = ref.weights(ref.edge_s())
    assert np.all(w[m:] == 0.0) and np.all(w[:m] == 1.0)
    assert np.abs(ref.state() - clean_opt).max() <= 1e-7
    assert position_error(ref.state(), clean_opt, clean[0]) <= 1e-7
    np.testing.assert_allclose(res["stage_mu"], res["mu0"] * 1.4 ** np.arange(25), rtol=1e-13)


def test_no_edge_ends_a_stage_near_the_ends_of_the_band(intel_run):
    """what the GPU comparison of the stage count rests on: at every stage's end (and after the closing iterations) no masked
    edge's s lies within a relative 1e-6 of that stage's lo or hi, so rounding cannot move an edge across a regime.
    Seed 1 satisfies it."""
    clean, outl, clean_opt, mask, ref, res = intel_run
    worst = np.inf
    stages = list(zip(res["stage_mu"], res["stage_s"])) + [(res["mu_last"], ref.edge_s())]
    for mu, s in stages:
        lo, hi = tls_band(DELTA, mu)
        sm = s[mask]
        worst = min(worst, np.abs(sm / lo - 1.0).min(), np.abs(sm / hi - 1.0).min())
    print("smallest relative distance of a masked s to a band end:", worst)
    assert worst > 1e-6
