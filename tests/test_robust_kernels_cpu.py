"""Robust kernels without a GPU: the CPU reference (tests/robust_reference.py, on the unchanged oracle) on intel.g2o with
false loop closures, the kernel formulas against their definition, and the ABI constants."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, g2o_path
from robust_reference import RobustReference, intel_with_outliers, position_error, rho, weight

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


@pytest.fixture(scope="module")
def outliers():
    from oracle.oracle import OracleGraph
    clean, outl = intel_with_outliers(g2o_path("intel"))
    oc = OracleGraph.from_arrays(*clean)
    oc.optimize(100)
    return clean, outl, oc.state()


def test_cauchy_irls_rejects_false_loop_closures(outliers):
    """50 random false loop closures (1 % of intel's edges): Cauchy, delta = 1, converges by the stop rule, lands within
    0.15 m of the clean file's optimum everywhere, and switches every false edge off (w < 0.01)."""
    clean, outl, clean_opt = outliers
    r = RobustReference(outl, "cauchy", 1.0)
    errors, norms = r.optimize(100)
    assert len(errors) - 1 <= 20 and norms[-1] < 1e-4
    assert position_error(r.state(), clean_opt, clean[0]) <= 0.15
    w = r.weights(r.edge_s())
    m = len(clean[2])
    assert w[m:].max() < 0.01
    assert np.median(w[:m]) > 0.5


def test_plain_least_squares_follows_the_false_loop_closures(outliers):
    clean, outl, clean_opt = outliers
    r = RobustReference(outl, None)
    r.optimize(100)
    assert position_error(r.state(), clean_opt, clean[0]) > 10.0


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
@pytest.mark.parametrize("delta", [0.3, 1.0, 7.0])
def test_weight_is_the_derivative_of_rho(kind, delta):
    s = np.concatenate([np.geomspace(1e-3, 1e4, 200) * delta * delta])
    s = s[np.abs(s - delta * delta) > 1e-3 * delta * delta]   # Huber's kink
    h = 1e-6 * s
    fd = (rho(kind, s + h, delta) - rho(kind, s - h, delta)) / (2 * h)
    np.testing.assert_allclose(weight(kind, s, delta), fd, rtol=1e-6)
    assert np.all(weight(kind, s, delta) <= 1.0) and np.all(weight(kind, s, delta) > 0.0)


@pytest.mark.parametrize("delta", [0.3, 1.0, 7.0])
def test_huber_is_continuous_at_delta_squared(delta):
    d2 = delta * delta
    below, above = rho("huber", d2 * (1 - 1e-12), delta), rho("huber", d2 * (1 + 1e-12), delta)
    assert abs(float(above - below)) <= 1e-9 * d2
    assert float(rho("huber", d2, delta)) == d2
    assert abs(float(weight("huber", d2 * (1 + 1e-12), delta)) - 1.0) < 1e-9


def test_negative_s_is_plain_least_squares():
    s = np.array([-3.0, -1e-9])
    for kind in ("huber", "cauchy"):
        np.testing.assert_array_equal(rho(kind, s, 1.0), s)
        np.testing.assert_array_equal(weight(kind, s, 1.0), [1.0, 1.0])


def test_header_robust_enum_matches_the_python_mirror():
    from rustrobotics_amd import _lib
    header = open(os.path.join(ROOT, "include", "rr_pgo.h")).read()
    vals = dict((k, int(v)) for k, v in re.findall(r"RR_PGO_ROBUST_(\w+)\s*=\s*(\d+)", header))
    assert vals == {"NONE": _lib.ROBUST_NONE, "HUBER": _lib.ROBUST_HUBER, "CAUCHY": _lib.ROBUST_CAUCHY}
    for name in ("rr_pgo_set_robust_kernel", "rr_pgo_edge_errors"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, header)


def test_cli_parses_the_robust_option():
    import argparse
    from rustrobotics_amd.__main__ import _robust_arg
    assert _robust_arg("cauchy:1") == ("cauchy", 1.0)
    assert _robust_arg("Huber:0.5") == ("huber", 0.5)
    for bad in ("cauchy", "tukey:1", "huber:0", "huber:-1", "cauchy:nan", "cauchy:inf", "cauchy:x"):
        with pytest.raises(argparse.ArgumentTypeError):
            _robust_arg(bad)
