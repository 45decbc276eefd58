"""K form of the back substitution (kernels.hip.h, kform_front) against the chain form it replaces (RR_PGO_SOLVE_KFORM=0).

The factorisation forms K = L11^-T L21^T and c = L11^-T y per LDS front, and the back substitution of such a front becomes one
GEMV: another summation order than the chain over 16-column blocks, so the two forms agree to rounding, within the
trajectory tolerances the other parity tests use (fp64: chi2 1e-7 relative per iteration, poses 1e-6; mixed: fp32 factor)."""
import numpy as np
import pytest

from conftest import g2o_path

pytestmark = pytest.mark.gpu

FILES = ["simulation-pose-landmark", "simulation-pose-pose", "intel", "input_M3500_g2o", "dlr", "sphere2500"]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


@pytest.mark.parametrize("prec", ["f64", "mixed"])
@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
@pytest.mark.parametrize("name", FILES)
def test_kform_follows_the_chain_form(api, name, solver, prec, monkeypatch):
    PoseGraph, Solver = api
    slv = getattr(Solver, solver)
    k = PoseGraph.new(g2o_path(name), slv, precision=prec)
    monkeypatch.setenv("RR_PGO_SOLVE_KFORM", "0")
    c = PoseGraph.new(g2o_path(name), slv, precision=prec)
    monkeypatch.delenv("RR_PGO_SOLVE_KFORM")
    sk, sc = k.stats(), c.stats()
    assert sk["solve_kform"] == 1 and sk["kform_bytes"] > 0 and sk["kform_flops"] > 0, sk
    assert sc["solve_kform"] == 0 and sc["kform_bytes"] == 0, sc
    # the K step is counted on its own key, not in the survey's once-per-datum figures
    assert sk["bytes_factor"] == sc["bytes_factor"] and sk["bytes_solve"] == sc["bytes_solve"]
    if prec == "f64":
        ek, ec = np.array(k.optimize(5)), np.array(c.optimize(5))
        np.testing.assert_allclose(ek, ec, rtol=1e-7)
        np.testing.assert_allclose(np.array(k.state()), np.array(c.state()), rtol=0, atol=1e-6)
    else:
        # fp32 factor: an iterate far from the answer carries the factor's rounding (cond(H) x 2^-24), another summation order
        # moves it by per cent; the fp64 gradient refines both forms to the same point (test_mixed_precision_reaches_the_f64_answer)
        ek, ec = np.array(k.optimize(30)), np.array(c.optimize(30))
        assert abs(ek[-1] - ec[-1]) <= 1e-6 * ec[-1], (ek[-1], ec[-1])
        # (dlr settles 7e-4 apart at equal chi2: a flat direction of its cost, met by the fp32 factor either way)
        np.testing.assert_allclose(np.array(k.state()), np.array(c.state()), rtol=0, atol=1e-3)


def test_kform_is_off_where_the_lds_fronts_only_run_on_the_level_schedule(api):
    """The 1M-edge lattice (BASELINE configs[3]): thousands of throughput-bound LDS fronts, no dataflow launch -- no K form."""
    from rustrobotics_amd import synthetic_grid_arrays
    g = api[0].from_arrays(*synthetic_grid_arrays(400, 250, 1000000), precision="mixed")
    st = g.stats()
    assert st["lds_dataflow"] == 0
    assert st["solve_kform"] == 0 and st["kform_bytes"] == 0 and st["kform_flops"] == 0
