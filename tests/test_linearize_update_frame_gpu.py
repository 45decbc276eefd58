"""The one frame of k_linearize / k_update (kernels.hip.h: SE(2) is D = 3, SE(3) is D = 6) on graphs of a few nodes (run with -m
gpu on an MI355X).

Cells: {SE(2) with landmarks, SE(3)} x {f64, mixed, f32} x {no kernel, Huber, Cauchy with a mask on every other edge} x
{Gauss-Newton, Levenberg-Marquardt}.  Per cell, optimize(6) of a default handle -- lambda, the reset of the loop state, the stop
word and the publication come from the device-side loop state -- gives the errors, norms and final state of a handle created
under RR_PGO_SYNC_OPTIMIZE=1, where the host supplies them: the branches of the frame that the two dimensions share.  Per f64 cell,
assemble() equals assemble() of a plain handle whose Omega is scaled by the weights of the CPU reference
(tests/robust_reference.py), at the initial state and at the state the call ended in.

No cell is left out: the bit-identity with the host loop is asserted elsewhere on the dataset files only
(test_gpu_parity.py::test_optimize_with_the_stop_rule_on_the_device_is_bit_identical_to_the_host_loop, without a kernel, in f64),
the weighted system on the dataset files only (test_robust_kernels_gpu.py), and the random graphs of test_gpu_parity.py are
compared with the oracle, not with the host loop."""
import numpy as np
import pytest

from random_graphs import random_graph
from robust_reference import INFO_LEN, RobustReference

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

GRAPHS = {
    "se2": lambda: random_graph(np.random.default_rng(1701), 12, 5, 8),
    "se3": lambda: random_graph(np.random.default_rng(1702), 10, 0, 6, se3=True),
}
KERNELS = ["none", "huber", "cauchy-masked"]


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


@pytest.fixture(scope="module")
def cases(api):
    """per graph: its arrays and a delta with edges on both sides of delta^2 at the initial state (computed once)"""
    out = {}
    for name, make in GRAPHS.items():
        arrays = make()
        s, _ = api[0].from_arrays(*arrays).edge_errors()
        out[name] = (arrays, float(np.sqrt(np.median(s[s > 0]))))
    return out


def _kernel(kernel, delta, n_edges):
    """(kind, delta, mask) as set_robust_kernel and RobustReference take them"""
    if kernel == "none":
        return None, 1.0, None
    if kernel == "huber":
        return "huber", delta, None
    return "cauchy", delta, (np.arange(n_edges) % 2 == 0).astype(np.int32)


def _assert_same_system(g, arrays, state, kind, delta, mask, lm, mixed_weights):
    """the tolerances of test_robust_kernels_gpu.py::test_assembled_system_equals_the_plain_system_with_weighted_information"""
    a = list(arrays)
    a[1] = np.asarray(state, np.float64)
    ref = RobustReference(a, kind, delta, mask)
    _, w = ref.weighted_graph()
    if kind is not None and mixed_weights:   # delta was chosen at the initial state: there both sides of delta^2 are taken
        assert (w < 1).any() and (w == 1).any()
    a[6] = np.asarray(a[6], np.float64) * w[np.repeat(np.arange(len(a[2])), [INFO_LEN[int(k)] for k in a[2]])]
    plain = type(g).from_arrays(*a)
    g.set_state(state)       # the same bits of the device form in both handles
    plain.set_state(state)
    lam = 0.37 if lm else 0.0
    br, bc, bo, vals, b = g.assemble(lam, lm)
    br2, bc2, bo2, vals2, b2 = plain.assemble(lam, lm)
    assert np.array_equal(br, br2) and np.array_equal(bc, bc2) and np.array_equal(bo, bo2)
    scale = np.abs(vals2).max()
    print("assemble: max |dH| / scale", np.abs(vals - vals2).max() / scale, " max |db|", np.abs(b - b2).max(),
          " against", 1e-11 * max(np.abs(b2).max(), 1e-3 * np.sqrt(scale)))
    assert np.abs(vals - vals2).max() <= 1e-12 * scale
    assert np.abs(b - b2).max() <= 1e-11 * max(np.abs(b2).max(), 1e-3 * np.sqrt(scale))
    assert vals.max() > 1e7   # the anchor prior is there, unweighted


@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", ["f64", "mixed", "f32"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_device_side_loop_state_equals_the_host_loop_and_the_weighted_system(api, cases, name, precision, kernel, solver, monkeypatch):
    PoseGraph, Solver = api
    arrays, delta = cases[name]
    kind, delta, mask = _kernel(kernel, delta, len(arrays[2]))
    fast = PoseGraph.from_arrays(*arrays, precision=precision, solver=getattr(Solver, solver))
    monkeypatch.setenv("RR_PGO_SYNC_OPTIMIZE", "1")
    slow = PoseGraph.from_arrays(*arrays, precision=precision, solver=getattr(Solver, solver))
    monkeypatch.delenv("RR_PGO_SYNC_OPTIMIZE")
    for g in (fast, slow):
        g.set_robust_kernel(kind, delta, mask)
    s0 = np.array(fast.state())
    ef, nf = fast.optimize(6, return_norms=True)
    es, ns = slow.optimize(6, return_norms=True)
    print(name, precision, kernel, solver, "errors", ef, "norms", nf)
    assert len(ef) >= 2 and np.all(np.isfinite(ef)) and np.all(np.isfinite(nf))
    assert len(ef) == len(es) and all(x == y for x, y in zip(ef, es)), (ef, es)
    assert len(nf) == len(ns) and all(x == y for x, y in zip(nf, ns)), (nf, ns)
    s1 = np.array(fast.state())
    assert np.all(s1 == np.array(slow.state()))
    if precision == "f64":
        lm = solver == "LevenbergMarquardt"
        _assert_same_system(fast, arrays, s0, kind, delta, mask, lm, True)
        _assert_same_system(fast, arrays, s1, kind, delta, mask, lm, False)
