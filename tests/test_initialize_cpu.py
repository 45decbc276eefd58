"""rr_pgo_initialize without a device: the numpy / scipy reference the GPU tests compare against (tests/chordal_reference.py)
is itself checked -- it recovers the truth of consistent measurements, it projects the reflection case onto Rx(pi), and on the
five datasets it reproduces the chi2 values DESIGN.md 4v quotes and leads the oracle's Gauss-Newton to their optima."""
import numpy as np
import pytest

from chordal_cases import (NOISE_FREE_REFERENCE_ERROR, RING_CASES, RING_IDS, RX_PI, reflection_graph, ring_graph)
from chordal_reference import all_at_node0, chordal_initialize, quat_to_rot, state_diff
from conftest import g2o_path
from oracle.oracle import OracleGraph
from robust_reference import oracle_arrays


@pytest.mark.parametrize("seed,se3,landmarks", RING_CASES, ids=RING_IDS)
def test_noise_free_measurements_are_recovered(seed, se3, landmarks):
    """The relaxation is tight when the measurements are consistent: from a scrambled state with node 0 held at the truth the
    reference returns the truth.  Its worst error over the four graphs is what NOISE_FREE_REFERENCE_ERROR writes down."""
    arrays, start = ring_graph(seed, se3, landmarks)
    out, info = chordal_initialize(arrays, start, held=[0])
    err = state_diff(arrays[0], out, arrays[1])
    print(f"noise-free ring se3={se3} landmarks={landmarks}: reference error {err:.3e}")
    assert err <= NOISE_FREE_REFERENCE_ERROR
    # the start really is far away
    assert state_diff(arrays[0], start, arrays[1]) > 1.0


def test_reflection_case_projects_onto_rx_pi():
    arrays, t3 = reflection_graph()
    out, info = chordal_initialize(arrays, held=[0, 1, 2])
    M3 = info["M"][3]
    assert np.allclose(M3, -np.diag([0.5, 1.5, 3.5]) / 5.5, rtol=0, atol=1e-15)
    assert np.linalg.det(M3) < 0
    assert np.max(np.abs(quat_to_rot(out[21 + 3:21 + 7]) - RX_PI)) <= 1e-15
    assert np.max(np.abs(out[21:24] - t3)) <= 1e-14
    assert np.array_equal(out[:21], arrays[1][:21])


# chi2 of the chordal state from "every node at node 0's pose" (relative 1e-6) | chi2 the oracle's Gauss-Newton reaches from
# there (relative 1e-8) | its iterations
DATASETS = [
    ("sphere2500", 1233.348, 727.149667, 10),
    ("torus3D", 15466.374, 14574.7464, 10),
    ("parking-garage", 1.41041, 1.23869058, 10),
    ("intel", 384.048, 359.996112, 15),
    ("input_M3500_g2o", 175.9075, 137.912951, 15),
]


@pytest.mark.parametrize("name,chi2_chordal,chi2_final,iters", DATASETS, ids=[d[0] for d in DATASETS])
def test_datasets(name, chi2_chordal, chi2_final, iters):
    o = OracleGraph.load(g2o_path(name))
    arrays = oracle_arrays(o)
    ef = arrays[3][np.flatnonzero((arrays[2] == 0) | (arrays[2] == 2))[0]]   # the anchor: from-node of the first pose-pose edge
    start = all_at_node0(arrays)
    out, _ = chordal_initialize(arrays, start, held=[int(ef)])
    arrays[1] = out
    g = OracleGraph.from_arrays(*arrays)
    chi2 = g.global_error()
    errors = g.optimize(iters)
    print(f"{name}: chi2 after the chordal initialisation {chi2:.6f}, after Gauss-Newton {errors[-1]:.8f} in {len(errors) - 1}")
    assert abs(chi2 - chi2_chordal) <= 1e-6 * chi2_chordal
    assert abs(errors[-1] - chi2_final) <= 1e-8 * chi2_final
