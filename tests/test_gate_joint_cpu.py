"""rr_pgo_gate_joint without a GPU: the exports and macros are declared everywhere they have to be, the chi-square table, the
--gate-joint file parser, and the conditions of the GPU comparisons: the CPU reference (tests/gate_joint_reference.py) is
quiet on the sets of tests/gate_joint_cases.py, decides both ways, no set sits at its threshold, and the cross blocks matter."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, g2o_path
from covariances_cases import FLOOR_MAX
from gate_cases import GATE_GRAPHS, candidates
from gate_joint_cases import joint_sets, set_dims
from gate_joint_reference import JointReference
from oracle.oracle import OracleGraph
from robust_reference import oracle_arrays


def test_gate_joint_exports_are_declared_in_header_mirror_and_integration_guide():
    from rustrobotics_amd import _lib, mapping
    header = open(os.path.join(ROOT, "include", "rr_pgo.h")).read()
    assert re.search(r"\bint\s+rr_pgo_gate_joint\s*\(\s*rr_pgo\s*\*h\s*,\s*int32_t\s+n_cand", header)
    assert re.search(r"\bint\s+rr_pgo_gate_joint_times\s*\(\s*const\s+rr_pgo\s*\*h", header)
    assert re.search(r"#define\s+RR_PGO_GATE_JOINT_MAX_DIM\s+48\b", header)
    assert re.search(r"#define\s+RR_PGO_GATE_JOINT_MAX_CAND\s+16\b", header)
    assert "#define RR_PGO_ABI_VERSION 4" in header   # two exports and two macros were added: no struct or enum changed
    assert _lib.ABI_VERSION == 4
    assert "rr_pgo_gate_joint" in _lib.EXPORTS and "rr_pgo_gate_joint_times" in _lib.EXPORTS
    assert (_lib.GATE_JOINT_MAX_DIM, _lib.GATE_JOINT_MAX_CAND) == (48, 16)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn rr_pgo_gate_joint(" in integration and "pub fn gate_joint(" in integration
    from rustrobotics_amd import PoseGraph
    assert callable(PoseGraph.gate_joint) and callable(PoseGraph.gate_joint_accept) and callable(PoseGraph.gate_joint_times)
    kinds = np.array([0, 1, 2, 1])
    assert list(mapping.gate_joint_dims(kinds, [[0, 1], [2, 2], [3]])) == [5, 12, 2]
    assert list(mapping.gate_joint_thresholds(kinds, [[0, 1], [2, 2], [3]])) == [11.070, 21.026, 5.991]
    assert list(mapping.gate_joint_thresholds(kinds, [[0, 1], [3]], 4.0)) == [4.0, 4.0]


def test_chi_square_table():
    from rustrobotics_amd import mapping
    T = mapping.CHI2_95
    assert len(T) == 49 and T[0] is None
    assert (T[2], T[3], T[6]) == (mapping.CHI2_95_2, mapping.CHI2_95_3, mapping.CHI2_95_6)
    assert (T[12], T[24], T[48]) == (21.026, 36.415, 65.171)
    assert all(T[d] < T[d + 1] for d in range(1, 48))
    assert all(round(T[d], 3) == T[d] for d in range(1, 49))
    try:
        from scipy.stats import chi2
    except ImportError:
        return   # (the comparison with SciPy is all that is left out)
    worst = max(abs(T[d] - float(chi2.ppf(0.95, d))) for d in range(1, 49))
    print(f"CHI2_95[1..48] against scipy.stats.chi2.ppf(0.95, d): worst difference {worst:.3g}")
    assert worst <= 5e-4


GATE_JOINT_FILE = """EDGE_SE2 3 7 1.5 -0.25 0.125 44.7 0 0 44.7 0 30.9
SET 0 1
# a landmark sighting, then the first candidate again
EDGE_SE2_XY 7 12 0.5 2.0 10 1 20
EDGE_SE2 7 3 0 0 0 1 0 0 1 0 1
SET 2 0 2
SET 1
"""


def test_gate_joint_file_parser(tmp_path):
    from rustrobotics_amd.__main__ import parse_gate_file, parse_gate_joint_file
    index = {3: 0, 7: 1, 12: 2}
    p = tmp_path / "sets.txt"
    p.write_text(GATE_JOINT_FILE)
    kind, a, b, meas, info, ids, sets = parse_gate_joint_file(str(p), index)
    assert kind == [0, 1, 0] and a == [0, 1, 1] and b == [1, 2, 0]
    assert ids == [(3, 7), (7, 12), (7, 3)]
    assert sets == [[0, 1], [2, 0, 2], [1]]
    assert meas == [1.5, -0.25, 0.125, 0.5, 2.0, 0, 0, 0]
    assert info == [44.7, 0, 0, 44.7, 0, 30.9, 10, 1, 20, 1, 0, 0, 1, 0, 1]
    # a SET line means nothing to --gate
    with pytest.raises(SystemExit) as ei:
        parse_gate_file(str(p), index)
    assert f"{p}:2:" in str(ei.value) and "SET" in str(ei.value)
    seventeen = " ".join(["0"] * 17)
    for text, line, word in ((GATE_JOINT_FILE + "SET 0 3\n", 8, "candidate 3"),
                             (GATE_JOINT_FILE + "SET -1\n", 8, "candidate -1"),
                             (GATE_JOINT_FILE + "SET\n", 8, "after SET"),
                             (GATE_JOINT_FILE + "SET 0 x\n", 8, "after SET"),
                             (GATE_JOINT_FILE + f"SET {seventeen}\n", 8, "at most 16"),
                             (GATE_JOINT_FILE + "EDGE_SE2 3 99 0 0 0 1 0 0 1 0 1\n", 8, "99"),
                             (GATE_JOINT_FILE.replace("EDGE_SE2_XY", "EDGE_XY"), 4, "EDGE_XY")):
        p.write_text(text)
        with pytest.raises(SystemExit) as ei:
            parse_gate_joint_file(str(p), index)
        assert "--gate-joint" in str(ei.value) and f"{p}:{line}:" in str(ei.value) and word in str(ei.value), str(ei.value)
    p.write_text("EDGE_SE2 3 7 0 0 0 1 0 0 1 0 1\n")
    with pytest.raises(SystemExit) as ei:
        parse_gate_joint_file(str(p), index)
    assert "no SET line" in str(ei.value)


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_reference_is_quiet_and_decides_both_ways(name):
    """The conditions of the GPU comparisons, per graph: the reference's two computations of S, d2 and the prefixes agree to
    FLOOR_MAX; every d2 is > 0; at the default threshold the reference accepts at least 3 and rejects at least 3 sets; no
    set lies within the tolerance of its threshold; and at least one set's joint d2 differs from the sum of its members'
    single d2 by more than 10 %: the cross blocks matter."""
    from rustrobotics_amd import PoseGraph
    assert callable(PoseGraph.gate_joint)   # (the feature these conditions serve)
    o = OracleGraph.load(g2o_path(name))
    if GATE_GRAPHS[name]:
        o.optimize(GATE_GRAPHS[name])
    arrays, state = oracle_arrays(o), o.state()
    cand = candidates(arrays, state)
    sets = joint_sets(len(cand[0]))
    ref = JointReference(arrays, state, cand, sets)
    print(ref.summary(name))
    dims = set_dims(cand[0], sets)
    assert len(sets) == 20 and max(dims) <= 48 and max(len(s) for s in sets) <= 16
    if name == "parking-garage":
        assert max(dims) == 48
    if name == "simulation-pose-landmark":
        assert any(len(set(int(cand[0][c]) for c in s)) == 2 for s in sets)   # SE2 and SE2_XY candidates in one set
    assert ref.floor_S <= FLOOR_MAX and ref.floor_d2 <= FLOOR_MAX and ref.floor_prefix <= FLOOR_MAX, (ref.floor_S, ref.floor_d2, ref.floor_prefix)
    assert np.all(ref.d2 > 0)
    assert np.sum(ref.accept) >= 3 and np.sum(~ref.accept) >= 3, (int(np.sum(ref.accept)), int(np.sum(~ref.accept)))
    assert not np.any(ref.undecided)
    for S, pre, d2 in zip(ref.S, ref.prefix, ref.d2):
        assert np.all(np.linalg.eigvalsh(S) > 0)
        assert np.all(np.diff(pre) >= 0) and pre[-1] == d2
    cross = np.abs(ref.d2 - ref.single_sum) / ref.single_sum
    print(f"{name}: joint d2 against the sum of the members' single d2: up to {float(np.max(cross)):.3g} relative "
          f"(set {sets[int(np.argmax(cross))]}: {ref.d2[int(np.argmax(cross))]:.4g} against {ref.single_sum[int(np.argmax(cross))]:.4g})")
    assert np.max(cross) > 0.10
