"""rr_pgo_gate_edges without a GPU: the export is declared everywhere it has to be, the CPU reference the GPU tests compare
with (tests/gate_reference.py) is quiet on the candidates of tests/gate_cases.py and decides both ways, and the --gate
file parser of the command line."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, g2o_path
from covariances_cases import FLOOR_MAX
from gate_cases import GATE_GRAPHS, candidates
from gate_reference import GateReference
from oracle.oracle import OracleGraph
from robust_reference import oracle_arrays


def test_gate_export_is_declared_in_header_mirror_and_integration_guide():
    from rustrobotics_amd import _lib
    header = open(os.path.join(ROOT, "include", "rr_pgo.h")).read()
    assert re.search(r"\bint\s+rr_pgo_gate_edges\s*\(\s*rr_pgo\s*\*h\s*,\s*int32_t\s+n_cand", header)
    assert re.search(r"\bint\s+rr_pgo_gate_times\s*\(\s*const\s+rr_pgo\s*\*h", header)
    assert "#define RR_PGO_ABI_VERSION 4" in header   # two exports were added: no struct or enum changed
    assert "rr_pgo_gate_edges" in _lib.EXPORTS and "rr_pgo_gate_times" in _lib.EXPORTS
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn rr_pgo_gate_edges(" in integration and "pub fn gate_edges(" in integration
    from rustrobotics_amd import PoseGraph
    assert callable(PoseGraph.gate_edges) and callable(PoseGraph.gate) and callable(PoseGraph.gate_times)
    from rustrobotics_amd import mapping
    assert (mapping.CHI2_95_2, mapping.CHI2_95_3, mapping.CHI2_95_6) == (5.991, 7.815, 12.592)
    kinds = np.array([0, 1, 2, 1])
    assert list(mapping.gate_thresholds(kinds)) == [7.815, 5.991, 12.592, 5.991]
    assert list(mapping.gate_thresholds(kinds, 3.0)) == [3.0] * 4
    assert list(mapping.gate_thresholds(kinds, {0: 1.0, 1: 2.0, 2: 3.0})) == [1.0, 2.0, 3.0, 2.0]


@pytest.mark.parametrize("name", list(GATE_GRAPHS))
def test_reference_is_quiet_and_decides_both_ways(name):
    """The condition of the GPU comparisons, per graph: the reference's two computations of d2 and S agree to FLOOR_MAX,
    every reference d2 is > 0, and at the default threshold the reference accepts at least 5 and rejects at least 5
    candidates.  With seed 31 no reference d2 lies within the tolerance of its threshold (checked here), so the GPU
    comparison of decisions leaves no candidate out."""
    from rustrobotics_amd import PoseGraph
    assert callable(PoseGraph.gate_edges)   # (the feature these conditions serve)
    o = OracleGraph.load(g2o_path(name))
    if GATE_GRAPHS[name]:
        o.optimize(GATE_GRAPHS[name])
    arrays, state = oracle_arrays(o), o.state()
    cand = candidates(arrays, state)
    ref = GateReference(arrays, state, cand)
    print(ref.summary(name))
    kinds = cand[0]
    assert ref.n >= 60
    assert len(set(int(v) for v in cand[1]) | set(int(v) for v in cand[2])) >= 24
    if name == "simulation-pose-landmark":
        assert np.sum(kinds == 1) >= 10 and np.sum(kinds == 0) >= 10
    assert ref.floor_d2 <= FLOOR_MAX and ref.floor_S <= FLOOR_MAX and ref.floor_chi2 <= FLOOR_MAX, (ref.floor_d2, ref.floor_S, ref.floor_chi2)
    assert np.all(ref.d2 > 0)
    assert np.sum(ref.accept) >= 5 and np.sum(~ref.accept) >= 5, (int(np.sum(ref.accept)), int(np.sum(~ref.accept)))
    assert not np.any(ref.undecided)
    for S in ref.S:
        assert np.all(np.linalg.eigvalsh(S) > 0)


GATE_FILE = """EDGE_SE2 3 7 1.5 -0.25 0.125 44.7 0 0 44.7 0 30.9
# a landmark sighting, then a 3-D edge
EDGE_SE2_XY 7 12 0.5 2.0 10 1 20
EDGE_SE3:QUAT 3 12 1 2 3 0 0 0 1 """ + " ".join(str(float(v)) for v in range(1, 22)) + "\n"


def test_gate_file_parser(tmp_path):
    from rustrobotics_amd.__main__ import parse_gate_file
    index = {3: 0, 7: 1, 12: 2}
    p = tmp_path / "cand.txt"
    p.write_text(GATE_FILE)
    kind, a, b, meas, info, ids = parse_gate_file(str(p), index)
    assert kind == [0, 1, 2] and a == [0, 1, 0] and b == [1, 2, 2]
    assert ids == [(3, 7), (7, 12), (3, 12)]
    assert meas == [1.5, -0.25, 0.125, 0.5, 2.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0]
    assert info == [44.7, 0, 0, 44.7, 0, 30.9, 10, 1, 20] + [float(v) for v in range(1, 22)]
    # an unknown id, an unknown tag, a short line: SystemExit with the line number
    for text, line, word in ((GATE_FILE + "EDGE_SE2 3 99 0 0 0 1 0 0 1 0 1\n", 5, "99"),
                             (GATE_FILE.replace("EDGE_SE2_XY", "EDGE_XY"), 3, "EDGE_XY"),
                             ("EDGE_SE2 3 7 0 0 0 1 0 0 1 0\n", 1, "9 values")):
        p.write_text(text)
        with pytest.raises(SystemExit) as ei:
            parse_gate_file(str(p), index)
        assert f"{p}:{line}:" in str(ei.value) and word in str(ei.value), str(ei.value)
