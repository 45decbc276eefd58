"""The inputs and references of tests/test_big_front_queries_gpu.py, without a GPU: the generator is deterministic, the host
analysis of the written g2o files reports fronts beyond LDS (under the pin the GPU test names for n = 5 and n = 6), the
references' own floors are within FLOOR_MAX on every case and state, and the references alone leave at most one gate
candidate undecided per case -- the cap tests/test_gate_gpu.py uses."""
import hashlib

import numpy as np
import pytest

from big_front_cases import (AUDIT_EDGES, LATTICES, N_LANDMARKS, QUERY_NODES, SEEDS, SIGHTINGS, STATES, arrays_of, at_state, audit_edges,
                             marginals_reference, ordered_pairs, query_case, se3_lattice, seeded_nodes)
from covariances_cases import FLOOR_MAX
from landmarks3d_cases import to_g2o

PIN = {"RR_PGO_ND_LEAF": "1000000", "RR_PGO_AMALG_NP": "72"}   # tests/test_big_front_queries_gpu.py, PINS
PINS = {"lattice5": PIN, "lattice6": PIN, "lattice7": {}, "landmarks6": {}}
# (n_supernodes, n_levels, max_front, max_pivot_cols, n_big_fronts) of the host analysis
ANALYSIS = {"lattice5": (32, 2, 186, 186, 1), "lattice6": (63, 3, 276, 264, 3), "lattice7": (110, 5, 312, 222, 10),
            "landmarks6": (82, 5, 444, 444, 10)}


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name", list(PINS))
def test_the_generator_is_deterministic(name):
    a = arrays_of(name)
    from big_front_cases import landmark_lattice
    b = landmark_lattice() if name == "landmarks6" else se3_lattice(LATTICES[name], SEEDS[LATTICES[name]])
    assert digest(a) == digest(b)
    nk, ns, ek, ef, et, em, ei = a
    n = 6 if name == "landmarks6" else LATTICES[name]
    n_lm = N_LANDMARKS if name == "landmarks6" else 0
    assert len(nk) == n ** 3 + n_lm and np.sum(nk == 2) == n ** 3
    assert len(ek) == 3 * n * n * (n - 1) + SIGHTINGS * n_lm
    assert (ef[0], et[0]) == (0, 1) and ek[0] == 2   # the first edge stays first: node 0 is the anchor
    assert len(ns) == 7 * n ** 3 + 3 * n_lm and len(em) == 7 * np.sum(ek == 2) + 3 * np.sum(ek == 3)
    deg = np.bincount(np.concatenate([ef, et]), minlength=len(nk))
    assert deg[:n ** 3].min() >= 3 and (n_lm == 0 or np.all(deg[n ** 3:] == SIGHTINGS))
    if name != "landmarks6":
        assert digest(a) != digest(se3_lattice(n, SEEDS[n] + 1))


@pytest.mark.parametrize("name", list(PINS))
def test_the_host_analysis_reports_fronts_beyond_lds(name, tmp_path, monkeypatch):
    from rustrobotics_amd import PoseGraph
    path = tmp_path / f"{name}.g2o"
    path.write_text(to_g2o(list(arrays_of(name))))
    for k, v in PINS[name].items():
        monkeypatch.setenv(k, v)
    s = PoseGraph.analyze(str(path))
    got = tuple(s[k] for k in ("n_supernodes", "n_levels", "max_front", "max_pivot_cols", "n_big_fronts"))
    print(f"{name} under {PINS[name]}: (n_supernodes, n_levels, max_front, max_pivot_cols, n_big_fronts) = {got}")
    assert got == ANALYSIS[name]
    assert s["n_big_fronts"] >= (1 if name == "lattice5" else 3)
    if name in ("lattice6", "lattice7"):
        assert s["max_front"] > s["max_pivot_cols"]


@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("name", list(LATTICES))
def test_the_references_floors_and_undecided_candidates(name, which):
    c = query_case(name, which)
    gate, joint = c["gate"], c["joint"]
    print(gate.summary(f"{name} {which}"))
    print(joint.summary(f"{name} {which}"))
    for f in (gate.floor_d2, gate.floor_S, gate.floor_chi2, joint.floor_d2, joint.floor_S, joint.floor_prefix):
        assert f <= FLOOR_MAX
    assert np.sum(gate.undecided) <= 1 and np.sum(joint.undecided) <= 1
    n = len(c["arrays"][0])
    nodes = seeded_nodes(n, [0])
    assert len(set(nodes)) == QUERY_NODES and nodes[0] == 0
    a, b = ordered_pairs(nodes)
    _, floor = marginals_reference(name, which).blocks(a, b)
    print(f"{name} {which}: all pairs of {QUERY_NODES} seeded nodes, noise floor {floor:.3g}")
    assert floor <= FLOOR_MAX
    if name == "lattice6":
        from check_edges_cases import reference
        edges = audit_edges(c["arrays"])
        assert len(set(edges.tolist())) == AUDIT_EDGES
        ref = reference(("big-fronts", name, which), c["arrays"], c["state"], edges)
        print(ref.summary(f"{name} {which}"))
        assert ref.floors_ok() and np.all(ref.compared) and not np.any(ref.singular)


@pytest.mark.parametrize("which", STATES)
def test_the_landmark_reference(which):
    from landmarks3d_reference import Landmarks3dReference
    arrays, _ = at_state("landmarks6", which)
    ref = Landmarks3dReference(list(arrays))
    sig = ref.sigma_pair()
    edges = audit_edges(arrays)
    _, d2, red, _, fR, fd, fc, fr = ref.check(edges, sig=sig)
    print(f"landmarks6 {which}: audit floors R {fR:.3g} d2 {fd.max():.3g} chi2 {fc.max():.3g} r {fr.max():.3g}; redundancy {red.min():.3g} .. {red.max():.3g}")
    assert np.all(np.isfinite(d2)) and max(fR, fd.max(), fc.max(), fr.max()) <= FLOOR_MAX
    assert np.any(arrays[2][edges] == 3) and np.any(arrays[2][edges] == 2)
    from test_landmarks3d_gpu import candidates as candidates3d
    cand = candidates3d(list(arrays), 51)
    _, gd2, _, fS, fd2 = ref.gate(cand, sig=sig)
    _, _, fSj, fdj = ref.gate_joint(cand, [[0, 6], [7, 1, 8], [2, 3], [9, 10, 11], [4, 9, 5, 6]], sig=sig)
    print(f"landmarks6 {which}: gate floors S {fS:.3g} d2 {fd2:.3g}, joint floors S {fSj:.3g} d2 {fdj:.3g}; d2 {gd2.min():.3g} .. {gd2.max():.3g}")
    assert max(fS, fd2, fSj, fdj) <= FLOOR_MAX
