"""The inputs of tests/test_queries_small_graphs_gpu.py without a GPU: on every graph of tests/query_small_cases.py, at both
states, the CPU references are quiet (the floors of the all-pairs blocks, of d2 and S, and of the joint d2, prefixes and S
are at most FLOOR_MAX), decide both ways, and leave at most one candidate and one set undecided.  The floors are printed
per graph."""
import numpy as np
import pytest

from conftest import g2o_path
from gate_cases import GATE_GRAPHS, candidates
from gate_joint_cases import set_dims
from oracle.oracle import OracleGraph
from query_small_cases import (ALL_PAIRS_MAX_NODES, BIG, DATASETS, FLOOR_MAX, GRAPHS, MAX_PAIRS, MID, SEEDED_NODES, STATES, all_pairs,
                               arrays_of, big_sets, case, references, set_dim, small_joint_sets, state_of)
from robust_reference import oracle_arrays


def check_floors(label, gate, joint):
    print(gate.summary(label))
    print(joint.summary(label))
    floors = dict(d2=gate.floor_d2, S=gate.floor_S, chi2=gate.floor_chi2, joint_d2=joint.floor_d2, joint_prefix=joint.floor_prefix,
                  joint_S=joint.floor_S)
    for what, f in floors.items():
        assert f <= FLOOR_MAX, (label, what, f)
    assert np.all(gate.d2 > 0) and np.all(joint.d2 > 0)
    assert np.sum(gate.undecided) <= 1 and np.sum(joint.undecided) <= 1
    for S in gate.S + joint.S:
        assert np.all(np.linalg.eigvalsh(S) > 0)


@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("name", GRAPHS)
def test_references_are_quiet_and_decide_both_ways(name, which):
    c = case(name, which)
    gate, joint = references((name, which), c["arrays"], c["state"], c["cand"], c["sets"])
    n = len(c["arrays"][0])
    nodes, a, b = all_pairs(n)
    blocks, floor = gate.ref.blocks(a, b)
    print(f"{name} {which}: {n} nodes, dim {gate.ref.n}, {len(blocks)} ordered pairs of {len(nodes)} nodes: floor {floor:.3g}; "
          f"condition number {np.linalg.cond(gate.ref.H):.3g}")
    assert floor <= FLOOR_MAX, (name, which, floor)
    assert len(nodes) == (n if n <= ALL_PAIRS_MAX_NODES else SEEDED_NODES)
    check_floors(f"{name} {which}", gate, joint)
    if gate.n >= 12:
        assert np.any(gate.accept) and np.any(~gate.accept)
        assert np.any(joint.accept) and np.any(~joint.accept)


def test_the_moved_state_is_another_state():
    for name in GRAPHS:
        x0, x1 = state_of(name, "initial"), state_of(name, "moved")
        assert x0.shape == x1.shape and np.max(np.abs(x1 - x0)) > 1e-3, name
        assert np.array_equal(x0, np.asarray(arrays_of(name)[1], np.float64))
        assert np.array_equal(x1, state_of(name, "moved"))   # the same bits every time it is asked for


def test_candidates_cover_the_pairs_and_the_special_cases():
    for name in GRAPHS:
        c = case(name, "initial")
        nk, _, ek, ef, et, _, _ = c["arrays"]
        kind, a, b, _, _ = c["cand"]
        poses = np.flatnonzero(nk != 1)
        n_pairs = len(poses) * (len(poses) - 1)
        stride = -(-n_pairs // MAX_PAIRS)
        n_pp = len(range(0, n_pairs, stride))
        assert n_pp <= MAX_PAIRS and np.all(kind[:n_pp] != 1) and np.all(a != b)
        if stride == 1:   # every ordered pose pair: every relation two fronts can have occurs
            assert set(zip(a[:n_pp].tolist(), b[:n_pp].tolist())) == {(int(p), int(q)) for p in poses for q in poses if p != q}
        anchor = int(ef[np.flatnonzero(ek != 1)[0]])
        assert a[n_pp] == anchor
        n_lm = int(np.sum(kind == 1))
        assert (n_lm > 0) == bool(np.any(nk == 1)) and np.all(nk[b[kind == 1]] == 1) and np.all(nk[a[kind == 1]] == 0)
        assert any(a[-1] == f and b[-1] == t for f, t in zip(ef, et))   # the copy of an existing edge comes last
    assert int(case("landmark-first", "initial")["cand"][1][2]) == 1   # the anchor is the `from` of the second edge


def test_joint_sets_reach_the_caps_and_say_what_they_leave_out():
    seen2, seen3, sizes3 = set(), set(), set()
    for name in GRAPHS:
        c = case(name, "initial")
        kind, sets = c["cand"][0], c["sets"]
        dims = set_dims(kind, sets)
        assert all(1 <= len(s) <= 16 for s in sets) and max(dims) <= 48
        assert all(0 <= q < len(kind) for s in sets for q in s)
        print(f"{name}: {len(kind)} candidates, {len(sets)} sets, D_s up to {max(dims)}, left out: {c['left_out'] or 'nothing'}")
        if np.any(kind == 2):
            seen3 |= set(dims)
            sizes3 |= {len(s) for s in sets}
        else:
            seen2 |= {d for d, s in zip(dims, sets) if len(s) >= 9}
            if name in MID or len(kind) >= 300:
                assert not [w for w in c["left_out"] if "SE2 candidates" in w], c["left_out"]
    assert {27, 32, 36, 44, 47, 48} <= seen2
    assert {6, 12, 42, 48} <= seen3 and {1, 2, 7, 8} <= sizes3
    # a graph too small for a shape says so
    for name in ("two-poses", "landmark-first", "se3-chain3", "clique5"):
        assert case(name, "initial")["left_out"], name
    # a set of 16 with one candidate three times
    kind = case("mid-se2", "initial")["cand"][0]
    triple = [s for s in small_joint_sets(kind)[0] if len(s) == 16 and max(s.count(q) for q in s) == 3]
    assert len(triple) == 1 and set_dim(kind, triple[0]) == 48
    assert BIG == (9, 12, 16)


@pytest.mark.parametrize("name", DATASETS)
def test_sets_of_9_to_16_on_dataset_files_are_quiet(name):
    """the inputs of the two dataset cases of the GPU file: the oracle's own state after GATE_GRAPHS[name] iterations"""
    o = OracleGraph.load(g2o_path(name))
    if GATE_GRAPHS[name]:
        o.optimize(GATE_GRAPHS[name])
    arrays, state = oracle_arrays(o), o.state()
    cand = candidates(arrays, state)
    sets = big_sets(cand[0])
    assert sorted(set(set_dims(cand[0], sets))) == [27, 36, 48] and sorted({len(s) for s in sets}) == [9, 12, 16]
    gate, joint = references(("cpu", name), arrays, state, cand, sets)
    check_floors(name, gate, joint)
    assert np.any(joint.accept) and np.any(~joint.accept)
