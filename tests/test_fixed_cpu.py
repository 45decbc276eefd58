"""rr_pgo_set_fixed without a GPU: the reference of tests/fixed_reference.py against itself and against the unchanged oracle,
the --fix ids of the command line, and the exports where they have to be declared."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from fixed_reference import FixedReference, one_free_node_system, reorder_for_fixed_anchor
from oracle.oracle import OracleGraph
from priors_reference import random_priors
from random_graphs import random_graph

CASES = {"se2": dict(n_pose=8, n_lm=3, n_extra=5, se3=False), "se3": dict(n_pose=8, n_lm=0, n_extra=5, se3=True)}


def graph(name):
    return random_graph(np.random.default_rng(17 if name == "se2" else 18), **CASES[name])


def anchor_of(arrays):
    return int(arrays[3][np.flatnonzero(arrays[2] != 1)[0]])


def plain_system(arrays, lam=0.0, lm=False):
    o = OracleGraph.from_arrays(*arrays)
    colptr, rowidx, vals, b = o.build_system(lam, lm)
    n = o.dim
    H = np.zeros((n, n))
    H[rowidx, np.repeat(np.arange(n), np.diff(colptr))] = vals
    return H + np.tril(H, -1).T, b


# ---- self-checks of the reference
@pytest.mark.parametrize("name", ["se2", "se3"])
@pytest.mark.parametrize("lm", [False, True])
def test_fixing_the_anchor_is_the_reduced_system_with_no_1e7_anywhere(name, lm):
    """The oracle's anchor carries the 1e7 on its own diagonal block only, so the system with the anchor fixed is the plain
    system with the anchor's rows and columns deleted: nothing of the term is left, under either keep_anchor."""
    arrays = graph(name)
    anchor = anchor_of(arrays)
    lam = 0.37 if lm else 0.0
    H0, b0 = plain_system(arrays, lam, lm)
    for keep in (True, False):
        ref = FixedReference(arrays, [anchor], keep_anchor=keep)
        H, b = ref.system(lam, lm)
        free = ref.free
        assert len(free) == len(b0) - len(ref.scalars(anchor)) and not set(free) & set(ref.scalars(anchor))
        scale = np.abs(H0[np.ix_(free, free)]).max()
        print(f"{name} lm={lm} keep_anchor={keep}: max|H| {np.abs(H).max():.3g}, max|H - plain| {np.abs(H - H0[np.ix_(free, free)]).max():.3g}")
        assert np.abs(H).max() < 1e7 < np.abs(H0).max()
        assert np.abs(H - H0[np.ix_(free, free)]).max() <= 1e-12 * scale     # (keep_anchor = 0: another edge order)
        assert np.abs(b - b0[free]).max() <= 1e-12 * max(np.abs(b0).max(), 1.0)
        np.linalg.cholesky(H)   # the fixed anchor fixes the gauge
        # the handle's form of it: identity rows, zero blocks, b = 0
        E, eb = ref.expected_system(lam, lm)
        idx = ref.scalars(anchor)
        assert np.array_equal(E[np.ix_(idx, idx)], np.eye(len(idx))) and np.all(eb[idx] == 0.0)
        assert np.all(E[np.ix_(idx, free)] == 0.0) and np.all(E[np.ix_(free, idx)] == 0.0)
        assert np.array_equal(E[np.ix_(free, free)], H)


@pytest.mark.parametrize("name", ["se2", "se3"])
def test_fixing_all_nodes_but_one_is_the_one_node_problem_built_by_hand(name):
    arrays = graph(name)
    n = len(arrays[0])
    anchor = anchor_of(arrays)
    for free in sorted({anchor, 3 if anchor != 3 else 4, n - 1}):   # the anchor, a pose, the last node (SE(2): a landmark)
        ref = FixedReference(arrays, [v for v in range(n) if v != free])
        H, b = ref.system()
        wH, wb = one_free_node_system(arrays, free)
        print(f"{name} free node {free}: max|H - want| {np.abs(H - wH).max():.3g} of {np.abs(wH).max():.3g}")
        assert H.shape == wH.shape
        assert np.abs(H - wH).max() <= 1e-12 * np.abs(wH).max()
        assert np.abs(b - wb).max() <= 1e-12 * max(np.abs(wb).max(), 1.0)
        dx = ref.step()
        assert np.all(dx[ref.fixed_scalars] == 0.0)
        np.testing.assert_allclose(dx[ref.scalars(free)], np.linalg.solve(wH, wb), rtol=1e-9)


@pytest.mark.parametrize("name", ["se2", "se3"])
def test_fixed_nodes_never_move_and_the_cost_counts_every_edge(name):
    arrays = graph(name)
    n = len(arrays[0])
    fixed = [1, 2, anchor_of(arrays)]
    node, meas, info = random_priors(np.random.default_rng(4), arrays, [1, 5], noise=0.3)   # one prior on a fixed node
    ref = FixedReference(arrays, fixed, priors=(node, meas, info))
    # chi2 = the plain graph's + the priors', fixed-fixed edges and the prior on the fixed node included
    s, _ = ref.base.prior_errors()
    np.testing.assert_allclose(ref.cost(), OracleGraph.from_arrays(*arrays).global_error() + s.sum(), rtol=1e-13)
    s0 = ref.state().copy()
    errors, norms, _ = ref.optimize(6)
    assert errors[-1] < errors[0] and len(norms) == len(errors) - 1
    soff = np.concatenate([[0], np.cumsum([{0: 3, 1: 2, 2: 7}[int(k)] for k in arrays[0]])])
    for v in range(n):
        same = np.allclose(ref.state()[soff[v]:soff[v + 1]], s0[soff[v]:soff[v + 1]], rtol=0, atol=1e-15)
        assert same == (v in ref.fixed), v
    # the conditional covariance: zeros at F, the inverse of the reduced H elsewhere, and the two inverses agree
    A, B = ref.sigma_pair()
    assert np.all(A[ref.fixed_scalars, :] == 0.0) and np.all(A[:, ref.fixed_scalars] == 0.0)
    H, _ = ref.system()
    assert np.abs(A[np.ix_(ref.free, ref.free)] @ H - np.eye(len(ref.free))).max() <= 1e-9
    _, floor = ref.blocks(list(range(n)), sig=(A, B))
    assert floor <= 1e-9


def test_reordering_puts_a_fixed_from_node_first_and_keeps_the_graph():
    arrays = graph("se2")
    last = int(arrays[3][np.flatnonzero(arrays[2] != 1)[-1]])   # the from-node of the last pose-pose edge
    assert last != anchor_of(arrays)
    new, order = reorder_for_fixed_anchor(arrays, [last])
    assert sorted(order.tolist()) == list(range(len(arrays[2])))
    assert new[2][0] != 1 and int(new[3][0]) == last == anchor_of(new)
    np.testing.assert_allclose(OracleGraph.from_arrays(*new).global_error(), OracleGraph.from_arrays(*arrays).global_error(), rtol=1e-13)
    with pytest.raises(AssertionError):
        reorder_for_fixed_anchor(arrays, [len(arrays[0]) - 1])   # a landmark is no from-node of a pose-pose edge


# ---- the command line
def test_fix_ids_map_to_node_indices():
    from rustrobotics_amd.__main__ import _ids_arg, fix_indices
    index = {10: 0, 11: 1, 40: 2, 7: 3}
    assert fix_indices(_ids_arg("40,10,7"), index) == [2, 0, 3]
    assert fix_indices(_ids_arg("11,11"), index) == [1, 1]          # the library counts a node listed twice once
    with pytest.raises(SystemExit) as e:
        fix_indices(_ids_arg("10,12"), index)
    assert "no vertex with id 12" in str(e.value)
    import argparse
    for bad in ("", "a,b", "-1"):
        with pytest.raises(argparse.ArgumentTypeError):
            _ids_arg(bad)


def test_free_anchor_needs_priors_or_fix():
    from rustrobotics_amd.__main__ import main
    with pytest.raises(SystemExit):
        main([os.path.join(ROOT, "tests", "golden", "g2o", "intel.g2o"), "--free-anchor"])


def test_the_loader_does_not_learn_the_fix_tag(tmp_path):
    """unknown tags stay RR_PGO_EPARSE, as the reference loader has it -- or ENODEVICE where the handle cannot be made at all"""
    from rustrobotics_amd import PoseGraph, PoseGraphError, _lib
    p = tmp_path / "fix.g2o"
    p.write_text("VERTEX_SE2 0 0 0 0\nVERTEX_SE2 1 1 0 0\nFIX 0\nEDGE_SE2 0 1 1 0 0 1 0 0 1 0 1\n")
    with pytest.raises(PoseGraphError) as e:
        PoseGraph.new(str(p))
    assert e.value.code in (_lib.EPARSE, _lib.ENODEVICE), e.value


# ---- the exports
def test_fixed_exports_are_declared_in_header_mirror_and_integration_guide():
    from rustrobotics_amd import PoseGraph, _lib
    header = open(os.path.join(ROOT, "include", "rr_pgo.h")).read()
    assert re.search(r"\bint\s+rr_pgo_set_fixed\s*\(\s*rr_pgo\s*\*h\s*,\s*int32_t\s+n_fixed\s*,\s*const\s+int32_t\s*\*node\s*,\s*int32_t\s+keep_anchor\s*\)", header)
    assert re.search(r"\bint32_t\s+rr_pgo_num_fixed\s*\(\s*const\s+rr_pgo\s*\*h\s*\)", header)
    assert re.search(r"\bint\s+rr_pgo_get_fixed\s*\(\s*const\s+rr_pgo\s*\*h\s*,\s*int32_t\s*\*out\s*\)", header)
    assert "#define RR_PGO_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4   # exports only
    for name in ("rr_pgo_set_fixed", "rr_pgo_num_fixed", "rr_pgo_get_fixed"):
        assert name in _lib.EXPORTS
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn rr_pgo_set_fixed(" in integration and "fn rr_pgo_num_fixed(" in integration
    assert "fn rr_pgo_get_fixed(" in integration and "pub fn set_fixed(" in integration
    for attr in ("set_fixed", "clear_fixed", "fixed_nodes"):
        assert callable(getattr(PoseGraph, attr))
    assert isinstance(PoseGraph.num_fixed, property)


def test_ctypes_signatures_and_null_handle():
    """where the library loads (it needs no device to load): the mirror's signatures, and a null handle is refused"""
    from rustrobotics_amd import _lib
    L = _lib.load()
    ip = C.POINTER(C.c_int32)
    assert L.rr_pgo_set_fixed.argtypes == [C.c_void_p, C.c_int32, ip, C.c_int32]
    assert L.rr_pgo_num_fixed.argtypes == [C.c_void_p] and L.rr_pgo_num_fixed.restype is C.c_int32
    assert L.rr_pgo_get_fixed.argtypes == [C.c_void_p, ip]
    node = np.zeros(1, np.int32)
    assert L.rr_pgo_set_fixed(None, 1, node.ctypes.data_as(ip), 1) == _lib.EINVAL and b"null" in L.rr_pgo_last_error()
    assert L.rr_pgo_num_fixed(None) == 0
    assert L.rr_pgo_get_fixed(None, node.ctypes.data_as(ip)) == _lib.EINVAL


def test_without_a_device_the_calls_fail_cleanly():
    """a handle needs the device: without one its creation is ENODEVICE, and the entry points refuse the null handle"""
    import torch
    from rustrobotics_amd import PoseGraph, PoseGraphError, _lib
    if torch.cuda.is_available():
        g = PoseGraph.from_arrays(*graph("se2"))
        g.set_fixed([1, 1, 0])
        assert g.num_fixed == 2 and g.fixed_nodes().tolist() == [0, 1]
        return
    with pytest.raises(PoseGraphError) as e:
        PoseGraph.from_arrays(*graph("se2"))
    assert e.value.code in (_lib.ENODEVICE, _lib.EINVAL), e.value
