"""rr_pgo_set_priors without a GPU: the reference of tests/priors_reference.py against itself and against the unchanged
oracle, the --priors parser of the command line, and the exports where they have to be declared."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle.oracle import OracleGraph
from priors_reference import NODE_DIM, PriorsReference, parse_expected, random_priors
from random_graphs import random_graph

CASES = [("se2", dict(n_pose=8, n_lm=3, n_extra=5, se3=False)), ("se3", dict(n_pose=8, n_lm=0, n_extra=5, se3=True))]


def graph(name):
    kw = dict(CASES)[name]
    return random_graph(np.random.default_rng(7 if name == "se2" else 8), **kw)


def plain_system(arrays, lam=0.0, lm=False):
    o = OracleGraph.from_arrays(*arrays)
    colptr, rowidx, vals, b = o.build_system(lam, lm)
    n = o.dim
    H = np.zeros((n, n))
    H[rowidx, np.repeat(np.arange(n), np.diff(colptr))] = vals
    return H + np.tril(H, -1).T, b


def priors_of(name, arrays, rng):
    """a pose prior, a landmark prior (SE(2)), two priors on one node, a prior on the anchor node"""
    nk, ef, ek = arrays[0], arrays[3], arrays[2]
    anchor = int(ef[np.flatnonzero(ek != 1)[0]])
    nodes = [5, anchor, 2, 2] + ([len(nk) - 1] if name == "se2" else [])
    return random_priors(rng, arrays, nodes)


@pytest.mark.parametrize("name", ["se2", "se3"])
@pytest.mark.parametrize("lm", [False, True])
def test_reduced_augmented_system_is_the_plain_system_plus_the_prior_terms(name, lm):
    """keep_anchor = 1: H and b of the reference = the oracle's system of the plain graph + B^T Omega B / - B^T Omega e of every
    prior, B and e from OracleGraph.linearize_edge on the augmented graph; only the prior nodes' diagonal blocks change."""
    arrays = graph(name)
    node, meas, info = priors_of(name, arrays, np.random.default_rng(3))
    ref = PriorsReference(arrays, node, meas, info)
    lam = 0.37 if lm else 0.0
    H, b = ref.system(lam, lm)
    H0, b0 = plain_system(arrays, lam, lm)
    want_H, want_b = H0.copy(), b0.copy()
    for p, v in enumerate(node):
        _, B, e = ref.g.linearize_edge(int(ref.prior_edge[p]))
        W = ref.prior_omega[p]
        idx = ref.scalars(v)
        want_H[np.ix_(idx, idx)] += B.T @ W @ B
        want_b[idx] -= B.T @ W @ e
    scale = np.abs(want_H).max()
    print(f"{name} lm={lm}: max|H - want| {np.abs(H - want_H).max():.3g}, max|b - want| {np.abs(b - want_b).max():.3g}, scale {scale:.3g}")
    assert np.abs(H - want_H).max() <= 1e-12 * scale
    assert np.abs(b - want_b).max() <= 1e-12 * max(np.abs(want_b).max(), 1.0)
    changed = np.abs(H - H0) > 0
    allowed = np.zeros_like(changed)
    for v in node:
        allowed[np.ix_(ref.scalars(v), ref.scalars(v))] = True
    assert not np.any(changed & ~allowed)
    assert H.max() > 1e7    # the anchor term is where it was
    # chi2 = the plain graph's + the priors' e^T Omega e
    s, w = ref.prior_errors()
    assert np.all(w == 1.0)
    np.testing.assert_allclose(ref.cost(), OracleGraph.from_arrays(*arrays).global_error() + s.sum(), rtol=1e-13)
    np.testing.assert_allclose(ref.prior_cost(), s.sum(), rtol=1e-15)


@pytest.mark.parametrize("name", ["se2", "se3"])
def test_pose_prior_first_moves_the_anchor_to_the_deleted_node(name):
    """keep_anchor = 0: the anchor block loses exactly its 1e7 and nothing else changes against keep_anchor = 1."""
    arrays = graph(name)
    node, meas, info = priors_of(name, arrays, np.random.default_rng(3))
    H1, b1 = PriorsReference(arrays, node, meas, info, keep_anchor=True).system()
    ref0 = PriorsReference(arrays, node, meas, info, keep_anchor=False)
    H0, b0 = ref0.system()
    anchor = int(arrays[3][np.flatnonzero(arrays[2] != 1)[0]])
    idx = ref0.scalars(anchor)
    D = H1 - H0
    want = np.zeros_like(D)
    want[idx, idx] = 1e7
    scale = np.abs(H0).max()
    print(f"{name}: largest entry with the anchor {H1.max():.3g}, without {H0.max():.3g}")
    assert np.abs(D - want).max() <= 1e-9 * 1e7 * 1e-7 + 1e-12 * scale   # (1e7 + h) - h in f64: an ulp of 1e7
    assert H0.max() < 1e7 <= H1.max()
    assert np.abs(b1 - b0).max() <= 1e-12 * max(np.abs(b1).max(), 1.0)
    np.linalg.cholesky(H0)   # the priors fix the gauge: positive definite


@pytest.mark.parametrize("name", ["se2", "se3"])
def test_prior_at_the_nodes_state_costs_nothing(name):
    arrays = graph(name)
    nk = arrays[0]
    nodes = list(range(len(nk)))
    node, meas, info = random_priors(np.random.default_rng(5), arrays, nodes, at_state=True)
    ref = PriorsReference(arrays, node, meas, info)
    s, _ = ref.prior_errors()
    bound = [1e-20 * np.abs(W).max() for W in ref.prior_omega]
    print(f"{name}: max s {s.max():.3g}, smallest bound {min(bound):.3g}")
    assert np.all(s <= bound)
    H, b = ref.system()
    _, b0 = plain_system(arrays)
    assert np.abs(b - b0).max() <= 1e-9 * max(np.abs(b0).max(), 1.0)   # B^T Omega e with e ~ 1e-16


@pytest.mark.parametrize("name", ["se2", "se3"])
def test_anchor_moves_without_its_term_and_stays_with_it(name):
    arrays = graph(name)
    anchor = int(arrays[3][np.flatnonzero(arrays[2] != 1)[0]])
    other = 6 if anchor != 6 else 5
    node, meas, info = random_priors(np.random.default_rng(9), arrays, [other, 1 if anchor != 1 else 2], noise=0.3)
    moved = {}
    for keep in (True, False):
        ref = PriorsReference(arrays, node, meas, info, keep_anchor=keep)
        bmax = float(np.abs(ref.system()[1]).max())
        dx = ref.step()
        moved[keep] = float(np.abs(dx[ref.scalars(anchor)]).max())
        errors, _ = ref.optimize(6)
        assert errors[-1] < errors[0]
    print(f"{name}: |dx| of the anchor with its term {moved[True]:.3g}, without {moved[False]:.3g}")
    # 1e7 on the anchor's diagonal against information of 1e2 .. 1e3 elsewhere: its step is of the order |b| / 1e7
    assert moved[True] <= 10.0 * bmax / 1e7 and moved[False] > 100.0 * moved[True]


def test_robust_flagged_priors_are_weighted_and_the_others_are_not():
    arrays = graph("se2")
    node, meas, info = random_priors(np.random.default_rng(11), arrays, [1, 3, 3, 9], noise=0.5)
    flags = [1, 0, 1, 0]
    ref = PriorsReference(arrays, node, meas, info, robust=flags, kind="huber", delta=1.0)
    s, w = ref.prior_errors()
    assert np.all(s > 1.0)            # every prior is beyond delta^2 ...
    assert np.all(w[[1, 3]] == 1.0) and np.all(w[[0, 2]] < 1.0)   # ... and only the flagged ones are weighted
    # the system: the flagged priors carry w Omega, the edges keep the kernel, the unflagged priors keep Omega
    scaled = info * np.repeat(w, [6 if arrays[0][v] == 0 else 3 for v in node])
    H, b = ref.system()
    H2, b2 = PriorsReference(arrays, node, meas, scaled, robust=None, kind="huber", delta=1.0).system()
    assert np.abs(H - H2).max() <= 1e-12 * np.abs(H2).max() and np.abs(b - b2).max() <= 1e-12 * np.abs(b2).max()
    # the cost: rho for the flagged ones, s for the others
    from robust_reference import rho
    want = np.where(np.array(flags) != 0, rho("huber", s, 1.0), s).sum()
    np.testing.assert_allclose(ref.prior_cost(), want, rtol=1e-14)


# ---- the command line's parser
def test_priors_file_parser(tmp_path):
    from rustrobotics_amd.__main__ import parse_priors_file
    ids = {10: 0, 11: 1, 40: 2}
    kinds = [0, 1, 0]
    text = ("# GPS fixes\n"
            "10 1.5 -2.25 0.125  100 0 0 100 0 1   # pose 10\n"
            "\n"
            "40 3 4 0.5 10 1 2 20 3 30\n"
            "11 7.5 8.5 4 0.5 9\n"
            "10 1.0 -2.0 0.1 1 0 0 1 0 1\n")
    p = tmp_path / "priors.txt"
    p.write_text(text)
    node, meas, info = parse_priors_file(str(p), ids, kinds)
    wn, wm, wi = parse_expected(text, ids, kinds)
    assert list(node) == list(wn) == [0, 2, 1, 0]
    assert np.array_equal(meas, wm) and np.array_equal(info, wi)
    assert len(meas) == 3 + 3 + 2 + 3 and len(info) == 6 + 6 + 3 + 6
    for bad, what in (("12 1 2 3 1 0 0 1 0 1\n", "no vertex with id 12"), ("10 1 2 3 1 0 0 1 0\n", "expected 9 values"),
                      ("11 1 2 3 1 0 0 1 0 1\n", "expected 5 values"), ("10 1 2 x 1 0 0 1 0 1\n", "expected a vertex id and numbers")):
        q = tmp_path / "bad.txt"
        q.write_text("# first line\n" + bad)
        with pytest.raises(SystemExit) as e:
            parse_priors_file(str(q), ids, kinds)
        assert what in str(e.value) and ":2:" in str(e.value), str(e.value)


def test_free_anchor_needs_a_priors_file():
    from rustrobotics_amd.__main__ import main
    with pytest.raises(SystemExit):
        main([os.path.join(ROOT, "tests", "golden", "g2o", "intel.g2o"), "--free-anchor"])


# ---- the exports
def test_priors_exports_are_declared_in_header_mirror_and_integration_guide():
    from rustrobotics_amd import PoseGraph, _lib
    header = open(os.path.join(ROOT, "include", "rr_pgo.h")).read()
    assert re.search(r"\bint\s+rr_pgo_set_priors\s*\(\s*rr_pgo\s*\*h\s*,\s*int32_t\s+n_priors\s*,\s*const\s+int32_t\s*\*node", header)
    assert re.search(r"\bint32_t\s+rr_pgo_num_priors\s*\(\s*const\s+rr_pgo\s*\*h\s*\)", header)
    assert re.search(r"\bint\s+rr_pgo_prior_errors\s*\(\s*rr_pgo\s*\*h\s*,\s*double\s*\*s_out", header)
    assert "#define RR_PGO_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4   # exports only
    for name in ("rr_pgo_set_priors", "rr_pgo_num_priors", "rr_pgo_prior_errors"):
        assert name in _lib.EXPORTS
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn rr_pgo_set_priors(" in integration and "fn rr_pgo_num_priors(" in integration
    assert "fn rr_pgo_prior_errors(" in integration and "pub fn set_priors(" in integration
    for attr in ("set_priors", "clear_priors", "prior_errors"):
        assert callable(getattr(PoseGraph, attr))
    assert isinstance(PoseGraph.num_priors, property)


def test_ctypes_signatures_and_null_handle():
    """where the library loads (it needs no device to load): the mirror's signatures, and a null handle is refused"""
    from rustrobotics_amd import _lib
    L = _lib.load()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    assert L.rr_pgo_set_priors.argtypes == [C.c_void_p, C.c_int32, ip, dp, dp, ip, C.c_int32]
    assert L.rr_pgo_num_priors.argtypes == [C.c_void_p] and L.rr_pgo_num_priors.restype is C.c_int32
    assert L.rr_pgo_prior_errors.argtypes == [C.c_void_p, dp, dp]
    node = np.zeros(1, np.int32)
    z, w = np.zeros(3), np.array([1.0, 0, 0, 1, 0, 1])
    rc = L.rr_pgo_set_priors(None, 1, node.ctypes.data_as(ip), z.ctypes.data_as(dp), w.ctypes.data_as(dp), None, 1)
    assert rc == _lib.EINVAL and b"null" in L.rr_pgo_last_error()
    assert L.rr_pgo_num_priors(None) == 0
    assert L.rr_pgo_prior_errors(None, z.ctypes.data_as(dp), None) == _lib.EINVAL
    assert NODE_DIM[0] == 3
