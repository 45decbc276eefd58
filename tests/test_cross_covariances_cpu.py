"""What tests/test_cross_covariances_gpu.py rests on, without a GPU: the library's two symbols, and the reference
(tests/cross_covariances_reference.py) on the cases of tests/query_small_cases.py -- its column floors, the size of every
block against its column (so that the normwise rule sees an error of the size of any single block), and its consistency
under row subsets and repeats."""
import ctypes as C

import numpy as np
import pytest

from covariances_cases import FLOOR_MAX
from cross_covariances_reference import CrossReference
from marginals_reference import MarginalsReference, graph_at_state, tolerance
from query_small_cases import ALL_PAIRS_MAX_NODES, GRAPHS, STATES, at_state, pair_nodes

CASES = [(name, which) for name in GRAPHS for which in STATES]
IDS = [f"{name}-{which}" for name, which in CASES]
_REFS = {}


def reference(name, which):
    if (name, which) not in _REFS:
        arrays, state = at_state(name, which)
        _REFS[(name, which)] = CrossReference.from_marginals(MarginalsReference(graph_at_state(arrays, state)))
    return _REFS[(name, which)]


def test_the_library_exports_both_symbols_and_the_binding_has_them():
    from rustrobotics_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("rr_pgo_cross_covariances", "rr_pgo_cross_covariances_times"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    L = _lib.load()
    assert len(L.rr_pgo_cross_covariances.argtypes) == 9 and len(L.rr_pgo_cross_covariances_times.argtypes) == 2
    # no handle: refused before anything else, and the message names the entry
    nv = C.c_int64(-1)
    assert L.rr_pgo_cross_covariances(None, 0, None, 0, None, None, None, None, C.byref(nv)) == _lib.EINVAL
    assert "rr_pgo_cross_covariances" in L.rr_pgo_last_error().decode() and nv.value == -1


@pytest.mark.parametrize("argv,word", [(["x.g2o", "--cross", "out.txt"], "--cross needs --columns"),
                                       (["x.g2o", "--columns", "1,2"], "need --cross"),
                                       (["x.g2o", "--cross", "out.txt", "--columns", "1,x"], "ID,ID")])
def test_cli_refuses_cross_without_columns(argv, word, capsys):
    from rustrobotics_amd.__main__ import main
    with pytest.raises(SystemExit) as ei:
        main(argv)
    assert ei.value.code == 2 and word in capsys.readouterr().err


@pytest.mark.parametrize("name,which", CASES, ids=IDS)
def test_column_floors_of_the_reference(name, which):
    ref = reference(name, which)
    cols = pair_nodes(len(ref.dims))
    floors = ref.floors(cols)
    print(f"{name} {which}: {len(cols)} column nodes, worst column floor {max(floors):.3g}")
    assert max(floors) <= FLOOR_MAX


@pytest.mark.parametrize("name,which", [c for c in CASES if c[0] not in ("mid-se2", "mid-se3")],
                         ids=[i for i, c in zip(IDS, CASES) if c[0] not in ("mid-se2", "mid-se3")])
def test_every_block_is_large_against_the_tolerance_of_its_column(name, which):
    """max|R_ab| / max|R_b| >= 100 x tolerance(floor) for every (row node, column node): an error of the size of any single
    block fails the normwise rule.  A condition on the inputs of the GPU comparison, not on the code under test."""
    ref = reference(name, which)
    n = len(ref.dims)
    assert n <= ALL_PAIRS_MAX_NODES
    cols = list(range(n))
    R, _, info = ref.full_columns(cols)
    tol = tolerance(max(f for _, _, f, _ in info))
    lo = np.inf
    for b, c0, _, scale in info:
        for a in range(n):
            lo = min(lo, float(np.max(np.abs(R[ref.scalars(a), c0:c0 + ref.dims[b]])) / scale))
    print(f"{name} {which}: smallest block against its column {lo:.3g} = {lo / tol:.3g} x the tolerance {tol:.3g}")
    assert lo >= 100.0 * tol


@pytest.mark.parametrize("name", ["landmark-first", "se2-1", "se3-2", "mid-se2"])
def test_row_subsets_and_repeats_are_consistent_with_the_full_columns(name):
    ref = reference(name, "initial")
    n = len(ref.dims)
    cols = pair_nodes(n)
    full, floor = ref.block(None, cols)
    assert full.shape == (ref.dim, int(np.sum(ref.dims[cols])))
    rng = np.random.default_rng(41)
    rows = [int(v) for v in rng.choice(n, min(n, 7), replace=False)]
    rows = rows + [rows[0]]
    rep = [cols[-1], cols[0], cols[-1]]
    sub, floor_sub = ref.block(rows, rep)
    co = np.concatenate([[0], np.cumsum(ref.dims[cols])]).astype(int)
    at = {b: k for k, b in enumerate(cols)}
    want = np.vstack([np.hstack([full[ref.scalars(a), co[at[b]]:co[at[b] + 1]] for b in rep]) for a in rows])
    assert np.array_equal(sub, want)
    assert floor_sub <= floor
    assert np.array_equal(sub[:ref.dims[rows[0]]], sub[-ref.dims[rows[0]]:])           # the repeated row node
    d = int(ref.dims[cols[-1]])
    assert np.array_equal(sub[:, :d], sub[:, -d:])                                       # the repeated column node
    # Sigma is symmetric: block (a, b) of one computation against block (b, a)^T, to the floor's tolerance of the two columns
    a, b = cols[0], cols[-1]
    ab, _ = ref.block([a], [b])
    ba, _ = ref.block([b], [a])
    scale = max(s for _, _, _, s in ref.full_columns([a, b])[2])
    assert np.max(np.abs(ab - ba.T)) <= tolerance(floor) * scale
