"""rr_pgo_cross_covariances on the MI355X against the CPU reference (tests/cross_covariances_reference.py).

The rule: a GPU column block G_b passes when max|G_b - R_b| / max|R_b| <= max(1e-12, 100 x floor), max|R_b| over the WHOLE
column, the floor being the worst disagreement of the reference's two f64 computations of the columns (at most FLOOR_MAX).
Every comparison prints its figures before it asserts.  tests/test_cross_covariances_cpu.py checks the reference alone.

The small graphs are the smallest shapes at which k_tree_bwd can go wrong: one root front of 6 .. 18 rows (nr = 0, one
partial 16-column block, every tile clamped on both sides), two to four fronts, multi-block pivot squares with nr no
multiple of 4 or 16 (the seeded random graphs), 41 and 90 fronts over several levels (mid-se2, mid-se3)."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import g2o_path
from covariances_cases import FAR_GRAPHS, far_nodes
from cross_covariances_reference import CrossReference, check_columns
from marginals_reference import MarginalsReference, graph_at_state, tolerance
from query_small_cases import GRAPHS, STATES, case, pair_nodes, references

pytestmark = pytest.mark.gpu

CASES = [(name, which) for name in GRAPHS for which in STATES]
IDS = [f"{name}-{which}" for name, which in CASES]
NODE_DIM = np.array([3, 2, 6])


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver
    return PoseGraph, PoseGraphSolver


_HANDLES, _REFS, _INTEL = {}, {}, {}


def handle(api, name, which):
    if (name, which) not in _HANDLES:
        _HANDLES[(name, which)] = api[0].from_arrays(*case(name, which)["arrays"])
    return _HANDLES[(name, which)]


def small_ref(name, which):
    """CrossReference of a small case on the MarginalsReference the other query tests of the case use"""
    if (name, which) not in _REFS:
        c = case(name, which)
        _REFS[(name, which)] = CrossReference.from_marginals(references((name, which), c["arrays"], c["state"], c["cand"], c["sets"])[0].ref)
    return _REFS[(name, which)]


def dataset_ref(g, key):
    """CrossReference of a dataset file at the handle's state"""
    if key not in _REFS:
        _REFS[key] = CrossReference.from_marginals(MarginalsReference(graph_at_state(g.graph_arrays(), g.state())))
    return _REFS[key]


def intel(api):
    """one intel handle at its initial state and its all-rows x far_nodes block, shared by the tests that only read it"""
    if not _INTEL:
        g = api[0].new(g2o_path("intel"))
        cols = far_nodes(g.num_nodes)
        _INTEL.update(g=g, cols=cols, X=g.cross_covariance(None, cols))
    return _INTEL["g"], _INTEL["cols"], _INTEL["X"]


def tree(g):
    s = g.stats()
    return {k: s[k] for k in ("n_supernodes", "n_levels", "max_front", "max_pivot_cols", "nnz_l_scalars", "n_big_fronts")}


def ref_kinds(g):
    return g.graph_arrays()[0]


def offsets(kinds, nodes):
    return np.concatenate([[0], np.cumsum(NODE_DIM[np.asarray(kinds)[np.asarray(nodes, int)]])]).astype(int)


def col_slices(kinds, cols):
    o = offsets(kinds, cols)
    return [slice(o[k], o[k + 1]) for k in range(len(cols))]


# ---- 1. small graphs: all rows x every node (n <= 80) or the seeded nodes ---------------------------------------------------

@pytest.mark.parametrize("name,which", CASES, ids=IDS)
def test_all_rows_of_the_columns_of_a_small_graph(api, name, which):
    g, ref = handle(api, name, which), small_ref(name, which)
    n = g.num_nodes
    print(f"{name} {which}: {tree(g)}")
    assert g.stats()["n_big_fronts"] == 0
    cols = pair_nodes(n)
    X = g.covariance_columns(cols)
    assert X.shape == (g.len, int(np.sum(ref.dims[cols])))
    check_columns(f"{name} {which} all rows x {len(cols)} column nodes", X, ref, None, cols)


# ---- 2. against rr_pgo_covariances, and block (a, b) against block (b, a)^T -------------------------------------------------

@pytest.mark.parametrize("name,which", CASES, ids=IDS)
def test_blocks_agree_with_the_pair_query_and_with_their_transposes(api, name, which):
    """cross block (a, b) lies in column b, block (b, a) in column a, and rr_pgo_covariances' block (a, b) passes its own rule
    relative to max|R_ab| <= max|R_b|: any two of them differ by at most tol_a max|R_a| + tol_b max|R_b|."""
    g, ref = handle(api, name, which), small_ref(name, which)
    nodes = pair_nodes(g.num_nodes)
    k = len(nodes)
    X = g.cross_covariance(nodes, nodes)
    _, _, info = ref.full_columns(nodes)
    bound = np.array([tolerance(f) * s for _, _, f, s in info])
    sl = col_slices(ref_kinds(g), nodes)
    vals, off = g.covariance_blocks(np.repeat(nodes, k).astype(np.int32), np.tile(nodes, k).astype(np.int32))
    worst_q, worst_t = 0.0, 0.0
    for i in range(k):
        for j in range(k):
            blk = X[sl[i], sl[j]]
            lim = bound[i] + bound[j]
            q = i * k + j
            dq = float(np.max(np.abs(blk - vals[off[q]:off[q + 1]].reshape(blk.shape))))
            dt = float(np.max(np.abs(blk - X[sl[j], sl[i]].T)))
            worst_q, worst_t = max(worst_q, dq / lim), max(worst_t, dt / lim)
    print(f"{name} {which}: {k * k} blocks, worst difference to rr_pgo_covariances {worst_q:.3g} of its bound, to the transposed block {worst_t:.3g} of its bound")
    assert worst_q <= 1.0 and worst_t <= 1.0


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------

def bit_case(api, name):
    if name == "intel":
        return intel(api)
    g = handle(api, name, "initial")
    cols = pair_nodes(g.num_nodes)
    return g, cols, g.cross_covariance(None, cols)


@pytest.mark.parametrize("name", ["se2-1", "se3-2", "mid-se2", "intel"])
def test_the_bits_of_a_block_depend_on_its_row_and_column_alone(api, name):
    g, cols, X = bit_case(api, name)
    n = g.num_nodes
    kinds = ref_kinds(g)
    sl = col_slices(kinds, cols)
    ro = offsets(kinds, range(n))
    assert np.array_equal(g.cross_covariance(None, cols), X)                       # a repeated call
    for k, b in enumerate(cols):                                                   # every column node alone
        assert np.array_equal(g.cross_covariance(None, [b]), X[:, sl[k]]), b
    back = cols[::-1]
    Xr = g.cross_covariance(None, back)
    for k, s in enumerate(col_slices(kinds, back)):                                # the list reversed
        assert np.array_equal(Xr[:, s], X[:, sl[len(cols) - 1 - k]]), back[k]
    rep = [cols[0], cols[-1], cols[0]] + list(cols) + [cols[len(cols) // 2]]
    at = {b: k for k, b in enumerate(cols)}
    Xp = g.cross_covariance(None, rep)
    for k, s in enumerate(col_slices(kinds, rep)):                                 # ... and with repeats
        assert np.array_equal(Xp[:, s], X[:, sl[at[rep[k]]]]), rep[k]
    rng = np.random.default_rng(41)
    rows = [int(v) for v in rng.choice(n, min(n, 12), replace=False)]
    rows = rows + [rows[0]]                                                        # a row subset with a repeat
    want = np.vstack([X[ro[v]:ro[v + 1]] for v in rows])
    assert np.array_equal(g.cross_covariance(rows, cols), want)
    for _ in range(20):                                                            # one (a, b) alone
        a, k = int(rng.integers(0, n)), int(rng.integers(0, len(cols)))
        assert np.array_equal(g.cross_covariance([a], [cols[k]]), X[ro[a]:ro[a + 1], sl[k]]), (a, cols[k])
    # (+0.0 and -0.0 are equal to array_equal: the sign bits of a repeated call too)
    assert np.array_equal(np.signbit(g.cross_covariance(None, cols)), np.signbit(X))


# ---- 4. a list cut by the workspace bound -------------------------------------------------------------------------------------

def test_a_column_list_cut_by_the_workspace_bound_gives_the_same_bits(api, monkeypatch):
    """48 seeded distinct column nodes of intel, all rows: 144 columns, at least 5 chunks.  One column node alone needs Z + U of
    its root path and V of ONE chunk (every front, the same figure for every node); rr_pgo_covariances' refusal of the pair
    (q, q) under the same bound names Z + U alone, so V is the difference.  The whole list needs at least 5 V, which is
    asserted to exceed the largest single need: the handle bounded by that figure must cut the list.  The cut changes no bit."""
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]

    def bounded(bound):
        monkeypatch.setenv("RR_PGO_TS_WS_BYTES", str(bound))
        g = PoseGraph.new(g2o_path("intel"))
        monkeypatch.delenv("RR_PGO_TS_WS_BYTES")
        return g

    def refused(call, pattern):
        with pytest.raises(PoseGraphError) as ei:
            call()
        assert ei.value.code == _lib.ENOMEM, ei.value
        msg = _lib.load().rr_pgo_last_error().decode()
        m = re.fullmatch(pattern, msg)
        assert m, msg
        return int(m.group(1))

    A = PoseGraph.new(g2o_path("intel"))
    nodes = [int(v) for v in np.random.default_rng(17).choice(A.num_nodes, 48, replace=False)]
    X = A.cross_covariance(None, nodes)
    B = bounded(1)
    need = [refused(lambda: B.cross_covariance(None, [v]), r"rr_pgo_cross_covariances: one column node needs (\d+) bytes of workspace") for v in nodes]
    zu = [refused(lambda: B.covariance_blocks([v], [v]), r"rr_pgo_covariances: one pair needs (\d+) bytes of workspace") for v in nodes]
    V = {a - b for a, b in zip(need, zu)}
    print(f"intel, 48 column nodes alone: workspace needs {min(need)} .. {max(need)} bytes, of which V of one chunk {sorted(V)}")
    assert len(V) == 1 and min(V) > 0
    assert 5 * min(V) > max(need)          # the whole list (at least 5 chunks) does not fit the bound of the next handle
    Cc = bounded(max(need))
    assert np.array_equal(Cc.cross_covariance(None, nodes), X)
    D = bounded(max(need) - 1)
    worst = nodes[int(np.argmax(need))]
    assert refused(lambda: D.cross_covariance(None, [worst]), r"rr_pgo_cross_covariances: one column node needs (\d+) bytes of workspace") == max(need)


# ---- 5. dataset files ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", ["initial", "optimized"])
@pytest.mark.parametrize("name", FAR_GRAPHS)
def test_all_rows_of_24_columns_of_a_dataset_file(api, name, state):
    if (name, state) == ("intel", "initial"):
        g, cols, X = intel(api)
    else:
        g = api[0].new(g2o_path(name))
        if state == "optimized":
            g.optimize(10)
        cols = far_nodes(g.num_nodes)
        X = g.cross_covariance(None, cols)
    print(f"{name} {state}: {tree(g)}, {g.num_nodes} nodes, {int(np.sum(ref_kinds(g) == 1))} landmarks")
    t = g.cross_covariances_times()
    print(f"{name} {state}: linearise + factor {t[0]:.3f} ms, forward + backward solve {t[1]:.3f} ms, gather + copy {t[2]:.3f} ms")
    check_columns(f"{name} {state} all rows x 24 column nodes", X, dataset_ref(g, (name, state)), None, cols)


# ---- 6. the handle is untouched ------------------------------------------------------------------------------------------------

def launch_counts(g):
    st = g.stats()
    return [st[k] for k in ("n_plain_iterations", "n_graph_replays", "n_loop_items", "n_graph_captures")]


@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
def test_optimize_around_cross_covariances_gives_the_same_bits(api, solver):
    PoseGraph, Solver = api
    a = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    b = PoseGraph.new(g2o_path("intel"), getattr(Solver, solver))
    cols = far_nodes(a.num_nodes)
    a.cross_covariance(None, cols)
    ea, na = a.optimize(10, return_norms=True)
    eb, nb = b.optimize(10, return_norms=True)
    assert np.array_equal(np.array(ea), np.array(eb)) and np.array_equal(np.array(na), np.array(nb))
    assert np.array_equal(a.state(), b.state())
    a.cross_covariance(cols[:5], cols[3:9])   # ... and between two optimize calls
    assert np.array_equal(np.array(a.optimize(3)), np.array(b.optimize(3)))
    assert np.array_equal(a.state(), b.state())
    assert launch_counts(a) == launch_counts(b)
    qa, qb = np.array(cols[:12], np.int32), np.array(cols[12:], np.int32)
    va, oa = a.covariance_blocks(qa, qb)
    vb, ob = b.covariance_blocks(qa, qb)
    assert np.array_equal(oa, ob) and np.array_equal(va, vb)


# ---- 7. robust weights, priors, fixed nodes -----------------------------------------------------------------------------------

def test_cauchy_weights_are_part_of_the_inverted_matrix(api):
    from robust_reference import RobustReference
    _, cols, plain = intel(api)
    g = api[0].new(g2o_path("intel"))
    g.set_robust_kernel("cauchy", 1.0)
    X = g.cross_covariance(None, cols)
    gw, w = RobustReference(g.graph_arrays(), "cauchy", 1.0).weighted_graph()
    assert np.min(w) < 0.5   # the weights matter at the initial state
    check_columns("intel cauchy delta 1, all rows x 24 column nodes", X, CrossReference.from_marginals(MarginalsReference(gw)), None, cols)
    assert np.max(np.abs(X - plain)) / np.max(np.abs(plain)) > 1e-3


def query_graph(dim):
    """the query graphs of tests/test_priors_gpu.py and tests/test_fixed_gpu.py: 28 / 26 nodes"""
    from random_graphs import random_graph
    if dim == "se2":
        return random_graph(np.random.default_rng(23), n_pose=22, n_lm=6, n_extra=14)
    return random_graph(np.random.default_rng(24), n_pose=26, n_lm=0, n_extra=14, se3=True)


@pytest.mark.parametrize("dim", ["se2", "se3"])
@pytest.mark.parametrize("keep", [1, 0])
def test_with_priors(api, dim, keep):
    from priors_reference import PriorsReference, random_priors
    arrays = query_graph(dim)
    n = len(arrays[0])
    node, meas, info = random_priors(np.random.default_rng(10), arrays, [4, 11, 11, n - 1, 17], noise=0.2)
    g = api[0].from_arrays(*arrays)
    g.optimize(3)
    plain = g.covariance_columns(list(range(n)))
    g.set_priors(node, meas, info, keep_anchor=bool(keep))
    ref = PriorsReference(arrays, node, meas, info, keep_anchor=keep)
    ref.set_state(g.state())
    cref = CrossReference.from_sigma_pair(ref.sigma_pair(), arrays[0])
    X = g.covariance_columns(list(range(n)))
    check_columns(f"{dim} priors keep_anchor={keep}, all rows x all {n} nodes", X, cref, None, list(range(n)))
    rows, cols = [5, n - 1, 0, 5], [11, 2, n - 1]
    check_columns(f"{dim} priors keep_anchor={keep}, 4 row nodes x 3 column nodes", g.cross_covariance(rows, cols), cref, rows, cols)
    assert np.max(np.abs(X - plain)) / np.max(np.abs(plain)) > 1e-3      # the priors are part of the inverted matrix


QUERY_F = {"se2": [3, 8, 15, 19, 25], "se3": [3, 8, 15, 19, 24]}     # (tests/test_fixed_gpu.py) se2: 25 is a landmark


@pytest.mark.parametrize("dim", ["se2", "se3"])
def test_with_fixed_nodes(api, dim):
    from fixed_reference import FixedReference
    arrays = query_graph(dim)
    n = len(arrays[0])
    F = QUERY_F[dim]
    g = api[0].from_arrays(*arrays)
    never = api[0].from_arrays(*arrays)
    g.optimize(3)
    never.optimize(3)
    st = g.state()
    g.set_fixed(F)
    ref = FixedReference(arrays, F)
    ref.set_state(st)
    cref = CrossReference.from_sigma_pair(ref.sigma_pair(), arrays[0])
    every = list(range(n))
    X = g.covariance_columns(every)
    o = offsets(arrays[0], every)
    for v in F:     # every entry of a fixed node's rows and columns is +0.0
        for Z in (X[o[v]:o[v + 1], :], X[:, o[v]:o[v + 1]]):
            assert np.all(Z == 0.0) and not np.any(np.signbit(Z)), v
    free = [v for v in every if v not in F]
    check_columns(f"{dim} fixed {F}, all rows x all {n} nodes", X, cref, None, every)
    check_columns(f"{dim} fixed {F}, the free rows x the free columns", g.cross_covariance(free, free), cref, free, free)
    sub = g.cross_covariance([F[0], free[0], F[1]], [free[1], F[2]])
    so = offsets(arrays[0], [F[0], free[0], F[1]])
    d = NODE_DIM[arrays[0][free[1]]]
    for Z in (sub[:, d:], sub[so[0]:so[1]], sub[so[2]:so[3]]):
        assert np.all(Z == 0.0) and not np.any(np.signbit(Z))
    assert np.array_equal(sub[so[1]:so[2], :d], X[o[free[0]]:o[free[0] + 1], o[free[1]]:o[free[1] + 1]])
    g.clear_fixed()
    assert np.array_equal(g.covariance_columns(every), never.covariance_columns(every))


# ---- 8. refusals and arguments --------------------------------------------------------------------------------------------------

def test_arguments_size_query_and_empty_lists(api):
    from rustrobotics_amd import _lib
    L = _lib.load()
    g = api[0].new(g2o_path("simulation-pose-landmark"))
    n = g.num_nodes
    dims = NODE_DIM[g.graph_arrays()[0]]
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    rows, cols = np.array([n - 1, 0, 3, 0], np.int32), np.array([2, n - 1, 2], np.int32)
    R, Cn = int(np.sum(dims[rows])), int(np.sum(dims[cols]))
    pr, pc = rows.ctypes.data_as(ip), cols.ctypes.data_as(ip)
    nv, ro, co = C.c_int64(-1), np.zeros(5, np.int64), np.zeros(4, np.int64)
    # the size query, with and without the offsets
    assert L.rr_pgo_cross_covariances(g._h, 4, pr, 3, pc, None, ro.ctypes.data_as(lp), co.ctypes.data_as(lp), C.byref(nv)) == 0
    assert nv.value == R * Cn and np.array_equal(np.diff(ro), dims[rows]) and np.array_equal(np.diff(co), dims[cols])
    nv.value = -1
    assert L.rr_pgo_cross_covariances(g._h, n, None, 3, pc, None, None, None, C.byref(nv)) == 0 and nv.value == g.len * Cn
    # the call itself, without offsets, against the Python wrapper
    out = np.full(R * Cn, -777.0)
    assert L.rr_pgo_cross_covariances(g._h, 4, pr, 3, pc, out.ctypes.data_as(dp), None, None, C.byref(nv)) == 0
    assert np.array_equal(out.reshape(R, Cn), g.cross_covariance(rows, cols))
    # empty lists: OK, nothing written, *n_vals = 0
    poison = np.full(8, -777.0)
    pp = poison.ctypes.data_as(dp)
    for args in ((4, pr, 0, None), (4, pr, 0, pc), (0, pr, 3, pc), (n, None, 0, None)):
        nv.value = -1
        assert L.rr_pgo_cross_covariances(g._h, args[0], args[1], args[2], args[3], pp, None, None, C.byref(nv)) == 0, args
        assert nv.value == 0 and np.all(poison == -777.0)
    assert g.cross_covariance([1, 2], []).shape == (int(np.sum(dims[[1, 2]])), 0)
    # every RR_PGO_EINVAL case: nothing is written, the message names the entry
    big = np.full(R * Cn + 64, -777.0)
    pb = big.ctypes.data_as(dp)
    bad_hi, bad_lo = np.array([0, n], np.int32), np.array([-1, 1], np.int32)
    einval = {
        "negative n_row": (-1, pr, 3, pc, C.byref(nv)),
        "negative n_col": (4, pr, -1, pc, C.byref(nv)),
        "col_node NULL with n_col > 0": (4, pr, 3, None, C.byref(nv)),
        "row_node NULL with n_row != num_nodes": (n - 1, None, 3, pc, C.byref(nv)),
        "row_node NULL with n_row 0": (0, None, 3, pc, C.byref(nv)),
        "a row node past the end": (2, bad_hi.ctypes.data_as(ip), 3, pc, C.byref(nv)),
        "a negative row node": (2, bad_lo.ctypes.data_as(ip), 3, pc, C.byref(nv)),
        "a column node past the end": (4, pr, 2, bad_hi.ctypes.data_as(ip), C.byref(nv)),
        "a negative column node": (4, pr, 2, bad_lo.ctypes.data_as(ip), C.byref(nv)),
        "n_vals NULL": (4, pr, 3, pc, None),
    }
    for what, (nr_, r_, nc_, c_, v_) in einval.items():
        nv.value = -1
        assert L.rr_pgo_cross_covariances(g._h, nr_, r_, nc_, c_, pb, None, None, v_) == _lib.EINVAL, what
        msg = L.rr_pgo_last_error().decode()
        print(what, "->", msg)
        assert "rr_pgo_cross_covariances" in msg, (what, msg)
        assert np.all(big == -777.0) and nv.value == -1, what
    ms = np.zeros(3)
    assert L.rr_pgo_cross_covariances_times(g._h, ms.ctypes.data_as(dp)) == 0 and np.all(ms >= 0) and ms[0] > 0
    assert L.rr_pgo_cross_covariances_times(g._h, None) == _lib.EINVAL


def test_unsupported_handles_say_why_in_the_words_of_the_pair_query(api):
    from rustrobotics_amd import _lib
    from rustrobotics_amd.mapping import PoseGraphError
    PoseGraph = api[0]
    handles = {
        "mixed": (PoseGraph.new(g2o_path("intel"), precision="mixed"), "MIXED"),
        "f32": (PoseGraph.new(g2o_path("intel"), precision="f32"), "F32"),
        "sphere2500": (PoseGraph.new(g2o_path("sphere2500")), "beyond LDS"),
    }
    for what, (h, word) in handles.items():
        said = []
        for call in (lambda: h.covariance_blocks([0], [1]), lambda: h.cross_covariance([0], [1])):
            with pytest.raises(PoseGraphError) as ei:
                call()
            assert ei.value.code == _lib.EUNSUPPORTED, (what, ei.value)
            said.append(_lib.load().rr_pgo_last_error().decode())
        print(what, "->", said[1])
        assert word in said[1] and said[1] == said[0].replace("rr_pgo_covariances", "rr_pgo_cross_covariances"), (what, said)


def test_after_extend_the_call_answers_for_the_grown_graph(api):
    from extend_cases import case as extend_case
    c = extend_case("simulation-pose-landmark")
    g = api[0].from_arrays(*c.base)
    before = g.covariance_columns([0, 2])
    args, kwargs = c.extend_args()
    g.extend(*args, **kwargs)
    fresh = api[0].from_arrays(*c.grown)
    assert np.array_equal(fresh.state(), g.state())
    n = g.num_nodes
    cols = [0, 2, n - 1]
    X = g.covariance_columns(cols)
    assert X.shape[0] == g.len > before.shape[0]
    assert np.array_equal(X, fresh.covariance_columns(cols))
    assert np.array_equal(g.cross_covariance([n - 1, 1], [n - 2]), fresh.cross_covariance([n - 1, 1], [n - 2]))
