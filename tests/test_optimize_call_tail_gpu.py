"""What rr_pgo_optimize leaves behind a call, and what runs straight behind it.

A call of the device-side loop (pgo_api.hip, optimize_pipelined) ends with the item that was enqueued behind the stop: its
linearisation publishes the final chi2 -- the call returns on that -- and the launches behind it return at the stop word,
having read nothing else: no ticket, flag, counter, partial, pose or ring slot.  They are still on the stream when the next
thing the handle is asked (another call, a restart, a query, its destruction) arrives.  None of that may change a bit:
every comparison here is of the errors list, the |dx| list and the gathered state, bit for bit.

The graphs are the smallest on which the tail can go wrong: 77 nodes (a handful of tasks: a stray ticket shows at once),
400 nodes, intel, and a 100 x 100 lattice whose top fronts are beyond LDS but whose iteration (40 launches) stays on the
device-side loop."""
import gc

import numpy as np
import pytest

from conftest import g2o_path

pytestmark = pytest.mark.gpu

GRAPHS = ["simulation-pose-landmark", "simulation-pose-pose", "intel", "lattice"]
SOLVERS = ["GaussNewton", "LevenbergMarquardt"]
REPEATS = 30


@pytest.fixture(scope="module")
def api():
    import os
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver, _lib
    assert os.path.exists(_lib.LIB_PATH), "HIP extension missing: the product path has no fallback"
    return PoseGraph, PoseGraphSolver


_lattice = []


def _new(api, name, solver="GaussNewton"):
    Solver = getattr(api[1], solver)
    if name != "lattice":
        return api[0].new(g2o_path(name), Solver)
    if not _lattice:
        from rustrobotics_amd import synthetic_grid_arrays
        _lattice.append(synthetic_grid_arrays(100, 100))
    g = api[0].from_arrays(*_lattice[0], precision="f64", solver=Solver)
    st = g.stats()
    assert 8 < st["n_launches_per_iter"] < 48 and st["n_big_fronts"] > 0   # fronts beyond LDS, still the device-side loop
    return g


def _host_loop(api, name, solver, monkeypatch):
    """A handle whose rr_pgo_optimize makes one host round trip per iteration: no items enqueued ahead, no tail."""
    monkeypatch.setenv("RR_PGO_SYNC_OPTIMIZE", "1")
    try:
        return _new(api, name, solver)
    finally:
        monkeypatch.delenv("RR_PGO_SYNC_OPTIMIZE")


def _call(g, iters=10):
    e, n = g.optimize(iters, return_norms=True)
    return np.array(e), np.array(n)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


_start = {}


def _start_state(api, name):
    """The initial state as rr_pgo_get_state / rr_pgo_set_state round-trip it, computed once per graph."""
    if name not in _start:
        _start[name] = np.array(_new(api, name).state())
    return _start[name]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", GRAPHS)
def test_back_to_back_calls_from_the_same_state(api, name, solver):
    """The benchmark's pattern: set_state(s0) + optimize(10), thirty times on one handle, nothing in between.  Every repeat
    is the first one, and the first one is the call a fresh handle makes."""
    s0 = _start_state(api, name)
    fresh = _new(api, name, solver)
    fresh.set_state(s0)
    want = _call(fresh) + (np.array(fresh.state()),)
    g = _new(api, name, solver)
    got = []
    for _ in range(REPEATS):
        g.set_state(s0)
        got.append(_call(g))
    state = np.array(g.state())
    for r, (e, n) in enumerate(got):
        assert _same((e, n), want[:2]), (name, solver, r, e, want[0])
    assert np.array_equal(state, want[2])


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", GRAPHS)
def test_the_shortest_call_behind_a_tail(api, name, solver, monkeypatch):
    """optimize(10) again and again WITHOUT a restart: on the converged state a call stops after its first iteration, so
    the previous call's tail is a large part of what the stream holds.  Nothing is read between the calls.  The same sequence on a host-loop
    handle started from the same state (every call is a function of the state it starts from, so call by call this is
    'the same call on a handle set to that state'), and the first of them on a fresh device-loop handle."""
    s0 = _start_state(api, name)
    g = _new(api, name, solver)
    g.set_state(s0)
    _call(g)
    s1 = np.array(g.state())
    g.set_state(s1)   # (rr_pgo_get_state / rr_pgo_set_state round-trip theta through atan2 and cos, sin: both handles start from the round trip)
    got = [_call(g) for _ in range(REPEATS)]
    end = np.array(g.state())
    if solver == "GaussNewton" and name != "lattice":
        assert all(len(e) == 2 for e, _ in got), [len(e) for e, _ in got]   # one iteration + the final chi2
    slow = _host_loop(api, name, solver, monkeypatch)
    slow.set_state(s1)
    for r in range(REPEATS):
        want = _call(slow)
        assert _same(got[r], want), (name, solver, r, got[r], want)
    assert np.array_equal(end, np.array(slow.state()))
    fresh = _new(api, name, solver)
    fresh.set_state(s1)
    assert _same(got[0], _call(fresh))


@pytest.mark.parametrize("name", GRAPHS)
def test_entry_points_straight_behind_a_call(api, name):
    """get_state, set_state of another state + optimize, chi2, a covariance query and iterate_async, each issued straight
    behind optimize(10) with no sync in between, return what they return behind an explicit sync."""
    s0 = _start_state(api, name)
    other = _new(api, name)
    other.set_state(s0)
    other.optimize(2)
    s_other = np.array(other.state())
    pairs = ([0, 1, 2], [0, 5, other.num_nodes - 1])
    a, b = _new(api, name), _new(api, name)

    def behind(fn):
        out = []
        for g, sync in ((a, False), (b, True)):
            g.set_state(s0)
            if sync:
                g.sync()
            g.optimize(10)
            if sync:
                g.sync()
            out.append(fn(g))
        return out

    ra, rb = behind(lambda g: np.array(g.state()))
    assert np.array_equal(ra, rb)

    def restart_elsewhere(g):
        g.set_state(s_other)
        return _call(g) + (np.array(g.state()),)
    ra, rb = behind(restart_elsewhere)
    assert _same(ra, rb), (name, ra[0], rb[0])

    ra, rb = behind(lambda g: g.global_error())
    assert ra == rb

    if other.stats()["n_big_fronts"] == 0:
        ra, rb = behind(lambda g: g.covariance_blocks(*pairs))
        assert _same(ra, rb)
    else:   # rr_pgo_covariances refuses graphs with fronts beyond LDS: what it returns is that refusal, behind a call as behind a sync
        from rustrobotics_amd import PoseGraphError

        def refused(g):
            with pytest.raises(PoseGraphError) as ei:
                g.covariance_blocks(*pairs)
            return str(ei.value)
        ra, rb = behind(refused)
        assert ra == rb and "fronts beyond LDS" in ra

    def iterate(g):
        g.iterate_async(3)
        g.sync()
        return np.array(g.state())
    ra, rb = behind(iterate)
    assert np.array_equal(ra, rb)


def test_two_handles_alternating_calls_from_one_thread(api):
    """Two handles whose calls alternate on one host thread: each handle's tail drains while the other handle's call starts.
    Each gets what it gets alone."""
    names = ["intel", "simulation-pose-pose"]
    alone = {}
    for n in names:
        g = _new(api, n)
        g.set_state(_start_state(api, n))
        alone[n] = _call(g) + (np.array(g.state()),)
    hs = {n: _new(api, n) for n in names}
    for r in range(10):
        for n in names:
            hs[n].set_state(_start_state(api, n))
            got = _call(hs[n])
            assert _same(got, alone[n][:2]), (n, r)
    for n in names:
        assert np.array_equal(np.array(hs[n].state()), alone[n][2])


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", GRAPHS)
def test_caps_of_zero_one_and_two_equal_the_host_loop(api, name, solver, monkeypatch):
    """optimize(0), optimize(1) and a cap reached before the stop rule fires (optimize(2): no item is enqueued behind a
    stop, the call ends with the chi2 item) -- list lengths and bits of the loop with one host round trip per iteration."""
    s0 = _start_state(api, name)
    fast = _new(api, name, solver)
    slow = _host_loop(api, name, solver, monkeypatch)
    for iters in (0, 1, 2, 10, 2, 0):
        fast.set_state(s0)
        slow.set_state(s0)
        ef, es = _call(fast, iters), _call(slow, iters)
        assert len(ef[0]) == len(es[0]) and len(ef[1]) == len(es[1]), (name, solver, iters)
        assert _same(ef, es), (name, solver, iters, ef, es)
        assert np.array_equal(np.array(fast.state()), np.array(slow.state()))
    if name == "intel" and solver == "GaussNewton":
        fast.set_state(s0)
        assert len(_call(fast, 2)[0]) == 3   # two iterations + the final chi2: the cap, not the stop rule


@pytest.mark.parametrize("name", ["simulation-pose-landmark", "intel"])
def test_destruction_right_behind_a_call(api, name):
    """The handle is dropped straight behind a call, its tail still on the stream; the next handle (which is handed the
    pooled stream and device memory of the dropped one) runs and gives the same bits."""
    want = None
    for _ in range(6):
        g = _new(api, name)
        got = _call(g)
        del g
        gc.collect()
        if want is None:
            want = got
        assert _same(got, want)
