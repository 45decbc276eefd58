"""Every way an iteration reaches the device gives the same bits, and the launch counters prove which way it went.

DESIGN.md promises one answer from the device-side loop of rr_pgo_optimize, its host loop with plain launches, its host loop
with replays of the captured hipGraph (what rr_pgo_optimize IS on handles of >= 48 launches per iteration), and
rr_pgo_iterate_async with plain launches or with replays.  Here each of them is run through sequences in which a call
leaves something behind for the next one -- the stop word of a call that ended by the stop rule or by a failed
factorisation, a graph captured before or behind such a call, a system linearised in another gauge -- and compared, bit for bit,
with a handle on which nothing but the state is carried from call to call: the host loop with plain launches
(launch_forms.py, form "ref").  That handle itself is held against the CPU oracle once per graph.

Two handles that both did nothing would agree too, so every sequence also asserts progress (the state moved, chi2 fell), and
every call is checked against rr_pgo_launch_counts (launch_forms.Handle): a leg that silently runs another form fails.

The graphs are the smallest on which each form can go wrong: 17 and 10 nodes with odd-sized fronts, a four-node graph whose
factorisation fails on an exact zero pivot, the 100 x 100 lattice (fronts beyond LDS; 10 launches per iteration: the device-side
loop) and the same lattice with one launch per step of its big levels (RR_PGO_FLOW=0: 101 launches per iteration, the host loop
with replays -- the path of the 1M-edge lattice at a hundredth of its size)."""
import numpy as np
import pytest

import launch_forms as lf
from launch_forms import Handle

pytestmark = pytest.mark.gpu

PRECISIONS = ["f64", "mixed", "f32"]
CASES = ([("se2", p) for p in PRECISIONS] + [("se3", p) for p in PRECISIONS] +
         [("lattice", "f64"), ("lattice", "f32"), ("lattice-levels", "f64")])


def _forms(graph):
    return ["a", "b", "c"] + (["d"] if graph == "lattice-levels" else [])


CASE_FORMS = [pytest.param(g, p, f, id="%s-%s-%s" % (g, p, f)) for g, p in CASES for f in _forms(g)]
# Whether optimize(50) ends by the stop rule decides what a sequence tests: only such a call leaves the stop word set.  So every
# (graph, precision, solver) has an expectation, asserted on the reference handle's list (_reference): the call ends by the
# rule unless the key is in NEVER_STOPS -- a case that silently stopped meeting the rule would pass without testing the leak.
# len(errors) itself where the CPU oracle gives it (fp64, small graphs; both solvers: four iterations): Gauss-Newton's |dx| is
# 5.5e-6 (se2) and 1.9e-5 (se3) at the stop against 3.1e-4 and 7.7e-4 in the iteration before it -- room on both sides of 1e-4
STOPS_AT = {(g, "f64", s): 5 for g in ("se2", "se3") for s in ("GaussNewton", "LevenbergMarquardt")}
# ... and where the rule is not met within the cap: the fp32 lattice (test_gpu_parity.py,
# test_device_side_loop_on_a_graph_with_fronts_beyond_lds_on_the_level_schedule: |dx| stays at the rounding noise of the fp32
# gradient, some 1e-3 .. 1e-4 on 10 000 poses); the sequence still runs, the cap reached and the word never set
NEVER_STOPS = {("lattice", "f32", "GaussNewton"), ("lattice", "f32", "LevenbergMarquardt")}


@pytest.fixture(scope="module")
def api():
    import os
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rustrobotics_amd import PoseGraph, PoseGraphSolver, PoseGraphError, _lib
    assert os.path.exists(_lib.LIB_PATH), "HIP extension missing: the product path has no fallback"
    return PoseGraph, PoseGraphSolver, PoseGraphError


_start, _ref = {}, {}


def _s0(api, graph, precision, monkeypatch):
    """The initial state as rr_pgo_get_state hands it out (in fp32: rounded), once per graph and precision; every sequence
    starts with set_state(s0) on both handles."""
    key = (graph, precision)
    if key not in _start:
        s = Handle(api, graph, "ref", monkeypatch, precision).state()
        s.setflags(write=False)
        _start[key] = s
    return _start[key]


def _reference(api, seq, graph, precision, solver, monkeypatch):
    """The trace of `seq` on the reference handle, computed once and shared; it ran no replay and no loop item."""
    key = (seq.__name__, graph, precision, solver)
    if key not in _ref:
        h = Handle(api, graph, "ref", monkeypatch, precision, solver)
        trace = seq(h, _s0(api, graph, precision, monkeypatch))
        c = h.counts()
        assert c[lf.PLAIN] > 0 and c[lf.REPLAY] == 0 and c[lf.ITEM] == 0 and c[lf.CAPTURE] == 0
        errors = dict(trace)["errors"]
        print("reference", key, "len(errors)", len(errors), "last |dx|", dict(trace)["norms"][-1])
        case, last_dx = (graph, precision, solver), dict(trace)["norms"][-1]
        by_rule = last_dx < 1e-4   # (:298-300: the loop ends behind the first iteration that meets this, or at its cap)
        assert by_rule == (case not in NEVER_STOPS), (case, len(errors), last_dx)
        assert len(errors) == lf.CAP + 1 or by_rule, (case, len(errors), last_dx)
        if case in STOPS_AT:
            assert len(errors) == STOPS_AT[case], (case, len(errors))
        _ref[key] = trace
    return _ref[key]


def _run(api, seq, graph, precision, form, solver, monkeypatch):
    s0 = _s0(api, graph, precision, monkeypatch)
    want = _reference(api, seq, graph, precision, solver, monkeypatch)
    h = Handle(api, graph, form, monkeypatch, precision, solver)
    got = seq(h, s0)
    assert lf.same(got, want) is None, (seq.__name__, graph, precision, form, lf.same(got, want))
    got = dict(got)
    # progress: two handles that both did nothing would agree as well
    assert not np.array_equal(got["state"], s0)
    assert got["chi2"] < got["errors"][0] and got["errors"][-1] < got["errors"][0]
    # the form, over the whole sequence (every single call was checked by the Handle)
    c = h.counts()
    host_loop, lm = h.launches >= lf.HOST_LOOP_FROM, solver != "GaussNewton"   # (the Levenberg-Marquardt host loop: plain launches)
    if form == "a":
        assert c[lf.PLAIN] > 0 and (c[lf.ITEM] > 0) == (not host_loop)
        assert (c[lf.REPLAY] > 0) == (host_loop and not lm)
    elif form == "b":
        assert c[lf.REPLAY] > 0 and c[lf.CAPTURE] == 1 and (c[lf.PLAIN] > 0) == (host_loop and lm)
        assert (c[lf.ITEM] > 0) == (not host_loop)
    elif form == "c":
        assert c[lf.REPLAY] > 0 and c[lf.CAPTURE] == 1 and c[lf.ITEM] == 0 and (c[lf.PLAIN] > 0) == lm
    else:
        assert c[lf.PLAIN] > 0 and c[lf.REPLAY] == 0 and c[lf.CAPTURE] == 0 and c[lf.ITEM] == 0
    return got, h


@pytest.mark.parametrize("graph,precision,form", CASE_FORMS)
def test_replay_behind_a_call_that_ended_by_the_stop_rule(api, graph, precision, form, monkeypatch):
    """S1: iterate_async(1) (under RR_PGO_FORCE_GRAPH this captures the graph), optimize(50) from the start state, then
    iterate_async(3) from the start state.  A device-side loop that ends by the stop rule leaves its stop word set; the
    three iterations behind it must run whether they are plain launches (which clear it in launch_linearize) or replays of
    a graph that was captured before the word was ever set (which holds no memset)."""
    _run(api, lf.s1, graph, precision, form, "GaussNewton", monkeypatch)


@pytest.mark.parametrize("graph,precision,form", CASE_FORMS)
def test_replay_behind_a_levenberg_marquardt_call(api, graph, precision, form, monkeypatch):
    """S2: the same on a Levenberg-Marquardt handle -- the call that sets the word drives other launches than the
    captured Gauss-Newton iteration (rr_pgo_iterate_async is Gauss-Newton either way)."""
    _run(api, lf.s1, graph, precision, form, "LevenbergMarquardt", monkeypatch)


@pytest.mark.parametrize("graph,precision,form", CASE_FORMS)
def test_graph_captured_behind_a_stop_is_the_graph_captured_before_it(api, graph, precision, form, monkeypatch):
    """S3: optimize(50) first, the capture behind it; then S1's tail.  The captured graph must not depend on what ran before
    its capture: one capture serves both replays, and the tail gives S1's bits."""
    got, h = _run(api, lf.s3, graph, precision, form, "GaussNewton", monkeypatch)
    tail = dict(_reference(api, lf.s1, graph, precision, "GaussNewton", monkeypatch))
    assert np.array_equal(got["state"], tail["state"]) and got["chi2"] == tail["chi2"]
    assert np.array_equal(got["errors"], tail["errors"]) and np.array_equal(got["norms"], tail["norms"])


@pytest.mark.parametrize("graph,precision,form", CASE_FORMS)
def test_replays_on_the_converged_state_around_other_entry_points(api, graph, precision, form, monkeypatch):
    """S4: optimize(50) and iterate_async(2) with no restart in between, then linearize_and_solve(), global_error() and
    assemble(0.37, True) -- each linearises in a gauge of its own, handed to its launches and to no other -- between two further
    iterate_async(1).  A replay holds its own arguments and must not care."""
    _run(api, lf.s4, graph, precision, form, "GaussNewton", monkeypatch)


# S7: both single-precision cases (the gauge transfer exists only with a single-precision factor; of these only the lattice
# has the big root front that takes it: test_the_f32_lattice_exercises_the_gauge_transfer), and the two forms of fp64 handle
S7_CASES = [("se2", "f64"), ("se2", "f32"), ("lattice", "f32"), ("lattice-levels", "f64")]


@pytest.mark.parametrize("solver", ["GaussNewton", "LevenbergMarquardt"])
@pytest.mark.parametrize("graph,precision,form", [pytest.param(g, p, f, id="%s-%s-%s" % (g, p, f)) for g, p in S7_CASES for f in _forms(g)])
def test_systems_in_another_gauge_between_iterations(api, graph, precision, form, solver, monkeypatch):
    """S7: optimize(50), iterate_async(1), then linearize_and_solve(0.37, True) -- the Levenberg-Marquardt form: no gauge
    transfer for this system, in its linearisation, its factorisation and its update alike -- update_nodes(dx, 1.0) and
    update_nodes(dx, -1.0) -- a caller's step never gets the anchor gauge -- linearize_and_solve() and iterate_async(1): both
    dx, the state after each update, the final state and chi2, under both solvers."""
    _run(api, lf.s7, graph, precision, form, solver, monkeypatch)


def test_the_f32_lattice_exercises_the_gauge_transfer(api, monkeypatch):
    """The precondition of the ("lattice", "f32") cases: on this lattice the gauge transfer is really on -- the first
    linearize_and_solve() of a handle created under RR_PGO_GAUGE=0 (anchor prior, no gauge term, no anchor gauge in the update)
    differs from the default handle's in at least one bit.  Both are steps of the same system: they agree to single precision."""
    default = Handle(api, "lattice", "ref", monkeypatch, "f32")
    monkeypatch.setenv("RR_PGO_GAUGE", "0")
    try:
        off = Handle(api, "lattice", "ref", monkeypatch, "f32")
    finally:
        monkeypatch.delenv("RR_PGO_GAUGE")
    a, b = default.linearize_and_solve(), off.linearize_and_solve()
    print("gauge on / off: first step differs in", int((a != b).sum()), "of", a.size, "entries, max", np.abs(a - b).max(), "of", np.abs(a).max())
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.abs(a).max() > 0
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_stage_one_follows_stage_zero_as_replays_and_as_plain_launches(api, precision, monkeypatch):
    """The two stages of a sharded handle (one rank, the 100 x 100 lattice), as replays of their captured graphs (default) and
    as plain launches (RR_PGO_NO_GRAPH=1): two Gauss-Newton pairs stage(0), stage(1); one pair stage(0, 0.37, True), stage(1)
    -- stage 1 left at its default lm: it factors the top fronts and updates in the gauge stage 0 linearised in, not in the
    one its captured graph holds; one more Gauss-Newton pair.  The scalars after every pair and the final state are equal bit
    for bit, and chi2 fell."""
    arrays = lf.arrays_of("lattice")

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            g = api[0].from_arrays(*arrays, precision=precision, sharded=True)
        finally:
            for k in env:
                monkeypatch.delenv(k)
        g.stage(2)
        t = [("chi2 before", g.stage_scalars()[0])]
        for i, first in enumerate([(0,), (0,), (0, 0.37, True), (0,)]):
            g.stage(*first)
            g.stage(1)
            t.append(("scalars %d" % i, np.array(g.stage_scalars())))
        g.stage(2)
        return t + [("state", np.array(g.state())), ("chi2", g.stage_scalars()[0])]

    replays, plain = run({}), run({"RR_PGO_NO_GRAPH": "1"})
    assert lf.same(replays, plain) is None, (precision, lf.same(replays, plain))
    got = dict(replays)
    print(precision, [(k, v) for k, v in replays if k != "state"])
    assert np.all(np.isfinite(got["state"])) and got["scalars 3"][0] < got["chi2 before"] and got["chi2"] < got["chi2 before"]


@pytest.mark.parametrize("form", ["a", "b"])
def test_replay_behind_a_failed_call_reports_the_failure_again(api, form, monkeypatch):
    """S5: a graph whose factorisation fails on an exact zero pivot.  iterate_async(1) + sync() reports RR_PGO_ENOTSPD,
    optimize(5) reports it (and ends its device-side loop through the stop word), and the iteration behind that call must
    run and report it again -- not return at the stop word and answer OK.  The state is untouched throughout."""
    PoseGraphError = api[2]
    h = Handle(api, "two-component", form, monkeypatch)
    s0 = h.state()

    def fails(call):
        with pytest.raises(PoseGraphError) as err:
            call()
        assert err.value.code == -5
        assert np.array_equal(h.state(), s0)

    def iterate():
        h.g.iterate_async(1)
        h.g.sync()

    fails(iterate)
    fails(lambda: h.g.optimize(5))
    fails(iterate)
    assert np.isfinite(h.global_error())
    plain, replays, items, captures = h.counts().tolist()
    assert items > 0
    assert (plain, replays, captures) == ((0, 2, 1) if form == "b" else (2, 0, 0))


@pytest.mark.parametrize("graph,precision", CASES)
def test_forms_without_a_stop_give_the_reference_bits(api, graph, precision, monkeypatch):
    """S6: k iterations below the stop (2 on the random graphs, 3 on the lattices) from the start state -- optimize(k) on the
    device-side loop (or, from 48 launches per iteration, the host loop with replays) and on the host loop with replays,
    iterate_async(k) as plain launches and as replays, profile(k): the same launches with the same arguments, so the state
    and chi2 of the reference's optimize(k), bit for bit."""
    k = 3 if graph.startswith("lattice") else 2
    s0 = _s0(api, graph, precision, monkeypatch)
    ref = Handle(api, graph, "ref", monkeypatch, precision)
    ref.set_state(s0)
    chi0 = ref.global_error()
    e, _ = ref.optimize(k)
    assert len(e) == k + 1   # the cap, not the stop rule
    want = (ref.state(), ref.global_error())
    assert not np.array_equal(want[0], s0) and want[1] < chi0 and e[0] == chi0 and e[-1] == want[1]
    runs = [("ref", "iterate"), ("a", "optimize"), ("c", "optimize"), ("a", "iterate"), ("b", "iterate")]
    if graph in ("se2", "lattice"):
        runs.append(("a", "profile"))
    if graph == "lattice-levels":
        runs += [("d", "optimize"), ("d", "iterate")]
    handles = {"ref": ref}
    for form, call in runs:
        if form not in handles:
            handles[form] = Handle(api, graph, form, monkeypatch, precision)
        h = handles[form]
        h.set_state(s0)
        if call == "optimize":
            eh, _ = h.optimize(k)
            assert np.array_equal(eh, e), (form, call, eh, e)
        else:
            getattr(h, call)(k)
        assert np.array_equal(h.state(), want[0]), (form, call)
        assert h.global_error() == want[1], (form, call)
    if graph == "lattice-levels":   # rr_pgo_optimize of this handle IS the host loop with replays; the switch gives plain launches
        assert handles["a"].counts().tolist() == [k, k, 0, 1]
        assert handles["d"].counts().tolist() == [2 * k, 0, 0, 0]
    else:
        ca = handles["a"].counts()
        assert ca[lf.REPLAY] == 0 and ca[lf.ITEM] == k + 1 and ca[lf.PLAIN] == (2 * k if graph in ("se2", "lattice") else k)
    assert handles["b"].counts().tolist() == [0, k, 0, 1]
    assert handles["c"].counts().tolist() == [0, k, 0, 1]


@pytest.mark.parametrize("graph", ["se2", "se3"])
def test_the_reference_handle_matches_the_cpu_oracle(api, graph, monkeypatch):
    """The handle everything above is compared with, against the CPU oracle, at the tolerances test_gpu_parity.py holds
    these random graphs to (test_random_ragged_graphs_match_the_oracle: first step 1e-8, chi2 trajectory rtol 1e-8, poses
    1e-7; test_random_se3_graphs_match_the_oracle: first step 1e-7, chi2 trajectory rtol 1e-7, poses not compared).  Mixed
    precision: the final chi2 to 1e-10 relative, the criterion of test_mixed_precision_reaches_the_f64_answer."""
    from oracle.oracle import OracleGraph
    arrays = lf.arrays_of(graph)
    tol, iters = (1e-8, 5) if graph == "se2" else (1e-7, 4)
    g, o = Handle(api, graph, "ref", monkeypatch), OracleGraph.from_arrays(*arrays)
    dx, odx = g.linearize_and_solve(), o.linearize_and_solve()
    print(graph, "first step", np.abs(dx - odx).max(), "of", np.abs(odx).max())
    assert np.abs(dx - odx).max() <= tol * max(1.0, np.abs(odx).max())
    eg, eo = g.optimize(iters)[0], o.optimize(iters)
    print(graph, "chi2", eg, eo)
    np.testing.assert_allclose(eg, eo, rtol=tol)
    if graph == "se2":
        print(graph, "poses", np.abs(g.state() - o.state()).max())
        assert np.abs(g.state() - o.state()).max() <= 1e-7
    gm, om = Handle(api, graph, "ref", monkeypatch, "mixed"), OracleGraph.from_arrays(*arrays)
    em, eo = gm.optimize(lf.CAP)[0], om.optimize(lf.CAP)
    print(graph, "mixed final chi2", em[-1], eo[-1], "iterations", len(em) - 1, len(eo) - 1)
    assert len(em) - 1 < lf.CAP   # converged by the stop rule
    assert abs(em[-1] - eo[-1]) <= 1e-10 * eo[-1]
