"""Helpers of tests/test_launch_forms_gpu.py: the graphs, the launch forms a handle can be created under, and a wrapper that
checks after every call that the call reached the device in the form it claims (include/rr_pgo.h, rr_pgo_launch_counts).

An iteration reaches the device as plain launches, as a replay of the captured hipGraph, or as an item of rr_pgo_optimize's
device-side loop.  Which of them depends on the switches read when the handle is created and on its launches per iteration
(pgo_api.hip, optimize / iterate_async):

    rr_pgo_optimize       device-side loop   unless RR_PGO_SYNC_OPTIMIZE or >= 48 launches per iteration
                          host loop          Gauss-Newton: replays if RR_PGO_FORCE_GRAPH, or if > 8 launches per iteration (or a
                                             graph captured earlier) and not RR_PGO_NO_GRAPH; else plain launches.
                                             Levenberg-Marquardt: plain launches
    rr_pgo_iterate_async  replays if RR_PGO_FORCE_GRAPH (and not RR_PGO_NO_GRAPH), else plain launches
    rr_pgo_profile        plain launches
"""
import numpy as np

from random_graphs import random_graph, two_component_graph

COUNTERS = ("n_plain_iterations", "n_graph_replays", "n_loop_items", "n_graph_captures")
PLAIN, REPLAY, ITEM, CAPTURE = range(4)
HOST_LOOP_FROM = 48   # launches per iteration from which rr_pgo_optimize keeps the host loop

# the switches of a form, set around the creation of the handle only.  "ref": the host loop with plain launches -- one round
# trip per iteration, no stop word, no captured graph: nothing but the state is carried from one call to the next.
# (RR_PGO_SYNC_OPTIMIZE alone is not that: above 8 launches per iteration -- both lattices -- the Gauss-Newton host loop
# replays the captured graph unless RR_PGO_NO_GRAPH is set as well; on the small graphs the second switch changes nothing)
FORM_ENV = {
    "ref": {"RR_PGO_SYNC_OPTIMIZE": "1", "RR_PGO_NO_GRAPH": "1"},
    "a": {},
    "b": {"RR_PGO_FORCE_GRAPH": "1"},
    "c": {"RR_PGO_SYNC_OPTIMIZE": "1", "RR_PGO_FORCE_GRAPH": "1"},
    "d": {"RR_PGO_NO_GRAPH": "1"},
}
# "lattice-levels": one launch per step of the levels of fronts beyond LDS -- 101 launches per iteration on the 100 x 100
# lattice (MI355X), so that rr_pgo_optimize itself is the host loop with replays, as on the 1M-edge lattice
GRAPH_ENV = {"lattice-levels": {"RR_PGO_FLOW": "0"}}
LATTICE_SIDE = 100

_arrays = {}


def arrays_of(graph):
    if graph not in _arrays:
        if graph == "se2":      # 12 poses, 5 landmarks: odd-sized fronts
            _arrays[graph] = random_graph(np.random.default_rng(1701), 12, 5, 8)
        elif graph == "se3":
            _arrays[graph] = random_graph(np.random.default_rng(1702), 10, 0, 6, se3=True)
        elif graph == "two-component":   # the unanchored pair's last pivot is exactly 0.0 in the very first iteration
            _arrays[graph] = two_component_graph()
        else:
            from rustrobotics_amd import synthetic_grid_arrays
            _arrays["lattice"] = _arrays["lattice-levels"] = synthetic_grid_arrays(LATTICE_SIDE, LATTICE_SIDE)
    return _arrays[graph]


class Handle:
    """A PoseGraph created under the switches of `form`, whose optimize / iterate_async / profile check the launch counters
    around the call: the iterations went out in the form the switches and the launch count say, and in no other."""

    def __init__(self, api, graph, form, monkeypatch, precision="f64", solver="GaussNewton"):
        env = dict(GRAPH_ENV.get(graph, {}))
        env.update(FORM_ENV[form])
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            self.g = api[0].from_arrays(*arrays_of(graph), precision=precision, solver=getattr(api[1], solver))
        finally:
            for k in env:
                monkeypatch.delenv(k)
        self.graph, self.form = graph, form
        self.lm = solver == "LevenbergMarquardt"
        self.sync_optimize = "RR_PGO_SYNC_OPTIMIZE" in env
        self.no_graph = "RR_PGO_NO_GRAPH" in env
        self.force_graph = "RR_PGO_FORCE_GRAPH" in env and not self.no_graph
        st = self.g.stats()
        self.launches = st["n_launches_per_iter"]
        if graph == "lattice":          # fronts beyond LDS, still the device-side loop
            assert 8 < self.launches < HOST_LOOP_FROM and st["n_big_fronts"] > 0, self.launches
        if graph == "lattice-levels":   # rr_pgo_optimize is the host loop
            assert self.launches >= HOST_LOOP_FROM and st["n_big_fronts"] > 0, self.launches
        assert self.counts().tolist() == [0, 0, 0, 0]

    def counts(self):
        st = self.g.stats()
        return np.array([st[k] for k in COUNTERS], np.int64)

    def _grew(self, before, want, what):
        d = (self.counts() - before).tolist()
        assert d[:3] == want, (self.graph, self.form, what, d, want)
        total = self.counts()
        # one capture serves every replay of the handle's life, and no handle captures a graph it never replays
        assert total[CAPTURE] == (1 if total[REPLAY] > 0 else 0), (self.graph, self.form, what, total.tolist())

    # -- the calls that put iterations on the stream
    def optimize(self, iters):
        before = self.counts()
        errors, norms = self.g.optimize(iters, return_norms=True)
        ran = len(errors) - 1
        # (the three branches deliberately restate the engine's own choice -- pgo_api.hip, Engine::optimize: the device-side
        # loop below 48 launches, `eager` in the host loop -- so that EVERY call is checked; a change of that rule is edited
        # here in step.  What each form must show over a whole sequence is stated without it, in the tests themselves)
        if not self.sync_optimize and self.launches < HOST_LOOP_FROM:
            # the device-side loop: the iterations that ran and the chi2 item that ends the call, for Levenberg-Marquardt
            # also the item of the initial error -- at most one item was enqueued behind a stop
            d = (self.counts() - before).tolist()
            assert ran + 1 <= d[ITEM] <= ran + 2, (self.graph, self.form, iters, d, ran)
            self._grew(before, [0, 0, d[ITEM]], "optimize")
        elif self.lm or ((self.no_graph or self.launches <= 8) and before[CAPTURE] == 0 and not self.force_graph):
            self._grew(before, [ran, 0, 0], "optimize")
        else:
            self._grew(before, [0, ran, 0], "optimize")
        return np.array(errors), np.array(norms)

    def iterate(self, iters):
        """iterate_async(iters) + sync()"""
        before = self.counts()
        self.g.iterate_async(iters)
        self._grew(before, [0, iters, 0] if self.force_graph else [iters, 0, 0], "iterate_async")
        self.g.sync()

    def profile(self, iters):
        before = self.counts()
        self.g.profile(iters)
        self._grew(before, [iters, 0, 0], "profile")

    # -- everything else goes straight to the handle
    def state(self):
        return np.array(self.g.state())

    def __getattr__(self, name):
        if name == "g":   # (creation failed)
            raise AttributeError(name)
        return getattr(self.g, name)


def same(a, b):
    """two traces -- lists of (label, array or scalar) -- equal bit for bit; returns the first label that differs"""
    assert [k for k, _ in a] == [k for k, _ in b]
    for (k, x), (_, y) in zip(a, b):
        if not np.array_equal(np.asarray(x), np.asarray(y)):
            return k
    return None


# ---- the sequences: each takes a Handle and the start state, returns a trace -------------------------------------------

CAP = 50


def s1(h, s0):
    """replay behind a stop: the first iterate_async captures, optimize(50) ends by the stop rule (or at its cap), the three
    iterations behind it must run"""
    h.set_state(s0)
    h.iterate(1)
    h.set_state(s0)
    e, n = h.optimize(CAP)
    t = [("errors", e), ("norms", n), ("state after optimize", h.state())]
    h.set_state(s0)
    h.iterate(3)
    return t + [("state", h.state()), ("chi2", h.global_error())]


def s3(h, s0):
    """capture behind a stop: the graph is captured by the first iterate_async, which comes behind an optimize(50)"""
    h.set_state(s0)
    e, n = h.optimize(CAP)
    h.iterate(2)
    t = [("errors", e), ("norms", n), ("state after 2", h.state())]
    h.set_state(s0)
    h.optimize(CAP)
    h.set_state(s0)
    h.iterate(3)
    return t + [("state", h.state()), ("chi2", h.global_error())]


def s4(h, s0):
    """replay on the converged state, and entry points that linearise in a gauge of their own (chi2 only; the reference's
    system with lambda) or in the iteration's between two replays"""
    h.set_state(s0)
    e, n = h.optimize(CAP)
    h.iterate(2)
    t = [("errors", e), ("norms", n), ("state after 2", h.state())]
    h.iterate(1)
    t.append(("dx", h.linearize_and_solve()))
    t.append(("chi2 between", h.global_error()))
    t += [("assemble %d" % i, x) for i, x in enumerate(h.assemble(0.37, True))]
    h.iterate(1)
    return t + [("state", h.state()), ("chi2", h.global_error())]


def s7(h, s0):
    """entry points whose system is linearised, factored and updated in another gauge than the iteration's, between iterations:
    the Levenberg-Marquardt form of linearize_and_solve (the gauge transfer is off for that system alone), a caller's step under
    both signs (never the anchor gauge), the Gauss-Newton form.  Every sequence of launches is told its gauge by whoever enqueues
    it, so none of them may change what the next one computes."""
    h.set_state(s0)
    e, n = h.optimize(CAP)
    h.iterate(1)
    t = [("errors", e), ("norms", n), ("state after 1", h.state())]
    dx = h.linearize_and_solve(0.37, True)
    t.append(("dx lm", dx))
    h.update_nodes(dx, 1.0)
    t.append(("state +dx", h.state()))
    h.update_nodes(dx, -1.0)
    t.append(("state -dx", h.state()))
    t.append(("dx", h.linearize_and_solve()))
    h.iterate(1)
    return t + [("state", h.state()), ("chi2", h.global_error())]
