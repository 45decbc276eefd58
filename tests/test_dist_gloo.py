"""N > 1 path on CPU: two gloo ranks drive bench.py's measurement contract (barrier, exactly K
steps, max-over-ranks time, whole-job aggregate).  The data path has no collective: every rank
optimises its own replica ('Multi-GPU')."""
import os
import sys
import time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import bench
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []

    def run_steps(k):
        calls.append(k)
        time.sleep(0.002 * k * (1 + rank))      # rank 1 is the slow replica

    def all_max(x):
        t = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    resets = []
    dt = bench.timed_steps(run_steps, lambda: None, dist.barrier, all_max, steps=10, warmup=3,
                           reset=lambda: resets.append(1))
    q.put((rank, dt, calls, len(resets), bench.dist_env()))
    dist.barrier()
    dist.destroy_process_group()


def test_timed_steps_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (r0, dt0, calls0, resets0, env0), (r1, dt1, calls1, resets1, env1) = res
    assert calls0 == [3, 10] and calls1 == [3, 10]          # W untimed, then exactly K timed
    assert resets0 == resets1 == 1
    assert abs(dt0 - dt1) < 1e-9                            # both ranks report the MAX
    assert dt0 >= 0.002 * 10 * 2 * 0.9                      # ... which is the slow rank's time
    assert env0 == (0, 0, 2) and env1 == (1, 1, 2)
    # whole-job value = units of ALL ranks / max time
    assert (2 * 10) / dt0 < 2 * 10 / (0.002 * 10 * 2 * 0.9)


# ---- the sharded Gauss-Newton driver over 2 gloo ranks (fake shards: the numerics are the GPU tests'
# business; this covers the stage / all-gather / all-reduce protocol of rustrobotics_amd.sharding.gauss_newton
# with REAL torch.distributed collectives, world_size 2)

class _FakeShard:
    """A 'graph' whose chi2 is sum_i (target_i - x_i)^2 over 8 entries, 4 owned by each rank, with the protocol
    of include/rr_pgo.h: stage 0 publishes the owned residuals in the rank's chunk of buffer 0 (all-gathered),
    stage 1 needs the GATHERED buffer (its step is the mean residual of the other rank's chunk added to its own
    residuals -- nonsense numerically, but it makes a missing all-gather visible), applies the owned step and
    leaves the partial (chi2, |dx|^2) in buffer 1 (all-reduced); stage 2 leaves the partial chi2 only."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        self.x = torch.zeros(8, dtype=torch.float64)
        self.target = torch.arange(8, dtype=torch.float64)
        self.xch = torch.zeros(8, dtype=torch.float64)
        self.scal = torch.zeros(2, dtype=torch.float64)
        self.log, self.own = [], slice(4 * rank, 4 * rank + 4)
        self.other = slice(4 * (1 - rank), 4 * (1 - rank) + 4)

    def stage(self, k):
        self.log.append(("stage", k))
        if k == 0:
            self.xch.zero_()
            self.xch[self.own] = (self.target - self.x)[self.own]
        elif k == 1:
            self.seen_other = getattr(self, 'seen_other', []) + [float(self.xch[self.other].abs().sum())]   # non-zero only after the all-gather
            step = self.xch[self.own].clone()
            self.scal[0] = float((self.xch[self.own] ** 2).sum())
            self.scal[1] = float((step ** 2).sum())
            self.x[self.own] += step
        else:
            self.scal[0] = float(((self.target - self.x)[self.own] ** 2).sum())
            self.scal[1] = 0.0

    def sync(self):
        self.log.append(("sync",))

    def stage_scalars(self):
        return float(self.scal[0]), float(self.scal[1]) ** 0.5


class _GlooCollectives:
    def __init__(self, g):
        self.g, self.calls = g, []

    def all_gather_boundary(self):
        self.calls.append("all_gather")
        g = self.g
        parts = [torch.zeros(4, dtype=torch.float64) for _ in range(g.world)]
        dist.all_gather(parts, g.xch[g.own].clone())
        g.xch.copy_(torch.cat(parts))

    def all_reduce_scalars(self):
        self.calls.append("all_reduce")
        dist.all_reduce(self.g.scal, op=dist.ReduceOp.SUM)


def _sharded_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    from rustrobotics_amd.sharding import gauss_newton
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = _FakeShard(rank, world)
    coll = _GlooCollectives(g)
    errors, norms = gauss_newton([g], 5, coll)
    q.put((rank, errors, norms, coll.calls, g.log[:6], g.x.tolist(), g.seen_other))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_driver_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, e0, n0, c0, log0, x0, s0), (_, e1, n1, c1, log1, x1, s1) = res
    expected0 = float(sum(i * i for i in range(8)))
    assert e0 == e1 == [expected0, 0.0, 0.0]        # one full step solves it; the 2nd iteration sees |dx| = 0 and stops
    assert n0 == n1 and abs(n0[0] - expected0 ** 0.5) < 1e-12 and n0[1] == 0.0     # |dx| summed over BOTH ranks
    # per iteration: all-gather then all-reduce; one more all-reduce for the final chi2 (stage 2)
    assert c0 == c1 == ["all_gather", "all_reduce", "all_gather", "all_reduce", "all_reduce"]
    assert log0[:4] == [("stage", 0), ("stage", 1), ("stage", 0), ("stage", 1)]
    assert x0 == [0.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0] and x1 == [0.0, 0.0, 0.0, 0.0, 4.0, 5.0, 6.0, 7.0]   # owned parts only
    assert s0 == [22.0, 0.0] and s1 == [6.0, 0.0]   # stage 1 saw the OTHER rank's chunk: the all-gather ran before it


def test_optimize_steps_runs_exactly_k_iterations_through_optimize_calls():
    """bench.py's timed region is whole rr_pgo_optimize calls (optimize(10) from the initial state, again and again): whatever the
    stop rule does, EXACTLY K iterations run -- the last call asks for what is left -- and every call starts from the initial state."""
    sys.path.insert(0, ROOT)
    import bench

    class Stub:
        def __init__(self, stops_after):
            self.stops_after, self.calls, self.restarts = stops_after, [], 0

        def restarter(self, state):
            def restart():
                self.restarts += 1
            return restart

        def optimize_count(self, n):
            done = min(n, self.stops_after)
            self.calls.append((n, done))
            return done

    for stops_after, steps in ((6, 200), (6, 20), (7, 5), (100, 25), (1, 3)):
        g = Stub(stops_after)
        bench.optimize_steps(g, object(), steps)
        assert sum(d for _, d in g.calls) == steps, (stops_after, steps, g.calls)
        assert all(n <= bench.OPTIMIZE_CALL for n, _ in g.calls) and g.restarts == len(g.calls)
        left = steps
        for n, d in g.calls:   # every call asks for optimize(10), or for what is left of K
            assert n == min(left, bench.OPTIMIZE_CALL)
            left -= d


def test_dump_outputs_writes_the_last_calls_arrays_and_caps_the_size(tmp_path):
    """bench.py --dump-outputs: the state and the chi2 / |dx| lists of the last optimize() call, float64; above the size limit
    the long arrays become the same seeded sample in every run and the short ones stay whole."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench

    class Stub:
        _opt_buf = (np.array([9.0, 5.0, 4.0, 0.0]), np.array([3.0, 1.0, 0.0]), type("N", (), {"value": 3})())

        def state(self):
            return np.arange(6.0)

    bench.dump_outputs(str(tmp_path / "a"), bench.last_call_outputs(Stub()))
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("state", "errors", "norm_dx")}
    assert got["state"].tolist() == list(range(6)) and got["errors"].tolist() == [9, 5, 4] and got["norm_dx"].tolist() == [3, 1]
    assert all(a.dtype == np.float64 for a in got.values())

    big = {"state": np.arange(100000, dtype=np.float32), "errors": np.arange(7.0)}
    limit = 8 * 20000
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big, limit=limit)
    s_b, s_c = np.load(tmp_path / "b" / "state.npy"), np.load(tmp_path / "c" / "state.npy")
    assert s_b.dtype == np.float64 and np.array_equal(s_b, s_c) and np.all(np.diff(s_b) > 0)
    assert s_b.nbytes + 7 * 8 <= limit and len(s_b) > 19000
    assert np.load(tmp_path / "b" / "errors.npy").tolist() == list(range(7))
