"""Launch-bound overhead of graphs with bearing-only / range-only edges: optimize(10) per iteration on the
`beacons` and `corridor` fixtures of tests/bearing_range_cases.py, in f64 / mixed / f32.

Each sample restarts the handle from the initial state (rr_pgo_set_state) and times ONE optimize(10) call with the host clock;
the call ends in a synchronise.  Printed: the iterations the call executed, the median and the spread (min - max) of the time
per iteration over `--calls` samples after `--warm` unrecorded ones.  No earlier code runs these graphs: the figures are
overheads of a launch-bound size, not a comparison.

  python scripts/gpu_bearing_range_times.py [--calls 200] [--warm 20]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bearing_range_cases import case  # noqa: E402
from rustrobotics_amd import PoseGraph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    a = ap.parse_args()
    for name in ("beacons", "corridor"):
        arrays = case(name)
        for precision in ("f64", "mixed", "f32"):
            g = PoseGraph.from_arrays(*arrays, precision=precision)
            restart = g.restarter(g.state())
            per_it, iters = [], 0
            for k in range(a.warm + a.calls):
                restart()
                t0 = time.perf_counter()
                iters = g.optimize_count(10)
                dt = time.perf_counter() - t0
                if k >= a.warm:
                    per_it.append(dt * 1e6 / iters)
            st = g.stats()
            print(f"{name} {precision}: {g.len} unknowns, {g.num_edges} edges, {st['n_launches_per_iter']} launches per iteration, "
                  f"{iters} iterations per call: {statistics.median(per_it):.1f} us per iteration "
                  f"(min {min(per_it):.1f}, max {max(per_it):.1f}; median of {a.calls})", flush=True)


if __name__ == "__main__":
    main()
