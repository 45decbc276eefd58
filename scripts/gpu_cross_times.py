"""Times of rr_pgo_cross_covariances on intel, M3500, dlr and parking-garage, beside its yardstick.

Per graph two queries -- all rows x one column node, all rows x 24 seeded column nodes -- each called warm `--calls` times;
the medians of the three HIP-event times of cross_covariances_times() are printed with the host wall time of the call.
The yardstick is the same answer through the interface the parent already has: rr_pgo_covariances over the N pairs (j, a)
of one column node a, on the same handle (its linearise + factor interval is the same work).

  python scripts/gpu_cross_times.py [--calls 25]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from covariances_cases import far_nodes  # noqa: E402
from rustrobotics_amd import PoseGraph  # noqa: E402


def median3(samples):
    return tuple(statistics.median(s[k] for s in samples) for k in range(3))


def timed(calls, call, times):
    for _ in range(3):
        call()
    walls, samples = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        walls.append((time.perf_counter() - t0) * 1e3)
        samples.append(times())
    return median3(samples), statistics.median(walls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    a = ap.parse_args()
    for name in ("intel", "input_M3500_g2o", "dlr", "parking-garage"):
        g = PoseGraph.new(os.path.join(ROOT, "tests", "golden", "g2o", name + ".g2o"))
        n = g.num_nodes
        cols = far_nodes(n)
        s = g.stats()
        print(f"{name}: {n} nodes, dim {g.len}, {s['n_supernodes']} fronts", flush=True)
        for label, c in (("all rows x 1 column node", cols[:1]), ("all rows x 24 column nodes", cols)):
            t, wall = timed(a.calls, lambda: g.cross_covariance(None, c), g.cross_covariances_times)
            print(f"{name}: rr_pgo_cross_covariances, {label}: linearise + factor {t[0]:.3f} ms, forward + backward solve {t[1]:.3f} ms, "
                  f"gather + copy {t[2]:.3f} ms, host wall of the call {wall:.3f} ms (median of {a.calls})", flush=True)
        every, one = np.arange(n, dtype=np.int32), np.full(n, cols[0], np.int32)
        t, wall = timed(a.calls, lambda: g.covariance_blocks(every, one), g.covariances_times)
        print(f"{name}: rr_pgo_covariances, the {n} pairs (j, a) of that one column node: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, "
              f"products + gather {t[2]:.3f} ms, host wall of the call {wall:.3f} ms (median of {a.calls})", flush=True)


if __name__ == "__main__":
    main()
