"""Times of rr_pgo_check_edges beside rr_pgo_marginals on the same handle.

Three queries -- every edge of intel, its non-consecutive edges only, 64 seeded edges of parking-garage -- each called warm
`--calls` times; the medians of the three HIP-event times of check_edges_times() and of the host wall time are printed, and
the median selected-inverse times of marginals_times() (all nodes) as the yardstick.

  python scripts/gpu_check_times.py [--calls 25]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rustrobotics_amd import PoseGraph  # noqa: E402


def median3(samples):
    return tuple(statistics.median(s[k] for s in samples) for k in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    a = ap.parse_args()
    for name in ("intel", "parking-garage"):
        g = PoseGraph.new(os.path.join(ROOT, "tests", "golden", "g2o", name + ".g2o"))
        ef, et = g.graph_arrays()[3:5]
        far = np.flatnonzero(np.abs(ef.astype(np.int64) - et) > 1).astype(np.int32)
        if name == "intel":
            queries = {"all edges": None, "non-consecutive edges": far}
        else:
            queries = {"64 seeded edges": np.random.default_rng(5).choice(g.num_edges, 64, replace=False).astype(np.int32)}
        for _ in range(3):
            g.marginals()
        sel = median3([(g.marginals(), g.marginals_times())[1] for _ in range(a.calls)])
        print(f"{name}: {g.num_nodes} nodes, {g.num_edges} edges; rr_pgo_marginals, all nodes: linearise + factor {sel[0]:.3f} ms, "
              f"selected inverse {sel[1]:.3f} ms, gather {sel[2]:.3f} ms (median of {a.calls})", flush=True)
        for label, edges in queries.items():
            for _ in range(3):
                g.check_edges(edges)
            walls, samples = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                g.check_edges(edges)
                walls.append((time.perf_counter() - t0) * 1e3)
                samples.append(g.check_edges_times())
            t = median3(samples)
            n = g.num_edges if edges is None else len(edges)
            print(f"{name}: {label} ({n}): linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, kernel + copy {t[2]:.3f} ms, "
                  f"host wall of the call {statistics.median(walls):.3f} ms (median of {a.calls})", flush=True)


if __name__ == "__main__":
    main()
