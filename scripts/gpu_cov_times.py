"""Times of rr_pgo_covariances on intel, M3500 and dlr, beside two yardsticks.

Per graph three queries -- the 576 ordered pairs of 24 seeded nodes, one pair, 400 seeded nodes paired at random -- each
called warm `--calls` times; the medians of the three HIP-event times of covariances_times() are printed.  Yardsticks: the
median selected-inverse time of marginals_times() on the same handle (all nodes), and the wall time of the CPU reference
(tests/marginals_reference.py, factorisations included) for the same query.

  python scripts/gpu_cov_times.py [--calls 25] [--no-reference]
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

from covariances_cases import far_pairs  # noqa: E402
from marginals_reference import MarginalsReference, graph_at_state  # noqa: E402
from rustrobotics_amd import PoseGraph  # noqa: E402


def median3(samples):
    return tuple(statistics.median(s[k] for s in samples) for k in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    for name in ("intel", "input_M3500_g2o", "dlr"):
        g = PoseGraph.new(os.path.join(ROOT, "tests", "golden", "g2o", name + ".g2o"))
        n = g.num_nodes
        _, fa, fb = far_pairs(n)
        rng = np.random.default_rng(5)
        many = rng.choice(n, 400, replace=False).astype(np.int32)
        queries = {"576 pairs of 24 nodes": (fa, fb), "one pair": (fa[1:2], fb[1:2]),
                   "400 nodes paired at random": (many, rng.permutation(many).astype(np.int32))}
        for _ in range(3):
            g.marginals()
        sel = median3([(g.marginals(), g.marginals_times())[1] for _ in range(a.calls)])
        print(f"{name}: {n} nodes; rr_pgo_marginals, all nodes: linearise + factor {sel[0]:.3f} ms, selected inverse {sel[1]:.3f} ms, "
              f"gather {sel[2]:.3f} ms (median of {a.calls})", flush=True)
        for label, (qa, qb) in queries.items():
            for _ in range(3):
                g.covariance_blocks(qa, qb)
            walls, samples = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                g.covariance_blocks(qa, qb)   # (a size query and the call)
                walls.append((time.perf_counter() - t0) * 1e3)
                samples.append(g.covariances_times())
            t = median3(samples)
            line = (f"{name}: {label}: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, products + gather {t[2]:.3f} ms, "
                    f"host wall of the call {statistics.median(walls):.3f} ms (median of {a.calls})")
            if not a.no_reference:
                t0 = time.perf_counter()
                MarginalsReference(graph_at_state(g.graph_arrays(), g.state())).blocks(qa, qb)
                line += f"; CPU reference {(time.perf_counter() - t0) * 1e3:.0f} ms"
            print(line, flush=True)


if __name__ == "__main__":
    main()
