"""Times of rr_pgo_marginals on trees with fronts beyond LDS (rr_pgo_set_marginals_big_fronts): sphere2500 and
torus3D after five Gauss-Newton iterations, and parking-garage (every front in LDS) as context.

Per graph two calls for the same answer, every node's diagonal block: rr_pgo_marginals (node_a == NULL), and
rr_pgo_covariances of the pairs (v, v) under rr_pgo_set_query_big_fronts -- the only way to those blocks without the
selected inverse of the fronts beyond LDS, hence the baseline.  Each warm, `--calls` times; the medians of the three
HIP-event times of the *_times are printed, the worst relative difference between the two answers, and whether the selected
inverse's interval is below the tree solve's.

  python scripts/gpu_marginals_big_times.py [--calls 20]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rustrobotics_amd import PoseGraph  # noqa: E402


def median3(samples):
    return tuple(statistics.median(s[k] for s in samples) for k in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    for name in ("sphere2500", "torus3D", "parking-garage"):
        g = PoseGraph.new(os.path.join(ROOT, "tests", "golden", "g2o", name + ".g2o"))
        g.query_big_fronts = True
        g.marginals_big_fronts = True
        g.optimize(5)
        s = g.stats()
        print(f"{name}: {g.num_nodes} nodes, {s['n_supernodes']} fronts, {s['n_big_fronts']} beyond LDS, max_front {s['max_front']}, "
              f"max_pivot_cols {s['max_pivot_cols']}", flush=True)
        every = np.arange(g.num_nodes, dtype=np.int32)
        calls = {"marginals, all nodes": (lambda: g.marginal_blocks(), g.marginals_times),
                 "covariances, all diagonal blocks": (lambda: g.covariance_blocks(every, every), g.covariances_times)}
        medians, values = {}, {}
        for label, (call, times) in calls.items():
            for _ in range(2):
                call()
            samples = []
            for _ in range(a.calls):
                values[label] = call()[0]
                samples.append(times())
            t = medians[label] = median3(samples)
            print(f"{name}: {label}: ms[3] = {t[0]:.3f} | {t[1]:.3f} | {t[2]:.3f} (median of {a.calls})", flush=True)
        m, c = values["marginals, all nodes"], values["covariances, all diagonal blocks"]
        sel, tree = medians["marginals, all nodes"][1], medians["covariances, all diagonal blocks"][1]
        print(f"{name}: worst difference between the two answers {np.max(np.abs(m - c)) / np.max(np.abs(c)):.3g} of the largest entry; "
              f"selected inverse {sel:.3f} ms, tree solve {tree:.3f} ms: {'below' if sel < tree else 'NOT below'} ({tree / sel:.1f}x)", flush=True)


if __name__ == "__main__":
    main()
