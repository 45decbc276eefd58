"""Times of the factor queries on trees with fronts beyond LDS (rr_pgo_set_query_big_fronts): sphere2500 and
torus3D, and parking-garage (every front in LDS) as context.

Per graph four calls -- rr_pgo_covariances of one pair and of the 576 ordered pairs of 24 seeded nodes, rr_pgo_gate_edges of
the candidates of tests/gate_cases.py (64 on these graphs), rr_pgo_cross_covariances of one full column (row_node == NULL,
one column node) -- each warm, `--calls` times; the medians of the three HIP-event times of the *_times are printed, and
the launches of the tree solve as the plan trace (RR_PGO_QUERY_TRACE=1) counts them.

  python scripts/gpu_big_front_times.py [--calls 20]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from covariances_cases import far_pairs  # noqa: E402
from gate_cases import candidates  # noqa: E402
from rustrobotics_amd import PoseGraph  # noqa: E402


def median3(samples):
    return tuple(statistics.median(s[k] for s in samples) for k in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    os.environ["RR_PGO_QUERY_TRACE"] = "1"   # read when a handle is created: the plan of every pass on stderr
    for name in ("sphere2500", "torus3D", "parking-garage"):
        g = PoseGraph.new(os.path.join(ROOT, "tests", "golden", "g2o", name + ".g2o"))
        g.query_big_fronts = True
        s = g.stats()
        print(f"{name}: {g.num_nodes} nodes, {s['n_supernodes']} fronts, {s['n_big_fronts']} beyond LDS, max_front {s['max_front']}, "
              f"max_pivot_cols {s['max_pivot_cols']}", flush=True)
        _, fa, fb = far_pairs(g.num_nodes)
        cand = candidates(g.graph_arrays(), g.state())
        calls = {"covariances, one pair": (lambda: g.covariance_blocks(fa[1:2], fb[1:2]), g.covariances_times),
                 "covariances, 576 pairs of 24 nodes": (lambda: g.covariance_blocks(fa, fb), g.covariances_times),
                 f"gate_edges, {len(cand[0])} candidates": (lambda: g.gate_edges(*cand), g.gate_times),
                 "cross_covariances, one full column": (lambda: g.cross_covariance(None, fa[1:2]), g.cross_covariances_times)}
        for label, (call, times) in calls.items():
            print(f"-- {name}: {label}", file=sys.stderr, flush=True)
            call()
            print("-- end of the traced call", file=sys.stderr, flush=True)
            for _ in range(2):
                call()
            samples = []
            for _ in range(a.calls):
                call()
                samples.append(times())
            t = median3(samples)
            print(f"{name}: {label}: ms[3] = {t[0]:.3f} | {t[1]:.3f} | {t[2]:.3f} (median of {a.calls})", flush=True)


if __name__ == "__main__":
    main()
