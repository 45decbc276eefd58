"""Cost of the priors in the linearisation: RR_PGO_K_LINEARIZE of rr_pgo_profile on intel.g2o and on the
1M-edge lattice, f64, in three configurations -- no priors, 40 priors, a prior on every node.

Every handle is optimised first (ten Gauss-Newton iterations: the profiled iterations then run at the optimum, where every
call does the same work), the priors sit at the nodes' states (Omega = diag(100, 100, 1)), three profiled calls warm up and
the median of the next `--calls` one-iteration calls is printed with the quartiles, in microseconds per k_linearize launch.
A library without rr_pgo_set_priors (the parent commit) prints its no-priors figure alone: run the script in both trees, in
one session, for the figure beside them.

  python scripts/gpu_prior_costs.py [--calls 25] [--lattice 400x250:1000000]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rustrobotics_amd import PoseGraph  # noqa: E402

WARMUP = 3


def linearize_us(g, calls):
    out = []
    for i in range(WARMUP + calls):
        ms, n = g.profile(1)["linearize"]
        if i >= WARMUP:
            out.append(1e3 * ms / n)
    q = statistics.quantiles(out, n=4)
    return statistics.median(out), q[0], q[2]


def priors_at_state(g, nodes):
    assert g.len == 3 * g.num_nodes    # an SE(2) graph without landmarks: three scalars per node
    st = g.state().reshape(-1, 3)
    return nodes.astype(np.int32), st[nodes].ravel(), np.tile([100.0, 0.0, 0.0, 100.0, 0.0, 1.0], len(nodes))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--lattice", default="400x250:1000000")
    a = ap.parse_args()
    wh, edges = a.lattice.split(":")
    w, h = (int(t) for t in wh.split("x"))
    graphs = [("intel", lambda: PoseGraph.new(os.path.join(ROOT, "tests", "golden", "g2o", "intel.g2o"))),
              (f"lattice {w}x{h}, {edges} edges", lambda: PoseGraph.synthetic_grid(w, h, int(edges)))]
    has_priors = hasattr(PoseGraph, "set_priors")
    for name, make in graphs:
        g = make()
        g.optimize(10)
        n = g.num_nodes
        configs = [("no priors", None)]
        if has_priors:
            rng = np.random.default_rng(45)
            configs += [("40 priors", np.sort(rng.choice(n, 40, replace=False))), ("a prior on every node", np.arange(n))]
        for label, nodes in configs:
            if nodes is not None:
                g.set_priors(*priors_at_state(g, nodes))
            med, q1, q3 = linearize_us(g, a.calls)
            bytes_lin = g.stats()["bytes_linearize"]
            print(f"{name}: {label}: k_linearize median {med:.2f} us (quartiles {q1:.2f} .. {q3:.2f}) over {a.calls} calls, "
                  f"bytes_linearize {bytes_lin:.0f}", flush=True)


if __name__ == "__main__":
    main()
