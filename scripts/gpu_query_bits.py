"""Bits and times of the three queries over the factor -- rr_pgo_marginals, rr_pgo_covariances, rr_pgo_gate_edges
 -- for comparing two builds of the library.

Per graph (intel, simulation-pose-landmark and every other graph of GATE_GRAPHS and FAR_GRAPHS without fronts beyond LDS), at
the state tests/gate_cases.py gates at (the other graphs: the initial state), each call is made once -- marginal_blocks(),
covariance_blocks on the far pairs of tests/covariances_cases.py, gate_edges(..., return_innovation=True) on the candidates
of tests/gate_cases.py -- and one SHA-256 per output array is printed.  Then each call is repeated `--calls` times behind
three warm-up calls: the medians of the three HIP-event times of its *_times() and of the host wall time of the call are
printed with the smallest and the largest sample.  Two builds compute the same when every `sha256` line is equal; run the
script several times on each, alternating, to see a build's own run-to-run spread beside their difference.

  python scripts/gpu_query_bits.py [--calls 25] [--root <tree whose rustrobotics_amd and tests are used>]
"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def spread(samples):
    return f"{statistics.median(samples):.3f} [{min(samples):.3f} .. {max(samples):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from covariances_cases import FAR_GRAPHS, far_pairs
    from gate_cases import GATE_GRAPHS, candidates
    from rustrobotics_amd import PoseGraph

    names = ["intel", "simulation-pose-landmark"]
    for n in list(GATE_GRAPHS) + FAR_GRAPHS:
        if n not in names:
            names.append(n)
    for name in names:
        g = PoseGraph.new(os.path.join(root, "tests", "golden", "g2o", name + ".g2o"))
        if g.stats()["n_big_fronts"] > 0:
            print(f"{name}: fronts beyond LDS, left out", flush=True)
            continue
        if GATE_GRAPHS.get(name):
            g.optimize(GATE_GRAPHS[name])
        _, qa, qb = far_pairs(g.num_nodes)
        cand = candidates(g.graph_arrays(), g.state())
        calls = {
            "marginals": (lambda g=g: g.marginal_blocks(), g.marginals_times, ("values", "offsets")),
            "covariances": (lambda g=g, qa=qa, qb=qb: g.covariance_blocks(qa, qb), g.covariances_times, ("values", "offsets")),
            "gate": (lambda g=g, cand=cand: g.gate_edges(*cand, return_innovation=True), g.gate_times, ("d2", "chi2", "S")),
        }
        for what, (call, times, outs) in calls.items():
            for label, arr in zip(outs, call()):
                arr = np.concatenate([np.ravel(s) for s in arr]) if isinstance(arr, list) else arr
                print(f"sha256 {name} {what} {label} {sha(arr)}", flush=True)
        for what, (call, times, _) in calls.items():
            for _ in range(3):
                call()
            walls, samples = [], []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                call()
                walls.append((time.perf_counter() - t0) * 1e3)
                samples.append(times())
            print(f"times {name} {what}: " + ", ".join(f"interval {k} {spread([s[k] for s in samples])} ms" for k in range(3)) +
                  f", host wall of the call {spread(walls)} ms (median [min .. max] of {a.calls})", flush=True)


if __name__ == "__main__":
    main()
