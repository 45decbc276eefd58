"""Times of rr_pgo_extend on intel and parking-garage, beside its yardstick.

Per graph: 1, 8 and 64 appended loop closures between the 24 seeded nodes of tests/covariances_cases.far_nodes, and 16 appended
poses chained by odometry to the last pose in guess mode (no node_state).  Every sample starts from a fresh handle on the file's
graph after `--iterations` Gauss-Newton iterations with a Cauchy kernel set (none of that is timed); the first three samples
are warm-up, the medians of the next `--calls` are printed: the host wall time of the call (with its minimum and quartiles:
the host is shared, and a handle's construction is not equally fast every time) and the three intervals of extend_times() --
analysis, engine (host wall clock), state carry + guess (HIP events).  The two routes alternate sample by sample.

Yardstick, timed in the same way on such a handle: what a caller had to do without the call -- state() + graph_arrays() +
from_arrays on the grown graph + set_state + set_robust_kernel (in guess mode the initial values of the new poses are
composed on the host from the state read back, tests/extend_reference.py).

A structure that is analysed for the first time misses the analysis cache on both routes, and a growing graph never repeats
a structure: the samples run with RR_PGO_ANALYSIS_CACHE=0 unless --analysis-cache is given (then every sample after the
first finds the analysis of its grown graph, on both routes).

  python scripts/gpu_extend_times.py [--calls 25] [--iterations 5] [--analysis-cache]
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

import extend_reference  # noqa: E402
import gate_cases  # noqa: E402
from covariances_cases import far_nodes  # noqa: E402
from rustrobotics_amd import PoseGraph  # noqa: E402

WARMUP = 3


def closures(arrays, count):
    """`count` pose-pose edges over the seeded nodes; measurement: a small motion (the timing does not depend on it)"""
    nk, _, ek, _, _, _, ei = arrays
    kind = 2 if np.any(nk == 2) else 0
    poses = [v for v in far_nodes(len(nk)) if nk[v] != 1]
    pairs = [(a, b) for a in poses for b in poses if a != b]
    pairs = [pairs[(7 * c) % len(pairs)] for c in range(count)]
    w = gate_cases.split_packed(ek, ei, gate_cases.INFO_LEN)[int(np.flatnonzero(ek == kind)[0])]
    z = np.array(gate_cases.IDENTITY[kind], np.float64)
    z[0] = 0.5
    return dict(node_kind=None, edge_kind=np.full(count, kind, np.int32), edge_from=np.array([p[0] for p in pairs], np.int32),
                edge_to=np.array([p[1] for p in pairs], np.int32), edge_meas=np.tile(z, count), edge_info=np.tile(w, count))


def odometry(arrays, count):
    """`count` new poses chained to the last pose of the graph"""
    nk, _, ek, _, _, _, ei = arrays
    kind = 2 if np.any(nk == 2) else 0
    n = len(nk)
    last = int(np.flatnonzero(nk == kind)[-1])
    w = gate_cases.split_packed(ek, ei, gate_cases.INFO_LEN)[int(np.flatnonzero(ek == kind)[0])]
    z = np.array(gate_cases.IDENTITY[kind], np.float64)
    z[0] = 0.5
    chain = [last] + [n + i for i in range(count)]
    return dict(node_kind=np.full(count, kind, np.int32), edge_kind=np.full(count, kind, np.int32),
                edge_from=np.array(chain[:-1], np.int32), edge_to=np.array(chain[1:], np.int32),
                edge_meas=np.tile(z, count), edge_info=np.tile(w, count))


def prepared(arrays, iterations):
    g = PoseGraph.from_arrays(*arrays)
    g.set_robust_kernel("cauchy", 1.0)
    if iterations:
        g.optimize(iterations)
    g.sync()
    return g


def by_extend(g, add):
    t0 = time.perf_counter()
    g.extend(add["edge_kind"], add["edge_from"], add["edge_to"], add["edge_meas"], add["edge_info"], node_kind=add["node_kind"])
    return (time.perf_counter() - t0) * 1e3, g.extend_times()


def by_new_handle(g, add):
    t0 = time.perf_counter()
    state = g.state()
    nk, ns, ek, ef, et, em, ei = g.graph_arrays()
    if add["node_kind"] is not None:   # initial values of the new poses from the state read back
        new = extend_reference.guess(nk, state, add["node_kind"], add["edge_kind"], add["edge_from"], add["edge_to"], add["edge_meas"])
        state = np.concatenate([state] + new)
        ns = np.concatenate([ns] + new)
        nk = np.concatenate([nk, add["node_kind"]])
    h = PoseGraph.from_arrays(nk, ns, np.concatenate([ek, add["edge_kind"]]), np.concatenate([ef, add["edge_from"]]),
                              np.concatenate([et, add["edge_to"]]), np.concatenate([em, add["edge_meas"]]),
                              np.concatenate([ei, add["edge_info"]]))
    h.set_state(state)
    h.set_robust_kernel("cauchy", 1.0)
    h.sync()
    return (time.perf_counter() - t0) * 1e3, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--analysis-cache", action="store_true")
    args = ap.parse_args()
    if not args.analysis_cache:
        os.environ["RR_PGO_ANALYSIS_CACHE"] = "0"
    print(f"analysis cache {'on' if args.analysis_cache else 'off'}; median of {args.calls} after {WARMUP} warm-up samples", flush=True)
    for name in ("intel", "parking-garage"):
        arrays = PoseGraph.new(os.path.join(ROOT, "tests", "golden", "g2o", name + ".g2o")).graph_arrays()
        cases = [(f"{c} closures", closures(arrays, c)) for c in (1, 8, 64)] + [("16 poses by odometry, guessed", odometry(arrays, 16))]
        for label, add in cases:
            walls, parts, yard = [], [], []
            for k in range(WARMUP + args.calls):
                g = prepared(arrays, args.iterations)
                wall, t = by_extend(g, add)
                chi_ext = g.global_error()
                g2 = prepared(arrays, args.iterations)
                wall_y, h = by_new_handle(g2, add)
                chi_new = h.global_error()
                if k >= WARMUP:
                    walls.append(wall)
                    parts.append(t)
                    yard.append(wall_y)
            t = tuple(statistics.median(p[i] for p in parts) for i in range(3))
            spread = lambda v: f"{statistics.median(v):.3f} ms (min {min(v):.3f}, quartiles {np.percentile(v, 25):.3f} - {np.percentile(v, 75):.3f})"   # noqa: E731
            print(f"{name}: {label}: rr_pgo_extend {spread(walls)} host wall (analysis {t[0]:.3f} ms, engine {t[1]:.3f} ms, "
                  f"state carry + guess {t[2]:.3f} ms); new-handle route {spread(yard)} host wall; "
                  f"extend the faster one in {sum(a < b for a, b in zip(walls, yard))} of {len(walls)} pairs; "
                  f"chi2 after: {chi_ext:.9g} against {chi_new:.9g}", flush=True)


if __name__ == "__main__":
    main()
