"""Times of rr_pgo_gate_edges on intel and parking-garage, beside its yardstick.

Per graph 1, 64 and 1024 candidates over the 24 seeded nodes of tests/covariances_cases.far_nodes (ordered pairs a != b, taken
round and round; the measurement is the relative pose at the state displaced as in tests/gate_cases.py), each called warm
`--calls` times; the medians of the three HIP-event times of gate_times() and of the host wall time of the call are printed.
Yardstick on the same handle: the same candidates through rr_pgo_covariances -- four blocks each (aa, ab, ba, bb), its
HIP-event times -- plus the host arithmetic that turns the blocks into d2 (numpy; the Jacobians come from the oracle once
and are not part of the time).

  python scripts/gpu_gate_times.py [--calls 25]
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

import gate_cases  # noqa: E402
from covariances_cases import far_nodes  # noqa: E402
from rustrobotics_amd import PoseGraph  # noqa: E402


def median3(samples):
    return tuple(statistics.median(s[k] for s in samples) for k in range(3))


def candidates(arrays, state, count):
    """`count` pose-pose candidates over the seeded nodes, built like tests/gate_cases.candidates"""
    nk, _, ek, ef, et, em, ei = arrays
    kind = 2 if np.any(nk == 2) else 0
    poses = [v for v in far_nodes(len(nk)) if nk[v] != 1]
    pairs = [(a, b) for a in poses for b in poses if a != b]
    pairs = [pairs[(7 * c) % len(pairs)] for c in range(count)]
    kinds = np.full(count, kind, np.int32)
    a = np.array([p[0] for p in pairs], np.int32)
    b = np.array([p[1] for p in pairs], np.int32)
    w = gate_cases.split_packed(ek, ei, gate_cases.INFO_LEN)[int(np.flatnonzero(ek == kind)[0])]
    info = np.tile(w, count)
    og = gate_cases.with_candidates(arrays, state, (kinds, a, b, np.tile(gate_cases.IDENTITY[kind], count), info))
    rng = np.random.default_rng(gate_cases.SEED)
    sigma = 1.0 / np.sqrt(np.diag(gate_cases.info_matrix(kind, w)))
    meas = []
    for c in range(count):
        z = og.linearize_edge(len(ek) + c)[2] + gate_cases.LADDER[c % 4] * sigma * rng.standard_normal(len(sigma))
        if kind == 2:
            z[3:6] *= min(1.0, gate_cases.QV_MAX / np.linalg.norm(z[3:6]))
            z = np.concatenate([z, [np.sqrt(1.0 - z[3:6] @ z[3:6])]])
        meas.append(z)
    return kinds, a, b, np.concatenate(meas), info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    args = ap.parse_args()
    for name, iters in (("intel", 0), ("parking-garage", 10)):
        g = PoseGraph.new(os.path.join(ROOT, "tests", "golden", "g2o", name + ".g2o"))
        if iters:
            g.optimize(iters)
        arrays, state = g.graph_arrays(), g.state()
        for count in (1, 64, 1024):
            cand = candidates(arrays, state, count)
            kinds, a, b, _, info = cand
            for _ in range(3):
                g.gate_edges(*cand)
            walls, samples = [], []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                d2, _ = g.gate_edges(*cand)
                walls.append((time.perf_counter() - t0) * 1e3)
                samples.append(g.gate_times())
            t = median3(samples)
            print(f"{name}: {count} candidates: rr_pgo_gate_edges: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, "
                  f"gate kernel + copy {t[2]:.3f} ms, host wall of the call {statistics.median(walls):.3f} ms (median of {args.calls})", flush=True)
            # ---- the yardstick: four covariance blocks per candidate and the arithmetic on the host
            og = gate_cases.with_candidates(arrays, state, cand)
            lin = [og.linearize_edge(len(arrays[2]) + c) for c in range(count)]
            A, B, E = (np.stack([x[k] for x in lin]) for k in range(3))
            d = A.shape[1]
            cov = np.linalg.inv(gate_cases.info_matrix(kinds[0], info[:gate_cases.INFO_LEN[int(kinds[0])]]))
            qa, qb = np.concatenate([a, a, b, b]), np.concatenate([a, b, a, b])
            for _ in range(3):
                g.covariance_blocks(qa, qb)
            walls, samples, hosts = [], [], []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                vals, _ = g.covariance_blocks(qa, qb)
                t1 = time.perf_counter()
                blk = vals.reshape(4, count, d, d)
                S = (cov + A @ blk[0] @ A.transpose(0, 2, 1) + A @ blk[1] @ B.transpose(0, 2, 1) + B @ blk[2] @ A.transpose(0, 2, 1)
                     + B @ blk[3] @ B.transpose(0, 2, 1))
                y = np.einsum("ci,ci->c", E, np.linalg.solve(S, E[:, :, None])[:, :, 0])
                t2 = time.perf_counter()
                walls.append((t1 - t0) * 1e3)
                hosts.append((t2 - t1) * 1e3)
                samples.append(g.covariances_times())
            t = median3(samples)
            worst = float(np.max(np.abs(y - d2) / np.abs(d2)))
            print(f"{name}: {count} candidates: rr_pgo_covariances, 4 blocks each: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, "
                  f"products + gather {t[2]:.3f} ms, host wall of the call {statistics.median(walls):.3f} ms, host arithmetic "
                  f"{statistics.median(hosts):.3f} ms; its d2 differs from the gate's by up to {worst:.3g} relative", flush=True)


if __name__ == "__main__":
    main()
