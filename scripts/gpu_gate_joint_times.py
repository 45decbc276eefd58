"""Times of rr_pgo_gate_joint on intel and parking-garage, beside its yardstick.

Per graph 1, 8 and 64 sets of 8 candidates over the 24 seeded nodes of tests/covariances_cases.far_nodes (the candidates of
scripts/gpu_gate_times.py, set s = candidates 8 s .. 8 s + 7), each called warm `--calls` times; the medians of the three
HIP-event times of gate_joint_times() and of the host wall time of the call are printed.
Yardstick on the same handle: the same sets through rr_pgo_covariances -- per set the lower block triangle of the joint
covariance of its distinct nodes, its HIP-event times -- plus the host arithmetic that turns the blocks into S_s, its
Cholesky factor and d2 (numpy; the Jacobians come from the oracle once and are not part of the time).

  python scripts/gpu_gate_joint_times.py [--calls 25]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gate_cases  # noqa: E402
from gpu_gate_times import candidates, median3  # noqa: E402
from rustrobotics_amd import PoseGraph  # noqa: E402

SET_SIZE = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    args = ap.parse_args()
    for name, iters in (("intel", 0), ("parking-garage", 10)):
        g = PoseGraph.new(os.path.join(ROOT, "tests", "golden", "g2o", name + ".g2o"))
        if iters:
            g.optimize(iters)
        arrays, state = g.graph_arrays(), g.state()
        node_dim = 6 if np.any(arrays[0] == 2) else 3
        for n_sets in (1, 8, 64):
            cand = candidates(arrays, state, SET_SIZE * n_sets)
            kinds, a, b, _, info = cand
            sets = [list(range(SET_SIZE * s, SET_SIZE * s + SET_SIZE)) for s in range(n_sets)]
            for _ in range(3):
                g.gate_joint(*cand, sets)
            walls, samples = [], []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                d2 = g.gate_joint(*cand, sets)
                walls.append((time.perf_counter() - t0) * 1e3)
                samples.append(g.gate_joint_times())
            t = median3(samples)
            print(f"{name}: {n_sets} sets of {SET_SIZE}: rr_pgo_gate_joint: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, "
                  f"joint kernel + copy {t[2]:.3f} ms, host wall of the call {statistics.median(walls):.3f} ms (median of {args.calls})", flush=True)
            # ---- the yardstick: the joint covariance of every set's nodes from one rr_pgo_covariances call, and the host arithmetic
            og = gate_cases.with_candidates(arrays, state, cand)
            lin = [og.linearize_edge(len(arrays[2]) + c) for c in range(len(kinds))]
            cov = np.linalg.inv(gate_cases.info_matrix(kinds[0], info[:gate_cases.INFO_LEN[int(kinds[0])]]))
            d = cov.shape[0]
            plans, qa, qb = [], [], []
            for members in sets:
                nodes = sorted(set(int(a[c]) for c in members) | set(int(b[c]) for c in members))
                at = {v: k for k, v in enumerate(nodes)}
                J = np.zeros((d * len(members), node_dim * len(nodes)))
                for k, c in enumerate(members):
                    J[d * k:d * k + d, node_dim * at[int(a[c])]:node_dim * at[int(a[c])] + node_dim] = lin[c][0]
                    J[d * k:d * k + d, node_dim * at[int(b[c])]:node_dim * at[int(b[c])] + node_dim] = lin[c][1]
                ia, ib = np.tril_indices(len(nodes))
                plans.append((J, np.concatenate([lin[c][2] for c in members]), len(nodes), ia, ib, len(qa)))
                qa += [nodes[i] for i in ia]
                qb += [nodes[j] for j in ib]
            qa, qb = np.array(qa, np.int32), np.array(qb, np.int32)
            omega_inv = np.kron(np.eye(SET_SIZE), cov)
            for _ in range(3):
                g.covariance_blocks(qa, qb)
            walls, samples, hosts = [], [], []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                vals, _ = g.covariance_blocks(qa, qb)
                t1 = time.perf_counter()
                blk = vals.reshape(-1, node_dim, node_dim)
                y = np.zeros(n_sets)
                for s, (J, e, k, ia, ib, q0) in enumerate(plans):
                    sig = np.zeros((k, k, node_dim, node_dim))
                    sig[ia, ib] = blk[q0:q0 + len(ia)]
                    sig[ib, ia] = blk[q0:q0 + len(ia)].transpose(0, 2, 1)
                    sig = sig.transpose(0, 2, 1, 3).reshape(k * node_dim, k * node_dim)
                    L = np.linalg.cholesky(omega_inv + J @ sig @ J.T)
                    x = np.linalg.solve(L, e)
                    y[s] = x @ x
                t2 = time.perf_counter()
                walls.append((t1 - t0) * 1e3)
                hosts.append((t2 - t1) * 1e3)
                samples.append(g.covariances_times())
            t = median3(samples)
            worst = float(np.max(np.abs(y - d2) / np.abs(d2)))
            print(f"{name}: {n_sets} sets of {SET_SIZE}: rr_pgo_covariances, {len(qa)} blocks: linearise + factor {t[0]:.3f} ms, tree solve {t[1]:.3f} ms, "
                  f"products + gather {t[2]:.3f} ms, host wall of the call {statistics.median(walls):.3f} ms, host arithmetic "
                  f"{statistics.median(hosts):.3f} ms; its d2 differs from the joint gate's by up to {worst:.3g} relative", flush=True)


if __name__ == "__main__":
    main()
