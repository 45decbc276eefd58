"""Bits of everything the linearisation and update kernels reach, for comparing two builds of the library (the library is
selected as scripts/ab_bench.py selects it).  One SHA-256 per output array is printed; two builds compute the same when the
`sha256` lines of their runs are equal.

  python scripts/gpu_frame_bits.py <library path relative to the repository> [part ...]

Parts (default: all): `frame` -- per graph (dlr, sphere2500, parking-garage, intel) and precision (f64, f32, mixed), with no
kernel, Huber, and Cauchy with a mask on every other edge: assemble (Gauss-Newton and Levenberg-Marquardt form), chi2, edge_errors,
linearize_solve, update with a caller's dx under both signs, optimize(5) under both solvers; `queries` -- the r15 list on intel,
simulation-pose-landmark and parking-garage in f64: set_state / state, marginals, covariances, gate_edges, gate_joint, extend;
`shards` -- two emulated ranks on a small lattice and on parking-garage."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rustrobotics_amd import _lib  # noqa: E402

_lib.LIB_PATH = os.path.join(ROOT, sys.argv[1])
import numpy as np  # noqa: E402

from rustrobotics_amd import PoseGraph, PoseGraphSolver, sharding, synthetic_grid_arrays  # noqa: E402


def path(name):
    return os.path.join(ROOT, "tests", "golden", "g2o", name + ".g2o")


def out(label, *arrays):
    for i, a in enumerate(arrays):
        a = np.concatenate([np.ravel(s) for s in a]) if isinstance(a, (list, tuple)) and len(a) and isinstance(a[0], np.ndarray) else a
        print(f"sha256 {label} [{i}] {hashlib.sha256(np.ascontiguousarray(np.asarray(a)).tobytes()).hexdigest()}", flush=True)


def frame():
    for name in ("dlr", "sphere2500", "parking-garage", "intel"):
        arrays = PoseGraph.new(path(name)).graph_arrays()
        E = len(arrays[2])
        for precision in ("f64", "f32", "mixed"):
            for kernel in ("none", "huber", "cauchy-masked"):
                tag = f"{name} {precision} {kernel}"
                handles = {s: PoseGraph.from_arrays(*arrays, precision=precision, solver=getattr(PoseGraphSolver, s))
                           for s in ("GaussNewton", "LevenbergMarquardt")}
                for g in handles.values():
                    if kernel == "huber":
                        g.set_robust_kernel("huber", 1.0)
                    elif kernel != "none":
                        g.set_robust_kernel("cauchy", 2.0, (np.arange(E) % 2 == 0).astype(np.int32))
                g = handles["GaussNewton"]
                s0 = np.array(g.state())
                out(tag + " assemble gn", *g.assemble(0.0, False))
                out(tag + " assemble lm", *g.assemble(0.37, True))
                out(tag + " chi2", np.array([g.global_error()]))
                out(tag + " edge_errors", *g.edge_errors())
                dx = g.linearize_and_solve()
                out(tag + " linearize_solve gn, lm", dx, g.linearize_and_solve(0.37, True))
                g.update_nodes(dx, 1.0)
                s1 = np.array(g.state())
                g.update_nodes(0.5 * dx, -1.0)
                out(tag + " update +, -", s1, np.array(g.state()))
                for solver, h in handles.items():
                    h.set_state(s0)
                    e, n = h.optimize(5, return_norms=True)
                    out(f"{tag} optimize {solver}", np.array(e), np.array(n), np.array(h.state()))


def queries():
    from covariances_cases import far_pairs
    from extend_cases import case
    from gate_cases import GATE_GRAPHS, candidates
    from gate_joint_cases import joint_sets
    for name in ("intel", "simulation-pose-landmark", "parking-garage"):
        g = PoseGraph.new(path(name))
        s0 = np.array(g.state())
        e = g.optimize(GATE_GRAPHS.get(name, 5))
        out(name + " optimize", np.array(e), np.array(g.state()))
        st = np.array(g.state())
        g.set_state(s0)
        a = np.array(g.state())
        g.set_state(st)
        out(name + " set_state", a, np.array(g.state()))
        out(name + " marginals", *g.marginal_blocks())
        _, qa, qb = far_pairs(g.num_nodes)
        out(name + " covariances", *g.covariance_blocks(qa, qb))
        cand = candidates(g.graph_arrays(), g.state())
        out(name + " gate_edges", *g.gate_edges(*cand, return_innovation=True))
        out(name + " gate_joint", *g.gate_joint(*cand, joint_sets(len(cand[0])), return_prefix=True, return_innovation=True))
        c = case(name)
        for with_state in (True, False):
            h = PoseGraph.from_arrays(*c.base)
            h.optimize(3)
            args, kw = c.extend_args(with_state)
            h.extend(*args, **kw)
            s = np.array(h.state())
            out(f"{name} extend node_state={with_state}", s, np.array(h.optimize(3)), np.array(h.state()))


def shards():
    # (the 60 x 40 lattice in f32: a single-precision factor with a big root front, the stages with the gauge transfer on)
    for label, arrays, precision in (("lattice 40x25", synthetic_grid_arrays(40, 25), "f64"),
                                     ("parking-garage", PoseGraph.new(path("parking-garage")).graph_arrays(), "f64"),
                                     ("lattice 60x40 f32", synthetic_grid_arrays(60, 40), "f32")):
        sh, coll = sharding.emulate(arrays, 2, precision)
        e, n = sharding.gauss_newton(sh, 5, coll)
        out("two ranks, " + label, np.array(e), np.array(n), np.array(sharding.gather_state(sh)))


if __name__ == "__main__":
    for part in (sys.argv[2:] or ["frame", "queries", "shards"]):
        {"frame": frame, "queries": queries, "shards": shards}[part]()
