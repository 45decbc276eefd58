"""CPU reference for rr_pgo_gate_edges (include/rr_pgo.h), built on the unchanged oracle and tests/marginals_reference.py.

The candidates are appended to the graph's arrays at the handle's state: `linearize_edge(n_edges + c)` of that graph gives
e, A, B.  Sigma = H^-1 comes from MarginalsReference on the graph WITHOUT the candidates.  S = Omega^-1 + J Sigma J^T and
d2 = e^T S^-1 e are computed twice, once from each of the reference's two independent computations of Sigma; the noise
floor of a quantity is the worst relative difference between the two, and a GPU value passes at
marginals_reference.tolerance(floor) = max(1e-12, 100 x floor).
chi2 = e^T Omega e does not depend on Sigma.  Its second computation is the oracle's own, at the state with every entry moved
by one unit in the last place: e is a difference of poses (coordinates of 100 m, errors of a millimetre on parking-garage),
so a rounding of the inputs -- the handle keeps (cos, sin) where the state array holds an angle -- already moves it by
|pose| / |e| units in the last place.  The same rule then gives chi2's tolerance.
"""
import numpy as np

from gate_cases import EDGE_DIM, INFO_LEN, info_matrix, split_packed, thresholds, with_candidates
from marginals_reference import MarginalsReference, graph_at_state, rel_diff, tolerance


class GateReference:
    def __init__(self, arrays, state, cand, h_graph=None):
        """h_graph: the oracle graph whose normal matrix is inverted (default: the graph of `arrays` at `state`; a robust
        kernel: RobustReference(...).weighted_graph()[0])"""
        kind, a, b, _, info = cand
        self.kind, self.a, self.b = kind, a, b
        self.n = len(kind)
        self.ref = MarginalsReference(graph_at_state(arrays, state) if h_graph is None else h_graph)
        og = with_candidates(arrays, state, cand)
        n_edges = len(arrays[2])
        self.lin = [og.linearize_edge(n_edges + c) for c in range(self.n)]   # (A, B, e)
        self.omega = [info_matrix(k, w) for k, w in zip(kind, split_packed(kind, info, INFO_LEN))]
        og1 = with_candidates(arrays, np.nextafter(np.asarray(state, np.float64), np.inf), cand)
        e1 = [og1.linearize_edge(n_edges + c)[2] for c in range(self.n)]
        self.floor_chi2 = max(abs(float(e @ W @ e) - float(l[2] @ W @ l[2])) / float(l[2] @ W @ l[2])
                              for e, l, W in zip(e1, self.lin, self.omega))
        XA, XB, pos = self.ref._columns(list(a) + list(b))
        self.S, self.d2, self.chi2, self.P = [], [], [], []
        self.cancellation = 0.0      # worst max|Sigma_joint| / max|J Sigma J^T|
        self.floor_d2 = self.floor_S = 0.0
        for c in range(self.n):
            A, B, e = self.lin[c]
            J = np.hstack([A, B])
            rows = np.concatenate([self.ref.scalars(a[c]), self.ref.scalars(b[c])])
            cols = np.concatenate([pos[int(v)] + np.arange(self.ref.dims[v]) for v in (a[c], b[c])])
            two = []
            for X in (XA, XB):
                sig = X[np.ix_(rows, cols)]
                sig = 0.5 * (sig + sig.T)
                P = J @ sig @ J.T
                S = np.linalg.inv(self.omega[c]) + 0.5 * (P + P.T)
                two.append((S, float(e @ np.linalg.solve(S, e)), P, sig))
            self.S.append(two[0][0])
            self.d2.append(two[0][1])
            self.P.append(two[0][2])
            self.chi2.append(float(e @ self.omega[c] @ e))
            self.floor_S = max(self.floor_S, rel_diff(two[0][0], two[1][0]))
            self.floor_d2 = max(self.floor_d2, abs(two[0][1] - two[1][1]) / abs(two[1][1]))
            self.cancellation = max(self.cancellation, float(np.max(np.abs(two[0][3])) / np.max(np.abs(two[0][2]))))
        self.d2 = np.array(self.d2)
        self.chi2 = np.array(self.chi2)
        self.floor = max(self.floor_d2, self.floor_S)
        self.tol_d2, self.tol_S, self.tol_chi2 = tolerance(self.floor_d2), tolerance(self.floor_S), tolerance(self.floor_chi2)
        self.threshold = thresholds(kind)
        self.accept = self.d2 <= self.threshold
        # candidates whose d2 lies within the tolerance of the threshold: left out of a comparison of decisions
        self.undecided = np.abs(self.d2 - self.threshold) <= self.tol_d2 * self.threshold

    def innovation_from_blocks(self, c, saa, sab, sbb):
        """S of candidate c from three covariance blocks of its nodes and the reference Jacobians"""
        A, B, _ = self.lin[c]
        P = A @ saa @ A.T + A @ sab @ B.T + B @ sab.T @ A.T + B @ sbb @ B.T
        return np.linalg.inv(self.omega[c]) + P

    def summary(self, label):
        return (f"{label}: {self.n} candidates, {int(np.sum(self.accept))} accepted / {int(np.sum(~self.accept))} rejected, "
                f"d2 in [{self.d2.min():.3g}, {self.d2.max():.3g}], floor d2 {self.floor_d2:.3g} S {self.floor_S:.3g} chi2 {self.floor_chi2:.3g}, "
                f"max|Sigma| / max|J Sigma J^T| up to {self.cancellation:.3g}, undecided {int(np.sum(self.undecided))}")


def check(label, what, got, want, floor, tol, floor_max):
    """print the worst relative difference of `what`, its floor and tolerance, then assert"""
    if np.ndim(want[0]) == 0:
        worst = float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(np.asarray(want))))
    else:
        worst = max(rel_diff(g, w) for g, w in zip(got, want))
    print(f"{label} {what}: {len(want)} candidates, worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert len(got) == len(want)
    assert floor <= floor_max, (label, what, floor)
    assert worst <= tol, (label, what, worst, tol)
    return worst


__all__ = ["GateReference", "check", "EDGE_DIM"]
