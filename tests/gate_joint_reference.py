"""CPU reference for rr_pgo_gate_joint (include/rr_pgo.h), built on GateReference (tests/gate_reference.py: the candidates'
e, A, B and Omega from the unchanged oracle) and MarginalsReference._columns (two independent computations of Sigma).

Per set: J_s stacks the candidates' [A B] over the set's distinct nodes, S_s = blockdiag(Omega_c^-1) + J_s Sigma J_s^T,
S_s = L L^T, y = L^-1 e_s, prefix(k) = the sum of y^2 over the rows of the first k + 1 candidates, d2 = the last prefix.
All of it is computed twice, once from each computation of Sigma: the noise floor of a quantity is the worst relative
difference between the two, and a GPU value passes at marginals_reference.tolerance(floor) = max(1e-12, 100 x floor)."""
import numpy as np

from gate_joint_cases import block_starts, set_dims
from gate_reference import GateReference
from marginals_reference import rel_diff, tolerance


def chi2_95(d):
    from rustrobotics_amd.mapping import CHI2_95
    return CHI2_95[int(d)]


class JointReference:
    def __init__(self, arrays, state, cand, sets, h_graph=None, gate=None):
        """gate: a GateReference of the same arrays, state, candidates and h_graph, if the caller has one"""
        self.gate = gate if gate is not None else GateReference(arrays, state, cand, h_graph=h_graph)
        g = self.gate
        self.kind, self.sets = cand[0], [list(s) for s in sets]
        self.dims = set_dims(self.kind, self.sets)
        ref = g.ref
        XA, XB, pos = ref._columns([int(g.a[c]) for s in self.sets for c in s] + [int(g.b[c]) for s in self.sets for c in s])
        self.S, self.d2, self.prefix, self.single_sum = [], [], [], []
        self.floor_S = self.floor_d2 = self.floor_prefix = 0.0
        for s, members in enumerate(self.sets):
            J, nodes = self.jacobian(s)
            rows = np.concatenate([ref.scalars(v) for v in nodes])
            cols = np.concatenate([pos[v] + np.arange(ref.dims[v]) for v in nodes])
            e = np.concatenate([g.lin[c][2] for c in members])
            two = []
            for X in (XA, XB):
                sig = X[np.ix_(rows, cols)]
                two.append(self._distances(s, J, 0.5 * (sig + sig.T), e))
            self.S.append(two[0][0])
            self.prefix.append(two[0][1])
            self.d2.append(two[0][1][-1])
            self.single_sum.append(float(sum(g.d2[c] for c in members)))
            self.floor_S = max(self.floor_S, rel_diff(two[0][0], two[1][0]))
            self.floor_prefix = max(self.floor_prefix, float(np.max(np.abs(two[0][1] - two[1][1]) / np.abs(two[1][1]))))
            self.floor_d2 = max(self.floor_d2, abs(two[0][1][-1] - two[1][1][-1]) / abs(two[1][1][-1]))
        self.d2, self.single_sum = np.array(self.d2), np.array(self.single_sum)
        self.tol_S, self.tol_d2, self.tol_prefix = tolerance(self.floor_S), tolerance(self.floor_d2), tolerance(self.floor_prefix)
        self.threshold = np.array([chi2_95(d) for d in self.dims])
        self.accept = self.d2 <= self.threshold
        self.undecided = np.abs(self.d2 - self.threshold) <= self.tol_d2 * self.threshold

    def jacobian(self, s):
        """(J_s over the distinct nodes of set s, those nodes in ascending order)"""
        g, members = self.gate, self.sets[s]
        nodes = sorted(set(int(g.a[c]) for c in members) | set(int(g.b[c]) for c in members))
        start, o = {}, 0
        for v in nodes:
            start[v] = o
            o += int(g.ref.dims[v])
        rows = block_starts(self.kind, members)
        J = np.zeros((rows[-1], o))
        for k, c in enumerate(members):
            A, B, _ = g.lin[c]
            va, vb = int(g.a[c]), int(g.b[c])
            J[rows[k]:rows[k + 1], start[va]:start[va] + A.shape[1]] += A
            J[rows[k]:rows[k + 1], start[vb]:start[vb] + B.shape[1]] += B
        return J, nodes

    def _distances(self, s, J, sigma, e):
        members = self.sets[s]
        rows = block_starts(self.kind, members)
        P = J @ sigma @ J.T
        S = 0.5 * (P + P.T)
        for k, c in enumerate(members):
            S[rows[k]:rows[k + 1], rows[k]:rows[k + 1]] += np.linalg.inv(self.gate.omega[c])
        y = np.linalg.solve(np.linalg.cholesky(S), e)
        return S, np.cumsum(y * y)[np.array(rows[1:]) - 1]

    def innovation_from_covariance(self, s, sigma):
        """S_s from the joint covariance of the set's distinct nodes (ascending, as `jacobian` orders them)"""
        J, _ = self.jacobian(s)
        members = self.sets[s]
        rows = block_starts(self.kind, members)
        S = J @ sigma @ J.T
        for k, c in enumerate(members):
            S[rows[k]:rows[k + 1], rows[k]:rows[k + 1]] += np.linalg.inv(self.gate.omega[c])
        return S

    def blockdiag_cov(self, s):
        members = self.sets[s]
        rows = block_starts(self.kind, members)
        W = np.zeros((rows[-1], rows[-1]))
        for k, c in enumerate(members):
            W[rows[k]:rows[k + 1], rows[k]:rows[k + 1]] = np.linalg.inv(self.gate.omega[c])
        return W

    def summary(self, label):
        return (f"{label}: {len(self.sets)} sets, D_s {min(self.dims)} .. {max(self.dims)}, {int(np.sum(self.accept))} accepted / "
                f"{int(np.sum(~self.accept))} rejected, d2 in [{self.d2.min():.3g}, {self.d2.max():.3g}], floor S {self.floor_S:.3g} "
                f"d2 {self.floor_d2:.3g} prefixes {self.floor_prefix:.3g}, undecided {int(np.sum(self.undecided))}, "
                f"closest d2 / threshold {float((self.d2 / self.threshold)[np.argmin(np.abs(self.d2 / self.threshold - 1))]):.4g}")


def check_each(label, what, got, want, floor, tol, floor_max):
    """entry-wise relative comparison of lists of arrays (prefixes): print the worst figure, the floor and the tolerance, then assert"""
    assert len(got) == len(want)
    worst = max(float(np.max(np.abs(np.asarray(g) - np.asarray(w)) / np.abs(np.asarray(w)))) for g, w in zip(got, want))
    print(f"{label} {what}: {len(want)} sets, worst relative difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}")
    assert floor <= floor_max, (label, what, floor)
    assert worst <= tol, (label, what, worst, tol)
    return worst
