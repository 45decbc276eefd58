"""CPU reference for rr_pgo_check_edges (include/rr_pgo.h), built on the unchanged oracle, tests/marginals_reference.py,
tests/robust_reference.py and tests/fixed_reference.py, as tests/gate_reference.py is.

For edge c of the graph at the handle's state, `linearize_edge(c)` of the oracle gives e, A, B.  With w the robust weight of
the edge (RobustReference.weights; 1 without a kernel or for an unmasked edge) and Sigma = H^-1 of the graph whose robustified
edges carry w Omega (RobustReference.weighted_graph):
    R = Omega^-1 / w - J Sigma J^T,   d2 = e^T R^-1 e,   r = trace(R w Omega) / d_e,   chi2 = e^T Omega e.
R, d2 and r are computed twice, once from each of the reference's two independent computations of Sigma.  The noise floor of
R and of d2 is the worst relative difference between the two over the COMPARED edges; the floor of r is the worst absolute
difference over all queried edges (r has scale 1).  A GPU value passes at marginals_reference.tolerance(floor) =
max(1e-12, 100 x floor), and every floor must be at most FLOOR_MAX = 1e-6.  chi2 takes its floor as gate_reference does: the
oracle's own value at the state with every entry moved by one unit in the last place.
Compared in d2 and R: every queried edge whose reference redundancy is at least MIN_REDUNDANCY = 0.01 -- no edge is left out
for any other reason.  Below that level R is a difference of two nearly equal matrices and d2 may be anything, NaN included:
those edges are compared in r only (their chi2 too: a bridge's residual is fitted exactly at an optimum, so its chi2 is zero up
to rounding and a relative difference means nothing there; tests/test_check_edges_gpu.py compares chi2 of EVERY edge with
rr_pgo_edge_errors bit for bit instead).
An edge with r >= MIN_REDUNDANCY whose smallest directional redundancy r_min is zero within tolerance(its floor) (`singular`) is compared in r, R and
r_min, not in d2: see CheckReference.  Where e itself is at rounding level -- the initial state of a dataset file, whose poses
were composed from the odometry, so the odometry edges' errors are zero up to rounding -- d2 inherits chi2's floor, which two
inversions of one H do not show: the robust fixtures are therefore taken at a moved state, where no error is that small.
`sig`: a pair of full n x n Sigmas from another reference (PriorsReference.sigma_pair, FixedReference.sigma_pair: priors,
fixed nodes, keep_anchor = 0) in place of MarginalsReference's."""
import numpy as np

from covariances_cases import FLOOR_MAX
from gate_cases import EDGE_DIM, INFO_LEN, info_matrix, split_packed
from marginals_reference import MarginalsReference, graph_at_state, rel_diff, tolerance
from robust_reference import RobustReference

MIN_REDUNDANCY = 0.01


def residual(e, A, B, omega, w, sig):
    """(R, d2, r, r_min) of one edge from the joint covariance `sig` of its two nodes; d2 is NaN where R is not positive
    definite; r_min is the smallest eigenvalue of Omega_w^1/2 R Omega_w^1/2 (their mean is r)"""
    J = np.hstack([A, B])
    sig = 0.5 * (sig + sig.T)
    P = J @ sig @ J.T
    R = np.linalg.inv(omega) / w - 0.5 * (P + P.T)
    r = float(np.trace(R @ (w * omega)) / len(e))
    d2 = float(e @ np.linalg.solve(R, e)) if np.all(np.linalg.eigvalsh(R) > 0) else float("nan")
    L = np.linalg.cholesky(w * omega)
    return R, d2, r, float(np.linalg.eigvalsh(L.T @ R @ L)[0])


class CheckReference:
    def __init__(self, arrays, state, edges=None, kind=None, delta=1.0, mask=None, sig=None):
        nk, _, ek, ef, et, em, ei = [np.asarray(a) for a in arrays]
        self.edges = np.arange(len(ek)) if edges is None else np.asarray(edges, np.int64)
        self.n = len(self.edges)
        at = list(arrays)
        at[1] = np.asarray(state, np.float64)
        og = graph_at_state(arrays, state)
        rob = RobustReference(at, kind, delta, mask)
        gw, w_all = rob.weighted_graph()
        self.w = np.asarray(w_all, np.float64)[self.edges]
        omega_all = split_packed(ek, ei, INFO_LEN)
        self.kind = ek[self.edges]
        self.omega = [info_matrix(ek[k], omega_all[k]) for k in self.edges]
        self.lin = [og.linearize_edge(int(k)) for k in self.edges]   # (A, B, e)
        og1 = graph_at_state(arrays, np.nextafter(np.asarray(state, np.float64), np.inf))
        self.chi2 = np.array([float(l[2] @ W @ l[2]) for l, W in zip(self.lin, self.omega)])
        chi2_1 = np.array([float(e @ W @ e) for e, W in ((og1.linearize_edge(int(k))[2], W) for k, W in zip(self.edges, self.omega))])
        a, b = ef[self.edges], et[self.edges]
        if sig is None:
            ref = MarginalsReference(gw)
            XA, XB, pos = ref._columns(list(a) + list(b))
            scal, dims = ref.scalars, ref.dims

            def joint(X, va, vb):
                rows = np.concatenate([scal(va), scal(vb)])
                cols = np.concatenate([pos[int(v)] + np.arange(dims[v]) for v in (va, vb)])
                return X[np.ix_(rows, cols)]
            pair = (XA, XB)
        else:
            off = og.node_offsets()
            dims = np.array([{0: 3, 1: 2, 2: 6}[int(k)] for k in nk])

            def joint(X, va, vb):
                idx = np.concatenate([np.arange(off[v], off[v] + dims[v]) for v in (va, vb)])
                return X[np.ix_(idx, idx)]
            pair = sig
        two = [[residual(l[2], l[0], l[1], W, w, joint(X, va, vb)) for l, W, w, va, vb in zip(self.lin, self.omega, self.w, a, b)]
               for X in pair]
        self.R = [t[0] for t in two[0]]
        self.d2 = np.array([t[1] for t in two[0]])
        self.r = np.array([t[2] for t in two[0]])
        self.r_min = np.array([t[3] for t in two[0]])
        d2_b, r_b, rmin_b = np.array([t[1] for t in two[1]]), np.array([t[2] for t in two[1]]), np.array([t[3] for t in two[1]])
        self.compared = self.r >= MIN_REDUNDANCY
        # PARTIAL redundancy: the rest of the graph determines the residual in some directions only (a pose whose heading one
        # landmark sighting alone fixes).  R is then singular to rounding in the others and d2 is NaN or a number that
        # rounding picks, whatever r is: such edges are compared in r and R, not in d2.  The main fixtures have none
        # (tests/test_check_edges_cpu.py asserts it); check_edges_cases.PARTIAL are the graphs kept for this case.
        self.floor_r = float(np.max(np.abs(self.r - r_b)))
        self.floor_rmin = float(np.max(np.abs(self.r_min - rmin_b)))
        self.tol_rmin = tolerance(self.floor_rmin)
        self.singular = self.compared & (self.r_min <= self.tol_rmin)   # zero within the reference's own noise
        cR = np.flatnonzero(self.compared)
        c = np.flatnonzero(self.compared & ~self.singular)
        self.floor_R = max([rel_diff(two[0][q][0], two[1][q][0]) for q in cR], default=0.0)
        with np.errstate(invalid="ignore"):
            rel = np.abs(self.d2[c] - d2_b[c]) / np.abs(d2_b[c])
        self.floor_d2 = float(np.max(rel)) if len(c) else 0.0   # (NaN -- R not positive definite on a compared edge -- fails the bound)
        # (a bridge's residual is fitted exactly at an optimum: its chi2 is zero up to rounding and has no relative floor)
        self.floor_chi2 = float(np.max(np.abs(chi2_1[c] - self.chi2[c]) / self.chi2[c])) if len(c) else 0.0
        self.tol_R, self.tol_d2 = tolerance(self.floor_R), tolerance(self.floor_d2)
        self.tol_r, self.tol_chi2 = tolerance(self.floor_r), tolerance(self.floor_chi2)

    def floors_ok(self):
        return all(f <= FLOOR_MAX for f in (self.floor_R, self.floor_d2, self.floor_r, self.floor_chi2))

    def summary(self, label):
        c = self.compared & ~self.singular
        d2 = self.d2[c]
        return (f"{label}: {self.n} edges, {int(np.sum(c))} compared in d2 and R (r >= {MIN_REDUNDANCY}), r in [{self.r.min():.3g}, {self.r.max():.3g}], "
                f"d2 in [{d2.min() if len(d2) else 0:.3g}, {d2.max() if len(d2) else 0:.3g}], floor d2 {self.floor_d2:.3g} R {self.floor_R:.3g} "
                f"r {self.floor_r:.3g} chi2 {self.floor_chi2:.3g}")

    def check(self, label, got):
        """got: the dict of PoseGraph.check_edges(..., return_residual=True).  Prints every worst figure, then asserts."""
        cR = np.flatnonzero(self.compared)
        c = np.flatnonzero(self.compared & ~self.singular)
        assert all(len(got[k]) == self.n for k in ("d2", "redundancy", "chi2", "R"))
        worst_r = float(np.max(np.abs(got["redundancy"] - self.r)))
        worst_chi2 = float(np.max(np.abs(got["chi2"][c] - self.chi2[c]) / self.chi2[c])) if len(c) else 0.0
        worst_d2 = float(np.max(np.abs(got["d2"][c] - self.d2[c]) / np.abs(self.d2[c]))) if len(c) else 0.0
        worst_R = max([rel_diff(got["R"][q], self.R[q]) for q in cR], default=0.0)
        if "redundancy_min" in got:   # the mirror's smallest directional redundancy, from the GPU's R and r
            worst_rmin = float(np.max(np.abs(got["redundancy_min"] - self.r_min)))
            print(f"{label}: smallest directional redundancy: worst difference {worst_rmin:.3g} absolute (floor {self.floor_rmin:.3g}, "
                  f"tolerance {self.tol_rmin:.3g}); {int(np.sum(self.singular))} edges with r >= {MIN_REDUNDANCY} are singular in a direction")
            assert self.floor_rmin <= FLOOR_MAX and worst_rmin <= self.tol_rmin, (label, "r_min", worst_rmin, self.tol_rmin)
        print(f"{label}: {self.n} edges, {len(cR)} compared in R, {len(c)} in d2; worst difference d2 {worst_d2:.3g} (floor {self.floor_d2:.3g}, "
              f"tolerance {self.tol_d2:.3g}), R {worst_R:.3g} (floor {self.floor_R:.3g}, tolerance {self.tol_R:.3g}), r {worst_r:.3g} absolute "
              f"(floor {self.floor_r:.3g}, tolerance {self.tol_r:.3g}), chi2 {worst_chi2:.3g} (floor {self.floor_chi2:.3g}, tolerance {self.tol_chi2:.3g})")
        assert self.floors_ok(), (label, self.floor_R, self.floor_d2, self.floor_r, self.floor_chi2)
        for q, k in enumerate(self.kind):
            assert got["R"][q].shape == (EDGE_DIM[int(k)],) * 2
        assert worst_r <= self.tol_r, (label, "r", worst_r, self.tol_r)
        assert worst_chi2 <= self.tol_chi2, (label, "chi2", worst_chi2, self.tol_chi2)
        assert not (worst_d2 > self.tol_d2) and np.all(np.isfinite(got["d2"][c])), (label, "d2", worst_d2, self.tol_d2)
        assert worst_R <= self.tol_R, (label, "R", worst_R, self.tol_R)


def pose_cycle_edges(arrays):
    """indices of the edges that lie on a cycle of pose-pose edges: the non-bridges of the pose-pose multigraph (two parallel
    edges form a cycle)"""
    nk, ek, ef, et = np.asarray(arrays[0]), np.asarray(arrays[2]), np.asarray(arrays[3]), np.asarray(arrays[4])
    n = len(nk)
    adj = [[] for _ in range(n)]
    for k in np.flatnonzero(ek != 1):
        adj[int(ef[k])].append((int(et[k]), int(k)))
        adj[int(et[k])].append((int(ef[k]), int(k)))
    disc, low, bridges, t = [-1] * n, [0] * n, set(), 0
    for root in range(n):
        if disc[root] >= 0:
            continue
        disc[root] = low[root] = t
        t += 1
        stack = [(root, -1, 0)]
        while stack:
            v, via, i = stack.pop()
            if i < len(adj[v]):
                stack.append((v, via, i + 1))
                u, k = adj[v][i]
                if k == via:
                    continue
                if disc[u] < 0:
                    disc[u] = low[u] = t
                    t += 1
                    stack.append((u, k, 0))
                else:
                    low[v] = min(low[v], disc[u])
            elif stack:
                p = stack[-1][0]
                low[p] = min(low[p], low[v])
                if low[v] > disc[p]:
                    bridges.add(via)
    return [int(k) for k in np.flatnonzero(ek != 1) if int(k) not in bridges]


__all__ = ["CheckReference", "residual", "pose_cycle_edges", "MIN_REDUNDANCY", "FLOOR_MAX"]
