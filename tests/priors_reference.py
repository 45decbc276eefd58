"""CPU reference for rr_pgo_set_priors (include/rr_pgo.h, "absolute priors"), built on the unchanged oracle.

A prior on node i is the edge of the node's kind from a FIXED identity pose to node i, so the reference augments the graph:
one node O of the pose kind, at the identity, is appended as the LAST node (the other nodes keep their offsets), and every
prior becomes an edge O -> node.  The reference system is og_build_system of the augmented graph with O's rows and columns
deleted; chi2 is og_global_error; a step solves the reduced dense system with numpy and applies og_update_nodes with
dx_O = 0, so O never moves.  (Beyond STEP_DENSE_MAX unknowns -- intel, parking-garage -- the same reduced matrix is kept sparse
and solved by SciPy's sparse LU where SciPy is there: four dense steps of intel's 5184 unknowns take 14 s, the sparse ones
under a second.)

The oracle's anchor is the from-node of the first pose-pose edge.  Prior edges appended AFTER the graph's edges leave it where
it was: keep_anchor = 1.  A pose prior placed FIRST in edge order makes O the anchor, and the deleted rows take the 1e7 with
them: keep_anchor = 0, exactly, with no subtraction of 1e7.

Robust kernels: the Omega of every robustified edge and of every robust-flagged prior is scaled by its weight at the state
being linearised (robust_reference.weight), as RobustReference.weighted_graph does; the cost is the sum of rho.

Queries: Sigma is the inverse of the reduced H, computed twice (dense LU inverse, Cholesky solve); the disagreement of the two
is the noise floor, and the formulas of the gate are restated here from the header.
"""
import numpy as np

from oracle.oracle import OracleGraph
from marginals_reference import rel_diff, tolerance
from robust_reference import EDGE_DIM, INFO_LEN, META_LEN, rho, weight

try:
    import scipy.sparse as _sp
    import scipy.sparse.linalg as _spla
except ImportError:
    _sp = _spla = None

STEP_DENSE_MAX = 2000
NODE_DIM = {0: 3, 1: 2, 2: 6}
STATE_LEN = {0: 3, 1: 2, 2: 7}
IDENTITY_STATE = {0: [0.0, 0.0, 0.0], 2: [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]}


def split(kinds, packed, length):
    out, o = [], 0
    for k in kinds:
        out.append(np.asarray(packed[o:o + length[int(k)]], np.float64))
        o += length[int(k)]
    assert o == len(packed)
    return out


def full_info(kind, packed):
    d = EDGE_DIM[int(kind)]
    m = np.zeros((d, d))
    m[np.triu_indices(d)] = packed
    return m + np.triu(m, 1).T


class PriorsReference:
    """arrays: og_create packing; node, meas, info: the arguments of rr_pgo_set_priors; robust: per prior (None: none);
    kind / delta / edge_mask: the handle's robust kernel (None: plain least squares)."""

    def __init__(self, arrays, node, meas, info, robust=None, keep_anchor=True, kind=None, delta=1.0, edge_mask=None):
        nk, ns, ek, ef, et, em, ei = [np.asarray(a) for a in arrays]
        node = np.asarray(node, np.int32)
        self.n_graph_nodes, self.n_graph_edges, self.P = len(nk), len(ek), len(node)
        self.pose_kind = 2 if np.any(nk == 2) else 0
        self.dO = NODE_DIM[self.pose_kind]
        self.sO = STATE_LEN[self.pose_kind]
        O = len(nk)
        pk = nk[node].astype(np.int32)                      # the prior's edge kind is its node's kind
        pm, pw = split(pk, meas, META_LEN), split(pk, info, INFO_LEN)
        self.prior_omega = [full_info(k, w) for k, w in zip(pk, pw)]
        self.keep_anchor = bool(keep_anchor)
        first = []
        if not self.keep_anchor:
            poses = np.flatnonzero(pk != 1)
            assert len(poses), "keep_anchor = 0 needs a pose prior: it is the edge that moves the oracle's anchor to O"
            first = [int(poses[0])]
        last = [p for p in range(self.P) if p not in first]
        order = first + [-1] + last                         # -1: the graph's edges
        self.prior_edge = np.zeros(self.P, np.int64)       # edge index of every prior in the augmented graph
        self.graph_edge0 = len(first)
        kinds, frm, to, ms, ws = [], [], [], [], []
        for p in order:
            if p < 0:
                kinds.append(ek); frm.append(ef); to.append(et); ms.append(em); ws.append(ei)
                continue
            self.prior_edge[p] = sum(len(k) for k in kinds)
            kinds.append([pk[p]]); frm.append([O]); to.append([node[p]]); ms.append(pm[p]); ws.append(pw[p])
        self.arrays = [np.concatenate([nk, [self.pose_kind]]).astype(np.int32),
                       np.concatenate([ns, IDENTITY_STATE[self.pose_kind]]),
                       np.concatenate(kinds).astype(np.int32), np.concatenate(frm).astype(np.int32),
                       np.concatenate(to).astype(np.int32), np.concatenate(ms).astype(np.float64),
                       np.concatenate(ws).astype(np.float64)]
        self.g = OracleGraph.from_arrays(*self.arrays)
        self.n = self.g.dim - self.dO
        self.offsets = self.g.node_offsets()[:-1]
        self.dims = np.array([NODE_DIM[int(k)] for k in nk], np.int32)
        assert self.g.node_offsets()[-1] == self.n          # O is last: deleting it moves nothing
        # robust setting
        self.kind, self.delta = kind, float(delta)
        m = len(self.arrays[2])
        self.mask = np.zeros(m, bool)
        g_edges = np.arange(self.graph_edge0, self.graph_edge0 + self.n_graph_edges)
        self.mask[g_edges] = True if edge_mask is None else np.asarray(edge_mask) != 0
        self.mask[self.prior_edge] = False if robust is None else np.asarray(robust) != 0
        if kind is None:
            self.mask[:] = False
        self.omega = [full_info(k, w) for k, w in zip(self.arrays[2], split(self.arrays[2], self.arrays[6], INFO_LEN))]
        self.info_rep = np.repeat(np.arange(m), [INFO_LEN[int(k)] for k in self.arrays[2]])

    # ---- state
    def state(self):
        return self.g.state()[:-self.sO]

    def set_state(self, state):
        a = list(self.arrays)
        a[1] = np.concatenate([np.asarray(state, np.float64), IDENTITY_STATE[self.pose_kind]])
        self.g = OracleGraph.from_arrays(*a)

    # ---- errors and cost
    def edge_s(self):
        """s = e^T Omega e of every edge of the augmented graph at the current state"""
        return np.array([float(e @ W @ e) for W, e in ((W, self.g.linearize_edge(k)[2]) for k, W in enumerate(self.omega))])

    def prior_errors(self):
        s = self.edge_s()
        w = np.where(self.mask, weight(self.kind, s, self.delta), 1.0)
        return s[self.prior_edge], w[self.prior_edge]

    def cost(self):
        if self.kind is None:
            return self.g.global_error()
        s = self.edge_s()
        return float(np.sum(np.where(self.mask, rho(self.kind, s, self.delta), s)))

    def prior_cost(self):
        s = self.edge_s()
        return float(np.sum(np.where(self.mask, rho(self.kind, s, self.delta), s)[self.prior_edge]))

    # ---- the system
    def weighted_graph(self):
        if self.kind is None:
            return self.g
        s = self.edge_s()
        w = np.where(self.mask, weight(self.kind, s, self.delta), 1.0)
        a = list(self.arrays)
        a[1] = self.g.state()
        a[6] = self.arrays[6] * w[self.info_rep]
        return OracleGraph.from_arrays(*a)

    def system(self, lam=0.0, lm=False):
        """(H, b): og_build_system of the augmented graph, O's rows and columns deleted"""
        colptr, rowidx, vals, b = self.weighted_graph().build_system(lam, lm)
        N = self.n + self.dO
        cols = np.repeat(np.arange(N), np.diff(colptr))
        H = np.zeros((N, N))
        H[rowidx, cols] = vals
        H = H + np.tril(H, -1).T
        return H[:self.n, :self.n].copy(), b[:self.n].copy()

    def block(self, H, r, c):
        return H[self.offsets[r]:self.offsets[r] + self.dims[r], self.offsets[c]:self.offsets[c] + self.dims[c]]

    # ---- the loop of og_optimize, with the reduced system
    def step(self, lam=0.0, lm=False):
        if self.n > STEP_DENSE_MAX and _sp is not None:
            colptr, rowidx, vals, b = self.weighted_graph().build_system(lam, lm)
            N = self.n + self.dO
            low = _sp.csc_matrix((vals, rowidx, colptr), shape=(N, N))
            H = (low + _sp.tril(low, -1).T).tocsc()[:self.n, :self.n]
            return _spla.splu(H.tocsc()).solve(b[:self.n])
        H, b = self.system(lam, lm)
        return np.linalg.solve(H, b)

    def update(self, dx, sign=1.0):
        self.g.update_nodes(np.concatenate([dx, np.zeros(self.dO)]), sign)

    def optimize(self, num_iterations, lm=False):
        tolerance_, lam = 1e-4, 0.01
        last_error = self.cost()
        errors, norms = [last_error], []
        for _ in range(num_iterations):
            dx = self.step(lam, lm)
            self.update(dx, 1.0)
            nrm = float(np.sqrt(np.dot(dx, dx)))
            error = self.cost()
            if lm:
                if last_error < error:
                    self.update(dx, -1.0)
                    lam *= 2.0
                else:
                    lam /= 2.0
            last_error = error
            norms.append(nrm)
            errors.append(error)
            if nrm < tolerance_:
                break
        return np.array(errors), np.array(norms)

    # ---- queries: Sigma = H^-1 twice
    def sigma_pair(self):
        H, _ = self.system(0.0, False)
        A = np.linalg.inv(H)
        L = np.linalg.cholesky(H)
        B = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(self.n)))
        return A, B

    def scalars(self, v):
        return np.arange(self.offsets[v], self.offsets[v] + self.dims[v])

    def blocks(self, node_a, node_b=None, sig=None):
        """([Sigma(a_q, b_q)], noise floor over these blocks)"""
        A, B = self.sigma_pair() if sig is None else sig
        node_b = node_a if node_b is None else node_b
        out, floor = [], 0.0
        for a, b in zip(node_a, node_b):
            X, Y = A[np.ix_(self.scalars(a), self.scalars(b))], B[np.ix_(self.scalars(a), self.scalars(b))]
            if a == b:
                X, Y = 0.5 * (X + X.T), 0.5 * (Y + Y.T)
            out.append(X.copy())
            floor = max(floor, rel_diff(X, Y))
        return out, floor

    def gate(self, cand, sig=None):
        """rr_pgo_gate_edges restated: per candidate S = Omega^-1 + J Sigma J^T, d2 = e^T S^-1 e, chi2 = e^T Omega e, from each
        of the two Sigmas: (S, d2, chi2, floor_S, floor_d2).  e, A, B: og_linearize_edge of the candidate appended to the graph."""
        kind, a, b, meas, info = cand
        nk, _, ek, ef, et, em, ei = self.arrays
        og = OracleGraph.from_arrays(nk, self.g.state(), np.concatenate([ek, kind]), np.concatenate([ef, a]), np.concatenate([et, b]),
                                     np.concatenate([em, meas]), np.concatenate([ei, info]))
        sig = self.sigma_pair() if sig is None else sig
        omegas = [full_info(k, w) for k, w in zip(kind, split(kind, info, INFO_LEN))]
        S, d2, chi2, fS, fd = [], [], [], 0.0, 0.0
        for c in range(len(kind)):
            A, B, e = og.linearize_edge(len(ek) + c)
            J = np.hstack([A, B])
            idx = np.concatenate([self.scalars(a[c]), self.scalars(b[c])])
            two = []
            for X in sig:
                s = X[np.ix_(idx, idx)]
                P = J @ (0.5 * (s + s.T)) @ J.T
                Sc = np.linalg.inv(omegas[c]) + 0.5 * (P + P.T)
                two.append((Sc, float(e @ np.linalg.solve(Sc, e))))
            S.append(two[0][0]); d2.append(two[0][1]); chi2.append(float(e @ omegas[c] @ e))
            fS = max(fS, rel_diff(two[0][0], two[1][0]))
            fd = max(fd, abs(two[0][1] - two[1][1]) / abs(two[1][1]))
        return S, np.array(d2), np.array(chi2), fS, fd


def random_priors(rng, arrays, nodes, at_state=False, noise=0.05):
    """(node, meas, info) of priors on `nodes`: z = the node's state (+ noise unless at_state), random SPD Omega"""
    nk, ns = np.asarray(arrays[0]), np.asarray(arrays[1], np.float64)
    soff = np.concatenate([[0], np.cumsum([STATE_LEN[int(k)] for k in nk])])
    meas, info = [], []
    for v in nodes:
        k = int(nk[v])
        z = ns[soff[v]:soff[v + 1]].copy()
        if not at_state:
            z = z + rng.normal(scale=noise, size=len(z))
            if k == 2:
                z[3:] /= np.linalg.norm(z[3:])
        d = EDGE_DIM[k]
        a = rng.normal(size=(d, d))
        m = (a @ a.T + d * np.eye(d)) * rng.uniform(0.5, 50.0)
        meas.append(z)
        info.append(m[np.triu_indices(d)])
    return np.asarray(nodes, np.int32), np.concatenate(meas), np.concatenate(info)


def parse_expected(text, id_to_index, node_kind):
    """what `--priors FILE` must give for `text`: restated rule -- NODE_ID then measurement and upper-triangle information
    in g2o's order for the node's kind; '#' starts a comment"""
    node, meas, info = [], [], []
    for line in text.splitlines():
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        v = id_to_index[int(tok[0])]
        k = int(node_kind[v])
        vals = [float(t) for t in tok[1:]]
        assert len(vals) == META_LEN[k] + INFO_LEN[k]
        node.append(v)
        meas.extend(vals[:META_LEN[k]])
        info.extend(vals[META_LEN[k]:])
    return np.array(node, np.int32), np.array(meas), np.array(info)


__all__ = ["PriorsReference", "random_priors", "parse_expected", "tolerance", "rel_diff"]
