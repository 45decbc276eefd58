"""CPU reference for rr_pgo_set_fixed (include/rr_pgo.h, "fixed nodes"), built on the unchanged oracle.

With F the fixed nodes, the reference system is og_build_system of the same graph with the rows and columns of F deleted:
eliminating dx_i = 0 leaves every free node's block and right-hand side as they are, the terms of its edges to fixed nodes
included.  A step solves the reduced system and applies og_update_nodes with zeros at F; chi2 is og_global_error (every edge
and every prior counts).  Priors and robust kernels compose by reusing PriorsReference as it is (an empty prior list is a
graph with one more node that no edge touches, whose rows are deleted there).

keep_anchor = 0 with a free anchor: nothing is subtracted.  The oracle's anchor is the from-node of the first pose-pose edge,
so the edges are reordered: a pose-pose edge whose `from` node is fixed comes first, and the deleted rows take the 1e7 with
them.  (The sums of H and chi2 are then taken in another edge order: differences of rounding, inside the tolerances.)  The
fixed set must contain such a node.

Queries: Sigma is the inverse of the reduced H, computed twice (dense LU inverse, Cholesky solve), embedded in the full
index space with zeros in the rows and columns of F: the covariance conditional on the fixed nodes.  The disagreement of the
two is the noise floor, as in priors_reference.py.
"""
import numpy as np

from marginals_reference import rel_diff, tolerance
from priors_reference import PriorsReference, STEP_DENSE_MAX, _sp, _spla


def reorder_for_fixed_anchor(arrays, fixed):
    """the graph with a pose-pose edge whose `from` node is in `fixed` moved to the front: the oracle's anchor is then fixed.
    Returns (arrays, order): order[k] = the original index of the reordered graph's edge k."""
    nk, ns, ek, ef, et, em, ei = [np.asarray(a) for a in arrays]
    fixed = set(int(v) for v in fixed)
    cand = [k for k in range(len(ek)) if ek[k] != 1 and int(ef[k]) in fixed]
    assert cand, "keep_anchor = 0 needs a fixed node that is the from-node of a pose-pose edge"
    order = np.array([cand[0]] + [k for k in range(len(ek)) if k != cand[0]])
    ml, il = {0: 3, 1: 2, 2: 7}, {0: 6, 1: 3, 2: 21}
    mo = np.concatenate([[0], np.cumsum([ml[int(k)] for k in ek])])
    io = np.concatenate([[0], np.cumsum([il[int(k)] for k in ek])])
    em2 = np.concatenate([em[mo[k]:mo[k + 1]] for k in order])
    ei2 = np.concatenate([ei[io[k]:io[k + 1]] for k in order])
    return (nk, ns, ek[order], ef[order], et[order], em2, ei2), order


class FixedReference:
    """arrays: og_create packing; fixed: node indices; priors: (node, meas, info) or (node, meas, info, robust) of
    rr_pgo_set_priors (kept with its anchor setting at 1), None: none; kind / delta: the handle's robust kernel on every
    edge."""

    def __init__(self, arrays, fixed, keep_anchor=True, priors=None, kind=None, delta=1.0):
        self.fixed = np.unique(np.asarray(fixed, np.int64))
        self.keep_anchor = bool(keep_anchor)
        if not self.keep_anchor:
            arrays, _ = reorder_for_fixed_anchor(arrays, self.fixed)
        node, meas, info, robust = (list(priors) + [None])[:4] if priors is not None else (np.zeros(0, np.int32), np.zeros(0), np.zeros(0), None)
        self.base = PriorsReference(arrays, node, meas, info, robust=robust, keep_anchor=True, kind=kind, delta=delta)
        b = self.base
        self.n, self.dims, self.offsets = b.n, b.dims, b.offsets
        is_fixed = np.zeros(self.n, bool)
        for v in self.fixed:
            is_fixed[b.scalars(v)] = True
        self.fixed_scalars = np.flatnonzero(is_fixed)
        self.free = np.flatnonzero(~is_fixed)
        if not self.keep_anchor:   # the term went with the deleted rows
            anchor = int(arrays[3][np.flatnonzero(np.asarray(arrays[2]) != 1)[0]])
            assert anchor in set(self.fixed.tolist())

    # ---- state and cost
    def state(self):
        return self.base.state()

    def set_state(self, state):
        self.base.set_state(state)

    def cost(self):
        return self.base.cost()

    def scalars(self, v):
        return self.base.scalars(v)

    # ---- the system
    def full_system(self, lam=0.0, lm=False):
        """(H, b) over all nodes: the oracle's system (with any priors), before anything is deleted"""
        return self.base.system(lam, lm)

    def system(self, lam=0.0, lm=False):
        """(H_ff, b_f): the rows and columns of F deleted"""
        H, b = self.full_system(lam, lm)
        return H[np.ix_(self.free, self.free)].copy(), b[self.free].copy()

    def expected_system(self, lam=0.0, lm=False):
        """(H, b) over all nodes as the handle assembles it: identity rows at F, zero blocks to F, b = 0 at F"""
        H, b = self.full_system(lam, lm)
        H[self.fixed_scalars, :] = 0.0
        H[:, self.fixed_scalars] = 0.0
        H[self.fixed_scalars, self.fixed_scalars] = 1.0
        b[self.fixed_scalars] = 0.0
        return H, b

    # ---- the loop of og_optimize with the reduced system
    def step(self, lam=0.0, lm=False):
        """dx over all nodes: the reduced solve, zeros at F"""
        dx = np.zeros(self.n)
        if len(self.free) == 0:
            return dx
        b = self.base
        if len(self.free) > STEP_DENSE_MAX and _sp is not None:
            colptr, rowidx, vals, rhs = b.weighted_graph().build_system(lam, lm)
            N = b.n + b.dO
            low = _sp.csc_matrix((vals, rowidx, colptr), shape=(N, N))
            H = (low + _sp.tril(low, -1).T).tocsc()[self.free, :][:, self.free]
            dx[self.free] = _spla.splu(H.tocsc()).solve(rhs[self.free])
            return dx
        H, rhs = self.system(lam, lm)
        dx[self.free] = np.linalg.solve(H, rhs)
        return dx

    def update(self, dx, sign=1.0):
        dx = np.array(dx, np.float64)
        dx[self.fixed_scalars] = 0.0
        self.base.update(dx, sign)

    def optimize(self, num_iterations, lm=False):
        """(errors, norms, rejections): the loop of PriorsReference.optimize, and how often Levenberg-Marquardt undid a step"""
        tolerance_, lam = 1e-4, 0.01
        last_error = self.cost()
        errors, norms, rejected = [last_error], [], 0
        for _ in range(num_iterations):
            dx = self.step(lam, lm)
            self.update(dx, 1.0)
            nrm = float(np.sqrt(np.dot(dx, dx)))
            error = self.cost()
            if lm:
                if last_error < error:
                    self.update(dx, -1.0)
                    lam *= 2.0
                    rejected += 1
                else:
                    lam /= 2.0
            last_error = error
            norms.append(nrm)
            errors.append(error)
            if nrm < tolerance_:
                break
        return np.array(errors), np.array(norms), rejected

    # ---- queries: the conditional Sigma twice, zeros at F
    def sigma_pair(self):
        H, _ = self.system(0.0, False)
        out = []
        A = np.linalg.inv(H)
        L = np.linalg.cholesky(H)
        B = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(len(self.free))))
        for X in (A, B):
            full = np.zeros((self.n, self.n))
            full[np.ix_(self.free, self.free)] = X
            out.append(full)
        return tuple(out)

    def is_fixed(self, v):
        return int(v) in set(self.fixed.tolist())

    def blocks(self, node_a, node_b=None, sig=None):
        """([Sigma(a_q, b_q)], noise floor over the blocks without a fixed node); a block with a fixed node is zero"""
        A, B = self.sigma_pair() if sig is None else sig
        node_b = node_a if node_b is None else node_b
        out, floor = [], 0.0
        for a, b in zip(node_a, node_b):
            X, Y = A[np.ix_(self.scalars(a), self.scalars(b))], B[np.ix_(self.scalars(a), self.scalars(b))]
            if a == b:
                X, Y = 0.5 * (X + X.T), 0.5 * (Y + Y.T)
            out.append(X.copy())
            # (two free nodes that only fixed nodes join are conditionally independent: their block is zero in both inverses)
            if not (self.is_fixed(a) or self.is_fixed(b)) and np.any(Y != 0.0):
                floor = max(floor, rel_diff(X, Y))
        return out, floor

    def gate(self, cand, sig=None):
        """PriorsReference.gate over the conditional Sigma: S = Omega^-1 + J Sigma J^T with zeros at F"""
        return self.base.gate(cand, sig=self.sigma_pair() if sig is None else sig)

    def gate_joint(self, cand, sets, sig=None):
        """rr_pgo_gate_joint restated: per set the stacked e_s, S_s = blockdiag(Omega_c^-1) + J_s Sigma J_s^T over the set's
        members, d2 = e_s^T S_s^-1 e_s, from each of the two Sigmas: (d2, floor_d2)"""
        from oracle.oracle import OracleGraph
        from priors_reference import full_info, split
        from robust_reference import INFO_LEN
        kind, a, b, meas, info = cand
        base = self.base
        nk, _, ek, ef, et, em, ei = base.arrays
        og = OracleGraph.from_arrays(nk, base.g.state(), np.concatenate([ek, kind]), np.concatenate([ef, a]), np.concatenate([et, b]),
                                     np.concatenate([em, meas]), np.concatenate([ei, info]))
        sig = self.sigma_pair() if sig is None else sig
        omegas = [full_info(k, w) for k, w in zip(kind, split(kind, info, INFO_LEN))]
        lin = [og.linearize_edge(len(ek) + c) for c in range(len(kind))]
        d2, floor = [], 0.0
        for members in sets:
            D = sum(len(lin[c][2]) for c in members)
            J = np.zeros((D, self.n))
            R = np.zeros((D, D))
            e = np.zeros(D)
            r = 0
            for c in members:
                A_, B_, e_ = lin[c]
                d = len(e_)
                J[r:r + d, self.scalars(a[c])] += A_
                J[r:r + d, self.scalars(b[c])] += B_
                R[r:r + d, r:r + d] = np.linalg.inv(omegas[c])
                e[r:r + d] = e_
                r += d
            two = []
            for X in sig:
                P = J @ (0.5 * (X + X.T)) @ J.T
                two.append(float(e @ np.linalg.solve(R + 0.5 * (P + P.T), e)))
            d2.append(two[0])
            floor = max(floor, abs(two[0] - two[1]) / abs(two[1]))
        return np.array(d2), floor


def one_free_node_system(arrays, free):
    """The problem in which every node but `free` is fixed, built by hand from og_linearize_edge: H = sum over the node's
    edges of J^T Omega J (+ 1e7 I when the node is the oracle's anchor), b = -sum J^T Omega e, J = the node's own Jacobian."""
    from oracle.oracle import OracleGraph
    from priors_reference import NODE_DIM
    o = OracleGraph.from_arrays(*arrays)
    ek, ef, et = np.asarray(arrays[2]), np.asarray(arrays[3]), np.asarray(arrays[4])
    d = NODE_DIM[int(arrays[0][free])]
    H, b = np.zeros((d, d)), np.zeros(d)
    for k in range(len(ek)):
        if free not in (int(ef[k]), int(et[k])):
            continue
        A, B, e = o.linearize_edge(k)
        W = o.edge_info(k)
        J = (A if int(ef[k]) == free else 0) + (B if int(et[k]) == free else 0)
        H += J.T @ W @ J
        b -= J.T @ W @ e
    anchor = int(ef[np.flatnonzero(ek != 1)[0]])
    if free == anchor:
        H += 1e7 * np.eye(d)
    return H, b


__all__ = ["FixedReference", "reorder_for_fixed_anchor", "one_free_node_system", "tolerance", "rel_diff"]
