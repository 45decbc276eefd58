"""CPU reference for 3-D graphs with point landmarks (include/rr_pgo.h: RR_PGO_NODE_XYZ, RR_PGO_EDGE_SE3_XYZ), plain numpy
in f64.  The C oracle does not know the two kinds, so nothing here calls it; tests/test_landmarks3d_cpu.py ties this file to
it on a pure SE(3) graph and checks the point edge's Jacobians against central differences in extended precision.

Definitions restated from the header (quaternions x, y, z, w):
  SE3 edge i -> j, measurement Z:   E = Z^-1 Xi^-1 Xj,  e = [t_E ; sign(w_E) vec(q_E)]                       
  SE3_XYZ edge pose (t, q) -> l:    p = R(q)^T (l - t),  e = p - z,   A = [-I | [p]x],  B = R(q)^T
  increments:  pose  t += R dt, q <- normalise(q (x) exp(dw));  landmark  l += dl
  prior on a node: the edge of its kind from the fixed identity pose
  system: H = sum J^T (w Omega) J (+ 1e7 I on the anchor, + lambda I), b = -sum J^T (w Omega) e; a fixed node has an
  identity block, b = 0 and zero off-diagonal blocks; its state never changes
Sigma = H^-1 is computed twice (LU inverse, Cholesky solves); the disagreement of the two is the noise floor, as in
marginals_reference.py.
"""
import numpy as np

from marginals_reference import rel_diff, tolerance
from robust_reference import rho, weight

NODE_DIM = {2: 6, 3: 3}
STATE_LEN = {2: 7, 3: 3}
EDGE_DIM = {2: 6, 3: 3}
META_LEN = {2: 7, 3: 3}
INFO_LEN = {2: 21, 3: 6}
ANCHOR = 1e7


# ---- quaternions and the two factors

def q_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def q_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def q_to_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def q_exp(dw):
    th = float(np.linalg.norm(dw))
    if th < 1e-12:
        return np.array([0.5 * dw[0], 0.5 * dw[1], 0.5 * dw[2], 1.0])
    return np.concatenate([np.sin(0.5 * th) / th * np.asarray(dw), [np.cos(0.5 * th)]])


def unit(q):
    return np.asarray(q, np.float64) / np.linalg.norm(q)


def se3_edge(xi, xj, z):
    """(e, A, B) of an SE3 edge; xi, xj, z: x y z qx qy qz qw, quaternions of unit length"""
    ti, qi, tj, qj, tz, qz = xi[:3], xi[3:], xj[:3], xj[3:], z[:3], z[3:]
    Ri, Rz = q_to_rot(qi), q_to_rot(qz)
    tC = Ri.T @ (tj - ti)
    qC = q_mul(q_conj(qi), qj)
    tE = Rz.T @ (tC - tz)
    qE = q_mul(q_conj(qz), qC)
    s = -1.0 if qE[3] < 0 else 1.0
    e = np.concatenate([tE, s * qE[:3]])
    A, B = np.zeros((6, 6), e.dtype), np.zeros((6, 6), e.dtype)
    B[:3, :3] = q_to_rot(qE)
    B[3:, 3:] = 0.5 * s * (qE[3] * np.eye(3) + skew(qE[:3]))
    A[:3, :3] = -Rz.T
    A[:3, 3:] = Rz.T @ skew(tC)
    for k in range(3):
        u = np.zeros(4, e.dtype)
        u[k] = 1.0
        A[3:, 3 + k] = -0.5 * s * q_mul(q_mul(q_conj(qz), u), qC)[:3]
    return e, A, B


def point_edge(x, l, z):
    """(e, A, B) of an SE3_XYZ edge from pose x (7) to landmark l (3), measurement z (3)"""
    R = q_to_rot(x[3:])
    p = R.T @ (np.asarray(l) - x[:3])
    return p - np.asarray(z), np.hstack([-np.eye(3), skew(p)]), R.T


IDENTITY = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def full_info(kind, packed):
    d = EDGE_DIM[int(kind)]
    m = np.zeros((d, d))
    m[np.triu_indices(d)] = packed
    return m + np.triu(m, 1).T


def split(kinds, packed, length):
    out, o = [], 0
    for k in kinds:
        out.append(np.asarray(packed[o:o + length[int(k)]], np.float64))
        o += length[int(k)]
    assert o == len(packed)
    return out


def normalised_state(nk, ns):
    """node states as the library holds them: quaternions of unit length"""
    out, o = [], 0
    for k in nk:
        s = np.array(ns[o:o + STATE_LEN[int(k)]], np.float64)
        if int(k) == 2:
            s[3:] = unit(s[3:])
        out.append(s)
        o += STATE_LEN[int(k)]
    return out


class Landmarks3dReference:
    """arrays: rr_pgo_graph_desc packing (node kinds 2 / 3, edge kinds 2 / 3).  priors: (node, meas, info[, robust]) of
    rr_pgo_set_priors with keep_anchor; fixed: nodes of rr_pgo_set_fixed with fixed_keep_anchor; kind / delta / edge_mask:
    the robust kernel."""

    def __init__(self, arrays, priors=None, keep_anchor=True, fixed=(), fixed_keep_anchor=True, kind=None, delta=1.0, edge_mask=None):
        nk, ns, ek, ef, et, em, ei = [np.asarray(a) for a in arrays]
        self.nk, self.ek, self.ef, self.et = nk.astype(int), ek.astype(int), ef.astype(int), et.astype(int)
        self.x = normalised_state(nk, ns)
        self.meas = split(ek, em, META_LEN)
        for k, m in zip(self.ek, self.meas):
            if k == 2:
                m[3:] = unit(m[3:])
        self.omega = [full_info(k, w) for k, w in zip(ek, split(ek, ei, INFO_LEN))]
        self.dims = np.array([NODE_DIM[int(k)] for k in nk])
        self.offsets = np.concatenate([[0], np.cumsum(self.dims)])[:-1]
        self.n = int(self.dims.sum())
        pp = np.flatnonzero(self.ek == 2)
        self.anchor = int(self.ef[pp[0]]) if len(pp) else -1
        self.kind, self.delta = kind, float(delta)
        self.mask = np.ones(len(ek), bool) if edge_mask is None else np.asarray(edge_mask) != 0
        self.pnode = np.zeros(0, int)
        self.pmeas, self.pomega, self.probust = [], [], np.zeros(0, bool)
        self.keep_anchor = True
        if priors is not None:
            node = np.asarray(priors[0], int)
            pk = self.nk[node]
            self.pnode = node
            self.pmeas = split(pk, priors[1], META_LEN)
            for k, m in zip(pk, self.pmeas):
                if k == 2:
                    m[3:] = unit(m[3:])
            self.pomega = [full_info(k, w) for k, w in zip(pk, split(pk, priors[2], INFO_LEN))]
            self.probust = np.zeros(len(node), bool) if len(priors) < 4 or priors[3] is None else np.asarray(priors[3]) != 0
            self.keep_anchor = bool(keep_anchor) or len(node) == 0
        self.fixed = sorted(set(int(v) for v in fixed))
        self.fixed_keep_anchor = bool(fixed_keep_anchor) or not self.fixed

    # ---- state
    def state(self):
        return np.concatenate(self.x)

    def set_state(self, state):
        self.x = normalised_state(self.nk, state)

    def scalars(self, v):
        return np.arange(self.offsets[v], self.offsets[v] + self.dims[v])

    # ---- the terms: (from node or -1, to node, e, A or None, B, Omega, robustified)
    def edge_term(self, k, dtype=np.float64):
        a, b = self.ef[k], self.et[k]
        if self.ek[k] == 2:
            e, A, B = se3_edge(self.x[a].astype(dtype), self.x[b].astype(dtype), self.meas[k].astype(dtype))
        else:
            e, A, B = point_edge(self.x[a].astype(dtype), self.x[b].astype(dtype), self.meas[k].astype(dtype))
        return a, b, e, A, B, self.omega[k], bool(self.kind) and bool(self.mask[k])

    def prior_term(self, p, dtype=np.float64):
        v = self.pnode[p]
        if self.nk[v] == 2:
            e, _, B = se3_edge(IDENTITY.astype(dtype), self.x[v].astype(dtype), self.pmeas[p].astype(dtype))
        else:
            e, _, B = point_edge(IDENTITY.astype(dtype), self.x[v].astype(dtype), self.pmeas[p].astype(dtype))
        return -1, v, e, None, B, self.pomega[p], bool(self.kind) and bool(self.probust[p])

    def terms(self, dtype=np.float64):
        return [self.edge_term(k, dtype) for k in range(len(self.ek))] + [self.prior_term(p, dtype) for p in range(len(self.pnode))]

    def edge_errors(self):
        s = np.array([float(t[2] @ t[5] @ t[2]) for t in (self.edge_term(k) for k in range(len(self.ek)))])
        w = np.where(self.mask & bool(self.kind), weight(self.kind, s, self.delta), 1.0)
        return s, w

    def prior_errors(self):
        s = np.array([float(t[2] @ t[5] @ t[2]) for t in (self.prior_term(p) for p in range(len(self.pnode)))])
        w = np.where(self.probust & bool(self.kind), weight(self.kind, s, self.delta), 1.0)
        return s, w

    def cost(self):
        c = 0.0
        for _, _, e, _, _, W, rob in self.terms():
            s = float(e @ W @ e)
            c += float(rho(self.kind, s, self.delta)) if rob else s
        return c

    # ---- the system
    def system(self, lam=0.0, lm=False, dtype=np.float64):
        """(H, b); dtype = np.longdouble evaluates every term and every sum in extended precision (solve_pair's second route)"""
        H, g = np.zeros((self.n, self.n), dtype), np.zeros(self.n, dtype)
        for a, b, e, A, B, W, rob in self.terms(dtype):
            if rob:
                W = W * float(weight(self.kind, float(e @ W @ e), self.delta))
            ib = self.scalars(b)
            H[np.ix_(ib, ib)] += B.T @ W @ B
            g[ib] += B.T @ W @ e
            if a >= 0:
                ia = self.scalars(a)
                H[np.ix_(ia, ia)] += A.T @ W @ A
                g[ia] += A.T @ W @ e
                H[np.ix_(ia, ib)] += A.T @ W @ B
                H[np.ix_(ib, ia)] += B.T @ W @ A
        if self.anchor >= 0 and self.keep_anchor and self.fixed_keep_anchor:
            ia = self.scalars(self.anchor)
            H[ia, ia] += ANCHOR
        if lm:
            H[np.arange(self.n), np.arange(self.n)] += lam
        b = -g
        for v in self.fixed:
            iv = self.scalars(v)
            H[iv, :] = 0.0
            H[:, iv] = 0.0
            H[iv, iv] = 1.0
            b[iv] = 0.0
        return H, b

    def block(self, H, r, c):
        return H[np.ix_(self.scalars(r), self.scalars(c))]

    # ---- the step and the loop of og_optimize
    def step(self, lam=0.0, lm=False):
        H, b = self.system(lam, lm)
        return np.linalg.solve(H, b)

    def update(self, dx, sign=1.0):
        for v in range(len(self.nk)):
            if v in self.fixed:
                continue
            d = sign * np.asarray(dx[self.scalars(v)], np.float64)
            x = self.x[v]
            if self.nk[v] == 3:
                self.x[v] = x + d
                continue
            t = x[:3] + q_to_rot(x[3:]) @ d[:3]
            q = unit(q_mul(x[3:], q_exp(d[3:])))
            self.x[v] = np.concatenate([t, q])

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
        for v in self.fixed:   # Sigma is conditional on the fixed nodes: their blocks are zero
            iv = self.scalars(v)
            for X in (A, B):
                X[iv, :] = 0.0
                X[:, iv] = 0.0
        return A, B

    def solve_pair(self, lam=0.0, lm=False):
        """dx by two independent routes and their disagreement, the reference's own error: the f64 system solved by LU, and
        the system evaluated in extended precision (near a minimum b is what is left of terms that cancel: its rounding, not
        the solve's, is then the larger part of dx's error), rounded once and solved by Cholesky"""
        H, b = self.system(lam, lm)
        x1 = np.linalg.solve(H, b)
        Hx, bx = self.system(lam, lm, np.longdouble)
        Hx, bx = Hx.astype(np.float64), bx.astype(np.float64)
        L = np.linalg.cholesky(Hx)
        x2 = np.linalg.solve(L.T, np.linalg.solve(L, bx))
        return x1, rel_diff(x1, x2)

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
            if np.abs(Y).max() > 0:
                floor = max(floor, rel_diff(X, Y))
        return out, floor

    def candidate_terms(self, cand):
        kind, a, b, meas, info = cand
        ms, ws = split(kind, meas, META_LEN), split(kind, info, INFO_LEN)
        out = []
        for c in range(len(kind)):
            if int(kind[c]) == 2:
                z = ms[c].copy()
                z[3:] = unit(z[3:])
                e, A, B = se3_edge(self.x[a[c]], self.x[b[c]], z)
            else:
                e, A, B = point_edge(self.x[a[c]], self.x[b[c]], ms[c])
            out.append((e, np.hstack([A, B]), np.concatenate([self.scalars(a[c]), self.scalars(b[c])]), full_info(kind[c], ws[c])))
        return out

    def gate(self, cand, sig=None):
        """rr_pgo_gate_edges restated: S = Omega^-1 + J Sigma J^T, d2 = e^T S^-1 e, chi2 = e^T Omega e from each of the two
        Sigmas: (S, d2, chi2, floor_S, floor_d2)"""
        sig = self.sigma_pair() if sig is None else sig
        S, d2, chi2, fS, fd = [], [], [], 0.0, 0.0
        for e, J, idx, W in self.candidate_terms(cand):
            two = []
            for X in sig:
                s = X[np.ix_(idx, idx)]
                P = J @ (0.5 * (s + s.T)) @ J.T
                Sc = np.linalg.inv(W) + 0.5 * (P + P.T)
                two.append((Sc, float(e @ np.linalg.solve(Sc, e))))
            S.append(two[0][0]); d2.append(two[0][1]); chi2.append(float(e @ W @ e))
            fS = max(fS, rel_diff(two[0][0], two[1][0]))
            fd = max(fd, abs(two[0][1] - two[1][1]) / abs(two[1][1]))
        return S, np.array(d2), np.array(chi2), fS, fd

    def gate_joint(self, cand, sets, sig=None):
        """rr_pgo_gate_joint restated: per set the stacked e, J over the union of the nodes, S = blockdiag(Omega^-1) + J Sigma
        J^T, d2 = e^T S^-1 e: (S, d2, floor_S, floor_d2)"""
        sig = self.sigma_pair() if sig is None else sig
        terms = self.candidate_terms(cand)
        S, d2, fS, fd = [], [], 0.0, 0.0
        for members in sets:
            e = np.concatenate([terms[c][0] for c in members])
            D = len(e)
            J = np.zeros((D, self.n))
            C = np.zeros((D, D))
            o = 0
            for c in members:
                ec, Jc, idx, W = terms[c]
                J[o:o + len(ec), idx] = Jc
                C[o:o + len(ec), o:o + len(ec)] = np.linalg.inv(W)
                o += len(ec)
            two = []
            for X in sig:
                P = J @ (0.5 * (X + X.T)) @ J.T
                Sc = C + 0.5 * (P + P.T)
                two.append((Sc, float(e @ np.linalg.solve(Sc, e))))
            S.append(two[0][0]); d2.append(two[0][1])
            fS = max(fS, rel_diff(two[0][0], two[1][0]))
            fd = max(fd, abs(two[0][1] - two[1][1]) / abs(two[1][1]))
        return S, np.array(d2), fS, fd

    def check(self, edges, sig=None):
        """rr_pgo_check_edges restated (no robust kernel): R = Omega^-1 - J Sigma J^T, d2 = e^T R^-1 e, r = trace(R Omega) / d_e:
        (R, d2, redundancy, chi2, floor_R, [floor of d2 per edge], [relative floor of chi2 per edge], [floor of r per edge]).
        The two routes differ in Sigma (LU, Cholesky) and in the
        edge's own terms: the second evaluates e, J and the products in extended precision and rounds R and e once -- R^-1
        amplifies the rounding of e and J by the edge's smallest directional redundancy, which two Sigmas alone do not show."""
        sig = self.sigma_pair() if sig is None else sig
        R, d2, red, chi2, fR, fd, fc, fr = [], [], [], [], 0.0, [], [], []
        for k in edges:
            a, b, e, A, B, W, _ = self.edge_term(k)
            idx = np.concatenate([self.scalars(a), self.scalars(b)])
            two = []
            for X, dtype in zip(sig, (np.float64, np.longdouble)):
                _, _, ex, Ax, Bx, _, _ = self.edge_term(k, dtype)
                J = np.hstack([Ax, Bx])
                s = X[np.ix_(idx, idx)].astype(dtype)
                P = J @ (0.5 * (s + s.T)) @ J.T
                Rc = (np.linalg.inv(W).astype(dtype) - 0.5 * (P + P.T)).astype(np.float64)
                e = ex.astype(np.float64)
                with np.errstate(all="ignore"):
                    try:
                        d = float(e @ np.linalg.solve(Rc, e))
                    except np.linalg.LinAlgError:
                        d = float("nan")
                two.append((Rc, d, float(ex @ W.astype(dtype) @ ex), float(np.trace(Rc @ W)) / len(e)))
            R.append(two[0][0]); d2.append(two[0][1]); chi2.append(two[0][2]); red.append(two[0][3])
            fc.append(abs(two[0][2] - two[1][2]) / two[1][2])
            fr.append(abs(two[0][3] - two[1][3]))
            fR = max(fR, float(np.abs(two[0][0] - two[1][0]).max() / np.abs(np.linalg.inv(W)).max()))
            fd.append(abs(two[0][1] - two[1][1]) / abs(two[1][1]) if np.isfinite(two[0][1]) and np.isfinite(two[1][1]) else float("inf"))
        return R, np.array(d2), np.array(red), np.array(chi2), fR, np.array(fd), np.array(fc), np.array(fr)


__all__ = ["Landmarks3dReference", "se3_edge", "point_edge", "q_mul", "q_conj", "q_to_rot", "q_exp", "unit", "skew",
           "full_info", "split", "rel_diff", "tolerance", "NODE_DIM", "STATE_LEN", "EDGE_DIM", "META_LEN", "INFO_LEN"]
