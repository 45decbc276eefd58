"""CPU reference for 2-D graphs with bearing-only and range-only landmark edges (RR_PGO_EDGE_SE2_BEARING = 4,
RR_PGO_EDGE_SE2_RANGE = 6; include/rr_pgo.h).  numpy f64 throughout and NO oracle: the C oracle does not know the two kinds.
tests/test_bearing_range_cpu.py holds this module to the oracle on a graph without them (H, b, chi2 of
simulation-pose-landmark.g2o) and pins the Jacobians of the two kinds to central differences in 50-digit arithmetic.

The model, restated from the header.  A pose is (t, theta), kept as (x, y, cos, sin) like the library keeps it; a landmark is
l.  Increments are additive: (x, y, theta) and (l_x, l_y).  With d = l - t, p = R(theta)^T d, rho = |d|:
    SE2      e = Log(Z^-1 X1^-1 X2)                        3 scalars (the oracle's pose-pose edge)
    SE2_XY   e = p - z                                      2 scalars (the oracle's pose-landmark edge)
    BEARING  e = wrap(atan2(p_y, p_x) - z) into (-pi, pi]   1 scalar;  A = [d_y, -d_x, -rho^2] / rho^2,  B = [-d_y, d_x] / rho^2
    RANGE    e = rho - z                                    1 scalar;  A = [-d_x, -d_y, 0] / rho,         B = [d_x, d_y] / rho
The system is H = sum w J^T Omega J (+ 1e7 I on the anchor's block, + lambda I under Levenberg-Marquardt), b = -sum w J^T Omega e,
w the robust weight (tests/robust_reference.py) of a robustified edge or prior and 1 otherwise; a prior is the edge of the
node's own kind from a fixed identity pose (tests/priors_reference.py); a fixed node has an identity block, zero blocks to
everything else and b = 0, and every free row is what it is without the fixed set (tests/fixed_reference.py).  Either
keep_anchor = 0 drops the anchor term.  Sigma is the inverse of the free part of H, computed twice (LU inverse, Cholesky
solve) and embedded with zeros at the fixed nodes: the disagreement of the two is the noise floor of every query, and a GPU
value passes at marginals_reference.tolerance(floor) = max(1e-12, 100 x floor)."""
import numpy as np

from marginals_reference import rel_diff, tolerance
from robust_reference import rho, weight

SE2, SE2_XY, BEARING, RANGE = 0, 1, 4, 6
EDGE_DIM = {0: 3, 1: 2, 4: 1, 6: 1}
META_LEN = {0: 3, 1: 2, 4: 1, 6: 1}
INFO_LEN = {0: 6, 1: 3, 4: 1, 6: 1}
NODE_DIM = {0: 3, 1: 2}
MIN_REDUNDANCY = 0.01   # tests/check_edges_reference.py
FLOOR_MAX = 1e-6        # tests/covariances_cases.py


def split(kinds, packed, length):
    out, o = [], 0
    for k in kinds:
        out.append(np.asarray(packed[o:o + length[int(k)]], np.float64))
        o += length[int(k)]
    assert o == len(packed), (o, len(packed))
    return out


def full_info(kind, packed):
    d = EDGE_DIM[int(kind)]
    m = np.zeros((d, d))
    m[np.triu_indices(d)] = packed
    return m + np.triu(m, 1).T


def pack_pose(kind, s):
    return np.array([s[0], s[1], np.cos(s[2]), np.sin(s[2])]) if int(kind) == 0 else np.array([s[0], s[1], 0.0, 0.0])


IDENTITY = np.array([0.0, 0.0, 1.0, 0.0])


def edge_terms(kind, x1, x2, z):
    """(e, A, B) of one edge: x1 the pose (x, y, cos, sin), x2 the `to` node in the same form, z the measurement as the
    header packs it (SE2: x, y, theta; SE2_XY: x, y; BEARING: radians; RANGE: metres)"""
    kind = int(kind)
    dx, dy = x2[0] - x1[0], x2[1] - x1[1]
    c, s = x1[2], x1[3]
    if kind == SE2:
        zc, zs = np.cos(z[2]), np.sin(z[2])
        # M = Rz^T R1^T; e_t = M (t2 - t1) - Rz^T z_t; e_theta = angle of M R2
        mc, ms = zc * c - zs * s, -(zc * s + zs * c)
        et = np.array([mc * dx - ms * dy, ms * dx + mc * dy]) - np.array([zc * z[0] + zs * z[1], -zs * z[0] + zc * z[1]])
        eth = np.arctan2(mc * x2[3] + ms * x2[2], mc * x2[2] - ms * x2[3])
        A = np.array([[-mc, ms, mc * dy + ms * dx], [-ms, -mc, ms * dy - mc * dx], [0.0, 0.0, -1.0]])
        B = np.array([[mc, -ms, 0.0], [ms, mc, 0.0], [0.0, 0.0, 1.0]])
        return np.array([et[0], et[1], eth]), A, B
    px, py = c * dx + s * dy, -s * dx + c * dy
    if kind == SE2_XY:
        e = np.array([px - z[0], py - z[1]])
        A = np.array([[-c, -s, py], [s, -c, -px]])
        B = np.array([[c, s], [-s, c]])
        return e, A, B
    r2 = dx * dx + dy * dy
    if kind == BEARING:
        cz, sz = np.cos(z[0]), np.sin(z[0])
        e = np.array([np.arctan2(cz * py - sz * px, cz * px + sz * py)])
        return e, np.array([[dy / r2, -dx / r2, -1.0]]), np.array([[-dy / r2, dx / r2]])
    assert kind == RANGE
    r = np.sqrt(r2)
    return np.array([r - z[0]]), np.array([[-dx / r, -dy / r, 0.0]]), np.array([[dx / r, dy / r]])


def edge_s_mp(kind, s1, s2, z, omega, dps=50):
    """e^T Omega e of one edge in `dps`-digit arithmetic, from the states as the header packs them (pose: x, y, theta)"""
    import mpmath as mp
    with mp.workdps(dps):
        f = lambda v: [mp.mpf(float(t)) for t in v]
        s1, s2, z = f(s1), f(s2), f(z)
        c, s = mp.cos(s1[2]), mp.sin(s1[2])
        dx, dy = s2[0] - s1[0], s2[1] - s1[1]
        px, py = c * dx + s * dy, -s * dx + c * dy
        kind = int(kind)
        if kind == SE2:
            zc, zs = mp.cos(z[2]), mp.sin(z[2])
            qx, qy = px - z[0], py - z[1]
            a = s2[2] - s1[2] - z[2]
            e = [zc * qx + zs * qy, -zs * qx + zc * qy, mp.atan2(mp.sin(a), mp.cos(a))]
        elif kind == SE2_XY:
            e = [px - z[0], py - z[1]]
        elif kind == BEARING:
            a = mp.atan2(py, px) - z[0]
            e = [mp.atan2(mp.sin(a), mp.cos(a))]
        else:
            e = [mp.sqrt(dx * dx + dy * dy) - z[0]]
        W = [[mp.mpf(float(omega[i][j])) for j in range(len(e))] for i in range(len(e))]
        return float(sum(e[i] * W[i][j] * e[j] for i in range(len(e)) for j in range(len(e))))


class BearingRangeReference:
    """arrays: rr_pgo_graph_desc packing; priors: (node, meas, info) or (node, meas, info, robust) of rr_pgo_set_priors, with
    keep_anchor; fixed: node indices of rr_pgo_set_fixed, with fixed_keep_anchor; kind / delta / edge_mask: the robust kernel."""

    def __init__(self, arrays, priors=None, keep_anchor=True, fixed=(), fixed_keep_anchor=True, kind=None, delta=1.0, edge_mask=None):
        nk, ns, ek, ef, et, em, ei = [np.asarray(a) for a in arrays]
        self.arrays = [nk.astype(np.int32), ns.astype(np.float64), ek.astype(np.int32), ef.astype(np.int32), et.astype(np.int32),
                       em.astype(np.float64), ei.astype(np.float64)]
        self.nk, self.ek, self.ef, self.et = self.arrays[0], self.arrays[2], self.arrays[3], self.arrays[4]
        self.N, self.E = len(nk), len(ek)
        self.dims = np.array([NODE_DIM[int(k)] for k in nk], np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(self.dims)])[:-1].astype(np.int64)
        self.soff = self.offsets          # a 2-D node's state has as many scalars as its step
        self.n = int(self.dims.sum())
        self.z = split(ek, em, META_LEN)
        self.omega = [full_info(k, w) for k, w in zip(ek, split(ek, ei, INFO_LEN))]
        pp = np.flatnonzero(ek == SE2)
        self.anchor = int(ef[pp[0]]) if len(pp) else -1
        self.set_state(ns)
        # priors
        if priors is None:
            priors = (np.zeros(0, np.int32), np.zeros(0), np.zeros(0), None)
        pn, pm, pw, prob = (list(priors) + [None])[:4]
        self.prior_node = np.asarray(pn, np.int64)
        self.P = len(self.prior_node)
        pk = self.nk[self.prior_node] if self.P else np.zeros(0, np.int32)
        self.prior_z = split(pk, pm, META_LEN)
        self.prior_omega = [full_info(k, w) for k, w in zip(pk, split(pk, pw, INFO_LEN))]
        self.prior_robust = np.zeros(self.P, bool) if prob is None else np.asarray(prob) != 0
        self.fixed = np.unique(np.asarray(fixed, np.int64))
        self.keep_anchor = bool(keep_anchor or self.P == 0) and bool(fixed_keep_anchor or len(self.fixed) == 0)
        is_fixed = np.zeros(self.n, bool)
        for v in self.fixed:
            is_fixed[self.scalars(v)] = True
        self.fixed_scalars, self.free = np.flatnonzero(is_fixed), np.flatnonzero(~is_fixed)
        self.kind, self.delta = kind, float(delta)
        self.mask = np.zeros(self.E, bool) if kind is None else (np.ones(self.E, bool) if edge_mask is None else np.asarray(edge_mask) != 0)
        if kind is None:
            self.prior_robust[:] = False

    # ---- state
    def scalars(self, v):
        return np.arange(self.offsets[v], self.offsets[v] + self.dims[v])

    def set_state(self, state):
        state = np.asarray(state, np.float64)
        self.x = [pack_pose(self.nk[v], state[self.soff[v]:self.soff[v] + self.dims[v]]) for v in range(self.N)]

    def state(self):
        out = []
        for v in range(self.N):
            x = self.x[v]
            out.extend([x[0], x[1], np.arctan2(x[3], x[2])] if self.nk[v] == 0 else [x[0], x[1]])
        return np.array(out)

    def update(self, dx, sign=1.0):
        """og_update_nodes: additive, the rotation multiplied by (cos, sin) of the step, no renormalisation; fixed nodes stay"""
        fx = set(self.fixed.tolist())
        for v in range(self.N):
            if v in fx:
                continue
            d = sign * np.asarray(dx)[self.scalars(v)]
            x = self.x[v].copy()
            x[0] += d[0]
            x[1] += d[1]
            if self.nk[v] == 0:
                c, s = np.cos(d[2]), np.sin(d[2])
                x[2], x[3] = x[2] * c - x[3] * s, x[2] * s + x[3] * c
            self.x[v] = x

    # ---- terms
    def lin(self, k):
        return edge_terms(self.ek[k], self.x[self.ef[k]], self.x[self.et[k]], self.z[k])

    def prior_lin(self, p):
        v = self.prior_node[p]
        e, _, B = edge_terms(self.nk[v], IDENTITY, self.x[v], self.prior_z[p])   # the edge of the node's own kind
        return e, B

    def edge_s(self):
        return np.array([float(e @ W @ e) for W, e in ((self.omega[k], self.lin(k)[0]) for k in range(self.E))])

    def edge_s_mp(self):
        st = self.state()
        return np.array([edge_s_mp(self.ek[k], st[self.soff[self.ef[k]]:][:3], st[self.soff[self.et[k]]:][:NODE_DIM[int(self.nk[self.et[k]])]],
                                   self.z[k], self.omega[k]) for k in range(self.E)])

    def prior_s(self):
        return np.array([float(e @ W @ e) for W, e in ((self.prior_omega[p], self.prior_lin(p)[0]) for p in range(self.P))])

    def edge_errors(self):
        s = self.edge_s()
        return s, np.where(self.mask, weight(self.kind, s, self.delta), 1.0)

    def prior_errors(self):
        s = self.prior_s()
        return s, np.where(self.prior_robust, weight(self.kind, s, self.delta), 1.0) if self.P else np.zeros(0)

    def cost(self):
        s, ps = self.edge_s(), self.prior_s()
        return float(np.sum(np.where(self.mask, rho(self.kind, s, self.delta), s)) +
                     (np.sum(np.where(self.prior_robust, rho(self.kind, ps, self.delta), ps)) if self.P else 0.0))

    # ---- the system
    def full_system(self, lam=0.0, lm=False):
        """(H, b) over all nodes before the fixed set overrules anything"""
        H, b = np.zeros((self.n, self.n)), np.zeros(self.n)
        _, w = self.edge_errors()
        for k in range(self.E):
            e, A, B = self.lin(k)
            W = w[k] * self.omega[k]
            i, j = self.scalars(self.ef[k]), self.scalars(self.et[k])
            H[np.ix_(i, i)] += A.T @ W @ A
            H[np.ix_(j, j)] += B.T @ W @ B
            H[np.ix_(i, j)] += A.T @ W @ B
            H[np.ix_(j, i)] += B.T @ W @ A
            b[i] -= A.T @ W @ e
            b[j] -= B.T @ W @ e
        if self.P:
            _, pw = self.prior_errors()
            for p in range(self.P):
                e, B = self.prior_lin(p)
                W = pw[p] * self.prior_omega[p]
                j = self.scalars(self.prior_node[p])
                H[np.ix_(j, j)] += B.T @ W @ B
                b[j] -= B.T @ W @ e
        if self.keep_anchor and self.anchor >= 0:
            i = self.scalars(self.anchor)
            H[i, i] += 1e7
        if lm:
            H[np.arange(self.n), np.arange(self.n)] += lam
        return H, b

    def system(self, lam=0.0, lm=False):
        """(H, b) as the handle assembles it: identity rows at the fixed nodes, zero blocks to them, b = 0 there"""
        H, b = self.full_system(lam, lm)
        f = self.fixed_scalars
        H[f, :] = 0.0
        H[:, f] = 0.0
        H[f, f] = 1.0
        b[f] = 0.0
        return H, b

    def free_system(self, lam=0.0, lm=False):
        H, b = self.full_system(lam, lm)
        return H[np.ix_(self.free, self.free)], b[self.free]

    def step(self, lam=0.0, lm=False):
        """dx over all nodes: a dense Cholesky solve of the free part, zeros at the fixed nodes"""
        H, b = self.free_system(lam, lm)
        L = np.linalg.cholesky(H)
        dx = np.zeros(self.n)
        dx[self.free] = np.linalg.solve(L.T, np.linalg.solve(L, b))
        return dx

    def optimize(self, num_iterations, lm=False):
        """the reference loop (:247-303): (errors, norms); stops when |dx| < 1e-4"""
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

    # ---- queries: Sigma twice, zeros at the fixed nodes
    def sigma_pair(self):
        H, _ = self.free_system(0.0, False)
        A = np.linalg.inv(H)
        L = np.linalg.cholesky(H)
        B = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(len(self.free))))
        out = []
        for X in (A, B):
            full = np.zeros((self.n, self.n))
            full[np.ix_(self.free, self.free)] = 0.5 * (X + X.T)
            out.append(full)
        return tuple(out)

    def blocks(self, node_a, node_b, sig):
        """([Sigma(a_q, b_q)], noise floor over the blocks)"""
        out, floor = [], 0.0
        for a, b in zip(node_a, node_b):
            X, Y = (S[np.ix_(self.scalars(a), self.scalars(b))] for S in sig)
            out.append(X.copy())
            if np.any(Y != 0.0):
                floor = max(floor, rel_diff(X, Y))
        return out, floor

    def cand_terms(self, cand):
        kind, a, b, meas, info = cand
        z = split(kind, meas, META_LEN)
        om = [full_info(k, w) for k, w in zip(kind, split(kind, info, INFO_LEN))]
        return [(edge_terms(kind[c], self.x[a[c]], self.x[b[c]], z[c]), om[c]) for c in range(len(kind))]

    def cand_s_mp(self, cand):
        """e^T Omega e of every candidate in 50-digit arithmetic: what the gate's chi2 takes its floor from"""
        kind, a, b, meas, info = cand
        z = split(kind, meas, META_LEN)
        om = [full_info(k, w) for k, w in zip(kind, split(kind, info, INFO_LEN))]
        st = self.state()
        return np.array([edge_s_mp(kind[c], st[self.soff[a[c]]:][:3], st[self.soff[b[c]]:][:self.dims[b[c]]], z[c], om[c]) for c in range(len(kind))])

    def gate(self, cand, sig):
        """rr_pgo_gate_edges restated: (S, d2, chi2, floor_S, floor_d2)"""
        _, a, b, _, _ = cand
        S, d2, chi2, fS, fd = [], [], [], 0.0, 0.0
        for c, ((e, A, B), W) in enumerate(self.cand_terms(cand)):
            J = np.hstack([A, B])
            idx = np.concatenate([self.scalars(a[c]), self.scalars(b[c])])
            two = []
            for X in sig:
                P = J @ X[np.ix_(idx, idx)] @ J.T
                Sc = np.linalg.inv(W) + 0.5 * (P + P.T)
                two.append((Sc, float(e @ np.linalg.solve(Sc, e))))
            S.append(two[0][0]); d2.append(two[0][1]); chi2.append(float(e @ W @ e))
            fS = max(fS, rel_diff(two[0][0], two[1][0]))
            fd = max(fd, abs(two[0][1] - two[1][1]) / abs(two[1][1]))
        return S, np.array(d2), np.array(chi2), fS, fd

    def gate_joint(self, cand, sets, sig):
        """rr_pgo_gate_joint restated: (d2 per set, floor)"""
        _, a, b, _, _ = cand
        terms = self.cand_terms(cand)
        d2, floor = [], 0.0
        for members in sets:
            D = sum(len(terms[c][0][0]) for c in members)
            J, R, e, r = np.zeros((D, self.n)), np.zeros((D, D)), np.zeros(D), 0
            for c in members:
                (e_, A_, B_), W = terms[c]
                d = len(e_)
                J[r:r + d, self.scalars(a[c])] += A_
                J[r:r + d, self.scalars(b[c])] += B_
                R[r:r + d, r:r + d] = np.linalg.inv(W)
                e[r:r + d] = e_
                r += d
            two = []
            for X in sig:
                P = J @ X @ J.T
                two.append(float(e @ np.linalg.solve(R + 0.5 * (P + P.T), e)))
            d2.append(two[0])
            floor = max(floor, abs(two[0] - two[1]) / abs(two[1]))
        return np.array(d2), floor

    def check(self, edges, sig):
        """rr_pgo_check_edges restated (tests/check_edges_reference.py): per edge R = Omega^-1 / w - J Sigma J^T, d2 = e^T R^-1 e,
        r = trace(R w Omega) / d_e and r_min, each from both Sigmas.  A dict with the values of the first, `compared` (r at least
        MIN_REDUNDANCY: d2 and R mean something), `singular` (r_min zero within its floor: d2 does not) and the floors."""
        _, w = self.edge_errors()
        two = []
        for X in sig:
            rows = []
            for k in edges:
                e, A, B = self.lin(k)
                J = np.hstack([A, B])
                idx = np.concatenate([self.scalars(self.ef[k]), self.scalars(self.et[k])])
                P = J @ X[np.ix_(idx, idx)] @ J.T
                Om = w[k] * self.omega[k]
                R = np.linalg.inv(self.omega[k]) / w[k] - 0.5 * (P + P.T)
                r = float(np.trace(R @ Om) / len(e))
                d2 = float(e @ np.linalg.solve(R, e)) if np.all(np.linalg.eigvalsh(R) > 0) else float("nan")
                L = np.linalg.cholesky(Om)
                rows.append((R, d2, r, float(np.linalg.eigvalsh(L.T @ R @ L)[0])))
            two.append(rows)
        R = [t[0] for t in two[0]]
        d2, r, rmin = (np.array([t[i] for t in two[0]]) for i in (1, 2, 3))
        d2b, rb, rminb = (np.array([t[i] for t in two[1]]) for i in (1, 2, 3))
        floor_r, floor_rmin = float(np.max(np.abs(r - rb))), float(np.max(np.abs(rmin - rminb)))
        compared = r >= MIN_REDUNDANCY
        singular = compared & (rmin <= tolerance(floor_rmin))
        cR, c = np.flatnonzero(compared), np.flatnonzero(compared & ~singular)
        floor_R = max([rel_diff(two[0][q][0], two[1][q][0]) for q in cR], default=0.0)
        with np.errstate(invalid="ignore"):
            floor_d2 = float(np.max(np.abs(d2[c] - d2b[c]) / np.abs(d2b[c]))) if len(c) else 0.0
        return {"R": R, "d2": d2, "r": r, "compared": compared, "singular": singular, "floor_r": floor_r, "floor_R": floor_R,
                "floor_d2": floor_d2, "floor_rmin": floor_rmin}


__all__ = ["BearingRangeReference", "edge_terms", "edge_s_mp", "split", "full_info", "tolerance", "rel_diff", "EDGE_DIM", "META_LEN",
           "INFO_LEN", "NODE_DIM", "MIN_REDUNDANCY", "FLOOR_MAX", "SE2", "SE2_XY", "BEARING", "RANGE"]
