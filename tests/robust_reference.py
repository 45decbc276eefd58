"""CPU reference for the robust kernels (include/rr_pgo.h, "robust kernels"), built on the unchanged oracle.

IRLS as the header defines it: at every linearisation each robustified edge's information matrix is scaled by
w = rho'(s), s = e^T Omega e, and the oracle solves that weighted system; the cost is sum rho(s).  The loop follows
og_optimize (oracle/pgo_oracle.c) statement by statement, with the robust cost in place of chi2.  The formulas are
restated here from the header, not imported from the package.
"""
import ctypes as C

import numpy as np

from oracle.oracle import OracleGraph, lib as oracle_lib

META_LEN = {0: 3, 1: 2, 2: 7}    # packed measurement length by edge kind
INFO_LEN = {0: 6, 1: 3, 2: 21}   # packed (upper triangle) information length by edge kind
EDGE_DIM = {0: 3, 1: 2, 2: 6}


def weight(kind, s, delta):
    s = np.asarray(s, np.float64)
    d2 = delta * delta
    if kind == "huber":
        return np.where(s > d2, delta / np.sqrt(np.where(s > d2, s, 1.0)), 1.0)
    if kind == "cauchy":
        return np.where(s > 0, 1.0 / (1.0 + s / d2), 1.0)
    return np.ones_like(s)


def rho(kind, s, delta):
    s = np.asarray(s, np.float64)
    d2 = delta * delta
    if kind == "huber":
        return np.where(s > d2, 2.0 * delta * np.sqrt(np.where(s > d2, s, 1.0)) - d2, s)
    if kind == "cauchy":
        return np.where(s > 0, d2 * np.log1p(np.where(s > 0, s, 0.0) / d2), s)
    return s.copy()


def oracle_arrays(o):
    """The graph held by OracleGraph `o` in rr_pgo_graph_desc / og_create packing (current state)."""
    L = oracle_lib()
    ek = o.edge_kinds()
    ef, et = o.edge_endpoints()
    meas, info = [], []
    buf = np.zeros(36)
    ptr = buf.ctypes.data_as(C.POINTER(C.c_double))
    for k, kind in enumerate(ek):
        L.og_get_edge_meas(o._h, k, ptr)
        meas.append(buf[:META_LEN[int(kind)]].copy())
        L.og_get_edge_info_full(o._h, k, ptr)
        d = EDGE_DIM[int(kind)]
        full = buf[:d * d].reshape(d, d)
        info.append(full[np.triu_indices(d)].copy())
    return [o.node_kinds(), o.state(), ek, ef, et, np.concatenate(meas), np.concatenate(info)]


def info_full(ek, info_packed):
    """per edge Omega as a 6 x 6 matrix, zero padded (2D edges)"""
    out = np.zeros((len(ek), 6, 6))
    off = 0
    for k, kind in enumerate(ek):
        d, n = EDGE_DIM[int(kind)], INFO_LEN[int(kind)]
        m = np.zeros((d, d))
        m[np.triu_indices(d)] = info_packed[off:off + n]
        out[k, :d, :d] = m + np.triu(m, 1).T
        off += n
    return out


class RobustReference:
    """Robust Gauss-Newton / Levenberg-Marquardt on the oracle.  `arrays`: og_create packing; `mask`: per edge,
    nonzero = robustified (None: every edge); kind None runs plain least squares through the same loop."""

    def __init__(self, arrays, kind, delta=1.0, mask=None):
        self.arrays = [np.asarray(a) for a in arrays]
        self.kind, self.delta = kind, float(delta)
        self.g = OracleGraph.from_arrays(*self.arrays)
        ek = self.arrays[2]
        self.m = len(ek)
        self.omega = info_full(ek, self.arrays[6])
        self.info_rep = np.repeat(np.arange(self.m), [INFO_LEN[int(k)] for k in ek])
        self.mask = np.ones(self.m, bool) if mask is None else np.asarray(mask) != 0
        self._e = np.zeros(6)
        self._a = np.zeros(36)
        self._b = np.zeros(36)

    def edge_s(self):
        """s_e = e^T Omega e of every edge at the current state (e from og_linearize_edge)"""
        L, h = oracle_lib(), self.g._h
        E = np.zeros((self.m, 6))
        pe, pa, pb = (x.ctypes.data_as(C.POINTER(C.c_double)) for x in (self._e, self._a, self._b))
        for k in range(self.m):
            self._e[:] = 0.0
            L.og_linearize_edge(h, k, pa, pb, pe)
            E[k] = self._e
        return np.einsum("ki,kij,kj->k", E, self.omega, E)

    def weights(self, s):
        return np.where(self.mask, weight(self.kind, s, self.delta), 1.0)

    def cost_terms(self, s):
        return np.where(self.mask, rho(self.kind, s, self.delta), s)

    def cost(self):
        return float(np.sum(self.cost_terms(self.edge_s())))

    def weighted_graph(self):
        """the oracle graph at the current state with every robustified edge's Omega scaled by its weight"""
        w = self.weights(self.edge_s())
        a = list(self.arrays)
        a[1] = self.g.state()
        a[6] = self.arrays[6] * w[self.info_rep]
        return OracleGraph.from_arrays(*a), w

    def optimize(self, num_iterations, lm=False):
        """og_optimize with sum rho in place of chi2: (errors, norms)"""
        tolerance, lam = 1e-4, 0.01
        last_error = self.cost()
        errors, norms = [last_error], []
        for _ in range(num_iterations):
            gw, _ = self.weighted_graph()
            dx = gw.linearize_and_solve(lam, lm)
            self.g.update_nodes(dx, 1.0)
            nrm = float(np.sqrt(np.dot(dx, dx)))
            error = self.cost()
            if lm:
                if last_error < error:
                    self.g.update_nodes(dx, -1.0)
                    lam *= 2.0
                else:
                    lam /= 2.0
            last_error = error
            norms.append(nrm)
            errors.append(error)
            if nrm < tolerance:
                break
        return np.array(errors), np.array(norms)

    def state(self):
        return self.g.state()


def intel_with_outliers(intel_path, K=50, seed=1):
    """intel.g2o + K false loop closures (the generator of the robust-kernel issue): node pairs from
    rng.integers(0, n, 2) with |i - j| > 50, measurements x, y ~ U(-3, 3), theta ~ U(-pi, pi), Omega = the element-wise
    median of the packed Omega of the file's loop closures (|from - to| > 1), appended after the file's edges.
    Returns (arrays of the clean file, arrays with the outliers)."""
    o = OracleGraph.load(intel_path)
    clean = oracle_arrays(o)
    nk, ns, ek, ef, et, em, ei = clean
    n = len(nk)
    rng = np.random.default_rng(seed)
    pairs = []
    while len(pairs) < K:
        i, j = rng.integers(0, n, 2)
        if abs(int(i) - int(j)) > 50:
            pairs.append((int(i), int(j)))
    xy = rng.uniform(-3, 3, (K, 2))
    th = rng.uniform(-np.pi, np.pi, K)
    assert np.all(ek == 0)
    info = ei.reshape(-1, 6)
    loops = np.abs(ef - et) > 1
    med = np.median(info[loops], axis=0)
    pf = np.array([p[0] for p in pairs], np.int32)
    pt = np.array([p[1] for p in pairs], np.int32)
    outl = [nk, ns, np.concatenate([ek, np.zeros(K, np.int32)]), np.concatenate([ef, pf]), np.concatenate([et, pt]),
            np.concatenate([em, np.column_stack([xy, th]).ravel()]), np.concatenate([ei, np.tile(med, K)])]
    return clean, outl


def position_error(state_a, state_b, node_kind):
    """max Euclidean distance between the positions of two SE(2) / XY state vectors"""
    lens = np.where(node_kind == 0, 3, 2)
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    pa = np.stack([state_a[offs], state_a[offs + 1]], 1)
    pb = np.stack([state_b[offs], state_b[offs + 1]], 1)
    return float(np.sqrt(((pa - pb) ** 2).sum(1)).max())
