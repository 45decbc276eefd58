"""CPU reference for rr_pgo_marginals (include/rr_pgo.h, "marginal covariances"), built on the unchanged oracle.

H is the oracle's normal matrix at the oracle graph's state (`OracleGraph.build_system(0, False)`: anchor prior included,
lambda = 0); Sigma = H^-1.  Two independent f64 computations of the queried blocks give the reference and the file's
NOISE FLOOR -- the worst per-block relative difference between the two, relative difference of a block = max|A - B| /
max|B|.  With SciPy: two sparse LU factorisations with different column orderings, solving for the unit columns of the
queried nodes.  Without it: a dense LU inverse against a dense Cholesky inverse (numpy only).

The tolerance of a GPU block is tolerance(floor) = max(1e-12, 100 x floor): the floor comes from the reference alone.
"""
import numpy as np

from oracle.oracle import OracleGraph

try:
    import scipy.sparse as _sp
    import scipy.sparse.linalg as _spla
except ImportError:   # keep a dense numpy route
    _sp = _spla = None

DENSE_MAX_DIM = 5184
NODE_DIM = {0: 3, 1: 2, 2: 6}


def rel_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def tolerance(floor):
    return max(1e-12, 100.0 * floor)


def graph_at_state(arrays, state):
    """OracleGraph of og_create arrays with the node states replaced by `state`"""
    a = list(arrays)
    a[1] = np.asarray(state, np.float64)
    return OracleGraph.from_arrays(*a)


class MarginalsReference:
    def __init__(self, oracle_graph, force_dense=False):
        o = self.o = oracle_graph
        self.n = o.dim
        self.offsets = o.node_offsets()
        self.dims = np.array([NODE_DIM[int(k)] for k in o.node_kinds()], np.int32)
        colptr, rowidx, vals, _ = o.build_system(0.0, False)
        cols = np.repeat(np.arange(self.n), np.diff(colptr))
        self.dense = force_dense or _sp is None or self.n <= DENSE_MAX_DIM
        if self.dense:
            H = np.zeros((self.n, self.n))
            H[rowidx, cols] = vals
            self.H = H + np.tril(H, -1).T
        else:
            low = _sp.csc_matrix((vals, rowidx, colptr), shape=(self.n, self.n))
            self.H = (low + _sp.tril(low, -1).T).tocsc()
        self._inv = None

    def scalars(self, node):
        return np.arange(self.offsets[node], self.offsets[node] + self.dims[node])

    def _columns(self, nodes):
        """(Sigma[:, cols] by method A, by method B, position of every node's first column)"""
        nodes = sorted(set(int(v) for v in nodes))
        pos, cols = {}, []
        for v in nodes:
            pos[v] = len(cols)
            cols.extend(self.scalars(v))
        cols = np.array(cols)
        if self.dense:
            if self._inv is None:
                A = np.linalg.inv(self.H)
                L = np.linalg.cholesky(self.H)
                Li = np.linalg.solve(L, np.eye(self.n))
                self._inv = (A, Li.T @ Li)
            return self._inv[0][:, cols], self._inv[1][:, cols], pos
        E = np.zeros((self.n, len(cols)))
        E[cols, np.arange(len(cols))] = 1.0
        XA = _spla.splu(self.H, permc_spec="COLAMD").solve(E)
        XB = _spla.splu(self.H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0).solve(E)
        return XA, XB, pos

    def blocks(self, node_a, node_b=None):
        """([Sigma(a_q, b_q)], noise floor over these blocks)"""
        node_a = [int(v) for v in node_a]
        node_b = node_a if node_b is None else [int(v) for v in node_b]
        XA, XB, pos = self._columns(node_b)
        out, floor = [], 0.0
        for a, b in zip(node_a, node_b):
            rows = self.scalars(a)
            cs = slice(pos[b], pos[b] + self.dims[b])
            A, B = XA[rows, cs], XB[rows, cs]
            if a == b:   # the result is symmetric: use that
                A, B = 0.5 * (A + A.T), 0.5 * (B + B.T)
            out.append(A.copy())
            floor = max(floor, rel_diff(A, B))
        return out, floor

    def joint(self, a, b):
        (saa, sbb, sab), floor = self.blocks([a, b, a], [a, b, b])
        return np.block([[saa, sab], [sab.T, sbb]]), floor
