"""CPU reference for rr_pgo_cross_covariances (include/rr_pgo.h, "covariances"), built on tests/marginals_reference.py.

The reference of a column node b is the block column Sigma[:, b], dim x d_b, by MarginalsReference's two independent f64
computations (`_columns`): R_b and R'_b.  floor_b = max|R_b - R'_b| / max|R_b|; the floor of a comparison is the maximum
over its column nodes and must be at most FLOOR_MAX (tests/covariances_cases.py).

The rule.  A GPU column block G_b (the rows asked for x the columns of b) passes when
    max|G_b - R_b| / max|R_b| <= tolerance(floor) = max(1e-12, 100 x floor),
max|R_b| being the maximum of the WHOLE column over all rows, also when only some rows are asked for: it is what a backward
solve bounds (the error of X = L^-T Z is normwise in the column, not in a block of it).  This is the project's existing
rule with the column as the unit.  Every comparison prints its worst figure, the floor, the tolerance and the worst
per-(row node, column node) block relative difference before it asserts; the per-block figure is printed, not asserted.

With priors or fixed nodes the two Sigmas of PriorsReference / FixedReference (`sigma_pair`) take the place of `_columns`:
CrossReference.from_sigma_pair.  A fixed node's rows and columns are zero in both; such a column has no scale and is left
out of the normwise comparison (the GPU test asserts its zeros by themselves).
"""
import numpy as np

from covariances_cases import FLOOR_MAX
from marginals_reference import NODE_DIM, tolerance


class CrossReference:
    """columns(nodes) -> (R, R') of the distinct nodes; offsets / dims: first scalar and size of every node"""

    def __init__(self, columns, offsets, dims):
        self._columns = columns
        self.offsets = np.asarray(offsets, np.int64)
        self.dims = np.asarray(dims, np.int64)
        self.dim = int(np.sum(self.dims))

    @classmethod
    def from_marginals(cls, ref):
        """ref: a MarginalsReference (its LU pair or its dense pair, whichever it uses)"""
        def columns(nodes):
            XA, XB, pos = ref._columns(nodes)
            return np.asarray(XA), np.asarray(XB), pos
        return cls(columns, ref.offsets, ref.dims)

    @classmethod
    def from_sigma_pair(cls, sig, node_kinds):
        """sig: the two full Sigmas of PriorsReference.sigma_pair / FixedReference.sigma_pair"""
        dims = np.array([NODE_DIM[int(k)] for k in node_kinds], np.int64)
        offsets = np.concatenate([[0], np.cumsum(dims)])[:-1]
        n = int(np.sum(dims))

        def columns(nodes):
            nodes = sorted(set(int(v) for v in nodes))
            pos, cols = {}, []
            for v in nodes:
                pos[v] = len(cols)
                cols.extend(range(offsets[v], offsets[v] + dims[v]))
            cols = np.array(cols, int)
            return sig[0][:n, cols], sig[1][:n, cols], pos
        return cls(columns, offsets, dims)

    def scalars(self, v):
        return np.arange(self.offsets[v], self.offsets[v] + self.dims[v])

    def row_scalars(self, rows):
        """the scalars of the row nodes stacked in order (None: every node: 0 .. dim)"""
        if rows is None:
            return np.arange(self.dim)
        return np.concatenate([self.scalars(int(v)) for v in rows]).astype(int) if len(rows) else np.zeros(0, int)

    def full_columns(self, cols):
        """(R, R', per column node: (node, first column, floor_b, max|R_b|)) -- dim x C, the columns in the order of `cols`,
        repeats included"""
        XA, XB, pos = self._columns(cols)
        take, info, c0 = [], [], 0
        for b in cols:
            b = int(b)
            cs = np.arange(pos[b], pos[b] + self.dims[b])
            A, B = XA[:, cs], XB[:, cs]
            scale = float(np.max(np.abs(A))) if A.size else 0.0
            floor = float(np.max(np.abs(A - B)) / scale) if scale > 0 else 0.0
            info.append((b, c0, floor, scale))
            take.extend(cs)
            c0 += int(self.dims[b])
        take = np.array(take, int)
        return XA[:, take], XB[:, take], info

    def block(self, rows, cols):
        """(Sigma[rows, cols] by the first computation, the floor of the comparison)"""
        R, _, info = self.full_columns(cols)
        return R[self.row_scalars(rows)], max([f for _, _, f, _ in info], default=0.0)

    def floors(self, cols):
        return [f for _, _, f, _ in self.full_columns(cols)[2]]


def check_columns(label, G, ref, rows, cols, full=None):
    """the rule of this file's docstring on G = cross_covariance(rows, cols); returns (worst, floor, tolerance).
    full: full_columns(cols) if the caller has it already."""
    R, _, info = ref.full_columns(cols) if full is None else full
    rs = ref.row_scalars(rows)
    want = R[rs]
    G = np.asarray(G)
    assert G.shape == want.shape, (label, G.shape, want.shape)
    floor = max([f for _, _, f, _ in info], default=0.0)
    tol = tolerance(floor)
    row_nodes = range(len(ref.dims)) if rows is None else [int(v) for v in rows]
    ro = np.concatenate([[0], np.cumsum([ref.dims[v] for v in row_nodes])]).astype(int)
    worst, worst_block, skipped = 0.0, 0.0, 0
    for b, c0, _, scale in info:
        cs = slice(c0, c0 + int(ref.dims[b]))
        if scale == 0.0:   # a fixed node's column: no scale; its zeros are the caller's to assert
            skipped += 1
            continue
        D = np.abs(G[:, cs] - want[:, cs])
        worst = max(worst, float(np.max(D)) / scale if D.size else 0.0)
        for k in range(len(row_nodes)):
            blk = np.abs(want[ro[k]:ro[k + 1], cs])
            if blk.size and np.max(blk) > 0:
                worst_block = max(worst_block, float(np.max(D[ro[k]:ro[k + 1]]) / np.max(blk)))
    print(f"{label}: {G.shape[0]} x {G.shape[1]} scalars, {len(info)} column nodes ({skipped} without scale), worst column relative "
          f"difference {worst:.3g}, noise floor {floor:.3g}, tolerance {tol:.3g}; worst per-block relative difference {worst_block:.3g} (not asserted)")
    assert floor <= FLOOR_MAX, (label, floor)
    assert worst <= tol, (label, worst, tol)
    return worst, floor, tol
