"""CPU reference for rr_pgo_initialize (include/rr_pgo.h, "initialisation from the measurements"): the chordal relaxation,
stated in numpy / scipy.sparse from the header's definition and independent of the device code.

    chordal_initialize(arrays, state=None, held=(), priors=None) -> (state, info)

arrays: rr_pgo_graph_desc packing (node_kind, node_state, edge_kind, edge_from, edge_to, edge_meas, edge_info); state: the
current state in node_state's packing (None: the arrays' own) -- only the HELD nodes' entries are read; held: node indices
(the fixed set plus, where it is kept, the anchor); priors: (node, meas, info) as rr_pgo_set_priors takes them.

Every stage is written as a weighted linear least-squares problem  min |A X - B|^2  over the free nodes' unknowns, with the
held nodes' values moved into B; it is solved by the normal equations A^T A X = A^T B (SciPy's sparse LU).  The rotation stage
solves the d rows of every M_i as d right-hand sides of one matrix; the projection is numpy's SVD.

info: "M" (per node: the relaxed d x d matrix of a free pose, in 2-D the vector u; None otherwise), "R" (the rotations),
"margin" (3-D: the smallest (s2 + sign(det M) s3) / s1 over the free poses, s1 >= s2 >= s3 the singular values of M -- the
nearest rotation is unique exactly when it is positive, and its sensitivity grows like its inverse; with det M < 0 it is the
relative gap of the two smallest singular values, with det M > 0 the projection is the polar factor and equal singular values
do no harm: a pose with a single edge to a held or well-determined neighbour has s1 = s2 = s3), "u_min" (2-D: the smallest |u|).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

STATE_LEN = {0: 3, 1: 2, 2: 7, 3: 3}
MEAS_LEN = {0: 3, 1: 2, 2: 7, 3: 3, 4: 1, 6: 1}
INFO_LEN = {0: 6, 1: 3, 2: 21, 3: 6, 4: 1, 6: 1}
EDGE_DIM = {0: 3, 1: 2, 2: 6, 3: 3, 4: 1, 6: 1}
POSE_KINDS, LANDMARK_KINDS = (0, 2), (1, 3)
PRIOR_EDGE_KIND = {0: 0, 1: 1, 2: 2, 3: 3}   # a prior is packed as the edge of its node's kind


def quat_to_rot(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rot_to_quat(R):
    """unit quaternion (x, y, z, w) with w >= 0, through the eigenvector of the largest eigenvalue of Bar-Itzhack's matrix"""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K)
    q = v[:, -1]
    return q if q[3] >= 0 else -q


def rot2(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s], [s, c]])


def full_info(d, packed):
    m = np.zeros((d, d))
    m[np.triu_indices(d)] = packed
    return m + np.triu(m, 1).T


def split(kinds, packed, length):
    out, o = [], 0
    for k in kinds:
        out.append(np.asarray(packed[o:o + length[int(k)]], np.float64))
        o += length[int(k)]
    assert o == len(packed), (o, len(packed))
    return out


def unpack_measurement(kind, m):
    """(t, R) of a pose-kind measurement or state; (t, None) of a point-kind one"""
    if kind == 0:
        return m[:2], rot2(m[2])
    if kind == 2:
        return m[:3], quat_to_rot(m[3:7])
    return np.asarray(m, np.float64), None


def project_so(M):
    """R = U diag(1, .., det(U V^T)) V^T: the nearest rotation in the Frobenius norm"""
    U, s, Vt = np.linalg.svd(M)
    D = np.eye(len(s))
    D[-1, -1] = np.linalg.det(U @ Vt)
    return U @ D @ Vt, s


class _LeastSquares:
    """min |A X - B|^2 with block rows appended one by one; unknown blocks of width d per free node"""

    def __init__(self, col_of, d, n_rhs):
        self.col_of, self.d, self.n_rhs = col_of, d, n_rhs
        self.rows, self.cols, self.vals, self.b, self.m = [], [], [], [], 0

    def add(self, terms, const):
        """one block row: sum over (node, matrix, known value or None) of matrix @ x_node, minus const (rows x n_rhs);
        a term of a held node carries its value (d x n_rhs) and moves to the right"""
        const = np.array(const, np.float64)
        r = const.shape[0]
        for node, mat, value in terms:
            if value is not None:
                const = const - mat @ value
                continue
            c0 = self.col_of[node]
            for i in range(r):
                for j in range(self.d):
                    self.rows.append(self.m + i); self.cols.append(c0 + j); self.vals.append(mat[i, j])
        self.b.append(const)
        self.m += r

    def solve(self, n_cols):
        A = sp.csr_matrix((self.vals, (self.rows, self.cols)), shape=(self.m, n_cols))
        B = np.vstack(self.b)
        H = (A.T @ A).tocsc()
        return spla.splu(H).solve(A.T @ B)


def chordal_initialize(arrays, state=None, held=(), priors=None):
    nk, ns, ek, ef, et, em, ei = [np.asarray(a) for a in arrays]
    state = np.asarray(ns if state is None else state, np.float64)
    N = len(nk)
    d = 3 if np.any(nk >= 2) else 2
    pose_kind = 2 if d == 3 else 0
    held = set(int(v) for v in held)
    cur = [unpack_measurement(int(k), s) for k, s in zip(nk, split(nk, state, STATE_LEN))]
    meas, infos = split(ek, em, MEAS_LEN), split(ek, ei, INFO_LEN)
    pr = []
    if priors is not None and len(priors[0]):
        pn = np.asarray(priors[0], np.int32)
        pk = [PRIOR_EDGE_KIND[int(nk[v])] for v in pn]
        pr = list(zip(pn, pk, split(pk, priors[1], MEAS_LEN), split(pk, priors[2], INFO_LEN)))
    is_pose = [int(k) in POSE_KINDS for k in nk]

    # ---- 1. rotations, relaxed: the rows of M_i as columns rho, every edge says rho_j = A rho_i
    # (3-D: A = R_ij^T; 2-D: u = (cos, sin) and A = Rot(theta_ij), one "row")
    free_pose = [i for i in range(N) if is_pose[i] and i not in held]
    col = {v: d * c for c, v in enumerate(free_pose)}
    n_rhs = d if d == 3 else 1

    def known_rot(i):   # a held pose's rows as columns (d x n_rhs)
        R = cur[i][1]
        return R.T.copy() if d == 3 else R[:, :1].copy()   # 2-D: u = first column of Rot(theta) = (cos, sin)

    ls = _LeastSquares(col, d, n_rhs)
    for k in range(len(ek)):
        if int(ek[k]) != pose_kind:
            continue
        i, j = int(ef[k]), int(et[k])
        if i in held and j in held:
            continue
        Rij = unpack_measurement(pose_kind, meas[k])[1]
        W = full_info(EDGE_DIM[pose_kind], infos[k])
        kappa = np.trace(W[d:, d:]) / 3.0 if d == 3 else W[2, 2]
        A = Rij.T if d == 3 else Rij
        w = np.sqrt(kappa)
        ls.add([(i, w * A, known_rot(i) if i in held else None), (j, -w * np.eye(d), known_rot(j) if j in held else None)],
               np.zeros((d, n_rhs)))
    for v, k, m, winfo in pr:
        v = int(v)
        if k != pose_kind or v in held:
            continue
        Rz = unpack_measurement(pose_kind, m)[1]
        W = full_info(EDGE_DIM[pose_kind], winfo)
        kappa = np.trace(W[d:, d:]) / 3.0 if d == 3 else W[2, 2]
        w = np.sqrt(kappa)
        ls.add([(v, w * np.eye(d), None)], w * (Rz.T if d == 3 else Rz[:, :1]))
    X = ls.solve(d * len(free_pose)) if free_pose else np.zeros((0, n_rhs))

    # ---- 2. projection
    R = [c[1] if is_pose[i] else None for i, c in enumerate(cur)]
    M = [None] * N
    margin, u_min = np.inf, np.inf
    for c, v in enumerate(free_pose):
        blk = X[d * c:d * c + d]
        if d == 3:
            M[v] = blk.T.copy()    # column k of blk is row k of M
            R[v], s = project_so(M[v])
            margin = min(margin, (s[1] + np.sign(np.linalg.det(M[v])) * s[2]) / s[0])
        else:
            u = blk[:, 0]
            M[v] = u.copy()
            nrm = np.linalg.norm(u)
            u_min = min(u_min, nrm)
            R[v] = np.array([[u[0], -u[1]], [u[1], u[0]]]) / nrm

    # ---- 3. positions
    free = [i for i in range(N) if i not in held]
    colp = {v: d * c for c, v in enumerate(free)}
    lp = _LeastSquares(colp, d, 1)

    def known_pos(i):
        return np.asarray(cur[i][0], np.float64).reshape(d, 1)

    for k in range(len(ek)):
        kind = int(ek[k])
        if kind in (4, 6):
            continue   # bearing-only / range-only: one scalar places nothing
        i, j = int(ef[k]), int(et[k])
        if i in held and j in held:
            continue
        W = full_info(EDGE_DIM[kind], infos[k])[:d, :d]
        L = np.linalg.cholesky(W)               # |v|^2_W = |L^T v|^2
        z = np.asarray(meas[k][:d], np.float64).reshape(d, 1)
        G = L.T @ R[i].T
        lp.add([(j, G, known_pos(j) if j in held else None), (i, -G, known_pos(i) if i in held else None)], L.T @ z)
    for v, k, m, winfo in pr:
        v = int(v)
        if v in held:
            continue
        W = full_info(EDGE_DIM[k], winfo)[:d, :d]
        L = np.linalg.cholesky(W)
        tz, Rz = unpack_measurement(k, m)
        Rz = np.eye(d) if Rz is None else Rz
        G = L.T @ Rz.T
        lp.add([(v, G, None)], G @ np.asarray(tz[:d], np.float64).reshape(d, 1))
    P = lp.solve(d * len(free))[:, 0] if free else np.zeros(0)

    # ---- the state
    out, o = state.copy(), 0
    for i in range(N):
        n = STATE_LEN[int(nk[i])]
        if i not in held:
            t = P[colp[i]:colp[i] + d]
            out[o:o + d] = t
            if is_pose[i]:
                if d == 3:
                    out[o + 3:o + 7] = rot_to_quat(R[i])
                else:
                    out[o + 2] = np.arctan2(R[i][1, 0], R[i][0, 0])
        o += n
    return out, {"M": M, "R": R, "margin": margin, "u_min": u_min}


# ---- comparing states with rotations as matrices

def state_rotations(nk, state):
    """per node: (position, rotation matrix or None)"""
    return [unpack_measurement(int(k), s) for k, s in zip(nk, split(nk, np.asarray(state, np.float64), STATE_LEN))]


def state_diff(nk, a, b):
    """the largest absolute difference of two states: positions entrywise, rotations as matrices (q and -q are the same)"""
    worst = 0.0
    for (ta, Ra), (tb, Rb) in zip(state_rotations(nk, a), state_rotations(nk, b)):
        worst = max(worst, float(np.max(np.abs(np.asarray(ta) - np.asarray(tb)))))
        if Ra is not None:
            worst = max(worst, float(np.max(np.abs(Ra - Rb))))
    return worst


def held_set(anchor, fixed=(), keep_anchor=True):
    """the held nodes of a handle: its fixed set and, while every keep_anchor setting says keep, its anchor"""
    s = set(int(v) for v in fixed)
    if keep_anchor and anchor >= 0:
        s.add(int(anchor))
    return sorted(s)


def all_at_node0(arrays):
    """the state "every node at node 0's pose": every pose takes node 0's state, every landmark node 0's position"""
    nk, ns = np.asarray(arrays[0]), np.asarray(arrays[1], np.float64)
    first = ns[:STATE_LEN[int(nk[0])]]
    d = 3 if np.any(nk >= 2) else 2
    return np.concatenate([first if int(k) in POSE_KINDS else first[:d] for k in nk])
