"""Seeded random pose graphs in rr_pgo_graph_desc packing, shared by tests/test_gpu_parity.py (the factor path against the
oracle) and tests/query_small_cases.py (the factor queries against their CPU references)."""
import numpy as np


def random_graph(rng, n_pose, n_lm, n_extra, se3=False):
    """A connected random graph in rr_pgo_graph_desc packing: a random spanning tree over the poses (so that the one prior on the
    from-node of the first pose-pose edge, :330-336, reaches everything), `n_extra` loop closures between random pose pairs
    (parallel edges and both directions allowed), `n_lm` landmarks seen from one to three random poses each (SE(2) only), full
    random SPD information matrices, measurements = ground truth relative poses + noise, initial state = ground truth + noise."""
    def spd(d):
        a = rng.normal(size=(d, d))
        m = a @ a.T + d * np.eye(d)
        return m * rng.uniform(0.5, 50.0)
    if se3:
        def q_mul(a, b):
            ax, ay, az, aw = a; bx, by, bz, bw = b
            return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                             aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])
        def q_rot(q, v):
            qv = np.array([*v, 0.0]); qc = np.array([-q[0], -q[1], -q[2], q[3]])
            return q_mul(q_mul(q, qv), qc)[:3]
        def rq():
            q = rng.normal(size=4); return q / np.linalg.norm(q) * np.sign(q[3] if q[3] != 0 else 1.0)
        T = [(rng.uniform(-5, 5, 3), rq()) for _ in range(n_pose)]
        pairs = [(int(rng.integers(0, i)), i) for i in range(1, n_pose)] + [tuple(int(x) for x in rng.choice(n_pose, 2, replace=False)) for _ in range(n_extra)]
        rng.shuffle(pairs[1:])
        nk = np.full(n_pose, 2, np.int32)
        ns = np.concatenate([np.concatenate([t + rng.normal(scale=0.05, size=3), (lambda q: q / np.linalg.norm(q))(q + rng.normal(scale=0.02, size=4))]) for t, q in T])
        ek, ef, et, em, ei = [], [], [], [], []
        for a, b in pairs:
            (ta, qa), (tb, qb) = T[a], T[b]
            qai = np.array([-qa[0], -qa[1], -qa[2], qa[3]])
            tz, qz = q_rot(qai, tb - ta), q_mul(qai, qb)
            qz = (qz + rng.normal(scale=0.01, size=4)); qz /= np.linalg.norm(qz)
            ek.append(2); ef.append(a); et.append(b)
            em.append(np.concatenate([tz + rng.normal(scale=0.02, size=3), qz]))
            ei.append(spd(6)[np.triu_indices(6)])
        return nk, ns, np.array(ek, np.int32), np.array(ef, np.int32), np.array(et, np.int32), np.concatenate(em), np.concatenate(ei)
    X = np.column_stack([rng.uniform(-10, 10, n_pose), rng.uniform(-10, 10, n_pose), rng.uniform(-np.pi, np.pi, n_pose)])
    Lm = rng.uniform(-10, 10, (n_lm, 2))
    pairs = [(int(rng.integers(0, i)), i) for i in range(1, n_pose)] + [tuple(int(x) for x in rng.choice(n_pose, 2, replace=False)) for _ in range(n_extra)]
    first, rest = pairs[:1], pairs[1:]
    sights = [(int(p), n_pose + l) for l in range(n_lm) for p in rng.choice(n_pose, int(rng.integers(1, 4)), replace=False)]
    rest = rest + sights
    order = rng.permutation(len(rest))
    edges = first + [rest[i] for i in order]          # (the first edge stays a pose-pose edge: the prior's anchor)
    nk = np.concatenate([np.zeros(n_pose, np.int32), np.ones(n_lm, np.int32)])
    ns = np.concatenate([(X + rng.normal(scale=[0.1, 0.1, 0.03], size=X.shape)).ravel(), (Lm + rng.normal(scale=0.1, size=Lm.shape)).ravel()])
    ek, ef, et, em, ei = [], [], [], [], []
    for a, b in edges:
        xa = X[a]
        c, s_ = np.cos(xa[2]), np.sin(xa[2])
        Rt = np.array([[c, s_], [-s_, c]])
        if b < n_pose:
            xb = X[b]
            z = np.concatenate([Rt @ (xb[:2] - xa[:2]), [xb[2] - xa[2]]]) + rng.normal(scale=[0.05, 0.05, 0.01])
            ek.append(0); em.append(z); ei.append(spd(3)[np.triu_indices(3)])
        else:
            z = Rt @ (Lm[b - n_pose] - xa[:2]) + rng.normal(scale=0.05, size=2)
            ek.append(1); em.append(z); ei.append(spd(2)[np.triu_indices(2)])
        ef.append(a); et.append(b)
    return nk, ns, np.array(ek, np.int32), np.array(ef, np.int32), np.array(et, np.int32), np.concatenate(em), np.concatenate(ei)


def two_component_graph(info_sign=1.0):
    """nodes 0-1 and 2-3 joined pairwise: the prior reaches only the first pair, the second is singular (exactly: the
    arithmetic of these integers is exact, the failing pivot is 0.0); info_sign = -1 makes H negative definite instead"""
    nk = np.zeros(4, np.int32)
    ns = np.array([0, 0, 0, 1, 0, 0, 5, 5, 0, 6, 5, 0], float)
    ek = np.zeros(2, np.int32)
    ef, et = np.array([0, 2], np.int32), np.array([1, 3], np.int32)
    # the second edge has a residual (a step would move its nodes); all headings are 0 and every entry a small dyadic
    # rational, so H is formed exactly and the unanchored pair's last pivot is exactly 0 in the very first iteration
    em = np.array([1, 0, 0, 1.5, 0.25, 0.0], float)
    ei = info_sign * np.tile([1, 0, 0, 1, 0, 1], 2).astype(float)
    return nk, ns, ek, ef, et, em, ei


# ---- the pieces of such a graph, for generators of other shapes (tests/query_small_cases.py); random_graph keeps its own
# copies: its seeded graphs are pinned by the order of its draws

def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def q_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def q_rot(q, v):
    return q_mul(q_mul(q, np.array([*v, 0.0])), q_conj(q))[:3]


def unit_quat(q):
    q = q / np.linalg.norm(q)
    return q if q[3] >= 0 else -q


def random_spd(rng, d):
    a = rng.normal(size=(d, d))
    return (a @ a.T + d * np.eye(d)) * rng.uniform(0.5, 50.0)


def pack_upper(d, m):
    return m[np.triu_indices(d)]


def se2_edge(rng, xa, xb):
    c, s = np.cos(xa[2]), np.sin(xa[2])
    Rt = np.array([[c, s], [-s, c]])
    if len(xb) == 3:
        return np.concatenate([Rt @ (xb[:2] - xa[:2]), [xb[2] - xa[2]]]) + rng.normal(scale=[0.05, 0.05, 0.01])
    return Rt @ (xb - xa[:2]) + rng.normal(scale=0.05, size=2)


def se3_edge(rng, Ta, Tb):
    (ta, qa), (tb, qb) = Ta, Tb
    qz = q_mul(q_conj(qa), qb) + rng.normal(scale=0.01, size=4)
    return np.concatenate([q_rot(q_conj(qa), tb - ta) + rng.normal(scale=0.02, size=3), qz / np.linalg.norm(qz)])
