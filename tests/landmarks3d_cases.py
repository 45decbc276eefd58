"""Seeded 3-D graphs with point landmarks for the tests of RR_PGO_NODE_XYZ / RR_PGO_EDGE_SE3_XYZ: noisy measurements, full
(non-diagonal) positive-definite information matrices, in rr_pgo_graph_desc packing, and the same graphs as g2o text.

  two-poses-one-point   2 poses, 1 pose-pose edge, 1 landmark seen from both: dim 15
  point-first           the same with the landmark as node 0 (its vertex line first): a 3-scalar node opens the scalar order
  room                  12 poses on a ring (odometry + one closure), 8 landmarks seen from 3 to 6 poses each and one landmark
                        seen once (a bridge): dim 99
  corridor              60 poses along a line with odometry, 40 landmarks seen from the (up to seven) poses near them: dim 480
"""
import numpy as np

from landmarks3d_reference import Landmarks3dReference, q_conj, q_exp, q_mul, q_to_rot, unit

CASES = ("two-poses-one-point", "point-first", "room", "corridor")


def spd(rng, d, lo=5.0, hi=200.0):
    a = rng.normal(size=(d, d))
    return (a @ a.T + d * np.eye(d)) * rng.uniform(lo, hi)


def pack_upper(m):
    return m[np.triu_indices(len(m))]


def compose(x, dt, dw):
    """x * (dt, Exp(dw))"""
    return np.concatenate([x[:3] + q_to_rot(x[3:]) @ np.asarray(dt), unit(q_mul(x[3:], q_exp(np.asarray(dw))))])


def between(xi, xj):
    """Xi^-1 Xj as x y z qx qy qz qw"""
    return np.concatenate([q_to_rot(xi[3:]).T @ (xj[:3] - xi[:3]), unit(q_mul(q_conj(xi[3:]), xj[3:]))])


class Builder:
    def __init__(self, rng):
        self.rng = rng
        self.kind, self.truth, self.init = [], [], []
        self.ek, self.ef, self.et, self.em, self.ei = [], [], [], [], []

    def pose(self, x):
        self.kind.append(2)
        self.truth.append(np.asarray(x, np.float64))
        self.init.append(compose(x, self.rng.normal(scale=0.08, size=3), self.rng.normal(scale=0.04, size=3)))
        return len(self.kind) - 1

    def point(self, l):
        self.kind.append(3)
        self.truth.append(np.asarray(l, np.float64))
        self.init.append(np.asarray(l) + self.rng.normal(scale=0.1, size=3))
        return len(self.kind) - 1

    def odometry(self, a, b):
        z = compose(between(self.truth[a], self.truth[b]), self.rng.normal(scale=0.02, size=3), self.rng.normal(scale=0.01, size=3))
        self.ek.append(2); self.ef.append(a); self.et.append(b); self.em.append(z); self.ei.append(pack_upper(spd(self.rng, 6)))

    def observe(self, a, l):
        x = self.truth[a]
        z = q_to_rot(x[3:]).T @ (self.truth[l] - x[:3]) + self.rng.normal(scale=0.03, size=3)
        self.ek.append(3); self.ef.append(a); self.et.append(l); self.em.append(z); self.ei.append(pack_upper(spd(self.rng, 3)))

    def arrays(self, order=None):
        """og_create packing; order: the node order (a permutation of the nodes as they were added)"""
        n = len(self.kind)
        order = list(range(n)) if order is None else list(order)
        new = np.zeros(n, np.int32)
        new[order] = np.arange(n)
        return [np.array([self.kind[v] for v in order], np.int32), np.concatenate([self.init[v] for v in order]),
                np.array(self.ek, np.int32), new[np.array(self.ef)].astype(np.int32), new[np.array(self.et)].astype(np.int32),
                np.concatenate(self.em), np.concatenate(self.ei)]


def random_pose(rng, t):
    return np.concatenate([np.asarray(t, np.float64), unit(rng.normal(size=4))])


def build(name):
    rng = np.random.default_rng({"two-poses-one-point": 31, "point-first": 31, "room": 32, "corridor": 33}[name])
    b = Builder(rng)
    if name in ("two-poses-one-point", "point-first"):
        p0 = b.pose(random_pose(rng, [0.0, 0.0, 0.0]))
        p1 = b.pose(compose(b.truth[p0], [1.0, 0.2, -0.1], [0.1, -0.2, 0.3]))
        l = b.point([0.7, 1.5, 0.4])
        b.odometry(p0, p1)
        b.observe(p0, l)
        b.observe(p1, l)
        return b.arrays([l, p0, p1] if name == "point-first" else None)
    if name == "room":
        poses = []
        for i in range(12):
            a = 2 * np.pi * i / 12
            x = np.concatenate([[3 * np.cos(a), 3 * np.sin(a), 0.3 * np.sin(3 * a)], unit([0.1 * np.sin(a), 0.1 * np.cos(a), np.sin(a / 2 + 0.8), np.cos(a / 2 + 0.8)])])
            poses.append(b.pose(x))
        lms = [b.point(rng.uniform([-4, -4, -1], [4, 4, 2])) for _ in range(8)]
        bridge = b.point([0.5, -0.5, 1.0])
        for i in range(11):
            b.odometry(poses[i], poses[i + 1])
        b.odometry(poses[11], poses[0])          # the closure
        for j, l in enumerate(lms):
            seen = sorted(rng.choice(12, 3 + j % 4, replace=False))
            for i in seen:
                b.observe(poses[i], l)
        b.observe(poses[5], bridge)
        # landmarks between the poses in node order, so that both orientations of the off-diagonal blocks occur
        order = []
        for i in range(12):
            order.append(poses[i])
            if i < 8:
                order.append(lms[i])
        order.append(bridge)
        return b.arrays(order)
    assert name == "corridor"
    poses = []
    x = random_pose(rng, [0.0, 0.0, 0.0])
    for i in range(60):
        poses.append(b.pose(x))
        x = compose(x, [0.5, 0.05 * np.sin(i), 0.02], [0.02, 0.03 * np.cos(i / 3), 0.05])
    lms = []
    for j in range(40):
        near = b.truth[poses[int(j * 1.5)]]
        lms.append(b.point(near[:3] + rng.uniform(-1.5, 1.5, size=3)))
    for i in range(59):
        b.odometry(poses[i], poses[i + 1])
    for j, l in enumerate(lms):
        c = int(j * 1.5)
        for i in range(max(0, c - 3), min(60, c + 4)):   # seven poses: any cut of the chain is spanned by three or more landmarks,
            b.observe(poses[i], l)                       # so no odometry edge is a bridge in any direction
    b.observe(poses[59], lms[37])    # ... the far end included: a third landmark for the last pose
    order = []
    for i in range(60):
        order.append(poses[i])
        if i % 3 != 2 and len(order) - (i + 1) < 40:
            order.append(lms[len(order) - (i + 1)])
    assert len(order) == 100
    return b.arrays(order)


_cache = {}


def case(name, state="initial"):
    """the arrays of a case at its initial state, or at the state after two reference Gauss-Newton iterations"""
    key = (name, state)
    if key not in _cache:
        arrays = build(name)
        if state == "iterated":
            ref = Landmarks3dReference(arrays)
            for _ in range(2):
                ref.update(ref.step())
            arrays = list(arrays)
            arrays[1] = ref.state()
        _cache[key] = arrays
    return [np.array(a, copy=True) for a in _cache[key]]


def bridge_edge(arrays):
    """the edge of `room` into the landmark that has no other"""
    nk, _, ek, ef, et = arrays[:5]
    deg = np.bincount(np.concatenate([ef, et]), minlength=len(nk))
    lone = [k for k in range(len(ek)) if ek[k] == 3 and deg[et[k]] == 1]
    assert len(lone) == 1
    return lone[0]


def to_g2o(arrays, ids=None, offset_line=True):
    """the graph as g2o text: VERTEX_SE3:QUAT / VERTEX_TRACKXYZ in node order, an identity PARAMS_SE3OFFSET, the edges"""
    nk, ns, ek, ef, et, em, ei = arrays
    ids = np.arange(len(nk)) if ids is None else ids
    fmt = lambda v: " ".join(repr(float(x)) for x in v)
    out, o = [], 0
    if offset_line:
        out.append("PARAMS_SE3OFFSET 0 0 0 0 0 0 0 1")
    for v, k in enumerate(nk):
        n = 7 if k == 2 else 3
        out.append(f"{'VERTEX_SE3:QUAT' if k == 2 else 'VERTEX_TRACKXYZ'} {ids[v]} {fmt(ns[o:o + n])}")
        o += n
    mo = io = 0
    for k in range(len(ek)):
        if ek[k] == 2:
            out.append(f"EDGE_SE3:QUAT {ids[ef[k]]} {ids[et[k]]} {fmt(em[mo:mo + 7])} {fmt(ei[io:io + 21])}")
            mo += 7; io += 21
        else:
            out.append(f"EDGE_SE3_TRACKXYZ {ids[ef[k]]} {ids[et[k]]} 0 {fmt(em[mo:mo + 3])} {fmt(ei[io:io + 6])}")
            mo += 3; io += 6
    return "\n".join(out) + "\n"
