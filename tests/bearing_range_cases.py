"""Seeded fixtures for the bearing-only / range-only tests, in rr_pgo_graph_desc packing: (node_kind, node_state, edge_kind,
edge_from, edge_to, edge_meas, edge_info).  Each is the smallest that exercises its point; tests/test_bearing_range_cpu.py
checks on the reference alone that each meets the conditions the GPU tests rely on (positive definite, cond <= 1e12, every
observed rho >= 0.5, Gauss-Newton converges within 20 iterations, noise floors <= 1e-6).

    tri       3 poses with odometry, ONE landmark seen by bearing from all three (11 unknowns)
    tri2      the same with two bearings only: both are bridges (redundancy 0), the 1-D counterpart of a landmark seen once
    beacons   6 poses on a loop, 3 landmarks with range edges only, each seen from 4 poses that are not collinear
    mixed     12 poses, 5 landmarks, all three landmark kinds; the landmark of node 0; a pair with a bearing AND a range edge
              (parallel edges); a bearing whose true value is within 0.05 rad of pi, measured on the other side of the cut;
              a landmark with 10 observations (the strided incidence loop of LIN_GROUP = 8 wraps)
    corridor  120 poses, 40 landmarks (440 unknowns): the tree has several levels
"""
import numpy as np

from bearing_range_reference import BEARING, RANGE, SE2, SE2_XY

CASES = ("tri", "tri2", "beacons", "mixed", "corridor")
SIGMA = {SE2: (0.02, 0.01), SE2_XY: 0.03, BEARING: 0.01, RANGE: 0.03}   # measurement noise (pose-pose: metres, radians)


def wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


class Builder:
    """true poses and landmarks in node order; edges measured from the truth with seeded noise; the initial state is the truth
    moved by seeded noise (poses 0.05 m / 0.02 rad, landmarks 0.1 m)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.kind, self.truth = [], []
        self.ek, self.ef, self.et, self.em, self.ei = [], [], [], [], []

    def pose(self, x, y, th):
        self.kind.append(0)
        self.truth.append(np.array([x, y, th], np.float64))
        return len(self.kind) - 1

    def landmark(self, x, y):
        self.kind.append(1)
        self.truth.append(np.array([x, y], np.float64))
        return len(self.kind) - 1

    def local(self, a, b):
        ta, tb = self.truth[a], self.truth[b]
        c, s = np.cos(ta[2]), np.sin(ta[2])
        d = tb[:2] - ta[:2]
        return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])

    def edge(self, kind, a, b, noise=None):
        """an edge a -> b measured from the truth; noise: the measurement's own noise vector (None: seeded)"""
        p = self.local(a, b)
        if kind == SE2:
            st, sa = SIGMA[SE2]
            z = np.array([p[0], p[1], wrap(self.truth[b][2] - self.truth[a][2])]) + (self.rng.normal(size=3) * [st, st, sa] if noise is None else noise)
            z[2] = wrap(z[2])
            info = [1 / st ** 2, 0.0, 0.0, 1 / st ** 2, 0.0, 1 / sa ** 2]
        elif kind == SE2_XY:
            s = SIGMA[SE2_XY]
            z = p + (self.rng.normal(size=2) * s if noise is None else noise)
            info = [1 / s ** 2, 0.3 / s ** 2, 1.5 / s ** 2]   # a full 2 x 2 information matrix
        elif kind == BEARING:
            s = SIGMA[BEARING]
            z = np.array([wrap(np.arctan2(p[1], p[0]) + (self.rng.normal() * s if noise is None else noise))])
            info = [1 / s ** 2]
        else:
            s = SIGMA[RANGE]
            z = np.array([np.hypot(p[0], p[1]) + (self.rng.normal() * s if noise is None else noise)])
            info = [1 / s ** 2]
        self.ek.append(kind); self.ef.append(a); self.et.append(b)
        self.em.extend(z); self.ei.extend(info)
        return len(self.ek) - 1

    def arrays(self):
        state = []
        for k, t in zip(self.kind, self.truth):
            state.extend(t + (self.rng.normal(size=3) * [0.05, 0.05, 0.02] if k == 0 else self.rng.normal(size=2) * 0.1))
        return (np.array(self.kind, np.int32), np.array(state, np.float64), np.array(self.ek, np.int32), np.array(self.ef, np.int32),
                np.array(self.et, np.int32), np.array(self.em, np.float64), np.array(self.ei, np.float64))


def tri(n_bearings=3):
    b = Builder(101)
    p = [b.pose(0.0, 0.0, 0.1), b.pose(2.0, 0.5, -0.2), b.pose(4.0, -0.3, 0.3)]
    l = b.landmark(2.2, 3.0)
    b.edge(SE2, p[0], p[1])
    b.edge(SE2, p[1], p[2])
    for i in range(n_bearings):
        b.edge(BEARING, p[i], l)
    return b.arrays()


def beacons():
    b = Builder(102)
    p = [b.pose(3.0 * np.cos(a), 2.0 * np.sin(a), a + np.pi / 2) for a in np.arange(6) * np.pi / 3]
    l = [b.landmark(5.0, 4.0), b.landmark(-4.5, 3.0), b.landmark(0.5, -5.0)]
    for i in range(6):
        b.edge(SE2, p[i], p[(i + 1) % 6])
    for j, lm in enumerate(l):
        for i in ((0, 1, 3, 4), (1, 2, 4, 5), (0, 2, 3, 5))[j]:
            b.edge(RANGE, p[i], lm)
    return b.arrays()


def mixed():
    """(arrays, marks): marks names what the tests of `mixed` look for -- `parallel`: the two edges of the pair seen twice,
    `many`: the landmark with ten observations, `cut`: the bearing measured across the cut (mixed_marks() returns it)"""
    b = Builder(103)
    MIXED = {}
    l0 = b.landmark(1.0, 3.0)                                  # node 0 is a landmark
    p = [b.pose(1.5 * i, 0.4 * np.sin(0.9 * i), 0.25 * np.cos(0.7 * i)) for i in range(12)]
    l = [l0, b.landmark(5.0, -3.0), b.landmark(9.0, 3.5), b.landmark(13.0, -3.0), b.landmark(16.0, 2.5)]
    for i in range(11):
        b.edge(SE2, p[i], p[i + 1])
    b.edge(SE2, p[0], p[4])
    b.edge(SE2, p[6], p[11])
    # l0: bearings and an XY;  l[1]: ranges and a bearing;  l[2]: 10 observations of every kind;  l[3], l[4]: mixed
    for i in (0, 1, 2):
        b.edge(BEARING, p[i], l[0])
    b.edge(SE2_XY, p[3], l[0])
    for i in (1, 2, 3, 5):
        b.edge(RANGE, p[i], l[1])
    MIXED["parallel"] = (b.edge(BEARING, p[4], l[1]), b.edge(RANGE, p[4], l[1]))    # the same pair twice
    MIXED["many"] = l[2]
    for n, i in enumerate(range(2, 12)):
        b.edge((BEARING, RANGE, SE2_XY)[n % 3], p[i], l[2])
    for i in (6, 7, 8, 9, 10):
        b.edge(BEARING if i % 2 else RANGE, p[i], l[3])
    b.edge(SE2_XY, p[9], l[3])
    for i in (8, 9, 10, 11):
        b.edge(RANGE if i % 2 else BEARING, p[i], l[4])
    # a landmark almost straight behind a pose: the true bearing is within 0.05 of pi, the measurement is past the cut
    q = b.pose(19.0, 2.4, 0.0)
    b.edge(SE2, p[11], q)
    true = np.arctan2(*b.local(q, l[4])[::-1])
    assert np.pi - 0.05 < true < np.pi, true
    MIXED["cut"] = b.edge(BEARING, q, l[4], noise=(np.pi - true) + 0.012)
    assert b.em[-1] < -3.0, b.em[-1]
    b.edge(RANGE, q, l[4])
    return b.arrays(), MIXED


def corridor():
    b = Builder(104)
    p = [b.pose(0.8 * i, 1.2 * np.sin(0.15 * i), np.arctan2(1.2 * 0.15 * np.cos(0.15 * i), 0.8)) for i in range(120)]   # heading along the path
    l = [b.landmark(2.4 * j + 1.0, (4.0 if j % 2 else -4.0) + 0.5 * np.sin(j)) for j in range(40)]
    for i in range(119):
        b.edge(SE2, p[i], p[i + 1])
    for i in range(0, 110, 17):
        b.edge(SE2, p[i], p[i + 9])
    n = 0
    for j in range(40):
        near = sorted(range(120), key=lambda i: abs(0.8 * i - (2.4 * j + 1.0)))[:5]
        for i in sorted(near):
            b.edge((BEARING, RANGE, BEARING, SE2_XY, RANGE)[n % 5], p[i], l[j])
            n += 1
    return b.arrays()


_CACHE = {}


def case(name):
    """the arrays of a fixture (built once; callers do not modify them)"""
    if name not in _CACHE:
        if name == "mixed":
            _CACHE["mixed"], _CACHE["mixed marks"] = mixed()
        else:
            _CACHE[name] = {"tri": tri, "tri2": lambda: tri(2), "beacons": beacons, "corridor": corridor}[name]()
    return _CACHE[name]


def mixed_marks():
    """the edge and node indices the tests of `mixed` name (see mixed())"""
    case("mixed")
    return _CACHE["mixed marks"]


TAGS = {SE2: "EDGE_SE2", SE2_XY: "EDGE_SE2_XY", BEARING: "EDGE_BEARING_SE2_XY", RANGE: "EDGE_RANGE_SE2_XY"}


def to_g2o(arrays, ids=None):
    """the graph as g2o text: vertices in node order, then edges in edge order (ids: the vertex ids, default the indices)"""
    from bearing_range_reference import INFO_LEN, META_LEN, split
    nk, ns, ek, ef, et, em, ei = arrays
    ids = list(range(len(nk))) if ids is None else ids
    st = split(nk, ns, {0: 3, 1: 2})
    lines = [f"{'VERTEX_SE2' if k == 0 else 'VERTEX_XY'} {ids[v]} " + " ".join(repr(float(x)) for x in st[v]) for v, k in enumerate(nk)]
    zs, ws = split(ek, em, META_LEN), split(ek, ei, INFO_LEN)
    for k in range(len(ek)):
        lines.append(f"{TAGS[int(ek[k])]} {ids[ef[k]]} {ids[et[k]]} " + " ".join(repr(float(x)) for x in list(zs[k]) + list(ws[k])))
    return "\n".join(lines) + "\n"
