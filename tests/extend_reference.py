"""CPU reference for the initial guess of rr_pgo_extend (include/rr_pgo.h): the composition of a known node with an edge's
measurement in numpy f64, and the host's step planner restated.

States and measurements are in rr_pgo_graph_desc packing: SE2 x, y, theta | XY x, y | SE3 x, y, z, qx, qy, qz, qw.
tests/test_extend_cpu.py validates `compose` with the unchanged oracle: a node guessed from one edge leaves that edge
without error."""
import numpy as np

EDGE_SE2, EDGE_SE2_XY, EDGE_SE3 = 0, 1, 2
MEAS_LEN = {0: 3, 1: 2, 2: 7}
STATE_LEN = {0: 3, 1: 2, 2: 7}


def rot2(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s], [s, c]])


def quat_mul(a, b):
    """Hamilton product, (x, y, z, w)"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_rot(q, v):
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R @ np.asarray(v, np.float64)


def compose(kind, src, z, inverse=False):
    """State of the node an edge of `kind` with measurement z determines from the state `src` of its other endpoint:
    to = from (+) z, or (inverse, pose-pose edges only) from = to (+) z^-1."""
    src, z = np.asarray(src, np.float64), np.asarray(z, np.float64)
    if kind == EDGE_SE2_XY:
        if inverse:
            raise ValueError("a landmark does not determine the pose that saw it")
        return src[:2] + rot2(src[2]) @ z
    if kind == EDGE_SE2:
        if not inverse:
            t = src[:2] + rot2(src[2]) @ z[:2]
            th = src[2] + z[2]
        else:
            th = src[2] - z[2]
            t = src[:2] - rot2(th) @ z[:2]
        return np.array([t[0], t[1], np.arctan2(np.sin(th), np.cos(th))])
    q, qz = src[3:] / np.linalg.norm(src[3:]), z[3:] / np.linalg.norm(z[3:])
    if not inverse:
        t = src[:3] + quat_rot(q, z[:3])
        r = quat_mul(q, qz)
    else:
        r = quat_mul(q, qz * np.array([-1.0, -1.0, -1.0, 1.0]))
        r = r / np.linalg.norm(r)
        t = src[:3] - quat_rot(r, z[:3])
    return np.concatenate([t, r / np.linalg.norm(r)])


def plan(n_old, n_new, edge_kind, edge_from, edge_to):
    """(steps, unreachable): steps = [(edge, src, dst, inverse)] in the order the host executes them; unreachable = the
    new nodes no step reaches (the call is then RR_PGO_EINVAL naming the first).  The ready set starts as the old nodes;
    the new edges are scanned in order until a scan adds no step."""
    ready = [True] * n_old + [False] * n_new
    steps = []
    added = True
    while added:
        added = False
        for k, (ek, f, t) in enumerate(zip(edge_kind, edge_from, edge_to)):
            f, t = int(f), int(t)
            if ready[f] and not ready[t] and t >= n_old:
                steps.append((k, f, t, False))
                ready[t] = True
                added = True
            elif ready[t] and not ready[f] and f >= n_old and int(ek) != EDGE_SE2_XY:
                steps.append((k, t, f, True))
                ready[f] = True
                added = True
    return steps, [v for v in range(n_old, n_old + n_new) if not ready[v]]


def split_states(node_kind, state):
    out, o = [], 0
    for k in node_kind:
        out.append(np.asarray(state[o:o + STATE_LEN[int(k)]], np.float64))
        o += STATE_LEN[int(k)]
    return out


def guess(old_kind, old_state, new_kind, edge_kind, edge_from, edge_to, edge_meas):
    """States of the new nodes (a list, one array per node) as the planned steps produce them from `old_state`"""
    states = split_states(old_kind, old_state) + [None] * len(new_kind)
    meas, o = [], 0
    for k in edge_kind:
        meas.append(np.asarray(edge_meas[o:o + MEAS_LEN[int(k)]], np.float64))
        o += MEAS_LEN[int(k)]
    steps, lost = plan(len(old_kind), len(new_kind), edge_kind, edge_from, edge_to)
    if lost:
        raise ValueError(f"unreachable nodes {lost}")
    for k, src, dst, inverse in steps:
        states[dst] = compose(int(edge_kind[k]), states[src], meas[k], inverse)
    return states[len(old_kind):]
