"""Graphs for the tests of rr_pgo_initialize (tests/test_initialize_cpu.py, tests/test_initialize_gpu.py), in
rr_pgo_graph_desc packing, and the bounds those tests share."""
import numpy as np

from random_graphs import pack_upper, q_conj, q_mul, q_rot, random_spd, unit_quat

# The reference's own worst error on the four noise-free graphs (tests/test_initialize_cpu.py measures it: 3.2e-14 at the
# seeds below, positions of order 10) is below this; the GPU test's f64 bound is 100 x this, which leaves room for
# another elimination order.
NOISE_FREE_REFERENCE_ERROR = 1e-13
NOISE_FREE_GPU_BOUND = 100 * NOISE_FREE_REFERENCE_ERROR

RING_POSES, RING_CHORDS, RING_LANDMARKS = 12, ((0, 5), (2, 9), (10, 4)), 4


def random_quat(rng):
    return unit_quat(rng.normal(size=4))


def rot2t(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, s], [-s, c]])


def measure(se3, xa, xb):
    """the exact measurement of node b from pose a (states in node_state packing)"""
    if se3:
        ta, qa = xa[:3], xa[3:7]
        if len(xb) == 7:
            return np.concatenate([q_rot(q_conj(qa), xb[:3] - ta), unit_quat(q_mul(q_conj(qa), xb[3:7]))])
        return q_rot(q_conj(qa), xb - ta)
    Rt = rot2t(xa[2])
    if len(xb) == 3:
        return np.concatenate([Rt @ (xb[:2] - xa[:2]), [np.arctan2(np.sin(xb[2] - xa[2]), np.cos(xb[2] - xa[2]))]])
    return Rt @ (xb - xa[:2])


def noisy(rng, se3, z, sigma_t=0.05, sigma_r=0.01):
    z = np.array(z, np.float64)
    if se3 and len(z) == 7:
        z[:3] += rng.normal(scale=sigma_t, size=3)
        q = z[3:] + rng.normal(scale=sigma_r, size=4)
        z[3:] = q / np.linalg.norm(q)
        return z
    if not se3 and len(z) == 3:
        return z + rng.normal(scale=[sigma_t, sigma_t, sigma_r])
    return z + rng.normal(scale=sigma_t, size=len(z))


def random_truth(rng, se3, n_pose, n_lm, scale=10.0):
    d = 3 if se3 else 2
    poses = [np.concatenate([rng.uniform(-scale, scale, d), random_quat(rng) if se3 else [rng.uniform(-np.pi, np.pi)]]) for _ in range(n_pose)]
    lms = [rng.uniform(-scale, scale, d) for _ in range(n_lm)]
    return poses + lms


def assemble(rng, se3, truth, n_pose, edges, noise):
    """edges: (from, to) node pairs, landmarks are the nodes from n_pose on; full random SPD information"""
    d = 3 if se3 else 2
    pose_kind, lm_kind = (2, 3) if se3 else (0, 1)
    nk = np.array([pose_kind] * n_pose + [lm_kind] * (len(truth) - n_pose), np.int32)
    ek, ef, et, em, ei = [], [], [], [], []
    for a, b in edges:
        z = measure(se3, truth[a], truth[b])
        if noise:
            z = noisy(rng, se3, z)
        point = b >= n_pose
        ek.append(lm_kind if point else pose_kind)
        ef.append(a); et.append(b); em.append(z)
        dim = d if point else (6 if se3 else 3)
        ei.append(pack_upper(dim, random_spd(rng, dim)))
    return [nk, np.concatenate(truth), np.array(ek, np.int32), np.array(ef, np.int32), np.array(et, np.int32),
            np.concatenate(em), np.concatenate(ei)]


def scrambled(rng, se3, truth, n_pose, keep=(0,)):
    """random rotations and positions of order 10 everywhere but at the nodes of `keep`, which stay at the truth"""
    fresh = random_truth(rng, se3, n_pose, len(truth) - n_pose)
    return np.concatenate([truth[i] if i in keep else fresh[i] for i in range(len(truth))])


def ring_graph(seed, se3, landmarks):
    """ring of 12 poses and 3 chords, noise-free, optionally 4 landmarks seen by 1, 2, 3 and 2 poses; returns
    (arrays at the truth, scrambled state with node 0 at the truth)"""
    rng = np.random.default_rng(seed)
    n_lm = RING_LANDMARKS if landmarks else 0
    truth = random_truth(rng, se3, RING_POSES, n_lm)
    edges = [(i, (i + 1) % RING_POSES) for i in range(RING_POSES)] + list(RING_CHORDS)
    if landmarks:
        edges += [(3, 12), (1, 13), (7, 13), (2, 14), (6, 14), (11, 14), (5, 15), (9, 15)]
    arrays = assemble(rng, se3, truth, RING_POSES, edges, noise=False)
    return arrays, scrambled(rng, se3, truth, RING_POSES)


RING_CASES = [(101, False, False), (102, True, False), (103, False, True), (104, True, True)]
RING_IDS = ["2d", "3d", "2d-landmarks", "3d-landmarks"]


def reflection_graph():
    """Four SE(3) poses; 0, 1, 2 are to be fixed with R = I; edges k -> 3 measure Rx(pi), Ry(pi), Rz(pi) with rotation
    information 2.5 I, 2 I, 1 I, so M_3 = -diag(0.5, 1.5, 3.5) / 5.5: negative determinant, distinct singular values, and the
    projection is exactly Rx(pi).  Returns (arrays, the position the translations put node 3 at)."""
    ident = [0.0, 0.0, 0.0, 1.0]
    t = [np.array([0.0, 0.0, 0.0]), np.array([4.0, 1.0, -2.0]), np.array([-3.0, 2.0, 5.0])]
    t3 = np.array([1.0, -2.0, 0.5])
    nk = np.full(4, 2, np.int32)
    ns = np.concatenate([np.concatenate([t[0], ident]), np.concatenate([t[1], ident]), np.concatenate([t[2], ident]),
                         np.concatenate([[9.0, 9.0, 9.0], unit_quat(np.array([0.3, -0.2, 0.5, 0.4]))])])
    quats = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    kappas = [2.5, 2.0, 1.0]
    em, ei = [], []
    for k in range(3):
        em.append(np.concatenate([t3 - t[k], quats[k]]))   # R_k = I: the measured translation is the difference
        ei.append(pack_upper(6, np.diag([1.0, 1.0, 1.0, kappas[k], kappas[k], kappas[k]])))
    return [nk, ns, np.full(3, 2, np.int32), np.array([0, 1, 2], np.int32), np.full(3, 3, np.int32), np.concatenate(em),
            np.concatenate(ei)], t3


RX_PI = np.diag([1.0, -1.0, -1.0])


def hub_graph(seed, se3):
    """A noisy star plus ring: pose 0 is the hub of 19 pose-pose edges (two full strides of the 8-lane group and a remainder
    of 3; both directions occur), the leaves 1 .. 12 are joined in pairs (degree 2), 13 .. 19 hang on the hub alone
    (degree 1); four landmarks seen from leaves, the last one by one pose only.  Returns (arrays with a noisy state, truth)."""
    rng = np.random.default_rng(seed)
    n_pose, n_lm = 20, 4
    truth = random_truth(rng, se3, n_pose, n_lm)
    edges = [(0, k) if k % 3 else (k, 0) for k in range(1, 20)]
    edges += [(k, k + 1) for k in range(1, 12, 2)]
    edges += [(2, 20), (5, 20), (14, 20), (3, 21), (17, 21), (8, 22), (9, 22), (19, 22), (13, 23)]
    order = [0] + [1 + int(i) for i in rng.permutation(len(edges) - 1)]   # (edge 0 stays first: its from-node 0 is the anchor)
    arrays = assemble(rng, se3, truth, n_pose, [edges[i] for i in order], noise=True)
    arrays[1] = scrambled(rng, se3, truth, n_pose)
    return arrays, np.concatenate(truth)
