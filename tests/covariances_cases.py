"""Query sets shared by tests/test_covariances_cpu.py and tests/test_covariances_gpu.py."""
import numpy as np

FAR_GRAPHS = ["intel", "input_M3500_g2o", "dlr", "parking-garage", "simulation-pose-landmark"]
FLOOR_MAX = 1e-6   # the reference's two computations must agree this well, or a comparison against it shows nothing


def far_nodes(n):
    """24 seeded nodes of a graph of n nodes"""
    return [int(v) for v in np.random.default_rng(31).choice(n, 24, replace=False)]


def far_pairs(n):
    """(nodes, node_a, node_b): the 24 seeded nodes and all 576 ordered pairs of them"""
    nodes = far_nodes(n)
    a = np.repeat(nodes, len(nodes)).astype(np.int32)
    b = np.tile(nodes, len(nodes)).astype(np.int32)
    return nodes, a, b


def joint_from_blocks(blocks, k):
    """dense joint matrix of k nodes from the k * k blocks of far_pairs' order"""
    return np.block([[blocks[i * k + j] for j in range(k)] for i in range(k)])
