"""The graphs and tree pins of the arrival-order tests, shared by tests/test_arrival_order_cpu.py (which proves on the host
tables that they contain the shapes that can go wrong) and tests/test_arrival_order_gpu.py (which runs them).  Nothing
here needs a GPU.

A handle created with both RR_PGO_ND_LEAF and RR_PGO_AMALG_NP set skips the engine's choice among candidate trees and is
analysed once, with the options `helper_env` restates for tests/native/arrival_order_check.cpp (pgo_api.hip,
analyze_handle: multilevel dissection up to 6000 nodes, chain merges up to 80 pivot columns, 48 with 6 x 6 blocks, the
dataflow schedule, 19000 scalars of LDS per front in f64).  TREES ties the two: the statistics of the helper's tree are
the statistics the GPU test demands of its handles."""
import numpy as np

from conftest import g2o_path

SHAPES = ("middle", "partial_last", "same_block", "three_distinct", "all_zero")

# (graph, pins): graph is a file of tests/golden/g2o or a name of query_small_cases.GRAPHS
GPU_CASES = [
    ("simulation-pose-pose", {"RR_PGO_ND_LEAF": "50", "RR_PGO_AMALG_NP": "16"}),
    ("simulation-pose-pose", {"RR_PGO_ND_LEAF": "1000000", "RR_PGO_AMALG_NP": "16"}),
    ("simulation-pose-landmark", {"RR_PGO_ND_LEAF": "1000000", "RR_PGO_AMALG_NP": "16"}),
    ("mid-se2", {"RR_PGO_ND_LEAF": "50", "RR_PGO_AMALG_NP": "16"}),
    ("mid-se3", {"RR_PGO_ND_LEAF": "50", "RR_PGO_AMALG_NP": "16"}),
]
INTEL = ("intel", {"RR_PGO_ND_LEAF": "50", "RR_PGO_AMALG_NP": "32"})   # the tree the engine picks for intel
# (n_supernodes, max_front, max_pivot_cols) of each case's tree in f64, as tests/native/arrival_order_check.cpp prints them under
# helper_env and as rr_pgo_stats reports them for the handle: the CPU test holds the helper to them and the GPU test its handles,
# so that the tables the helper inspects are the tables the GPU runs (a change of analyze_handle's defaults fails both)
TREES = {
    "simulation-pose-pose-leaf50-np16": (26, 126, 99),
    "simulation-pose-pose-leaf1000000-np16": (25, 135, 126),
    "simulation-pose-landmark-leaf1000000-np16": (4, 71, 71),
    "mid-se2-leaf50-np16": (41, 136, 130),
    "mid-se3-leaf50-np16": (90, 174, 102),
    "intel-leaf50-np32": (157, 165, 108),
}
GOLDEN = ("simulation-pose-pose", "simulation-pose-landmark", "intel", "input_M3500_g2o", "dlr", "parking-garage", "sphere2500", "torus3D")


def case_id(case):
    return case[0] + "-leaf" + case[1]["RR_PGO_ND_LEAF"] + "-np" + case[1]["RR_PGO_AMALG_NP"]


def arrays_of(graph):
    from query_small_cases import arrays_of as small
    return small(graph)


def is_file(graph):
    return graph in GOLDEN


def helper_env(pins, se3, lds=19000):
    """the environment of arrival_order_check that restates a handle created under `pins`"""
    return {"LEAF": pins["RR_PGO_ND_LEAF"], "AMALG_NP": pins["RR_PGO_AMALG_NP"], "ML": "1", "FLOW": "1",
            "MERGE_NC": "48" if se3 else "80", "LDS": str(lds)}


def write_g2o(arrays, path):
    """rr_pgo_graph_desc arrays as a g2o file: node states with all their digits (the dissection may cut along a coordinate)"""
    nk, ns, ek, ef, et, em, ei = arrays
    tag_n, len_n = {0: "VERTEX_SE2", 1: "VERTEX_XY", 2: "VERTEX_SE3:QUAT"}, {0: 3, 1: 2, 2: 7}
    tag_e, len_m, len_i = {0: "EDGE_SE2", 1: "EDGE_SE2_XY", 2: "EDGE_SE3:QUAT"}, {0: 3, 1: 2, 2: 7}, {0: 6, 1: 3, 2: 21}
    ns, em, ei = np.asarray(ns, np.float64), np.asarray(em, np.float64), np.asarray(ei, np.float64)
    with open(path, "w") as f:
        o = 0
        for i, k in enumerate(nk):
            f.write(" ".join([tag_n[int(k)], str(i)] + [repr(float(v)) for v in ns[o:o + len_n[int(k)]]]) + "\n")
            o += len_n[int(k)]
        om = oi = 0
        for k, a, b in zip(ek, ef, et):
            k = int(k)
            vals = list(em[om:om + len_m[k]]) + list(ei[oi:oi + len_i[k]])
            f.write(" ".join([tag_e[k], str(int(a)), str(int(b))] + [repr(float(v)) for v in vals]) + "\n")
            om += len_m[k]
            oi += len_i[k]


def graph_file(graph, tmp_dir):
    """(path of the graph as a g2o file, whether it has 6 x 6 blocks)"""
    if is_file(graph):
        return g2o_path(graph), graph in ("parking-garage", "sphere2500", "torus3D")
    arrays = arrays_of(graph)
    path = tmp_dir / (graph + ".g2o")
    if not path.exists():
        write_g2o(arrays, path)
    return str(path), bool(np.any(np.asarray(arrays[0]) == 2))
