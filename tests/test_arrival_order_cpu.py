"""Arrival order of the pivot columns and the children's due blocks (symbolic.cpp step 5) on the host tables,
through tests/native/arrival_order_check.cpp: a host replay of the factorisation in the kernel's order (children added at
their due block) against mf_host_check's residual bound, no scatter destination left of a child's due block, due
non-decreasing along every child list, the same supernode partition with the switch on and off, and the histogram of due.

Runs on the eight files of tests/golden/g2o, on the random graphs of tests/random_graphs.py (as query_small_cases draws
them, the two mid-sized ones included) and on a 12 x 9 lattice whose fronts all fit LDS -- and proves that the graphs
tests/test_arrival_order_gpu.py runs, under the pins it runs them with, contain the shapes that can go wrong
(arrival_order_cases.SHAPES): a child due in a middle block, one due in a partial last block, two due at the same block, a
front with three or more distinct due values, a front whose children are all due at 0."""
import os
import re
import subprocess

import pytest

from arrival_order_cases import GOLDEN, GPU_CASES, INTEL, SHAPES, TREES, case_id, graph_file, helper_env
from conftest import ROOT

CSRC = os.path.join(ROOT, "rustrobotics_amd", "csrc")


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    exe = tmp_path_factory.mktemp("native") / "arrival_order_check"
    srcs = [os.path.join(ROOT, "tests", "native", "arrival_order_check.cpp")] + [
        os.path.join(CSRC, f) for f in ("symbolic.cpp", "g2o_loader.cpp", "synth_grid.cpp")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, *srcs, "-lpthread", "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def graphs_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("graphs")


def run(helper, args, env):
    out = subprocess.run([helper, *args], env={**os.environ, **env}, capture_output=True, text=True)
    print(" ".join(args), env)
    print(out.stdout + out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
    m = re.search(r"^cases: (.*)$", out.stdout, re.M)
    shapes = {k: v == "1" for k, v in (kv.split("=") for kv in m.group(1).split())}
    hist = {int(k): int(v) for k, v in re.findall(r" (\d+):(\d+)", re.search(r"^due histogram:(.*?)\(", out.stdout, re.M).group(1))}
    return shapes, hist, out.stdout


@pytest.mark.parametrize("lds", [19000, 38000])
@pytest.mark.parametrize("name", GOLDEN)
def test_golden_files(helper, graphs_dir, name, lds):
    """every file under both LDS budgets, on the deepest dissection the engine tries and without any"""
    path, se3 = graph_file(name, graphs_dir)
    for leaf in ("50", "1000000"):
        shapes, hist, text = run(helper, [path], helper_env({"RR_PGO_ND_LEAF": leaf, "RR_PGO_AMALG_NP": "16"}, se3, lds))
        if "beyond LDS" in text:
            assert set(hist) <= {0}, hist       # fronts beyond LDS: today's order, every child before the panel
        else:
            assert any(k > 0 for k in hist), hist


def test_fronts_beyond_lds_keep_the_elimination_order(helper, graphs_dir):
    """sphere2500 in f64 has fronts beyond LDS under every tree: the helper fails if such a graph is reordered or has a due > 0"""
    path, se3 = graph_file("sphere2500", graphs_dir)
    _, hist, text = run(helper, [path], helper_env({"RR_PGO_ND_LEAF": "50", "RR_PGO_AMALG_NP": "72"}, se3, 19000))
    assert "beyond LDS" in text and set(hist) <= {0}


def _small_names():
    from query_small_cases import GRAPHS
    return GRAPHS


@pytest.mark.parametrize("name", [f"se2-{s}" for s in range(12)] + [f"se3-{s}" for s in range(4)] +
                         ["two-poses", "landmark-first", "se3-chain3", "clique5", "mid-se2", "mid-se3"])
def test_random_graphs(helper, graphs_dir, name):
    assert name in _small_names()
    path, se3 = graph_file(name, graphs_dir)
    for leaf in ("8", "1000000"):
        run(helper, [path], helper_env({"RR_PGO_ND_LEAF": leaf, "RR_PGO_AMALG_NP": "16"}, se3))


def test_lattice_with_lds_fronts_only(helper):
    for env in ({"LEAF": "1000000", "FLOW": "1"}, {"LEAF": "16", "ML": "1", "FLOW": "1", "LDS": "38000"}):
        _, hist, text = run(helper, ["grid", "12", "9"], env)
        assert "beyond LDS" not in text
        assert any(k > 0 for k in hist), hist


# what each (graph, pins) of the GPU test must contain; together they cover SHAPES, and the first one has all five
EXPECT = {
    "simulation-pose-pose-leaf50-np16": SHAPES,
    "simulation-pose-pose-leaf1000000-np16": ("middle", "partial_last", "same_block", "three_distinct"),
    "simulation-pose-landmark-leaf1000000-np16": ("middle", "same_block"),
    "mid-se2-leaf50-np16": ("middle", "partial_last", "same_block", "three_distinct"),
    "mid-se3-leaf50-np16": SHAPES,
    "intel-leaf50-np32": SHAPES,
}


@pytest.mark.parametrize("case", GPU_CASES + [INTEL], ids=case_id)
def test_the_gpu_tests_graphs_contain_the_shapes(helper, graphs_dir, case):
    """under the options of an f64 handle (the only ones with arrival order): the shapes, and the tree statistics the GPU test
    demands of its handles"""
    graph, pins = case
    path, se3 = graph_file(graph, graphs_dir)
    shapes, hist, text = run(helper, [path], helper_env(pins, se3))
    for s in EXPECT[case_id(case)]:
        assert shapes[s], (case_id(case), s, hist)
    tree = tuple(int(v) for v in re.search(r"^tree: n_supernodes=(\d+) max_front=(\d+) max_pivot_cols=(\d+)$", text, re.M).groups())
    assert tree == TREES[case_id(case)], (case_id(case), tree)


def test_the_expectations_cover_every_shape():
    assert set(EXPECT) == {case_id(c) for c in GPU_CASES + [INTEL]}
    assert set(EXPECT[case_id(GPU_CASES[0])]) == set(SHAPES)
