"""What tests/test_marginals_big_fronts_cpu.py (the inputs and references alone) and tests/test_marginals_big_fronts_gpu.py
(rr_pgo_marginals under rr_pgo_set_marginals_big_fronts) ask of the cases of tests/big_front_cases.py: every node's diagonal
block and both endpoints of every edge, and the fixed-node set-up of tests/test_big_front_queries_gpu.py.  Nothing here
needs a GPU; every reference is built once and left unchanged."""
import numpy as np

from big_front_cases import at_state, marginals_reference, seeded_nodes

_CACHE = {}


def all_edges(arrays):
    """(from, to) of every edge, in edge order"""
    return np.asarray(arrays[3], np.int32).copy(), np.asarray(arrays[4], np.int32).copy()


def lattice_blocks(name, which):
    """dict(diag, floor_diag, a, b, cross, floor_cross) of a pose lattice at a state: every node's block, every edge's cross block"""
    key = ("lattice", name, which)
    if key not in _CACHE:
        arrays, _ = at_state(name, which)
        ref = marginals_reference(name, which)
        diag, floor_diag = ref.blocks(range(len(arrays[0])))
        a, b = all_edges(arrays)
        cross, floor_cross = ref.blocks(a, b)
        _CACHE[key] = dict(diag=diag, floor_diag=floor_diag, a=a, b=b, cross=cross, floor_cross=floor_cross)
    return _CACHE[key]


def landmark_blocks(which):
    """the same of the landmark case (Landmarks3dReference: 6 x 6, 3 x 3 and 6 x 3 blocks)"""
    key = ("landmarks6", which)
    if key not in _CACHE:
        from landmarks3d_reference import Landmarks3dReference
        arrays, _ = at_state("landmarks6", which)
        ref = Landmarks3dReference(list(arrays))
        sig = ref.sigma_pair()
        diag, floor_diag = ref.blocks(list(range(len(arrays[0]))), sig=sig)
        a, b = all_edges(arrays)
        cross, floor_cross = ref.blocks(a, b, sig=sig)
        _CACHE[key] = dict(diag=diag, floor_diag=floor_diag, a=a, b=b, cross=cross, floor_cross=floor_cross)
    return _CACHE[key]


def fixed_case(in_root=()):
    """dict(arrays, F, priors, prior_nodes, diag, a, b, cross, floor) of lattice6 at its initial state with 20 seeded poses
    fixed (those of `in_root` first: the GPU test passes two nodes of the root front), five priors on free poses and
    keep_anchor = 0 -- the set-up of test_fixed_nodes_and_priors in tests/test_big_front_queries_gpu.py"""
    key = ("fixed", tuple(int(v) for v in in_root))
    if key not in _CACHE:
        from fixed_reference import FixedReference
        from priors_reference import random_priors
        arrays, _ = at_state("lattice6", "initial")
        n = len(arrays[0])
        rng = np.random.default_rng(1977)
        F = sorted(seeded_nodes(n, list(in_root), count=20, seed=1978))
        free = [v for v in range(n) if v not in F]
        prior_nodes = sorted(int(v) for v in rng.choice(free, 5, replace=False))
        priors = random_priors(rng, arrays, prior_nodes, noise=0.05)
        ref = FixedReference(arrays, F, keep_anchor=False, priors=priors)
        sig = ref.sigma_pair()
        diag, f0 = ref.blocks(list(range(n)), sig=sig)
        a, b = all_edges(arrays)
        cross, f1 = ref.blocks(a, b, sig=sig)
        _CACHE[key] = dict(arrays=arrays, F=F, priors=priors, prior_nodes=prior_nodes, diag=diag, a=a, b=b, cross=cross, floor=max(f0, f1))
    return _CACHE[key]
