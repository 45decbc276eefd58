"""The conditions tests/test_marginals_big_fronts_gpu.py puts on its inputs alone, without a GPU: the references' own noise
floors stay within FLOOR_MAX for the lists that test asks -- every diagonal block and every edge's cross block of the three
pose lattices at both states, of the landmark case, and of the fixed-node set-up (here with the 20 seeded poses alone: which
nodes lie in the root front is known on the GPU only, where that test asserts its own floor)."""
import numpy as np
import pytest

from big_front_cases import LATTICES, STATES, at_state
from covariances_cases import FLOOR_MAX
from marginals_big_cases import all_edges, fixed_case, landmark_blocks, lattice_blocks


def shapes_ok(c, arrays):
    nk, ek = np.asarray(arrays[0]), np.asarray(arrays[2])
    dims = np.where(nk == 2, 6, 3)
    assert [d.shape for d in c["diag"]] == [(k, k) for k in dims]
    assert len(c["cross"]) == len(ek) and all(x.shape == (dims[a], dims[b]) for x, a, b in zip(c["cross"], c["a"], c["b"]))


@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("name", list(LATTICES))
def test_the_floors_of_all_nodes_and_all_edges(name, which):
    c = lattice_blocks(name, which)
    arrays, _ = at_state(name, which)
    print(f"{name} {which}: {len(c['diag'])} diagonal blocks, noise floor {c['floor_diag']:.3g}; {len(c['cross'])} edge blocks, noise floor {c['floor_cross']:.3g}")
    shapes_ok(c, arrays)
    a, b = all_edges(arrays)
    assert np.array_equal(a, c["a"]) and np.array_equal(b, c["b"])
    assert c["floor_diag"] <= FLOOR_MAX and c["floor_cross"] <= FLOOR_MAX


@pytest.mark.parametrize("which", STATES)
def test_the_floors_of_the_landmark_case(which):
    c = landmark_blocks(which)
    arrays, _ = at_state("landmarks6", which)
    print(f"landmarks6 {which}: {len(c['diag'])} diagonal blocks, noise floor {c['floor_diag']:.3g}; {len(c['cross'])} edge blocks, noise floor {c['floor_cross']:.3g}")
    shapes_ok(c, arrays)
    assert {d.shape[0] for d in c["diag"]} == {3, 6}
    assert c["floor_diag"] <= FLOOR_MAX and c["floor_cross"] <= FLOOR_MAX


def test_the_floor_of_the_fixed_case():
    c = fixed_case()
    F = c["F"]
    print(f"lattice6 with fixed poses {F} and priors on {c['prior_nodes']}: noise floor {c['floor']:.3g}")
    assert len(F) == 20 and not set(F) & set(c["prior_nodes"])
    assert c["floor"] <= FLOOR_MAX
    assert all(not np.any(c["diag"][v]) for v in F)
    assert any(np.any(c["diag"][v]) for v in range(len(c["diag"])) if v not in F)
