"""Sets of candidates shared by tests/test_gate_joint_cpu.py and tests/test_gate_joint_gpu.py (rr_pgo_gate_joint): ordered
lists of indices into gate_cases.candidates (n candidates, displaced by LADDER[c % 8] sigma).

  - for every rung l of the ladder the first 8 and the first 2 of {c : c % 8 == l}: the members of such a set are displaced
    alike, so the low rungs pass and the high rungs fail;
  - the first 8 candidates and the last 8 (on a graph with landmarks: SE2_XY candidates and the copied SE2 edge);
  - a one-candidate set, and a candidate twice in one set (two independent measurements).
On parking-garage a set of 8 has D_s = 48, the cap (RR_PGO_GATE_JOINT_MAX_DIM)."""
from gate_cases import EDGE_DIM

LADDER_LEN = 8


def joint_sets(n):
    sets = []
    for rung in range(LADDER_LEN):
        members = [c for c in range(n) if c % LADDER_LEN == rung]
        sets.append(members[:8])
        sets.append(members[:2])
    sets.append(list(range(8)))
    sets.append(list(range(n - 8, n)))
    sets.append([0])
    sets.append([3, 3])
    return sets


def set_dims(kind, sets):
    return [sum(EDGE_DIM[int(kind[c])] for c in s) for s in sets]


def block_starts(kind, members):
    """first stacked scalar of every member, and D_s last"""
    o = [0]
    for c in members:
        o.append(o[-1] + EDGE_DIM[int(kind[c])])
    return o
