"""Bearing-only and range-only landmark edges (RR_PGO_EDGE_SE2_BEARING, RR_PGO_EDGE_SE2_RANGE) without a device: the numpy
reference the GPU tests compare against is itself checked -- the Jacobians of the two kinds against central differences in
50-digit arithmetic, its pose-pose and pose-landmark parts against the C oracle -- the fixtures meet the conditions the GPU
tests rely on, and the g2o loader, the mirror's tables and the CLI's file parsers know the new kinds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, g2o_path
from bearing_range_cases import CASES, case, mixed_marks, to_g2o
from bearing_range_reference import BEARING, FLOOR_MAX, RANGE, SE2, SE2_XY, BearingRangeReference, edge_terms
from oracle.oracle import OracleGraph
from robust_reference import oracle_arrays

CSRC = os.path.join(ROOT, "rustrobotics_amd", "csrc")
EPARSE = -3   # RR_PGO_EPARSE


@pytest.fixture(scope="module")
def lib():
    from rustrobotics_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC])
    return _lib.load()


# ---- (a) the Jacobians of the two kinds ---------------------------------------------------------------------------------

def mp_error(mp, kind, pose, l, z, dp, dl):
    """e of the edge at the pose (x, y, theta) + dp and the landmark l + dl, in mpmath: the model of the header, with the wrap
    taken as atan2(sin, cos)"""
    x, y, th = (pose[i] + dp[i] for i in range(3))
    dx, dy = l[0] + dl[0] - x, l[1] + dl[1] - y
    if kind == RANGE:
        return mp.sqrt(dx * dx + dy * dy) - z
    c, s = mp.cos(th), mp.sin(th)
    a = mp.atan2(-s * dx + c * dy, c * dx + s * dy) - z
    return mp.atan2(mp.sin(a), mp.cos(a))


def configurations():
    """seeded (kind, pose, landmark, z): rho from 0.5 to 50, headings over the circle, bearing errors near +pi and -pi"""
    rng = np.random.default_rng(61)
    out = []
    for rho in (0.5, 0.9, 3.0, 12.0, 50.0):
        for _ in range(3):
            pose = np.array([rng.normal() * 5, rng.normal() * 5, rng.uniform(-np.pi, np.pi)])
            ang = rng.uniform(-np.pi, np.pi)
            l = pose[:2] + rho * np.array([np.cos(ang), np.sin(ang)])
            bearing = np.arctan2(np.sin(ang - pose[2]), np.cos(ang - pose[2]))
            out.append((RANGE, pose, l, rho + rng.normal() * 0.1))
            out.append((BEARING, pose, l, bearing + rng.normal() * 0.05))
            for off in (np.pi - 0.01, -(np.pi - 0.01), np.pi - 1e-6):   # the error itself near the cut
                out.append((BEARING, pose, l, float(np.arctan2(np.sin(bearing - off), np.cos(bearing - off)))))
    return out


def test_jacobians_against_central_differences():
    """A and B of the reference against central differences of e under the additive increments (x, y, theta) and (l_x, l_y),
    50 digits, step 1e-10: exact to about 1e-20 relative (h^2), so the closed forms must agree to f64 rounding, 1e-13 of the
    largest entry (the bound of tests/test_landmarks3d_cpu.py).  e itself: 1e-14 of max(1, |e|) -- but where z is within
    1e-6 of the cut the f64 sum bearing - z has already lost the digits that |e - pi| needs, hence e is compared as an angle."""
    import mpmath as mp
    mp.mp.dps = 50
    h = mp.mpf(10) ** -10
    worst_all = 0.0
    for kind, pose, l, z in configurations():
        e, A, B = edge_terms(kind, np.array([pose[0], pose[1], np.cos(pose[2]), np.sin(pose[2])]), np.array([l[0], l[1], 0.0, 0.0]), [z])
        assert e.shape == (1,) and A.shape == (1, 3) and B.shape == (1, 2)
        f = lambda v: [mp.mpf(float(t)) for t in v]
        args = (kind, f(pose), f(l), mp.mpf(float(z)))
        zero3, zero2 = [mp.mpf(0)] * 3, [mp.mpf(0)] * 2
        e0 = mp_error(mp, *args, zero3, zero2)
        de = float(mp.atan2(mp.sin(e0 - mp.mpf(float(e[0]))), mp.cos(e0 - mp.mpf(float(e[0]))))) if kind == BEARING else float(e0) - e[0]
        assert abs(de) <= 1e-14 * max(1.0, abs(e[0]), np.abs(pose).max()), (kind, pose, l, z, de)
        assert -np.pi < e[0] <= np.pi
        J = np.zeros(5)
        for c in range(5):
            d = [mp.mpf(0)] * 5
            d[c] = h
            ep = mp_error(mp, *args, d[:3], d[3:])
            d[c] = -h
            em = mp_error(mp, *args, d[:3], d[3:])
            diff = ep - em
            if kind == BEARING:   # (a step across the cut moves e by 2 pi: the derivative is that of the angle)
                diff = mp.atan2(mp.sin(diff), mp.cos(diff))
            J[c] = float(diff / (2 * h))
        worst = np.abs(np.hstack([A, B])[0] - J).max()
        worst_all = max(worst_all, worst / max(1.0, np.abs(J).max()))
        assert worst <= 1e-13 * max(1.0, np.abs(J).max()), (kind, pose, l, z, np.hstack([A, B]), J)
    print(f"worst disagreement of a Jacobian entry, relative to max(1, max|J|): {worst_all:.3g}")


def test_bearing_error_is_the_wrapped_difference():
    """e = wrap(atan2(p_y, p_x) - z) into (-pi, pi]: a true bearing just short of pi measured just past the cut gives a small e"""
    pose, l = np.array([0.0, 0.0, 1.0, 0.0]), np.array([-3.0, 0.1, 0.0, 0.0])
    true = np.arctan2(0.1, -3.0)
    e, _, _ = edge_terms(BEARING, pose, l, [-(np.pi - 0.01)])
    np.testing.assert_allclose(e[0], true - np.pi - 0.01, rtol=0, atol=1e-15)
    e, _, _ = edge_terms(BEARING, pose, l, [np.pi])
    assert abs(e[0] - (true - np.pi)) <= 1e-15


# ---- (b) the reference against the oracle, on a graph without the new kinds ---------------------------------------------

def test_reference_equals_the_oracle_on_pose_landmark_graph():
    """simulation-pose-landmark.g2o: H, b and chi2 of the numpy reference against og_build_system / og_global_error, at
    1e-12 of max|H|, 1e-11 of max|b| and 1e-12 relative (the figures tests/landmarks3d_reference.py was held to), plain and
    with lambda; then one step and the update"""
    o = OracleGraph.load(g2o_path("simulation-pose-landmark"))
    arrays = oracle_arrays(o)
    ref = BearingRangeReference(arrays)
    np.testing.assert_allclose(ref.cost(), o.global_error(), rtol=1e-12)
    for lam, lm in ((0.0, False), (0.37, True)):
        colptr, rowidx, vals, b = o.build_system(lam, lm)
        n = o.dim
        H = np.zeros((n, n))
        H[rowidx, np.repeat(np.arange(n), np.diff(colptr))] = vals
        H = H + np.tril(H, -1).T
        H2, b2 = ref.system(lam, lm)
        print(f"lm={lm}: H worst {np.abs(H - H2).max():.3g} of {np.abs(H).max():.3g}, b worst {np.abs(b - b2).max():.3g} of {np.abs(b).max():.3g}")
        assert np.abs(H - H2).max() <= 1e-12 * np.abs(H).max()
        assert np.abs(b - b2).max() <= 1e-11 * np.abs(b).max()
    s = ref.edge_s()
    for k in (0, 5, len(s) - 1):
        A, B, e = o.linearize_edge(k)
        np.testing.assert_allclose(s[k], float(e @ o.edge_info(k) @ e), rtol=1e-12)
    dx = ref.step()
    ref.update(dx)
    o.update_nodes(dx, 1.0)
    np.testing.assert_allclose(ref.state(), o.state(), rtol=0, atol=1e-12)
    e_ref, _ = BearingRangeReference(arrays).optimize(10)
    e_o = OracleGraph.from_arrays(*arrays).optimize(10)
    assert len(e_ref) == len(e_o)
    np.testing.assert_allclose(e_ref, e_o, rtol=1e-7)


# ---- (c) the fixtures ---------------------------------------------------------------------------------------------------

def observed_rho(ref):
    return np.array([np.hypot(*(ref.x[ref.et[k]][:2] - ref.x[ref.ef[k]][:2])) for k in range(ref.E) if ref.ek[k] != SE2])


@pytest.mark.parametrize("name", CASES + ("beacons-fixed",))
def test_fixture_meets_its_conditions(name):
    """at the initial and at the converged state: H is positive definite with cond(H) <= 1e12 and every observed rho >= 0.5; the
    reference Gauss-Newton loop stops by its rule within 20 iterations; every noise floor of the two-Sigma rule is at most
    FLOOR_MAX (tri2: both bearings are bridges, r = 0, and nothing else is compared for them)"""
    arrays = case(name.split("-")[0])
    fixed = [v for v in range(len(arrays[0])) if arrays[0][v] == 1] if name.endswith("-fixed") else []
    # (surveyed beacons fix the gauge: the 1e7 anchor term on a pose at its noisy initial value would fight them)
    ref = BearingRangeReference(arrays, fixed=fixed, fixed_keep_anchor=not fixed)
    for label in ("initial", "converged"):
        if label == "converged":
            errors, norms = ref.optimize(20)
            assert len(norms) < 20 and norms[-1] < 1e-4, (name, norms)
            print(f"{name}: chi2 {errors[0]:.6g} -> {errors[-1]:.6g} in {len(norms)} iterations")
        H, _ = ref.free_system()
        np.linalg.cholesky(H)
        cond = np.linalg.cond(H)
        rho_min = observed_rho(ref).min()
        print(f"{name} {label}: {ref.n} unknowns, {ref.E} edges, cond(H) {cond:.3g}, smallest observed rho {rho_min:.3g}")
        assert cond <= 1e12 and rho_min >= 0.5
        sig = ref.sigma_pair()
        chk = ref.check(range(ref.E), sig)
        floors = {k: v for k, v in chk.items() if k.startswith("floor")}
        print(f"{name} {label}: {floors}, r in [{chk['r'].min():.3g}, {chk['r'].max():.3g}]")
        assert all(v <= FLOOR_MAX for v in floors.values()), floors
        nodes = list(range(ref.N))
        _, floor = ref.blocks(nodes, nodes, sig)
        assert floor <= FLOOR_MAX
        if name == "tri2":
            br = np.flatnonzero(ref.ek == BEARING)
            assert len(br) == 2 and np.all(np.abs(chk["r"][br]) <= 1e-9), chk["r"]
    # per-edge errors: the reference's f64 against 50 digits
    s, s_mp = ref.edge_s(), ref.edge_s_mp()
    floor = float(np.max(np.abs(s - s_mp) / np.maximum(s_mp, 1e-300)))
    print(f"{name}: per-edge e^T Omega e, f64 against 50 digits: worst relative {floor:.3g}")
    if name != "tri2":    # (its bridges are fitted exactly: s is zero up to rounding and has no relative floor)
        assert floor <= FLOOR_MAX


def test_mixed_holds_what_it_is_for():
    arrays = case("mixed")
    nk, _, ek, ef, et, em, _ = arrays
    assert nk[0] == 1                                                      # a landmark sits at node 0
    assert {int(k) for k in ek} == {SE2, SE2_XY, BEARING, RANGE}
    a, b = mixed_marks()["parallel"]
    assert (ef[a], et[a]) == (ef[b], et[b]) and {int(ek[a]), int(ek[b])} == {BEARING, RANGE}
    assert np.sum(et == mixed_marks()["many"]) >= 9
    ref = BearingRangeReference(arrays)
    k = mixed_marks()["cut"]
    x1, x2 = ref.x[ef[k]], ref.x[et[k]]
    d = x2[:2] - x1[:2]
    pred = np.arctan2(-x1[3] * d[0] + x1[2] * d[1], x1[2] * d[0] + x1[3] * d[1])
    assert ek[k] == BEARING and pred > np.pi - 0.1 and ref.z[k][0] < -3.0 and abs(ref.lin(k)[0][0]) < 0.2


def test_corridor_tree_has_several_levels(lib, tmp_path):
    from rustrobotics_amd import _lib
    opt, st = _lib.Options(), _lib.Stats()
    lib.rr_pgo_default_options(C.byref(opt))
    p = tmp_path / "corridor.g2o"
    p.write_text(to_g2o(case("corridor")))
    assert lib.rr_pgo_analyze_g2o(str(p).encode(), C.byref(opt), C.byref(st)) == 0, lib.rr_pgo_last_error().decode()
    print(f"corridor: {st.n_supernodes} fronts, widest pivot block {st.max_pivot_cols}")
    assert st.n_supernodes >= 4


# ---- (d) the loader -------------------------------------------------------------------------------------------------------

def analyse(lib, tmp_path, name, text):
    from rustrobotics_amd import _lib
    opt, st = _lib.Options(), _lib.Stats()
    lib.rr_pgo_default_options(C.byref(opt))
    p = tmp_path / name
    p.write_text(text)
    rc = lib.rr_pgo_analyze_g2o(str(p).encode(), C.byref(opt), C.byref(st))
    return rc, lib.rr_pgo_last_error().decode(), st


@pytest.mark.parametrize("name", CASES)
def test_loader_reads_both_tags(lib, tmp_path, name):
    arrays = case(name)
    rc, msg, st = analyse(lib, tmp_path, "ok.g2o", to_g2o(arrays))
    assert rc == 0, msg
    assert st.nnz_h_blocks == len(arrays[0]) + len(arrays[2])     # every edge has its block: parallel edges are two edges with two blocks


def test_loader_failures_name_their_line(lib, tmp_path):
    lines = to_g2o(case("tri")).splitlines()   # 0-2: poses, 3: the landmark, 4-5: EDGE_SE2, 6-8: EDGE_BEARING_SE2_XY
    assert lines[6].startswith("EDGE_BEARING_SE2_XY")

    def text(edit):
        ls = list(lines)
        edit(ls)
        return "\n".join(ls) + "\n"

    def count(ls):
        ls[6] = ls[6] + " 1.0"
    rc, msg, _ = analyse(lib, tmp_path, "count.g2o", text(count))
    assert rc == EPARSE and msg.startswith("line 7:") and "expected 2 values" in msg, msg

    def short(ls):
        ls[7] = " ".join(ls[7].split()[:-1])
    rc, msg, _ = analyse(lib, tmp_path, "short.g2o", text(short))
    assert rc == EPARSE and msg.startswith("line 8:") and "expected 2 values" in msg, msg

    for bad in ("0", "-4.0"):
        def info(ls, bad=bad):
            ls[8] = " ".join(ls[8].split()[:-1] + [bad])
        rc, msg, _ = analyse(lib, tmp_path, "info.g2o", text(info))
        assert rc == EPARSE and msg.startswith("line 9:") and "information value must be positive" in msg, msg

    def range_info(ls):
        ls.append("EDGE_RANGE_SE2_XY 0 3 3.0 0")
    rc, msg, _ = analyse(lib, tmp_path, "rinfo.g2o", text(range_info))
    assert rc == EPARSE and msg.startswith("line 10:") and "information value must be positive" in msg, msg

    def pose_to_pose(ls):
        ls.append("EDGE_BEARING_SE2_XY 0 1 0.3 100")
    rc, msg, _ = analyse(lib, tmp_path, "pp.g2o", text(pose_to_pose))
    assert rc == EPARSE and msg.startswith("line 10:") and "EDGE_BEARING_SE2_XY goes from an SE2 pose to an XY landmark" in msg, msg

    def landmark_to_landmark(ls):
        ls.insert(4, "VERTEX_XY 9 1 1")
        ls.append("EDGE_BEARING_SE2_XY 3 9 0.3 100")
    rc, msg, _ = analyse(lib, tmp_path, "ll.g2o", text(landmark_to_landmark))
    assert rc == EPARSE and msg.startswith("line 11:") and "goes from an SE2 pose to an XY landmark" in msg, msg

    def backwards(ls):
        ls.append("EDGE_RANGE_SE2_XY 3 0 3.0 100")
    rc, msg, _ = analyse(lib, tmp_path, "back.g2o", text(backwards))
    assert rc == EPARSE and msg.startswith("line 10:") and "EDGE_RANGE_SE2_XY goes from an SE2 pose to an XY landmark" in msg, msg

    # stock g2o's other bearing / range spellings stay unsupported tags
    rc, msg, _ = analyse(lib, tmp_path, "tag.g2o", text(lambda ls: ls.append("EDGE_SE2_POINTXY_BEARING 0 3 0.3 100")))
    assert rc == EPARSE and msg.startswith("line 10:") and "unsupported tag" in msg, msg


def test_neither_kind_sets_the_anchor(lib, tmp_path):
    """a graph whose only edges are bearing and range edges has no pose-pose edge: it loads, and nothing anchors it"""
    text = "VERTEX_SE2 0 0 0 0\nVERTEX_XY 1 2 1\nEDGE_BEARING_SE2_XY 0 1 0.46 100\nEDGE_RANGE_SE2_XY 0 1 2.2 100\n"
    rc, msg, st = analyse(lib, tmp_path, "noanchor.g2o", text)
    assert rc == 0, msg
    assert st.nnz_h_blocks == 4   # two diagonal blocks, and a block for each of the two parallel edges


# ---- (e) the mirror and the CLI's parsers ----------------------------------------------------------------------------------

def test_python_tables_know_the_new_kinds():
    from rustrobotics_amd import mapping
    from rustrobotics_amd.__main__ import GATE_TAGS
    for k in (4, 6):
        assert mapping.GATE_EDGE_DIM[k] == 1 and mapping.GATE_MEAS_LEN[k] == 1 and mapping.GATE_INFO_LEN[k] == 1
        assert mapping.GATE_DEFAULT_THRESHOLD[k] == mapping.CHI2_95[1] == 3.841
    assert 5 not in mapping.KNOWN_KINDS and 7 not in mapping.KNOWN_KINDS and 5 not in mapping.GATE_DEFAULT_THRESHOLD
    assert GATE_TAGS["EDGE_BEARING_SE2_XY"] == 4 and GATE_TAGS["EDGE_RANGE_SE2_XY"] == 6
    assert list(mapping.gate_thresholds([4, 6, 1, 0])) == [3.841, 3.841, mapping.CHI2_95_2, mapping.CHI2_95_3]
    assert list(mapping.gate_joint_dims([4, 6, 1, 0], [[0, 1, 2, 3], [0, 1], [3, 0]])) == [7, 2, 4]
    assert list(mapping.gate_joint_thresholds([4, 6, 1, 0], [[0, 1, 2, 3], [1]])) == [mapping.CHI2_95[7], mapping.CHI2_95[1]]
    header = open(os.path.join(ROOT, "include", "rr_pgo.h")).read()
    assert "RR_PGO_EDGE_SE2_BEARING = 4" in header and "RR_PGO_EDGE_SE2_RANGE = 6" in header and "reserved" in header


def test_mirror_refuses_arrays_of_the_wrong_length():
    """one measurement value and one information value per edge of the kinds: the mirror's length checks of gate_edges,
    gate_joint and extend refuse anything else before the library is called (no handle is needed to get that far)"""
    from rustrobotics_amd import PoseGraph
    g = PoseGraph.__new__(PoseGraph)
    g._h = None
    for fn in (lambda k, m, w: g.gate_edges([k], [0], [1], m, w), lambda k, m, w: g.extend([k], [0], [1], m, w),
               lambda k, m, w: g.gate_joint([k], [0], [1], m, w, [[0]])):
        for k in (BEARING, RANGE):
            for m, w in (([0.3, 0.1], [100.0]), ([0.3], [100.0, 0.0, 100.0]), ([], [100.0]), ([0.3], [])):
                with pytest.raises(ValueError) as e:
                    fn(k, m, w)
                assert "do not have the length the edge kinds ask for" in str(e.value)


def test_file_parsers_read_both_tags(tmp_path):
    from rustrobotics_amd.__main__ import parse_extend_file, parse_gate_file
    p = tmp_path / "cand.txt"
    p.write_text("EDGE_BEARING_SE2_XY 4 9 0.25 400\nEDGE_RANGE_SE2_XY 4 9 3.5 100\nEDGE_SE2_XY 4 9 1 2 10 0 10\nSET 0 1 2\n")
    sets = []
    kind, a, b, meas, info, ids = parse_gate_file(str(p), {4: 0, 9: 1}, sets=sets)
    assert (kind, a, b) == ([4, 6, 1], [0, 0, 0], [1, 1, 1])
    assert meas == [0.25, 3.5, 1.0, 2.0] and info == [400.0, 100.0, 10.0, 0.0, 10.0] and sets == [(4, [0, 1, 2])]
    p.write_text("EDGE_BEARING_SE2_XY 4 9 0.25\n")
    with pytest.raises(SystemExit) as e:
        parse_gate_file(str(p), {4: 0, 9: 1})
    assert "expected 2 values after the ids, got 1" in str(e.value), str(e.value)
    p.write_text("VERTEX_XY 12 1.0 2.0\nEDGE_RANGE_SE2_XY 4 12 2.5 100\nEDGE_BEARING_SE2_XY 4 12 0.1 400\n")
    nkind, nid, nstate, kind, a, b, meas, info = parse_extend_file(str(p), {4: 0, 9: 1})
    assert (nkind, nid, nstate, kind, a, b, meas, info) == ([1], [12], [1.0, 2.0], [6, 4], [0, 0], [2, 2], [2.5, 0.1], [100.0, 400.0])
    # the messages about an unknown tag name the two tags
    p.write_text("EDGE_BEARING 4 9 0.25 400\n")
    for parse in (parse_gate_file, parse_extend_file):
        with pytest.raises(SystemExit) as e:
            parse(str(p), {4: 0, 9: 1})
        assert "unknown tag 'EDGE_BEARING'" in str(e.value) and "EDGE_BEARING_SE2_XY, EDGE_RANGE_SE2_XY" in str(e.value), str(e.value)
