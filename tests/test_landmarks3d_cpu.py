"""3-D point landmarks (RR_PGO_NODE_XYZ, RR_PGO_EDGE_SE3_XYZ) without a device: the numpy reference the GPU tests compare
against is itself checked -- the point edge's Jacobians against central differences in 50-digit arithmetic, its SE(3) part
against the C oracle -- and the g2o loader and the Python tables know the new kinds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, g2o_path
from landmarks3d_cases import CASES, case, to_g2o
from landmarks3d_reference import Landmarks3dReference, point_edge
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


# ---- (a) the Jacobians of the point edge ------------------------------------------------------------------------------

def mp_error(mp, t, q, l, z, dt, dw, dl):
    """e of the point edge at the pose (t, q) * (dt, Exp(dw)) and the landmark l + dl, in mpmath"""
    def qmul(a, b):
        return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]

    def rot(q, v):   # q (x) (v, 0) (x) q^-1
        r = qmul(qmul(q, list(v) + [mp.mpf(0)]), [-q[0], -q[1], -q[2], q[3]])
        return r[:3]

    th = mp.sqrt(sum(w * w for w in dw))
    dq = [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)] if th == 0 else [mp.sin(th / 2) / th * w for w in dw] + [mp.cos(th / 2)]
    rdt = rot(q, dt)
    t2 = [t[i] + rdt[i] for i in range(3)]
    q2 = qmul(q, dq)
    n = mp.sqrt(sum(c * c for c in q2))
    q2 = [c / n for c in q2]
    d = [l[i] + dl[i] - t2[i] for i in range(3)]
    p = rot([-q2[0], -q2[1], -q2[2], q2[3]], d)
    return [p[i] - z[i] for i in range(3)]


def test_point_edge_jacobians_against_central_differences():
    """A = [-I | [p]x] and B = R^T against central differences of e under the stated increments (right increment on the pose,
    additive on the landmark), 50 digits, step 1e-10: the rule of tests/golden/se3_jacobians.json.  The differences are exact
    to about 1e-20 (h^2), so the closed forms must agree to f64 rounding: 1e-13 of the largest entry."""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(41)
    quats = [rng.normal(size=4) for _ in range(4)]
    quats.append(np.array([0.3, -0.5, 0.2, -0.7]))                                   # w < 0
    ax = np.array([0.6, -0.48, 0.64])
    quats.append(np.concatenate([np.sin((np.pi - 1e-4) / 2) * ax, [np.cos((np.pi - 1e-4) / 2)]]))   # a rotation near pi
    h = mp.mpf(10) ** -10
    for q in quats:
        q = q / np.linalg.norm(q)
        t, l, z = rng.normal(size=3) * 3, rng.normal(size=3) * 3, rng.normal(size=3)
        e, A, B = point_edge(np.concatenate([t, q]), l, z)
        qm = [mp.mpf(float(c)) for c in q]
        nq = mp.sqrt(sum(c * c for c in qm))
        qm = [c / nq for c in qm]
        args = ([mp.mpf(float(c)) for c in t], qm, [mp.mpf(float(c)) for c in l], [mp.mpf(float(c)) for c in z])
        zero = [mp.mpf(0)] * 3
        e0 = mp_error(mp, *args, zero, zero, zero)
        assert max(abs(float(e0[i]) - e[i]) for i in range(3)) <= 1e-14 * max(1.0, np.abs(e).max())
        J = np.zeros((3, 9))
        for c in range(9):
            d = [[mp.mpf(0)] * 3 for _ in range(3)]
            d[c // 3][c % 3] = h
            ep = mp_error(mp, *args, *d)
            d[c // 3][c % 3] = -h
            em = mp_error(mp, *args, *d)
            J[:, c] = [float((ep[i] - em[i]) / (2 * h)) for i in range(3)]
        worst = np.abs(np.hstack([A, B]) - J).max()
        print(f"q = {q}: worst {worst:.3g}, max|J| {np.abs(J).max():.3g}")
        assert worst <= 1e-13 * max(1.0, np.abs(J).max())


# ---- (b) the SE(3) part of the reference against the oracle ---------------------------------------------------------

def test_se3_part_of_the_reference_equals_the_oracle():
    """the first 30 poses of parking-garage and the edges among them: H, b and chi2 of the numpy reference against
    og_build_system / og_global_error (1e-12 of max|H|, 1e-11 of max|b|, 1e-12 relative), plain and with lambda.
    At the file's own state the residuals are the rounding of the file's decimals (chi2 = 3.8e-10, e about 1e-7 from
    coordinates of size 10): there e carries a relative error of 1e-16 * 10 / 1e-7 = 1e-8 in any f64 code, so chi2 and b are
    compared at a second, seeded state a few centimetres and degrees away, where they are well conditioned; H, which does not
    depend on e, is compared at both."""
    nk, ns, ek, ef, et, em, ei = oracle_arrays(OracleGraph.load(g2o_path("parking-garage")))
    keep = np.flatnonzero((ef < 30) & (et < 30))
    arrays = [nk[:30], ns[:30 * 7], ek[keep], ef[keep], et[keep], em.reshape(-1, 7)[keep].ravel(), ei.reshape(-1, 21)[keep].ravel()]
    rng = np.random.default_rng(43)
    moved = Landmarks3dReference(arrays)
    moved.update(rng.normal(scale=0.05, size=moved.n))
    for label, state in (("file state", arrays[1]), ("moved", moved.state())):
        a = list(arrays)
        a[1] = state
        o = OracleGraph.from_arrays(*a)
        ref = Landmarks3dReference(a)
        print(f"{label}: chi2 {ref.cost():.15g} against {o.global_error():.15g}")
        if label == "moved":
            np.testing.assert_allclose(ref.cost(), o.global_error(), rtol=1e-12)
        for lam, lm in ((0.0, False), (0.37, True)):
            colptr, rowidx, vals, b = o.build_system(lam, lm)
            n = o.dim
            H = np.zeros((n, n))
            H[rowidx, np.repeat(np.arange(n), np.diff(colptr))] = vals
            H = H + np.tril(H, -1).T
            H2, b2 = ref.system(lam, lm)
            print(f"{label} lm={lm}: H worst {np.abs(H - H2).max():.3g} of {np.abs(H).max():.3g}, b worst {np.abs(b - b2).max():.3g} of {np.abs(b).max():.3g}")
            assert np.abs(H - H2).max() <= 1e-12 * np.abs(H).max()
            if label == "moved":
                assert np.abs(b - b2).max() <= 1e-11 * np.abs(b).max()
        # one step and the update: the states agree
        dx = ref.step()
        ref.update(dx)
        o.update_nodes(dx, 1.0)
        np.testing.assert_allclose(ref.state(), o.state(), rtol=0, atol=1e-12)


# ---- (c) the loader ---------------------------------------------------------------------------------------------------

def analyse(lib, tmp_path, name, text):
    from rustrobotics_amd import _lib
    opt, st = _lib.Options(), _lib.Stats()
    lib.rr_pgo_default_options(C.byref(opt))
    p = tmp_path / name
    p.write_text(text)
    rc = lib.rr_pgo_analyze_g2o(str(p).encode(), C.byref(opt), C.byref(st))
    return rc, lib.rr_pgo_last_error().decode(), st


@pytest.mark.parametrize("name", CASES)
def test_loader_reads_the_three_tags(lib, tmp_path, name):
    arrays = case(name)
    rc, msg, st = analyse(lib, tmp_path, "ok.g2o", to_g2o(arrays))
    assert rc == 0, msg
    pairs = {(min(a, b), max(a, b)) for a, b in zip(arrays[3], arrays[4])}
    assert st.nnz_h_blocks == len(arrays[0]) + len(pairs)
    if name == "corridor":
        print(f"corridor: {st.n_supernodes} fronts in {st.n_levels} levels, widest pivot block {st.max_pivot_cols}")
        # (rr_pgo_stats counts schedule steps, not tree levels: test_corridor_tree_is_deep_and_mixes_the_kinds looks at the tree)
        assert st.n_supernodes >= 4 and st.max_pivot_cols > 6


def native(tmp_path, source):
    exe = tmp_path / source.replace(".cpp", "")
    srcs = [os.path.join(ROOT, "tests", "native", source)] + [os.path.join(CSRC, f) for f in ("symbolic.cpp", "g2o_loader.cpp", "synth_grid.cpp")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", CSRC, *srcs, "-o", str(exe)])
    return str(exe)


def test_corridor_tree_is_deep_and_mixes_the_kinds(tmp_path):
    """what the corridor case is for: under the options of an f64 handle its elimination tree has at least 3 levels and a front
    whose pivot columns hold poses and landmarks (tests/native/landmark_tree_check.cpp reads the symbolic tables); and the
    host-only multifrontal walk of the same tables (tests/native/mf_host_check.cpp), with the blocks of 6 and 3 scalars,
    solves a random SPD system on the pattern of room and of corridor"""
    files = {}
    for name in ("room", "corridor"):
        files[name] = tmp_path / f"{name}.g2o"
        files[name].write_text(to_g2o(case(name)))
    out = subprocess.run([native(tmp_path, "landmark_tree_check.cpp"), str(files["corridor"])], capture_output=True, text=True, check=True).stdout
    print(out)
    tok = out.split()
    got = {tok[i]: int(tok[i + 1]) for i in range(0, len(tok), 2)}
    assert got["depth"] >= 3 and got["mixed"] >= 1 and got["widest_mixed"] > 6, got
    mfcheck = native(tmp_path, "mf_host_check.cpp")
    for name, env in (("room", {"FLOW": "1"}), ("corridor", {"FLOW": "1"}), ("corridor", {"LDS": "2000"})):
        r = subprocess.run([mfcheck, str(files[name])], capture_output=True, text=True, env={**os.environ, **env})
        print(name, env, r.stdout.strip().splitlines()[-2:])
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (name, env, r.stdout)


def test_loader_failures_name_their_line(lib, tmp_path):
    arrays = case("two-poses-one-point")
    lines = to_g2o(arrays).splitlines()   # 0: PARAMS, 1-3: vertices, 4: EDGE_SE3, 5-6: EDGE_SE3_TRACKXYZ

    def text(edit):
        ls = list(lines)
        edit(ls)
        return "\n".join(ls) + "\n"

    def offset(ls):
        ls[0] = "PARAMS_SE3OFFSET 0 0.1 0 0 0 0 0 1"
    rc, msg, _ = analyse(lib, tmp_path, "offset.g2o", text(offset))
    assert rc == EPARSE and msg.startswith("line 1:") and "sensor offsets are not supported" in msg, msg

    def count(ls):
        ls[5] = ls[5] + " 1.0"
    rc, msg, _ = analyse(lib, tmp_path, "count.g2o", text(count))
    assert rc == EPARSE and msg.startswith("line 6:") and "expected 9 values" in msg, msg

    def backwards(ls):
        tok = ls[6].split()
        tok[1], tok[2] = tok[2], tok[1]
        ls[6] = " ".join(tok)
    rc, msg, _ = analyse(lib, tmp_path, "backwards.g2o", text(backwards))
    assert rc == EPARSE and msg.startswith("line 7:") and "from an SE3 pose to an XYZ landmark" in msg, msg

    def mixed(ls):
        ls.insert(4, "VERTEX_SE2 77 0 0 0")
    rc, msg, _ = analyse(lib, tmp_path, "mixed.g2o", text(mixed))
    assert rc == EPARSE and msg.startswith("line 5:") and "mixed 2D / 3D" in msg, msg

    # the parameter id is an unsigned integer; FIX and every other tag stay errors
    def pid(ls):
        tok = ls[5].split()
        tok[3] = "x"
        ls[5] = " ".join(tok)
    rc, msg, _ = analyse(lib, tmp_path, "pid.g2o", text(pid))
    assert rc == EPARSE and msg.startswith("line 6:"), msg
    rc, msg, _ = analyse(lib, tmp_path, "fix.g2o", text(lambda ls: ls.append("FIX 0")))
    assert rc == EPARSE and msg.startswith("line 8:") and "unsupported tag" in msg, msg


# ---- (d) the Python tables ----------------------------------------------------------------------------------------------

def test_python_tables_know_the_new_kinds():
    from rustrobotics_amd import mapping
    from rustrobotics_amd.__main__ import GATE_TAGS, VERTEX_TAGS
    assert mapping.GATE_EDGE_DIM[3] == 3 and mapping.GATE_MEAS_LEN[3] == 3 and mapping.GATE_INFO_LEN[3] == 6
    assert mapping.GATE_DEFAULT_THRESHOLD[3] == mapping.CHI2_95_3
    assert mapping.NODE_DIM == (3, 2, 6, 3) and mapping.NODE_STATE_LEN == (3, 2, 7, 3)
    assert GATE_TAGS["EDGE_SE3_TRACKXYZ"] == 3 and VERTEX_TAGS["VERTEX_TRACKXYZ"] == 3
    assert list(mapping.gate_thresholds([2, 3])) == [mapping.CHI2_95_6, mapping.CHI2_95_3]
    assert list(mapping.gate_joint_dims([2, 3, 3], [[0, 1], [1, 2]])) == [9, 6]
    header = open(os.path.join(ROOT, "include", "rr_pgo.h")).read()
    assert "RR_PGO_NODE_XYZ = 3" in header and "RR_PGO_EDGE_SE3_XYZ = 3" in header


def test_gate_file_parser_reads_trackxyz(tmp_path):
    from rustrobotics_amd.__main__ import parse_gate_file
    p = tmp_path / "cand.txt"
    p.write_text("EDGE_SE3_TRACKXYZ 4 9 0 1 2 3 10 0 0 10 0 10\n")
    kind, a, b, meas, info, ids = parse_gate_file(str(p), {4: 0, 9: 1})
    assert (kind, a, b, meas, info, ids) == ([3], [0], [1], [1.0, 2.0, 3.0], [10.0, 0.0, 0.0, 10.0, 0.0, 10.0], [(4, 9)])


def test_gate_file_messages_name_the_parameter_id(tmp_path):
    from rustrobotics_amd.__main__ import parse_gate_file
    p = tmp_path / "cand.txt"
    p.write_text("EDGE_SE3_TRACKXYZ 4 9 0 1 2 3 10 0 0 10 0\n")
    with pytest.raises(SystemExit) as e:
        parse_gate_file(str(p), {4: 0, 9: 1})
    assert "expected 9 values after the ids, a parameter id, got 8" in str(e.value), str(e.value)
    p.write_text("EDGE_SE3_TRACKXYZ 4 9 x 1 2 3 10 0 0 10 0 10\n")
    with pytest.raises(SystemExit) as e:
        parse_gate_file(str(p), {4: 0, 9: 1})
    assert "expected two vertex ids, a parameter id and 9 numbers after EDGE_SE3_TRACKXYZ" in str(e.value), str(e.value)
