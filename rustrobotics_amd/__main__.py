"""Non-interactive counterpart of the reference's example and bench for this path.

  python -m rustrobotics_amd <file.g2o> [--solver GaussNewton|LevenbergMarquardt] [--iterations 50]
                                        [--precision f64|f32|mixed] [--plot]
      = examples/mapping/pose_graph_optimization.rs:49-50   PoseGraph::new(file, solver)?.optimize(50, true, plot)
        (the reference picks file / solver / plot from interactive menus; --plot writes img/{name}-{iteration}-{solver}.svg
        before the first and after every iteration, like :266-268, :294-296)

  --robust huber:DELTA | cauchy:DELTA  (both modes): a robust kernel on every edge (include/rr_pgo.h); the errors printed
      are then the robust cost

  --gnc DELTA[:loops|all]  (example mode): instead of the plain optimisation, graduated non-convexity on truncated least squares
      (rr_pgo_optimize_gnc): DELTA^2 is the chi-square quantile beyond which an edge is an outlier (3.3682 for 0.99 at 3 degrees
      of freedom); `loops` (the default) robustifies the edges with |from - to| > 1 and trusts the odometry, `all` every edge
      (a node whose every edge is rejected then ends the run: not positive definite).  Prints the stages, mu0, mu_last and
      the indices of the rejected edges; everything printed afterwards sees the final weights

  --priors FILE  (both modes): absolute priors (rr_pgo_set_priors), one per line: NODE_ID (the g2o vertex id), then the
      measurement and the upper triangle of the information matrix in g2o's order for the node's kind (SE2 pose: x y theta
      and 6 values; XY landmark: x y and 3; SE3 pose: x y z qx qy qz qw and 21); `#` starts a comment.  A vertex may be
      named any number of times.  With --free-anchor the 1e7 term on the anchor node is dropped and the priors alone fix
      the gauge.  Both apply before --robust and the optimisation; the report prints the priors' share of the final cost

  --fix ID,ID,...  (both modes): hold these g2o vertex ids constant (rr_pgo_set_fixed): they never move, and the
      covariances and gates printed afterwards are conditional on them.  With --free-anchor the fixed set (plus any
      priors) fixes the gauge.  Applied before --robust and the optimisation

  --init chordal  (both modes): before the optimisation, replace the state of every free vertex by the chordal relaxation of
      the graph (rr_pgo_initialize: relaxed rotations, projection onto SO(d), positions); fixed vertices and the kept anchor
      stay.  Applied after --priors and --fix, which it reads, and before --robust, which it ignores.  The example mode
      prints chi2 before and after the initialisation and the call's three times

  --marginals FILE  (example mode): after the optimisation, one line per node -- id, d, the upper triangle of its d x d
      covariance block (rr_pgo_marginals; f64 handles whose fronts all live in LDS)

  --joint ID,ID,...  (example mode): after the optimisation, the joint covariance of the listed g2o vertex ids -- any
      nodes, joined by an edge or not (rr_pgo_covariances) -- one matrix row per line

  --cross FILE --columns ID,ID,... [--rows ID,ID,...]  (example mode): after the optimisation, the rectangular block
      Sigma[rows, columns] of the listed g2o vertex ids (rr_pgo_cross_covariances; no --rows: every vertex) -- one line per
      (row vertex, column vertex) block: the two ids, d_r, d_c, the d_r x d_c values row-major -- and the call's three times

  --gate FILE  (example mode): after the optimisation, gate the candidate edges of FILE -- EDGE_SE2 / EDGE_SE2_XY /
      EDGE_BEARING_SE2_XY / EDGE_RANGE_SE2_XY / EDGE_SE3:QUAT / EDGE_SE3_TRACKXYZ lines in the loader's field order, between vertex ids of the loaded graph, not part of it -- and print
      one line per candidate: ids, Mahalanobis distance d2, e^T Omega e, accept / reject at the 0.95 chi-square quantile
      (rr_pgo_gate_edges).  With --accept the accepted candidates are then added to the live handle (rr_pgo_extend), the
      optimisation runs again, and chi2 before and after is printed

  --extend FILE  (example mode): after the optimisation, append the VERTEX_* / EDGE_* lines of FILE (the loader's tags and
      field order; new vertices need ids the graph does not have, edges may join old and new vertices) to the live handle
      (rr_pgo_extend), optimise again and print chi2 before and after.  With --guess the file's vertex values are ignored
      and the new vertices are initialised on the device along the new edges

  --gate-joint FILE  (example mode): candidate lines as for --gate, plus lines `SET i j k ...` that name candidates by
      their 0-based order in the file; after the optimisation one line per set: members, D_s, joint Mahalanobis distance
      d2, the 0.95 chi-square quantile of D_s degrees of freedom, accept / reject, the prefix distances
      (rr_pgo_gate_joint)

  python -m rustrobotics_amd <file.g2o> --bench [--repeats 20]
      = benches/graph_slam.rs:9-10   PoseGraph::new("dataset/g2o/intel.g2o", GaussNewton)?.optimize(10, false, false)
        timed end to end like criterion does: parsing, symbolic analysis, device setup and the ten
        Gauss-Newton iterations are ALL inside the timed closure; prints mean / median / min in ms.
"""
import argparse
import statistics
import sys
import time

from .mapping import PoseGraph, PoseGraphSolver


def _robust_arg(text):
    kind, sep, delta = text.partition(":")
    kind = kind.strip().lower()
    try:
        d = float(delta)
    except ValueError:
        d = float("nan")
    if kind not in ("huber", "cauchy") or not sep or not (d > 0 and d != float("inf")):
        raise argparse.ArgumentTypeError(f"expected huber:DELTA or cauchy:DELTA with DELTA > 0, got {text!r}")
    return kind, d


def _gnc_arg(text):
    delta, sep, which = text.partition(":")
    which = which.strip().lower() if sep else "loops"
    try:
        d = float(delta)
    except ValueError:
        d = float("nan")
    if which not in ("loops", "all") or not (d > 0 and d != float("inf")):
        raise argparse.ArgumentTypeError(f"expected DELTA, DELTA:loops or DELTA:all with DELTA > 0, got {text!r}")
    return d, which


def gnc_report(g, delta, which):
    import numpy as np
    mask = None
    if which == "loops":
        _, _, _, ef, et, _, _ = g.graph_arrays()
        mask = (np.abs(ef.astype(np.int64) - et.astype(np.int64)) > 1).astype(np.int32)
    print(f"Loaded graph with {g.num_nodes} nodes and {g.num_edges} edges")
    print(f"graduated non-convexity, truncated least squares: delta {delta:g}, "
          f"{'every edge' if mask is None else f'{int(mask.sum())} loop closures'} robustified")
    res = g.optimize_gnc(delta, mask)
    for t, (mu, cost) in enumerate(zip(res["stage_mu"], res["stage_cost"])):
        print(f"stage {t:3} : mu = {mu:.6g}, cost = {cost:.5f}")
    _, w = g.edge_errors()
    rejected = np.flatnonzero((w == 0.0) & (mask != 0 if mask is not None else True))
    print(f"{res['n_stages']} stages ({'converged' if res['converged'] else 'NOT converged: fractional weights remain'}), "
          f"mu0 {res['mu0']:.6g}, mu_last {res['mu_last']:.6g}, {res['final_iterations_run']} closing iterations, "
          f"final cost {res['cost_last']:.9g}")
    print(f"{res['n_rejected']} edges rejected, {res['n_fractional']} fractional: {' '.join(str(int(k)) for k in rejected)}")


def write_marginals(g, path):
    import ctypes as C

    import numpy as np
    from . import _lib
    d = _lib.GraphDesc()
    _lib.load().rr_pgo_get_graph(g._h, C.byref(d))
    n = d.n_nodes
    ids = np.ctypeslib.as_array(d.node_id, (n,)) if (n and d.node_id) else np.arange(n)
    with open(path, "w") as f:
        for i, blk in zip(ids, g.marginals()):
            k = len(blk)
            f.write(f"{int(i)} {k} " + " ".join(f"{v:.17g}" for v in blk[np.triu_indices(k)]) + "\n")
    print(f"marginal covariances of {n} nodes written to {path}")


def _ids_arg(text):
    try:
        ids = [int(t) for t in text.split(",")]
    except ValueError:
        ids = []
    if not ids or min(ids) < 0:
        raise argparse.ArgumentTypeError(f"expected ID,ID,... (g2o vertex ids), got {text!r}")
    return ids


def print_joint(g, ids):
    import ctypes as C

    import numpy as np
    from . import _lib
    d = _lib.GraphDesc()
    _lib.load().rr_pgo_get_graph(g._h, C.byref(d))
    n = d.n_nodes
    file_ids = np.ctypeslib.as_array(d.node_id, (n,)) if (n and d.node_id) else np.arange(n)
    index = {int(v): k for k, v in enumerate(file_ids)}
    missing = [i for i in ids if i not in index]
    if missing:
        raise SystemExit(f"--joint: no vertex with id {missing[0]} in the file")
    J = g.covariance([index[i] for i in ids])
    print(f"joint covariance of vertices {','.join(str(i) for i in ids)} ({J.shape[0]} x {J.shape[0]}):")
    for row in J:
        print(" ".join(f"{v:.17g}" for v in row))


def write_cross(g, path, columns, rows):
    import numpy as np
    index = _node_index(g)
    for flag, ids in (("--columns", columns), ("--rows", rows or [])):
        missing = [i for i in ids if i not in index]
        if missing:
            raise SystemExit(f"{flag}: no vertex with id {missing[0]} in the file")
    by_index = sorted(index, key=index.get)
    row_ids = rows if rows else by_index
    dim = np.take((3, 2, 6), g.graph_arrays()[0])
    X = g.cross_covariance([index[i] for i in rows] if rows else None, [index[i] for i in columns])
    ro = np.concatenate([[0], np.cumsum([dim[index[i]] for i in row_ids])]).astype(int)
    co = np.concatenate([[0], np.cumsum([dim[index[i]] for i in columns])]).astype(int)
    with open(path, "w") as f:
        for r, i in enumerate(row_ids):
            for c, j in enumerate(columns):
                blk = X[ro[r]:ro[r + 1], co[c]:co[c + 1]]
                f.write(f"{i} {j} {blk.shape[0]} {blk.shape[1]} " + " ".join(f"{v:.17g}" for v in blk.ravel()) + "\n")
    t = g.cross_covariances_times()
    print(f"cross covariances of {len(row_ids)} x {len(columns)} vertices ({X.shape[0]} x {X.shape[1]} scalars) written to {path}; "
          f"linearise + factor {t[0]:.3f} ms, forward + backward solve {t[1]:.3f} ms, gather + copy {t[2]:.3f} ms")


GATE_TAGS = {"EDGE_SE2": 0, "EDGE_SE2_XY": 1, "EDGE_SE3:QUAT": 2, "EDGE_SE3_TRACKXYZ": 3,
             "EDGE_BEARING_SE2_XY": 4, "EDGE_RANGE_SE2_XY": 6}   # (the range tag is build-defined: include/rr_pgo.h)


_PARAM_ID = {"EDGE_SE3_TRACKXYZ": ", a parameter id"}   # what the messages about such a line add


def _edge_values(tok):
    """The numbers of an edge line behind its two vertex ids.  EDGE_SE3_TRACKXYZ carries the id of its sensor-offset
    parameter there first (g2o text, as the loader reads it): an unsigned integer, otherwise ignored."""
    if tok[0] == "EDGE_SE3_TRACKXYZ":
        if int(tok[3]) < 0:
            raise ValueError(tok[3])
        return [float(t) for t in tok[4:]]
    return [float(t) for t in tok[3:]]


def parse_gate_file(path, index, sets=None, flag="--gate"):
    """Candidate edges of a --gate file as (kind, from, to, meas, info, ids) in rr_pgo_graph_desc packing; `index` maps a
    g2o vertex id to the node's index.  Needs no device.  An unknown tag or id is a SystemExit that names the line.
    sets: a list that receives (line number, [candidate, ...]) of every `SET i j k ...` line (--gate-joint)."""
    from .mapping import GATE_INFO_LEN, GATE_MEAS_LEN
    kind, a, b, meas, info, ids = [], [], [], [], [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if sets is not None and tok[0] == "SET":
                try:
                    members = [int(t) for t in tok[1:]]
                except ValueError:
                    members = []
                if not members:
                    raise SystemExit(f"{flag}: {path}:{no}: expected candidate numbers after SET")
                sets.append((no, members))
                continue
            if tok[0] not in GATE_TAGS:
                raise SystemExit(f"{flag}: {path}:{no}: unknown tag {tok[0]!r} (EDGE_SE2, EDGE_SE2_XY, EDGE_BEARING_SE2_XY, EDGE_RANGE_SE2_XY, "
                                 "EDGE_SE3:QUAT or EDGE_SE3_TRACKXYZ)")
            k = GATE_TAGS[tok[0]]
            nm, ni = GATE_MEAS_LEN[k], GATE_INFO_LEN[k]
            try:
                i, j = int(tok[1]), int(tok[2])
                vals = _edge_values(tok)
            except (ValueError, IndexError):
                raise SystemExit(f"{flag}: {path}:{no}: expected two vertex ids{_PARAM_ID.get(tok[0], '')} and {nm + ni} numbers after {tok[0]}")
            if len(vals) != nm + ni:
                raise SystemExit(f"{flag}: {path}:{no}: expected {nm + ni} values after the ids{_PARAM_ID.get(tok[0], '')}, got {len(vals)}")
            for v in (i, j):
                if v not in index:
                    raise SystemExit(f"{flag}: {path}:{no}: no vertex with id {v} in the graph")
            kind.append(k)
            a.append(index[i])
            b.append(index[j])
            meas.extend(vals[:nm])
            info.extend(vals[nm:])
            ids.append((i, j))
    return kind, a, b, meas, info, ids


def parse_priors_file(path, index, node_kind):
    """A --priors file as (node, meas, info) in the packing of rr_pgo_set_priors.  `index` maps a g2o vertex id to the
    node's index, node_kind[index] is the node's kind.  Needs no device.  A short line, a bad number or an unknown vertex
    is a SystemExit that names the line."""
    from .mapping import GATE_INFO_LEN, GATE_MEAS_LEN
    node, meas, info = [], [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            try:
                i = int(tok[0])
                vals = [float(t) for t in tok[1:]]
            except ValueError:
                raise SystemExit(f"--priors: {path}:{no}: expected a vertex id and numbers")
            if i not in index:
                raise SystemExit(f"--priors: {path}:{no}: no vertex with id {i} in the graph")
            k = int(node_kind[index[i]])
            nm, ni = GATE_MEAS_LEN[k], GATE_INFO_LEN[k]
            if len(vals) != nm + ni:
                raise SystemExit(f"--priors: {path}:{no}: expected {nm + ni} values after the id "
                                 f"({nm} of the measurement, {ni} of the information), got {len(vals)}")
            node.append(index[i])
            meas.extend(vals[:nm])
            info.extend(vals[nm:])
    return node, meas, info


def fix_indices(ids, index):
    """The node indices of the g2o vertex ids of --fix.  `index` maps a vertex id to the node's index.  Needs no device.
    An unknown vertex is a SystemExit that names it."""
    missing = [i for i in ids if i not in index]
    if missing:
        raise SystemExit(f"--fix: no vertex with id {missing[0]} in the graph")
    return [index[i] for i in ids]


def apply_priors_file(g, path, free_anchor):
    node, meas, info = parse_priors_file(path, _node_index(g), g.graph_arrays()[0])
    g.set_priors(node, meas, info, keep_anchor=not free_anchor)
    return len(node)


def print_prior_share(g):
    import numpy as np
    s, _ = g.prior_errors()
    total = g.global_error()
    # the cost of a prior is rho(s): s itself unless the prior is flagged robust (the CLI flags none)
    share = float(np.sum(s))
    print(f"priors: {len(s)} priors carry {share:.9g} of the final cost {total:.9g} ({100.0 * share / total if total else 0.0:.3g} %)")


VERTEX_TAGS = {"VERTEX_SE2": 0, "VERTEX_XY": 1, "VERTEX_SE3:QUAT": 2, "VERTEX_TRACKXYZ": 3}


def parse_extend_file(path, index, n_nodes=None, flag="--extend"):
    """An --extend file as (node_kind, node_id, node_state, edge_kind, from, to, meas, info) in rr_pgo_graph_desc packing.
    `index` maps the g2o vertex ids of the live graph to node indices (n_nodes: their number, default len(index)); the
    file's vertices get the indices behind them, in file order, and its edges may name old and new vertices, before or
    after the vertex line.  Needs no device.  An unknown tag, a repeated id, a short line or an unknown vertex is a
    SystemExit that names the line."""
    from .mapping import GATE_INFO_LEN, GATE_MEAS_LEN
    n_old = len(index) if n_nodes is None else n_nodes
    index = dict(index)
    nkind, nid, nstate, edges = [], [], [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if tok[0] in VERTEX_TAGS:
                k = VERTEX_TAGS[tok[0]]
                nv = GATE_MEAS_LEN[k]
                try:
                    i = int(tok[1])
                    vals = [float(t) for t in tok[2:]]
                except (ValueError, IndexError):
                    raise SystemExit(f"{flag}: {path}:{no}: expected a vertex id and {nv} numbers after {tok[0]}")
                if len(vals) != nv:
                    raise SystemExit(f"{flag}: {path}:{no}: expected {nv} values after the id, got {len(vals)}")
                if i < 0 or i in index:
                    raise SystemExit(f"{flag}: {path}:{no}: vertex id {i} is negative or already in use")
                index[i] = n_old + len(nkind)
                nkind.append(k)
                nid.append(i)
                nstate.extend(vals)
                continue
            if tok[0] not in GATE_TAGS:
                raise SystemExit(f"{flag}: {path}:{no}: unknown tag {tok[0]!r} (VERTEX_SE2, VERTEX_XY, VERTEX_SE3:QUAT, "
                                 "VERTEX_TRACKXYZ, EDGE_SE2, EDGE_SE2_XY, EDGE_BEARING_SE2_XY, EDGE_RANGE_SE2_XY, EDGE_SE3:QUAT or "
                                 "EDGE_SE3_TRACKXYZ)")
            k = GATE_TAGS[tok[0]]
            nm, ni = GATE_MEAS_LEN[k], GATE_INFO_LEN[k]
            try:
                i, j = int(tok[1]), int(tok[2])
                vals = _edge_values(tok)
            except (ValueError, IndexError):
                raise SystemExit(f"{flag}: {path}:{no}: expected two vertex ids{_PARAM_ID.get(tok[0], '')} and {nm + ni} numbers after {tok[0]}")
            if len(vals) != nm + ni:
                raise SystemExit(f"{flag}: {path}:{no}: expected {nm + ni} values after the ids{_PARAM_ID.get(tok[0], '')}, got {len(vals)}")
            edges.append((no, k, i, j, vals))
    kind, a, b, meas, info = [], [], [], [], []
    for no, k, i, j, vals in edges:   # (an edge may come before the vertex line it names)
        for v in (i, j):
            if v not in index:
                raise SystemExit(f"{flag}: {path}:{no}: no vertex with id {v} in the graph or in the file")
        kind.append(k)
        a.append(index[i])
        b.append(index[j])
        meas.extend(vals[:GATE_MEAS_LEN[k]])
        info.extend(vals[GATE_MEAS_LEN[k]:])
    return nkind, nid, nstate, kind, a, b, meas, info


def _node_index(g):
    import ctypes as C

    import numpy as np
    from . import _lib
    d = _lib.GraphDesc()
    _lib.load().rr_pgo_get_graph(g._h, C.byref(d))
    n = d.n_nodes
    file_ids = np.ctypeslib.as_array(d.node_id, (n,)) if (n and d.node_id) else np.arange(n)
    return {int(v): k for k, v in enumerate(file_ids)}


def _reoptimize(g, what, iterations):
    before = g.global_error()
    errors = g.optimize(iterations)
    print(f"{what}: {g.num_nodes} nodes, {g.num_edges} edges; chi2 before {before:.9g}, after {errors[-1]:.9g} "
          f"({len(errors) - 1} iterations)")


def accept_gated(g, path, iterations):
    """--gate FILE --accept: the candidates the gate accepts join the live handle, then the optimisation runs again."""
    import numpy as np
    from .mapping import GATE_INFO_LEN, GATE_MEAS_LEN, gate_thresholds
    kind, a, b, meas, info, ids = parse_gate_file(path, _node_index(g))
    d2, _ = g.gate_edges(kind, a, b, meas, info)
    keep = [c for c in range(len(kind)) if d2[c] <= gate_thresholds(kind)[c]]
    if not keep:
        print("--accept: no candidate passed the gate, the graph is unchanged")
        return
    mo = np.concatenate([[0], np.cumsum(np.take(GATE_MEAS_LEN, kind))]).astype(int)
    io = np.concatenate([[0], np.cumsum(np.take(GATE_INFO_LEN, kind))]).astype(int)
    g.extend([kind[c] for c in keep], [a[c] for c in keep], [b[c] for c in keep],
             np.concatenate([meas[mo[c]:mo[c + 1]] for c in keep]), np.concatenate([info[io[c]:io[c + 1]] for c in keep]))
    _reoptimize(g, f"--accept: {len(keep)} of {len(kind)} candidates added ({' '.join(f'{ids[c][0]}-{ids[c][1]}' for c in keep)})", iterations)


def check_edges_report(g, remove, iterations):
    """--check-edges: the edges that disagree with the rest of the graph (rr_pgo_check_edges), worst first; with
    --remove-suspects they leave the live handle (rr_pgo_remove_edges) and the optimisation runs again."""
    from .mapping import gate_thresholds
    ids = {k: v for v, k in _node_index(g).items()}
    kind, ef, et = g.graph_arrays()[2:5]
    c = g.check_edges(return_residual=True)
    suspects = g.suspect_edges(checked=c)      # (from the one query)
    thr = gate_thresholds(kind)
    bridges = int((c["redundancy"] < 0.01).sum())
    from .mapping import SINGULAR_DIRECTION
    partial = int(((c["redundancy"] >= 0.01) & (c["redundancy_min"] <= SINGULAR_DIRECTION)).sum())
    print(f"check of {g.num_edges} edges (suspect: redundancy >= 0.01, no direction of the residual unconstrained, d2 above the 0.95 "
          f"chi-square quantile); {bridges} edges below redundancy 0.01 and {partial} with an unconstrained direction carry no information:")
    for k in suspects:
        print(f"edge {k} {ids[int(ef[k])]} {ids[int(et[k])]} d2 {c['d2'][k]:.9g} redundancy {c['redundancy'][k]:.6g} "
              f"chi2 {c['chi2'][k]:.9g} threshold {thr[k]:g}")
    if not len(suspects):
        print("no suspect edge")
    if remove and len(suspects):
        g.remove_edges(suspects)
        _reoptimize(g, f"--remove-suspects: {len(suspects)} edges removed", iterations)


def extend_from_file(g, path, guess, iterations):
    nkind, nid, nstate, kind, a, b, meas, info = parse_extend_file(path, _node_index(g), g.num_nodes)
    g.extend(kind, a, b, meas, info, node_kind=nkind if nkind else None,
             node_state=None if (guess or not nkind) else nstate, node_id=nid if nkind else None)
    how = " (initial values guessed on the device)" if guess and nkind else ""
    _reoptimize(g, f"--extend: {len(nkind)} vertices{how} and {len(kind)} edges of {path} added", iterations)


def parse_gate_joint_file(path, index):
    """A --gate-joint file: (kind, from, to, meas, info, ids, sets).  Candidate lines as in a --gate file; a line
    `SET i j k ...` names candidates by their 0-based order in the file (before or after the line).  Needs no device.
    No SET line, a member out of range, a set beyond the caps of rr_pgo_gate_joint: a SystemExit that names the line."""
    from . import _lib
    from .mapping import GATE_EDGE_DIM
    raw = []
    kind, a, b, meas, info, ids = parse_gate_file(path, index, raw, "--gate-joint")
    if not raw:
        raise SystemExit(f"--gate-joint: {path}: no SET line")
    for no, members in raw:
        for c in members:
            if not 0 <= c < len(kind):
                raise SystemExit(f"--gate-joint: {path}:{no}: no candidate {c} in the file ({len(kind)} candidates)")
        dim = sum(GATE_EDGE_DIM[kind[c]] for c in members)
        if len(members) > _lib.GATE_JOINT_MAX_CAND or dim > _lib.GATE_JOINT_MAX_DIM:
            raise SystemExit(f"--gate-joint: {path}:{no}: a set holds at most {_lib.GATE_JOINT_MAX_CAND} candidates and "
                             f"{_lib.GATE_JOINT_MAX_DIM} error scalars, this one {len(members)} and {dim}")
    return kind, a, b, meas, info, ids, [members for _, members in raw]


def print_gate(g, path):
    import ctypes as C

    import numpy as np
    from . import _lib
    from .mapping import gate_thresholds
    d = _lib.GraphDesc()
    _lib.load().rr_pgo_get_graph(g._h, C.byref(d))
    n = d.n_nodes
    file_ids = np.ctypeslib.as_array(d.node_id, (n,)) if (n and d.node_id) else np.arange(n)
    kind, a, b, meas, info, ids = parse_gate_file(path, {int(v): k for k, v in enumerate(file_ids)})
    d2, chi2 = g.gate_edges(kind, a, b, meas, info)
    thr = gate_thresholds(kind)
    print(f"gate of {len(kind)} candidate edges from {path} (accept: d2 <= the 0.95 chi-square quantile):")
    for c, (i, j) in enumerate(ids):
        print(f"{i} {j} d2 {d2[c]:.9g} chi2 {chi2[c]:.9g} threshold {thr[c]:g} {'accept' if d2[c] <= thr[c] else 'reject'}")


def print_gate_joint(g, path):
    import ctypes as C

    import numpy as np
    from . import _lib
    from .mapping import gate_joint_dims, gate_joint_thresholds
    d = _lib.GraphDesc()
    _lib.load().rr_pgo_get_graph(g._h, C.byref(d))
    n = d.n_nodes
    file_ids = np.ctypeslib.as_array(d.node_id, (n,)) if (n and d.node_id) else np.arange(n)
    kind, a, b, meas, info, _, sets = parse_gate_joint_file(path, {int(v): k for k, v in enumerate(file_ids)})
    d2, prefix = g.gate_joint(kind, a, b, meas, info, sets, return_prefix=True)
    dims, thr = gate_joint_dims(kind, sets), gate_joint_thresholds(kind, sets)
    print(f"joint gate of {len(sets)} sets over {len(kind)} candidate edges from {path} (accept: d2 <= the 0.95 chi-square quantile):")
    for s, members in enumerate(sets):
        print(f"SET {' '.join(str(c) for c in members)} D {dims[s]} d2 {d2[s]:.9g} threshold {thr[s]:g} "
              f"{'accept' if d2[s] <= thr[s] else 'reject'} prefixes {' '.join(f'{v:.9g}' for v in prefix[s])}")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m rustrobotics_amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file", help="g2o file (SE2, SE2 + XY landmarks, or SE3:QUAT)")
    ap.add_argument("--solver", choices=[s.name for s in PoseGraphSolver], default="GaussNewton")
    ap.add_argument("--iterations", type=int, default=None, help="default 50 (example) / 10 (--bench)")
    ap.add_argument("--precision", choices=["f64", "f32", "mixed"], default="f64")
    ap.add_argument("--plot", action="store_true", help="the example's third menu: write ./img/{name}-{iteration}-{solver}.svg")
    ap.add_argument("--bench", action="store_true", help="time new() + optimize(10, false, false) like benches/graph_slam.rs")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--robust", type=_robust_arg, default=None, metavar="KIND:DELTA",
                    help="robust kernel on every edge: huber:DELTA or cauchy:DELTA")
    ap.add_argument("--gnc", type=_gnc_arg, default=None, metavar="DELTA[:loops|all]",
                    help="optimise by graduated non-convexity on truncated least squares; loops (default): edges with |from - to| > 1")
    ap.add_argument("--priors", metavar="FILE", default=None,
                    help="absolute priors, one per line: NODE_ID, measurement, upper triangle of the information")
    ap.add_argument("--free-anchor", action="store_true",
                    help="with --priors and / or --fix: drop the 1e7 term on the anchor node, they alone fix the gauge")
    ap.add_argument("--fix", type=_ids_arg, metavar="ID,ID,...", default=None,
                    help="hold these g2o vertex ids constant: they never move, covariances and gates are conditional on them")
    ap.add_argument("--init", choices=["chordal"], default=None,
                    help="before the optimisation: initialise every free vertex from the measurements (chordal relaxation)")
    ap.add_argument("--marginals", metavar="FILE", default=None,
                    help="after the optimisation write every node's covariance block: id, d, upper triangle")
    ap.add_argument("--joint", type=_ids_arg, metavar="ID,ID,...", default=None,
                    help="after the optimisation print the joint covariance of these g2o vertex ids (any nodes)")
    ap.add_argument("--cross", metavar="FILE", default=None,
                    help="after the optimisation write the blocks of Sigma[rows, columns]: the two ids, d_r, d_c, the values")
    ap.add_argument("--columns", type=_ids_arg, metavar="ID,ID,...", default=None, help="with --cross: the column vertices")
    ap.add_argument("--rows", type=_ids_arg, metavar="ID,ID,...", default=None,
                    help="with --cross: the row vertices (default: every vertex, in the graph's order)")
    ap.add_argument("--gate", metavar="FILE", default=None,
                    help="after the optimisation gate the candidate EDGE_* lines of FILE: d2, e^T Omega e, accept / reject")
    ap.add_argument("--accept", action="store_true",
                    help="with --gate: add the accepted candidates to the live handle, optimise again, print chi2 before and after")
    ap.add_argument("--extend", metavar="FILE", default=None,
                    help="after the optimisation append the VERTEX_* / EDGE_* lines of FILE to the live handle and optimise again")
    ap.add_argument("--guess", action="store_true",
                    help="with --extend: ignore the file's vertex values, initialise the new vertices on the device")
    ap.add_argument("--gate-joint", metavar="FILE", default=None,
                    help="after the optimisation gate the SET lines of FILE jointly: D_s, d2, threshold, accept / reject, prefixes")
    ap.add_argument("--check-edges", action="store_true",
                    help="after the optimisation audit the graph's own edges: leave-one-out d2, redundancy, e^T Omega e of the suspects")
    ap.add_argument("--remove-suspects", action="store_true",
                    help="with --check-edges: take the suspects out of the live handle, optimise again, print chi2 before and after")
    a = ap.parse_args(argv)
    if a.remove_suspects and not a.check_edges:
        ap.error("--remove-suspects needs --check-edges")
    if a.accept and not a.gate:
        ap.error("--accept needs --gate FILE")
    if a.cross and not a.columns:
        ap.error("--cross needs --columns ID,ID,...")
    if (a.columns or a.rows) and not a.cross:
        ap.error("--columns and --rows need --cross FILE")
    if a.gnc and (a.bench or a.robust):
        ap.error("--gnc is an optimisation of its own: not with --bench or --robust")
    if a.guess and not a.extend:
        ap.error("--guess needs --extend FILE")
    if a.free_anchor and not (a.priors or a.fix):
        ap.error("--free-anchor needs --priors FILE or --fix ID,ID,...")
    solver = PoseGraphSolver[a.solver]
    report_init = not a.bench

    def new():
        g = PoseGraph.new(a.file, solver, precision=a.precision)
        if a.priors:
            apply_priors_file(g, a.priors, a.free_anchor)
        if a.fix:
            g.set_fixed(fix_indices(a.fix, _node_index(g)), keep_anchor=not a.free_anchor)
        if a.init:
            before = g.global_error() if report_init else None
            g.initialize(a.init)
            if report_init:
                ms = g.initialize_times()
                print(f"{a.init} initialisation: chi2 before {before:.9g}, after {g.global_error():.9g} "
                      f"(rotations {ms[0]:.3f} ms, positions {ms[1]:.3f} ms, call {ms[2]:.3f} ms)")
        if a.robust:
            g.set_robust_kernel(*a.robust)
        return g

    if not a.bench:
        if a.robust:
            print(f"robust kernel {a.robust[0]}, delta {a.robust[1]:g}")
        g = new()
        if a.priors:
            print(f"{g.num_priors} priors from {a.priors}" + (", anchor term dropped" if a.free_anchor else ""))
        if a.fix:
            print(f"{g.num_fixed} vertices held fixed" + (", anchor term dropped" if a.free_anchor else ""))
        if a.gnc:
            gnc_report(g, *a.gnc)
        else:
            g.optimize(50 if a.iterations is None else a.iterations, True, a.plot)
        if a.priors:
            print_prior_share(g)
        if a.marginals:
            write_marginals(g, a.marginals)
        if a.joint:
            print_joint(g, a.joint)
        if a.cross:
            write_cross(g, a.cross, a.columns, a.rows)
        if a.gate:
            print_gate(g, a.gate)
        if a.gate_joint:
            print_gate_joint(g, a.gate_joint)
        if a.gate and a.accept:
            accept_gated(g, a.gate, 50 if a.iterations is None else a.iterations)
        if a.extend:
            extend_from_file(g, a.extend, a.guess, 50 if a.iterations is None else a.iterations)
        if a.check_edges:
            check_edges_report(g, a.remove_suspects, 50 if a.iterations is None else a.iterations)
        return 0
    iters = 10 if a.iterations is None else a.iterations
    new().optimize(iters, False, False)   # warm-up: library load, HIP context
    ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        errors = new().optimize(iters, False, False)
        ms.append((time.perf_counter() - t0) * 1e3)
    rob = f" with {a.robust[0]}:{a.robust[1]:g}" if a.robust else ""
    print(f"graph_slam: new() + optimize({iters}, false, false){rob} on {a.file}: mean {statistics.mean(ms):.3f} ms, "
          f"median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms over {a.repeats} runs; "
          f"{len(errors) - 1} iterations run, final {'robust cost' if a.robust else 'chi2'} {errors[-1]:.9g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
