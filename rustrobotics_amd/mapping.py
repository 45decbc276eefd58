"""Host-side mirror of the reference's `robotics::mapping` public surface
(reference src/mapping/mod.rs:6: `PoseGraph`, `PoseGraphSolver`), on top of the
C ABI of librr_pgo.so.  Same names, argument meaning and error behaviour:

  PoseGraph.new(file_path, solver)        pose_graph_optimization.rs:215-227
  PoseGraph.optimize(num_iterations, log, plot) -> list of chi2   :247-303
  PoseGraph.plot()                        :375-431   img/{name}-{iteration}-{solver:?}.svg

`optimize(n, False, False)` is ONE rr_pgo_optimize call (the loop, its stop rule and the Levenberg-Marquardt decisions
run on the device).  With `log` or `plot` the loop runs here, one iteration at a time through rr_pgo_linearize_solve /
rr_pgo_update / rr_pgo_chi2 in the reference's order, so that the lines are printed and the figures written as the
iterations complete (:258-268, :288-296).
"""
import ctypes as C
import enum

import numpy as np

from . import _lib


class PoseGraphSolver(enum.Enum):
    """pose_graph_optimization.rs:28-32"""
    GaussNewton = 0
    LevenbergMarquardt = 1


class PoseGraphError(RuntimeError):
    """Stands in for the reference's Box<dyn Error>."""

    def __init__(self, code, message):
        super().__init__(f"[{code}] {message}")
        self.code = code


# 0.95 quantiles of the chi-square distribution with 2, 3 and 6 degrees of freedom (the default gate), and the error
# dimension, measurement length and packed information length of an edge by kind (RR_PGO_EDGE_SE2, _SE2_XY, _SE3, _SE3_XYZ,
# _SE2_BEARING = 4, _SE2_RANGE = 6; 5 and 7 are reserved, unknown kinds: the 0 at index 5 is a place holder nothing reads)
CHI2_95_1, CHI2_95_2, CHI2_95_3, CHI2_95_6 = 3.841, 5.991, 7.815, 12.592
GATE_DEFAULT_THRESHOLD = {0: CHI2_95_3, 1: CHI2_95_2, 2: CHI2_95_6, 3: CHI2_95_3, 4: CHI2_95_1, 6: CHI2_95_1}
# ... and with 1 .. 48 degrees of freedom (CHI2_95[d]; the default of PoseGraph.gate_joint_accept: d = D_s)
CHI2_95 = (None,
           3.841, 5.991, 7.815, 9.488, 11.070, 12.592, 14.067, 15.507, 16.919, 18.307, 19.675, 21.026,
           22.362, 23.685, 24.996, 26.296, 27.587, 28.869, 30.144, 31.410, 32.671, 33.924, 35.172, 36.415,
           37.652, 38.885, 40.113, 41.337, 42.557, 43.773, 44.985, 46.194, 47.400, 48.602, 49.802, 50.998,
           52.192, 53.384, 54.572, 55.758, 56.942, 58.124, 59.304, 60.481, 61.656, 62.830, 64.001, 65.171)
GATE_EDGE_DIM = (3, 2, 6, 3, 1, 0, 1)
GATE_MEAS_LEN = (3, 2, 7, 3, 1, 0, 1)
GATE_INFO_LEN = (6, 3, 21, 6, 1, 0, 1)
# the same by node kind (RR_PGO_NODE_SE2, _XY, _SE3, _XYZ): scalars of the step and of the state; a node's state has the
# length of the measurement of the edge of its kind
NODE_DIM = (3, 2, 6, 3)
NODE_STATE_LEN = (3, 2, 7, 3)
KNOWN_KINDS = (0, 1, 2, 3, 4, 6)      # edge kinds
KNOWN_NODE_KINDS = (0, 1, 2, 3)


def gate_thresholds(edge_kind, threshold=None):
    """per-candidate threshold of PoseGraph.gate: a scalar, a per-kind mapping, or None (the 0.95 quantiles)"""
    kind = np.asarray(edge_kind, np.int64)
    if threshold is None:
        threshold = GATE_DEFAULT_THRESHOLD
    if hasattr(threshold, "keys"):
        return np.array([float(threshold[int(k)]) for k in kind])
    return np.full(kind.shape, float(threshold))


def gate_joint_dims(edge_kind, sets):
    """D_s of every set: the sum of its candidates' error dimensions"""
    kind = np.asarray(edge_kind, np.int64)
    return np.array([int(sum(GATE_EDGE_DIM[int(kind[c])] for c in s)) for s in sets], np.int64)


def gate_joint_thresholds(edge_kind, sets, threshold=None):
    """per-set threshold of PoseGraph.gate_joint_accept: a scalar, or None (the 0.95 quantile of D_s degrees of freedom)"""
    dims = gate_joint_dims(edge_kind, sets)
    if threshold is None:
        return np.array([CHI2_95[int(d)] for d in dims], np.float64)
    return np.full(dims.shape, float(threshold))


def directional_redundancy(R, omega, redundancy):
    """The smallest redundancy of an edge over the directions of its residual.  The eigenvalues of R Omega_w lie in [0, 1]
    and their mean is the redundancy r; the smallest one says how well the rest of the graph determines the WORST determined
    direction.  It is 0 when part of the residual is a bridge -- a pose seen by one landmark only has its heading fixed by
    nothing else, whatever r says -- and R is then singular to rounding and d2 carries no information (NaN, or a huge
    number that rounding picks).  R, omega: d_e x d_e, omega the UNWEIGHTED information; the robust weight cancels:
    lambda_min(R Omega_w) = r d_e lambda_min(R Omega) / trace(R Omega)."""
    L = np.linalg.cholesky(np.asarray(omega, np.float64))
    lam = np.linalg.eigvalsh(L.T @ np.asarray(R, np.float64) @ L)
    tr = float(np.sum(lam))
    return float(redundancy) * len(lam) * float(lam[0]) / tr if tr > 0.0 else 0.0


# An eigenvalue of R Omega_w below this is not told from 0: R = Omega_w^-1 - P is a difference of matrices of size 1, and half
# of the 16 digits is the usual line between a number and its rounding (the numerical-rank convention).
SINGULAR_DIRECTION = float(np.sqrt(np.finfo(np.float64).eps))


def select_suspects(kind, d2, redundancy, redundancy_min, threshold=None, min_redundancy=0.01, min_directional=SINGULAR_DIRECTION):
    """Positions of the suspects among checked edges, by falling d2: redundancy at least min_redundancy, no direction of the
    residual that nothing else constrains (the smallest directional redundancy above min_directional: R is singular to
    rounding otherwise, and d2 is NaN or a number that rounding picks), and d2 above the threshold of
    gate_thresholds(kind, threshold).  A NaN d2 is no suspect."""
    d2 = np.asarray(d2, np.float64)
    ok = (np.asarray(redundancy) >= min_redundancy) & (np.asarray(redundancy_min) > min_directional)
    with np.errstate(invalid="ignore"):
        hit = np.flatnonzero(ok & (d2 > gate_thresholds(kind, threshold)))
    return hit[np.argsort(-d2[hit], kind="stable")]


def _check(rc):
    if rc != 0:
        raise PoseGraphError(rc, _lib.load().rr_pgo_last_error().decode())


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class PoseGraph:
    def __init__(self, handle, solver, name=""):
        self._h = handle
        self.solver = solver
        self.name = name
        self.iteration = 0

    # -- constructors -----------------------------------------------------------
    @classmethod
    def new(cls, file_path, solver=PoseGraphSolver.GaussNewton, precision="f64", device=-1):
        """PoseGraph::new(file_path, solver)."""
        L = _lib.load()
        opt = _lib.Options()
        L.rr_pgo_default_options(C.byref(opt))
        opt.precision = _lib.PRECISIONS[precision]
        opt.device = device
        opt.solver = solver.value
        h = C.c_void_p()
        _check(L.rr_pgo_load_g2o(str(file_path).encode(), C.byref(opt), C.byref(h)))
        import os
        return cls(h, solver, os.path.splitext(os.path.basename(str(file_path)))[0])

    @classmethod
    def from_arrays(cls, node_kind, node_state, edge_kind, edge_from, edge_to, edge_meas, edge_info,
                    solver=PoseGraphSolver.GaussNewton, precision="f64", device=-1, node_id=None,
                    rank=0, world_size=1, sharded=False):
        L = _lib.load()
        keep = [np.ascontiguousarray(node_kind, np.int32), np.ascontiguousarray(node_state, np.float64),
                np.ascontiguousarray(edge_kind, np.int32), np.ascontiguousarray(edge_from, np.int32),
                np.ascontiguousarray(edge_to, np.int32), np.ascontiguousarray(edge_meas, np.float64),
                np.ascontiguousarray(edge_info, np.float64)]
        d = _lib.GraphDesc()
        d.n_nodes = len(keep[0])
        d.node_kind = _ip(keep[0])
        if node_id is not None:
            ids = np.ascontiguousarray(node_id, np.uint32)
            keep.append(ids)
            d.node_id = ids.ctypes.data_as(C.POINTER(C.c_uint32))
        d.node_state = _dp(keep[1])
        d.n_edges = len(keep[2])
        d.edge_kind = _ip(keep[2])
        d.edge_from = _ip(keep[3])
        d.edge_to = _ip(keep[4])
        d.edge_meas = _dp(keep[5])
        d.edge_info = _dp(keep[6])
        opt = _lib.Options()
        L.rr_pgo_default_options(C.byref(opt))
        opt.precision = _lib.PRECISIONS[precision]
        opt.device = device
        opt.solver = solver.value
        opt.rank, opt.world_size = rank, world_size
        opt.sharded = 1 if sharded else 0
        h = C.c_void_p()
        _check(L.rr_pgo_create(C.byref(d), C.byref(opt), C.byref(h)))
        return cls(h, solver)

    @classmethod
    def synthetic_grid(cls, width, height, n_edges=0, seed_meas=42, seed_init=43, **kw):
        """BASELINE config 4 graph, built by the library's own generator."""
        arrays = synthetic_grid_arrays(width, height, n_edges, seed_meas, seed_init)
        return cls.from_arrays(*arrays, **kw)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None and getattr(_lib, "_lib", None) is not None:   # not during interpreter teardown
            _lib._lib.rr_pgo_destroy(h)
            self._h = None

    # -- fields -------------------------------------------------------------------
    @property
    def len(self):
        return _lib.load().rr_pgo_dim(self._h)

    @property
    def num_nodes(self):
        return _lib.load().rr_pgo_num_nodes(self._h)

    @property
    def num_edges(self):
        return _lib.load().rr_pgo_num_edges(self._h)

    @property
    def anchor_node(self):
        return _lib.load().rr_pgo_anchor_node(self._h)

    def graph_arrays(self):
        """The parsed graph in rr_pgo_graph_desc packing (copies)."""
        L = _lib.load()
        d = _lib.GraphDesc()
        _check(L.rr_pgo_get_graph(self._h, C.byref(d)))
        n, m = d.n_nodes, d.n_edges
        nk = np.ctypeslib.as_array(d.node_kind, (n,)).copy() if n else np.zeros(0, np.int32)
        ek = np.ctypeslib.as_array(d.edge_kind, (m,)).copy() if m else np.zeros(0, np.int32)
        ns = int(np.sum(np.take(NODE_STATE_LEN, nk)))
        nm = int(np.sum(np.take(GATE_MEAS_LEN, ek)))
        ni = int(np.sum(np.take(GATE_INFO_LEN, ek)))
        return (nk, np.ctypeslib.as_array(d.node_state, (ns,)).copy(), ek,
                np.ctypeslib.as_array(d.edge_from, (m,)).copy(), np.ctypeslib.as_array(d.edge_to, (m,)).copy(),
                np.ctypeslib.as_array(d.edge_meas, (nm,)).copy(), np.ctypeslib.as_array(d.edge_info, (ni,)).copy())

    # -- the path -------------------------------------------------------------------
    def global_error(self):
        """global_error(&graph), :537-574"""
        out = C.c_double()
        _check(_lib.load().rr_pgo_chi2(self._h, C.byref(out)))
        return out.value

    def linearize_and_solve(self, lam=0.0, lm=False):
        """build_linear_system(lambda)?.solve()?, :271,:371-373"""
        dx = np.zeros(self.len)
        _check(_lib.load().rr_pgo_linearize_solve(self._h, lam, int(lm), _dp(dx)))
        return dx

    def update_nodes(self, dx, sign=1.0):
        """update_nodes(dx), :229-245"""
        dx = np.ascontiguousarray(dx, np.float64)
        if dx.shape != (self.len,):
            raise ValueError("dx has the wrong length")
        _check(_lib.load().rr_pgo_update(self._h, _dp(dx), sign))

    def optimize(self, num_iterations, log=False, plot=False, return_norms=False):
        """optimize(num_iterations, log, plot) -> Vec<f64> of chi2, :247-303"""
        if log or plot:
            return self._optimize_stepwise(num_iterations, log, plot, return_norms)
        L = _lib.load()
        errors = np.zeros(num_iterations + 1)
        norms = np.zeros(max(num_iterations, 1))
        n = C.c_int32()
        _check(L.rr_pgo_optimize(self._h, num_iterations, _dp(errors), C.byref(n), _dp(norms)))
        errors = errors[:n.value]
        self.iteration += n.value - 1
        if return_norms:
            return list(errors), list(norms[:n.value - 1])
        return list(errors)

    def _optimize_stepwise(self, num_iterations, log, plot, return_norms):
        """:247-303 statement by statement, for the calls that print or plot between iterations."""
        lm = self.solver == PoseGraphSolver.LevenbergMarquardt
        tolerance, lam, norms = 1e-4, 0.01, []          # :253-255
        last_error = self.global_error()
        errors = [last_error]
        if log:                                         # :258-265
            print(f"Loaded graph with {self.num_nodes} nodes and {self.num_edges} edges")
            print(f"initial error :{errors[-1]:.5f}", flush=True)
        if plot:                                        # :266-268
            self.plot()
        for i in range(num_iterations):
            self.iteration += 1
            dx = self.linearize_and_solve(lam, lm)      # :271 (lambda reaches the diagonal only for Levenberg-Marquardt, :362-366)
            self.update_nodes(dx)
            norm_dx = float(np.sqrt(np.dot(dx, dx)))    # :273
            error = self.global_error()
            if lm:                                      # :275-282
                if last_error < error:
                    self.update_nodes(dx, -1.0)
                    lam *= 2.0
                else:
                    lam /= 2.0
            last_error = error
            norms.append(norm_dx)
            errors.append(error)
            if log:                                     # :288-293
                print(f"step {i:3} : |dx| = {norm_dx:3.5f}, error = {errors[-1]:3.5f}", flush=True)
            if plot:                                    # :294-296
                self.plot()
            if norm_dx < tolerance:                     # :298-300
                break
        return (errors, norms) if return_norms else errors

    # -- robust kernels (include/rr_pgo.h, "robust kernels") ----------------------------
    def set_robust_kernel(self, kind, delta=1.0, edge_mask=None):
        """Robust kernel of every later linearisation: kind None (plain least squares), "huber" or "cauchy"; delta in the
        units of sqrt(e^T Omega e); edge_mask: per edge, nonzero = robustified (None: every edge).  chi2 and the errors
        optimize() returns are then the robust cost sum rho(e^T Omega e)."""
        key = kind.lower() if isinstance(kind, str) else kind
        if key not in _lib.ROBUST_KERNELS:
            raise ValueError(f"unknown robust kernel {kind!r}: None, 'huber' or 'cauchy'")
        mask = None
        if edge_mask is not None:
            mask = np.ascontiguousarray(edge_mask).astype(np.int32)
            if mask.shape != (self.num_edges,):
                raise ValueError("edge_mask needs one entry per edge")
        _check(_lib.load().rr_pgo_set_robust_kernel(self._h, _lib.ROBUST_KERNELS[key], float(delta),
                                                    None if mask is None else _ip(mask)))

    def _edge_mask(self, edge_mask):
        if edge_mask is None:
            return None
        mask = np.ascontiguousarray(edge_mask).astype(np.int32)
        if mask.shape != (self.num_edges,):
            raise ValueError("edge_mask needs one entry per edge")
        return mask

    # -- truncated least squares and graduated non-convexity (include/rr_pgo.h, rr_pgo_optimize_gnc) ----
    def set_robust_tls(self, delta, mu=1.0, edge_mask=None):
        """Truncated least squares with continuation parameter mu as the handle's robust kernel: w = 1 up to
        mu / (mu + 1) delta^2, w = 0 from (mu + 1) / mu delta^2 on, delta sqrt(mu (mu + 1) / s) - mu in between."""
        mask = self._edge_mask(edge_mask)
        _check(_lib.load().rr_pgo_set_robust_tls(self._h, float(delta), float(mu), None if mask is None else _ip(mask)))

    def set_robust_mu(self, mu):
        """mu of the truncated-least-squares kernel alone (the mask and delta stay)."""
        _check(_lib.load().rr_pgo_set_robust_mu(self._h, float(mu)))

    @property
    def robust_setting(self):
        """(kind, delta, mu) of the handle's robust kernel: kind 0 none, 1 huber, 2 cauchy, 3 truncated least squares; mu is 0
        for the kinds without one."""
        kind, delta, mu = C.c_int32(), C.c_double(), C.c_double()
        _check(_lib.load().rr_pgo_get_robust(self._h, C.byref(kind), C.byref(delta), C.byref(mu)))
        return kind.value, delta.value, mu.value

    def optimize_gnc(self, delta, edge_mask=None, mu_factor=1.4, max_stages=100, inner_iterations=1, final_iterations=20):
        """rr_pgo_optimize_gnc: graduated non-convexity on truncated least squares from the current state.  delta^2 is the
        chi-square quantile beyond which a masked edge (None: every edge; usually the loop closures) counts as an outlier.
        Returns a dict of the result fields plus stage_mu and stage_cost (one entry per stage run).  The handle keeps the
        kernel at mu_last: edge_errors()[1] == 0 names the rejected edges."""
        L = _lib.load()
        opt = _lib.GncOptions()
        L.rr_pgo_default_gnc_options(C.byref(opt))
        opt.delta, opt.mu_factor = float(delta), float(mu_factor)
        opt.max_stages, opt.inner_iterations, opt.final_iterations = int(max_stages), int(inner_iterations), int(final_iterations)
        mask = self._edge_mask(edge_mask)
        res = _lib.GncResult()
        n = max(opt.max_stages, 1)
        stage_mu, stage_cost = np.zeros(n), np.zeros(n)
        _check(L.rr_pgo_optimize_gnc(self._h, C.byref(opt), None if mask is None else _ip(mask), C.byref(res), _dp(stage_mu),
                                     _dp(stage_cost)))
        out = {name: getattr(res, name) for name, _ in _lib.GncResult._fields_}
        out["stage_mu"], out["stage_cost"] = stage_mu[:res.n_stages].copy(), stage_cost[:res.n_stages].copy()
        return out

    def gnc_times(self):
        """HIP-event milliseconds of the last optimize_gnc call: (scans, stages, closing iterations)."""
        return self._times(_lib.load().rr_pgo_gnc_times)

    def edge_errors(self):
        """(s, w): e^T Omega e of every edge at the current state and its robust weight (1 without a kernel), file order."""
        s, w = np.zeros(self.num_edges), np.zeros(self.num_edges)
        _check(_lib.load().rr_pgo_edge_errors(self._h, _dp(s), _dp(w)))
        return s, w

    # -- priors (include/rr_pgo.h, "absolute priors") --------------------------------------
    def set_priors(self, node, meas, info, robust=None, keep_anchor=True):
        """Replace the handle's prior list.  node: node index per prior; meas, info: flat, packed in prior order as an
        edge of the node's kind is (SE2 pose 3 | 6, XY landmark 2 | 3, SE3 pose 7 | 21); robust: per prior, nonzero = under
        the handle's robust kernel (None: none); keep_anchor False drops the 1e7 anchor term, the priors alone then fix
        the gauge.  Takes effect from the next linearisation on; an empty list clears."""
        node = np.ascontiguousarray(node, np.int32).reshape(-1)
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1)
        info = np.ascontiguousarray(info, np.float64).reshape(-1)
        flags = None
        if robust is not None:
            flags = np.ascontiguousarray(robust).astype(np.int32).reshape(-1)
            if flags.shape != node.shape:
                raise ValueError("robust needs one entry per prior")
        # the library reads the packed arrays prior by prior, up to the first node it refuses: they must reach that far
        d = _lib.GraphDesc()
        _check(_lib.load().rr_pgo_get_graph(self._h, C.byref(d)))
        nk = np.ctypeslib.as_array(d.node_kind, (d.n_nodes,)) if d.n_nodes else np.zeros(0, np.int32)
        bad = np.flatnonzero((node < 0) | (node >= len(nk)))
        kinds = nk[node[:int(bad[0])] if len(bad) else node]
        need_m, need_i = int(np.sum(np.take(GATE_MEAS_LEN, kinds))), int(np.sum(np.take(GATE_INFO_LEN, kinds)))
        if (len(meas) < need_m or len(info) < need_i) if len(bad) else (len(meas) != need_m or len(info) != need_i):
            raise ValueError("meas / info do not have the length the priors' node kinds ask for")
        _check(_lib.load().rr_pgo_set_priors(self._h, len(node), _ip(node), _dp(meas), _dp(info),
                                             None if flags is None else _ip(flags), 1 if keep_anchor else 0))

    def clear_priors(self):
        """Back to a handle without priors (the anchor term is kept again)."""
        _check(_lib.load().rr_pgo_set_priors(self._h, 0, None, None, None, None, 1))

    @property
    def num_priors(self):
        return _lib.load().rr_pgo_num_priors(self._h)

    def prior_errors(self):
        """(s, w): e^T Omega e of every prior at the current state and its robust weight (1 unless flagged and a kernel is
        set), in the order of the set_priors call."""
        n = self.num_priors
        s, w = np.zeros(n), np.zeros(n)
        _check(_lib.load().rr_pgo_prior_errors(self._h, _dp(s), _dp(w)))
        return s, w

    # -- fixed nodes (include/rr_pgo.h, "fixed nodes") --------------------------------------
    def set_fixed(self, nodes, keep_anchor=True):
        """Replace the set of nodes held constant (node indices; a node listed twice counts once).  A fixed node never
        moves, its dx is 0, and covariances and gates are conditional on it.  keep_anchor False drops the 1e7 anchor
        term: the fixed set (plus any priors) then fixes the gauge.  Takes effect from the next linearisation on; an
        empty list clears."""
        nodes = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        _check(_lib.load().rr_pgo_set_fixed(self._h, len(nodes), _ip(nodes) if len(nodes) else None, 1 if keep_anchor else 0))

    def clear_fixed(self):
        """Back to a handle without fixed nodes (the anchor term is kept again)."""
        _check(_lib.load().rr_pgo_set_fixed(self._h, 0, None, 1))

    @property
    def num_fixed(self):
        return _lib.load().rr_pgo_num_fixed(self._h)

    def fixed_nodes(self):
        """The distinct fixed nodes, ascending."""
        out = np.zeros(self.num_fixed, np.int32)
        _check(_lib.load().rr_pgo_get_fixed(self._h, _ip(out) if len(out) else None))
        return out

    # -- initialisation from the measurements (include/rr_pgo.h, rr_pgo_initialize) ------------
    INIT_METHODS = {"chordal": 0}

    def initialize(self, method="chordal"):
        """rr_pgo_initialize: replace the state of every free node by the chordal relaxation of the graph (relaxed rotations,
        projection onto SO(d), positions).  Fixed nodes and a kept anchor are held at their current state; the robust setting
        plays no part.  method: "chordal", or the C enum's integer."""
        if isinstance(method, str):
            if method not in self.INIT_METHODS:
                raise ValueError(f"unknown initialisation method {method!r}: 'chordal'")
            method = self.INIT_METHODS[method]
        _check(_lib.load().rr_pgo_initialize(self._h, int(method)))

    def initialize_times(self):
        """HIP-event milliseconds of the last initialize call: (rotation stages with the projection, position stage, whole call)."""
        return self._times(_lib.load().rr_pgo_initialize_times)

    # -- factor queries on fronts beyond LDS (include/rr_pgo.h, "factor queries on fronts beyond LDS") --
    @property
    def query_big_fronts(self):
        """Whether covariance_blocks, cross_covariances, gate_edges, gate_joint and check_edges answer on a graph with fronts
        beyond LDS (stats()["n_big_fronts"] != 0).  Off by default: such graphs are refused.  extend and remove_edges keep it."""
        return bool(_lib.load().rr_pgo_get_query_big_fronts(self._h))

    @query_big_fronts.setter
    def query_big_fronts(self, on):
        _check(_lib.load().rr_pgo_set_query_big_fronts(self._h, 1 if on else 0))

    @property
    def marginals_big_fronts(self):
        """Whether marginal_blocks answers on a graph with fronts beyond LDS (stats()["n_big_fronts"] != 0).  Off by default:
        such graphs are refused.  Independent of query_big_fronts.  extend and remove_edges keep it."""
        return bool(_lib.load().rr_pgo_get_marginals_big_fronts(self._h))

    @marginals_big_fronts.setter
    def marginals_big_fronts(self, on):
        _check(_lib.load().rr_pgo_set_marginals_big_fronts(self._h, 1 if on else 0))

    # -- marginal covariances (include/rr_pgo.h, "marginal covariances") -----------------
    def marginal_blocks(self, node_a=None, node_b=None):
        """rr_pgo_marginals as it is: (values, offsets) of the queried blocks of Sigma = H^-1 at the current state.
        node_a None: every node's diagonal block; node_b None: the diagonal blocks of node_a."""
        L = _lib.load()
        a = None if node_a is None else np.ascontiguousarray(node_a, np.int32)
        b = None if node_b is None else np.ascontiguousarray(node_b, np.int32)
        if b is not None and (a is None or a.shape != b.shape):
            raise ValueError("node_a and node_b need the same length")
        nq = self.num_nodes if a is None else len(a)
        off = np.zeros(nq + 1, np.int64)
        nv = C.c_int64()
        pa, pb = (None if a is None else _ip(a)), (None if b is None else _ip(b))
        po = off.ctypes.data_as(C.POINTER(C.c_int64))
        _check(L.rr_pgo_marginals(self._h, nq, pa, pb, None, po, C.byref(nv)))
        vals = np.zeros(nv.value)
        _check(L.rr_pgo_marginals(self._h, nq, pa, pb, _dp(vals), po, C.byref(nv)))
        return vals, off

    def marginals(self, nodes=None):
        """Covariance of every node (or of `nodes`): a list of d x d arrays, tangent coordinates in dx's order."""
        vals, off = self.marginal_blocks(nodes)
        out = []
        for q in range(len(off) - 1):
            d = int(round(np.sqrt(off[q + 1] - off[q])))
            out.append(vals[off[q]:off[q + 1]].reshape(d, d).copy())
        return out

    def joint_marginal(self, a, b):
        """[[S_aa, S_ab], [S_ab^T, S_bb]] of two nodes that share a front of the factor (every pair joined by an edge
        does), from one call."""
        vals, off = self.marginal_blocks([a, b, a], [a, b, b])
        da, db = int(round(np.sqrt(off[1] - off[0]))), int(round(np.sqrt(off[2] - off[1])))
        saa, sbb = vals[off[0]:off[1]].reshape(da, da), vals[off[1]:off[2]].reshape(db, db)
        sab = vals[off[2]:off[3]].reshape(da, db)
        return np.block([[saa, sab], [sab.T, sbb]])

    def _times(self, fn):
        ms = np.zeros(3)
        _check(fn(self._h, _dp(ms)))
        return tuple(float(v) for v in ms)

    def marginals_times(self):
        """HIP-event milliseconds of the last marginals call: (linearise + factor, selected inverse, gather)."""
        return self._times(_lib.load().rr_pgo_marginals_times)

    # -- covariances of arbitrary pairs (include/rr_pgo.h, rr_pgo_covariances) -----------
    def covariance_blocks(self, node_a, node_b):
        """rr_pgo_covariances as it is: (values, offsets) of the blocks Sigma(node_a[q], node_b[q]) at the current state,
        for ANY pairs of nodes (a == b: the diagonal block); a node may appear in any number of queries."""
        L = _lib.load()
        a = np.ascontiguousarray(node_a, np.int32)
        b = np.ascontiguousarray(node_b, np.int32)
        if a.ndim != 1 or a.shape != b.shape:
            raise ValueError("node_a and node_b need the same length")
        nq = len(a)
        off = np.zeros(nq + 1, np.int64)
        nv = C.c_int64()
        po = off.ctypes.data_as(C.POINTER(C.c_int64))
        _check(L.rr_pgo_covariances(self._h, nq, _ip(a), _ip(b), None, po, C.byref(nv)))
        vals = np.zeros(nv.value)
        _check(L.rr_pgo_covariances(self._h, nq, _ip(a), _ip(b), _dp(vals), po, C.byref(nv)))
        return vals, off

    def covariance(self, nodes):
        """Dense joint covariance of a set of nodes, (sum d) x (sum d), blocks in the order of `nodes`: the lower block
        triangle from one rr_pgo_covariances call, mirrored (so the result is symmetric bit for bit)."""
        nodes = [int(v) for v in nodes]
        k = len(nodes)
        ia, ib = np.tril_indices(k)
        a = np.array([nodes[i] for i in ia], np.int32)
        b = np.array([nodes[j] for j in ib], np.int32)
        vals, off = self.covariance_blocks(a, b)
        dims = [0] * k
        for q in range(len(ia)):
            if ia[q] == ib[q]:
                dims[ia[q]] = int(round(np.sqrt(off[q + 1] - off[q])))
        start = np.concatenate([[0], np.cumsum(dims)]).astype(int)
        out = np.zeros((start[-1], start[-1]))
        for q in range(len(ia)):
            i, j = int(ia[q]), int(ib[q])
            blk = vals[off[q]:off[q + 1]].reshape(dims[i], dims[j])
            out[start[i]:start[i + 1], start[j]:start[j + 1]] = blk
            if i != j:
                out[start[j]:start[j + 1], start[i]:start[i + 1]] = blk.T
        return out

    def covariances_times(self):
        """HIP-event milliseconds of the last covariance call: (linearise + factor, tree solve, products + gather)."""
        return self._times(_lib.load().rr_pgo_covariances_times)

    # -- Sigma[rows, cols] by a backward solve (include/rr_pgo.h, rr_pgo_cross_covariances) ----
    def cross_covariance(self, rows, cols):
        """rr_pgo_cross_covariances: the (R, C) block Sigma[rows, cols] at the current state -- the scalars of the nodes
        of `rows` stacked in that order by the scalars of the nodes of `cols`, each node's in dx's order.  rows None: every
        node in node order, so row i is scalar i of dx.  A node may repeat in either list."""
        L = _lib.load()
        r = None if rows is None else np.ascontiguousarray(rows, np.int32)
        c = np.ascontiguousarray(cols, np.int32)
        if c.ndim != 1 or (r is not None and r.ndim != 1):
            raise ValueError("rows and cols are flat lists of node indices")
        nr, nc = (self.num_nodes if r is None else len(r)), len(c)
        roff, coff = np.zeros(nr + 1, np.int64), np.zeros(nc + 1, np.int64)
        nv = C.c_int64()
        pr, pc = (None if r is None else _ip(r)), (_ip(c) if nc else None)
        pro, pco = roff.ctypes.data_as(C.POINTER(C.c_int64)), coff.ctypes.data_as(C.POINTER(C.c_int64))
        _check(L.rr_pgo_cross_covariances(self._h, nr, pr, nc, pc, None, pro, pco, C.byref(nv)))
        out = np.zeros((int(roff[-1]), int(coff[-1])))
        if nv.value:
            _check(L.rr_pgo_cross_covariances(self._h, nr, pr, nc, pc, _dp(out), pro, pco, C.byref(nv)))
        return out

    def covariance_columns(self, cols):
        """The block columns Sigma[:, cols], (dim, C): how the nodes of `cols` co-vary with every scalar of the graph, for
        one forward solve on their root paths and one backward sweep of the tree."""
        return self.cross_covariance(None, cols)

    def cross_covariances_times(self):
        """HIP-event milliseconds of the last cross_covariance call: (linearise + factor, forward + backward solve,
        gather + copy)."""
        return self._times(_lib.load().rr_pgo_cross_covariances_times)

    # -- Mahalanobis gate of candidate loop closures (include/rr_pgo.h, rr_pgo_gate_edges) ----
    def gate_edges(self, edge_kind, edge_from, edge_to, edge_meas, edge_info, return_innovation=False):
        """rr_pgo_gate_edges: (d2, chi2) of candidate edges that are not part of the graph, in rr_pgo_graph_desc packing --
        d2 = e^T S^-1 e with S = Omega^-1 + J Sigma J^T at the current state, chi2 = e^T Omega e.  With return_innovation
        also the list of the d_e x d_e matrices S (1 x 1 for an SE2_BEARING or SE2_RANGE candidate, which packs one
        measurement value and one information value)."""
        L = _lib.load()
        kind = np.ascontiguousarray(edge_kind, np.int32)
        a = np.ascontiguousarray(edge_from, np.int32)
        b = np.ascontiguousarray(edge_to, np.int32)
        meas = np.ascontiguousarray(edge_meas, np.float64).ravel()
        info = np.ascontiguousarray(edge_info, np.float64).ravel()
        if kind.ndim != 1 or a.shape != kind.shape or b.shape != kind.shape:
            raise ValueError("edge_kind, edge_from and edge_to need the same length")
        known = np.isin(kind, KNOWN_KINDS)   # (an unknown kind is the library's to refuse: the lengths are then not checked)
        if np.all(known):
            if len(meas) != int(np.sum(np.take(GATE_MEAS_LEN, kind))) or len(info) != int(np.sum(np.take(GATE_INFO_LEN, kind))):
                raise ValueError("edge_meas / edge_info do not have the length the edge kinds ask for")
        n = len(kind)
        d2, chi2 = np.zeros(n), np.zeros(n)
        off = np.zeros(n + 1, np.int64)
        vals = None
        if return_innovation:
            vals = np.zeros(36 * max(n, 1))
        _check(L.rr_pgo_gate_edges(self._h, n, _ip(kind), _ip(a), _ip(b), _dp(meas), _dp(info), _dp(d2), _dp(chi2),
                                   None if vals is None else _dp(vals), off.ctypes.data_as(C.POINTER(C.c_int64))))
        if not return_innovation:
            return d2, chi2
        dims = [int(round(np.sqrt(off[c + 1] - off[c]))) for c in range(n)]
        return d2, chi2, [vals[off[c]:off[c + 1]].reshape(dims[c], dims[c]).copy() for c in range(n)]

    def gate(self, edge_kind, edge_from, edge_to, edge_meas, edge_info, threshold=None):
        """Boolean mask d2 <= threshold of the candidates (True: accept).  threshold: a scalar, a mapping from edge kind
        (0 SE2, 1 SE2_XY, 2 SE3, 3 SE3_XYZ, 4 SE2_BEARING, 6 SE2_RANGE) to a scalar, or None: the 0.95 chi-square quantile
        of the edge's dimension (3.841 for the two one-scalar kinds)."""
        d2, _ = self.gate_edges(edge_kind, edge_from, edge_to, edge_meas, edge_info)
        return d2 <= gate_thresholds(edge_kind, threshold)

    def gate_times(self):
        """HIP-event milliseconds of the last gate_edges call: (linearise + factor, tree solve, gate kernel + copy)."""
        return self._times(_lib.load().rr_pgo_gate_times)

    # -- joint compatibility of sets of candidates (include/rr_pgo.h, rr_pgo_gate_joint) ------
    def gate_joint(self, edge_kind, edge_from, edge_to, edge_meas, edge_info, sets, return_prefix=False,
                   return_innovation=False):
        """rr_pgo_gate_joint: d2 of every set of `sets` -- ordered lists of indices into the candidates, which are given as
        for gate_edges.  d2[s] = e_s^T S_s^-1 e_s with the stacked errors e_s and the joint innovation covariance S_s.
        return_prefix adds the list of per-set arrays of prefix distances (entry k: the set cut after its candidate k),
        return_innovation the list of the D_s x D_s matrices S_s; the result is d2 alone or a tuple in that order."""
        L = _lib.load()
        kind = np.ascontiguousarray(edge_kind, np.int32)
        a = np.ascontiguousarray(edge_from, np.int32)
        b = np.ascontiguousarray(edge_to, np.int32)
        meas = np.ascontiguousarray(edge_meas, np.float64).ravel()
        info = np.ascontiguousarray(edge_info, np.float64).ravel()
        if kind.ndim != 1 or a.shape != kind.shape or b.shape != kind.shape:
            raise ValueError("edge_kind, edge_from and edge_to need the same length")
        if np.all(np.isin(kind, KNOWN_KINDS)):   # (an unknown kind is the library's to refuse)
            if len(meas) != int(np.sum(np.take(GATE_MEAS_LEN, kind))) or len(info) != int(np.sum(np.take(GATE_INFO_LEN, kind))):
                raise ValueError("edge_meas / edge_info do not have the length the edge kinds ask for")
        sets = [np.asarray(s, np.int32).ravel() for s in sets]
        ns = len(sets)
        ptr = np.zeros(ns + 1, np.int32)
        ptr[1:] = np.cumsum([len(s) for s in sets])
        flat = np.ascontiguousarray(np.concatenate(sets) if ns else np.zeros(0), np.int32)
        d2, prefix = np.zeros(ns), np.zeros(max(len(flat), 1))
        off = np.zeros(ns + 1, np.int64)
        vals = np.zeros(_lib.GATE_JOINT_MAX_DIM ** 2 * max(ns, 1)) if return_innovation else None
        _check(L.rr_pgo_gate_joint(self._h, len(kind), _ip(kind), _ip(a), _ip(b), _dp(meas), _dp(info), ns, _ip(ptr), _ip(flat),
                                   _dp(d2), _dp(prefix) if return_prefix else None, None if vals is None else _dp(vals),
                                   off.ctypes.data_as(C.POINTER(C.c_int64))))
        out = [d2]
        if return_prefix:
            out.append([prefix[ptr[s]:ptr[s + 1]].copy() for s in range(ns)])
        if return_innovation:
            dims = [int(round(np.sqrt(off[s + 1] - off[s]))) for s in range(ns)]
            out.append([vals[off[s]:off[s + 1]].reshape(dims[s], dims[s]).copy() for s in range(ns)])
        return d2 if len(out) == 1 else tuple(out)

    def gate_joint_accept(self, edge_kind, edge_from, edge_to, edge_meas, edge_info, sets, threshold=None):
        """Boolean per set, d2 <= threshold (True: the candidates of the set are jointly compatible).  threshold: a scalar,
        or None: the 0.95 chi-square quantile of D_s degrees of freedom (CHI2_95)."""
        d2 = self.gate_joint(edge_kind, edge_from, edge_to, edge_meas, edge_info, sets)
        return d2 <= gate_joint_thresholds(edge_kind, sets, threshold)

    def gate_joint_times(self):
        """HIP-event milliseconds of the last gate_joint call: (linearise + factor, tree solve, joint kernel + copy)."""
        return self._times(_lib.load().rr_pgo_gate_joint_times)

    # -- growing a live handle (include/rr_pgo.h, rr_pgo_extend) -------------------------------
    def extend(self, edge_kind, edge_from, edge_to, edge_meas, edge_info, node_kind=None, node_state=None, node_id=None):
        """rr_pgo_extend: append nodes (node_kind; None: none) and edges, in rr_pgo_graph_desc packing, to this handle.
        The estimate of the old nodes stays on the device, bit for bit; new nodes take node_state, or -- node_state None --
        an initial value composed on the device along the new edges.  Returns (first_new_node, first_new_edge)."""
        L = _lib.load()
        kind = np.ascontiguousarray(edge_kind, np.int32).ravel()
        a = np.ascontiguousarray(edge_from, np.int32).ravel()
        b = np.ascontiguousarray(edge_to, np.int32).ravel()
        meas = np.ascontiguousarray(edge_meas, np.float64).ravel()
        info = np.ascontiguousarray(edge_info, np.float64).ravel()
        if a.shape != kind.shape or b.shape != kind.shape:
            raise ValueError("edge_kind, edge_from and edge_to need the same length")
        if np.all(np.isin(kind, KNOWN_KINDS)):   # (an unknown kind is the library's to refuse: the lengths are then not checked)
            if len(meas) != int(np.sum(np.take(GATE_MEAS_LEN, kind))) or len(info) != int(np.sum(np.take(GATE_INFO_LEN, kind))):
                raise ValueError("edge_meas / edge_info do not have the length the edge kinds ask for")
        nk = np.zeros(0, np.int32) if node_kind is None else np.ascontiguousarray(node_kind, np.int32).ravel()
        if node_kind is None and (node_state is not None or node_id is not None):
            raise ValueError("node_state / node_id without node_kind")
        st = ids = None
        if node_state is not None:
            st = np.ascontiguousarray(node_state, np.float64).ravel()
            if np.all(np.isin(nk, KNOWN_NODE_KINDS)) and len(st) != int(np.sum(np.take(NODE_STATE_LEN, nk))):
                raise ValueError("node_state does not have the length the node kinds ask for")
        if node_id is not None:
            ids = np.ascontiguousarray(node_id, np.uint32).ravel()
            if ids.shape != nk.shape:
                raise ValueError("node_id needs one entry per new node")
        first = (self.num_nodes, self.num_edges)
        _check(L.rr_pgo_extend(self._h, len(nk), _ip(nk), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                               None if st is None else _dp(st), len(kind), _ip(kind), _ip(a), _ip(b), _dp(meas), _dp(info)))
        return first

    def extend_times(self):
        """Milliseconds of the last extend call: (symbolic analysis, engine construction -- host wall clock; state carry +
        initial guess -- HIP events)."""
        return self._times(_lib.load().rr_pgo_extend_times)

    # -- audit of the graph's own edges (include/rr_pgo.h, rr_pgo_check_edges, rr_pgo_remove_edges) ----
    def check_edges(self, edges=None, return_residual=False):
        """rr_pgo_check_edges: a dict with, per queried edge (None: every edge), d2 = e^T R^-1 e -- the leave-one-out
        distance, R = Omega_w^-1 - J Sigma J^T the covariance of the residual -- redundancy = trace(R Omega_w) / d_e in
        [0, 1] (0: a bridge, d2 then says nothing) and chi2 = e^T Omega e.  With return_residual also R, the list of the
        d_e x d_e matrices, and redundancy_min, the smallest directional redundancy (directional_redundancy): where it is
        near 0 part of the residual is a bridge and d2 says nothing either, whatever the mean r is."""
        L = _lib.load()
        idx = None if edges is None else np.ascontiguousarray(edges, np.int32).ravel()
        n = self.num_edges if idx is None else len(idx)
        d2, red, chi2 = np.zeros(n), np.zeros(n), np.zeros(n)
        off = np.zeros(n + 1, np.int64)
        vals = np.zeros(36 * max(n, 1)) if return_residual else None
        _check(L.rr_pgo_check_edges(self._h, n, None if idx is None else _ip(idx), _dp(d2), _dp(red), _dp(chi2),
                                    None if vals is None else _dp(vals), off.ctypes.data_as(C.POINTER(C.c_int64))))
        out = {"d2": d2, "redundancy": red, "chi2": chi2}
        if return_residual:
            dims = [int(round(np.sqrt(off[c + 1] - off[c]))) for c in range(n)]
            out["R"] = [vals[off[c]:off[c + 1]].reshape(dims[c], dims[c]).copy() for c in range(n)]
            ek, ei = self.graph_arrays()[2], self.graph_arrays()[6]
            io = np.concatenate([[0], np.cumsum(np.take(GATE_INFO_LEN, ek))]).astype(int)
            rmin = np.zeros(n)
            for c in range(n):
                k = c if idx is None else int(idx[c])
                W = np.zeros((dims[c], dims[c]))
                W[np.triu_indices(dims[c])] = ei[io[k]:io[k + 1]]
                # (an edge of weight exactly 0 under truncated least squares: R is NaN, and so is every figure of it)
                rmin[c] = directional_redundancy(out["R"][c], W + np.triu(W, 1).T, red[c]) if np.isfinite(out["R"][c]).all() else np.nan
            out["redundancy_min"] = rmin
        return out

    def suspect_edges(self, threshold=None, min_redundancy=0.01, edges=None, checked=None, min_directional=SINGULAR_DIRECTION):
        """Indices of the edges (of `edges`; None: every edge) that disagree with the rest of the graph: redundancy at least
        min_redundancy and d2 above the threshold -- a scalar, a mapping from edge kind to a scalar, or None: the 0.95
        chi-square quantile of the edge's dimension -- sorted by falling d2.  An edge part of whose residual nothing else
        constrains (smallest directional redundancy at most min_directional: R singular to rounding, d2 meaningless
        whatever r says) is never named.  checked: the result of check_edges(edges, return_residual=True), if the caller
        has it already."""
        idx = np.arange(self.num_edges, dtype=np.int32) if edges is None else np.ascontiguousarray(edges, np.int32).ravel()
        c = self.check_edges(None if edges is None else idx, return_residual=True) if checked is None else checked
        kind = self.graph_arrays()[2][idx]
        return idx[select_suspects(kind, c["d2"], c["redundancy"], c["redundancy_min"], threshold, min_redundancy, min_directional)]

    def check_edges_times(self):
        """HIP-event milliseconds of the last check_edges call: (linearise + factor, tree solve, kernel + copy)."""
        return self._times(_lib.load().rr_pgo_check_edges_times)

    def remove_edges(self, edges):
        """rr_pgo_remove_edges: take the listed edges out of this handle (a duplicate counts once).  The remaining edges keep
        their order and are renumbered compactly; the estimate stays on the device, bit for bit; anchor_node may change."""
        idx = np.ascontiguousarray(edges, np.int32).ravel()
        _check(_lib.load().rr_pgo_remove_edges(self._h, len(idx), _ip(idx)))

    def remove_edges_times(self):
        """Milliseconds of the last remove_edges call: (symbolic analysis, engine construction -- host wall clock; state
        carry -- HIP events)."""
        return self._times(_lib.load().rr_pgo_remove_edges_times)

    # -- PoseGraph::plot, :375-431 -------------------------------------------------------
    def plot_data(self):
        """What the reference's figure shows: the poses (blue circles), the same poses joined in the order of their ids
        (red line), the landmarks if there are any (red stars).  SE(3) graphs are `todo!()` in the reference (:398-399) and stay
        refused, so that a caller of the reference's figure meets the reference's behaviour; a 3-D graph with XYZ landmarks has
        no counterpart there (build-defined kinds), and is shown as its x-y projection, landmarks as points like the 2-D ones."""
        L = _lib.load()
        d = _lib.GraphDesc()
        _check(L.rr_pgo_get_graph(self._h, C.byref(d)))
        n = d.n_nodes
        kinds = np.ctypeslib.as_array(d.node_kind, (n,)) if n else np.zeros(0, np.int32)
        if np.any(kinds == 2) and not np.any(kinds == 3):
            raise PoseGraphError(_lib.EUNSUPPORTED, "plot of an SE(3) graph: todo!() in the reference (pose_graph_optimization.rs:398-399)")
        ids = np.ctypeslib.as_array(d.node_id, (n,)).astype(np.int64) if (n and d.node_id) else np.arange(n)
        st = self.state()
        # (a 3-D graph with XYZ landmarks, build-defined: its x-y projection, the landmarks as points like the 2-D ones)
        offs = np.concatenate([[0], np.cumsum(np.take(NODE_STATE_LEN, kinds))])[:-1].astype(np.int64)
        xy = np.stack([st[offs], st[offs + 1]], 1) if n else np.zeros((0, 2))
        pose = (kinds == 0) | (kinds == 2)
        order = np.argsort(ids[pose], kind="stable")
        return {"poses": xy[pose], "poses_seq": xy[pose][order], "landmarks": xy[~pose],
                "file": f"img/{self.name}-{self.iteration}-{self.solver.name}.svg"}

    def plot(self, directory="."):
        """Writes the figure as SVG (the reference goes through plotpy / matplotlib; here the file is written directly)."""
        import os
        pd = self.plot_data()
        pts = [pd["poses"], pd["landmarks"]]
        allp = np.concatenate([p for p in pts if len(p)]) if any(len(p) for p in pts) else np.zeros((1, 2))
        lo, hi = allp.min(0), allp.max(0)
        span = float(max(hi[0] - lo[0], hi[1] - lo[1], 1e-9))      # equal axes (:425)
        size, margin = 640.0, 40.0
        scale = (size - 2 * margin) / span

        def px(p):
            return margin + (p[0] - lo[0]) * scale, size - margin - (p[1] - lo[1]) * scale

        out = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{size:.0f}" height="{size:.0f}" viewBox="0 0 {size:.0f} {size:.0f}">',
               '<rect width="100%" height="100%" fill="white"/>']
        if len(pd["poses_seq"]):
            path = " ".join(f"{x:.2f},{y:.2f}" for x, y in map(px, pd["poses_seq"]))
            out.append(f'<polyline points="{path}" fill="none" stroke="red" stroke-width="1"/>')
        for p in pd["poses"]:
            x, y = px(p)
            out.append(f'<circle cx="{x:.2f}" cy="{y:.2f}" r="2" fill="blue"/>')
        for p in pd["landmarks"]:
            x, y = px(p)
            out.append(f'<text x="{x:.2f}" y="{y:.2f}" fill="red" font-size="12" text-anchor="middle" dominant-baseline="central">*</text>')
        out.append("</svg>")
        path = os.path.join(directory, pd["file"])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")
        return path

    def optimize_count(self, num_iterations):
        """rr_pgo_optimize with the buffers of the previous call: the iterations it executed (len(errors) - 1).
        What bench.py's timed loop calls -- optimize() itself, without this mirror's list building around it."""
        buf = getattr(self, "_opt_buf", None)
        if buf is None or len(buf[0]) < num_iterations + 1:
            errors, norms, n = np.zeros(num_iterations + 1), np.zeros(max(num_iterations, 1)), C.c_int32()
            buf = self._opt_buf = (errors, norms, n, _lib.load().rr_pgo_optimize, _dp(errors), C.byref(n), _dp(norms))
        rc = buf[3](self._h, num_iterations, buf[4], buf[5], buf[6])
        if rc != 0:
            _check(rc)
        done = buf[2].value - 1
        self.iteration += done
        return done

    def restarter(self, state):
        """A callable that puts the handle back into `state` (rr_pgo_set_state with everything bound once)."""
        state = np.ascontiguousarray(state, np.float64).copy()
        assert state.shape == (_lib.load().rr_pgo_state_len(self._h),)
        fn, h, ptr = _lib.load().rr_pgo_set_state, self._h, _dp(state)

        def restart(_keep=state):
            rc = fn(h, ptr)
            if rc != 0:
                _check(rc)
        return restart

    def state(self):
        out = np.zeros(_lib.load().rr_pgo_state_len(self._h))
        _check(_lib.load().rr_pgo_get_state(self._h, _dp(out)))
        return out

    def set_state(self, state):
        state = np.ascontiguousarray(state, np.float64)
        assert state.shape == (_lib.load().rr_pgo_state_len(self._h),)
        _check(_lib.load().rr_pgo_set_state(self._h, _dp(state)))

    # -- inspection / measurement ------------------------------------------------------
    def assemble(self, lam=0.0, lm=False):
        """Assembled normal matrix as (row_node, col_node, [blocks]) and b."""
        L = _lib.load()
        nb, nv = C.c_int32(), C.c_int64()
        _check(L.rr_pgo_assemble(self._h, lam, int(lm), C.byref(nb), None, None, None, None, C.byref(nv), None))
        br = np.zeros(nb.value, np.int32)
        bc = np.zeros(nb.value, np.int32)
        bo = np.zeros(nb.value, np.int64)
        vals = np.zeros(nv.value)
        b = np.zeros(self.len)
        _check(L.rr_pgo_assemble(self._h, lam, int(lm), C.byref(nb), _ip(br), _ip(bc),
                                 bo.ctypes.data_as(C.POINTER(C.c_int64)), _dp(vals), C.byref(nv), _dp(b)))
        return br, bc, bo, vals, b

    # -- sharding ONE graph over ranks (include/rr_pgo.h, "sharding") --------------------------------
    def exchange_info(self, which):
        """(device pointer, element count, element size) of exchange buffer `which` (0: boundary update
        matrices, all-gathered; 1: the two partial sums chi2 and |dx|^2, all-reduced)."""
        ptr, n, es = C.c_void_p(), C.c_int64(), C.c_int32()
        _check(_lib.load().rr_pgo_exchange_buffer(self._h, which, C.byref(ptr), C.byref(n), C.byref(es)))
        return ptr.value, n.value, es.value

    def bind_exchange(self, which, dev_ptr, n_elems):
        _check(_lib.load().rr_pgo_set_exchange_buffer(self._h, which, C.c_void_p(dev_ptr), n_elems))

    def stage(self, stage, lam=0.0, lm=False):
        _check(_lib.load().rr_pgo_stage(self._h, stage, lam, int(lm)))

    def stage_scalars(self):
        chi, nrm = C.c_double(), C.c_double()
        _check(_lib.load().rr_pgo_stage_scalars(self._h, C.byref(chi), C.byref(nrm)))
        return chi.value, nrm.value

    def node_owner(self):
        """rank owning every node, -1 = shared (top separators, anchor); zeros on an unsharded handle"""
        out = np.zeros(self.num_nodes, np.int32)
        _check(_lib.load().rr_pgo_node_owner(self._h, _ip(out)))
        return out

    def stream_ptr(self):
        """hipStream_t of the handle as an integer (torch.cuda.ExternalStream takes it)"""
        return int(_lib.load().rr_pgo_stream(self._h) or 0)

    def iterate_async(self, iters):
        _check(_lib.load().rr_pgo_iterate_async(self._h, iters))

    def sync(self):
        _check(_lib.load().rr_pgo_sync(self._h))

    def stats(self):
        s = _lib.Stats()
        _check(_lib.load().rr_pgo_get_stats(self._h, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in _lib.Stats._fields_ if k != "reserved"}
        # form of the back substitution of the LDS fronts (rr_pgo_solve_form): kept apart from bytes_factor / bytes_solve
        kform, kb, kf = C.c_int32(0), C.c_double(0), C.c_double(0)
        _check(_lib.load().rr_pgo_solve_form(self._h, C.byref(kform), C.byref(kb), C.byref(kf)))
        out.update(solve_kform=int(kform.value), kform_bytes=float(kb.value), kform_flops=float(kf.value))
        # iterations enqueued so far, by launch form (rr_pgo_launch_counts): host-side counters of this handle's engine
        counts = (C.c_int64 * 4)()
        _check(_lib.load().rr_pgo_launch_counts(self._h, counts))
        out.update(n_plain_iterations=int(counts[0]), n_graph_replays=int(counts[1]), n_loop_items=int(counts[2]),
                   n_graph_captures=int(counts[3]))
        return out

    @staticmethod
    def analyze(file_path, precision="f64"):
        """Host-only: parse + symbolic analysis, the statistics a handle on the file would report (no device needed)."""
        opt = _lib.Options()
        _lib.load().rr_pgo_default_options(C.byref(opt))
        opt.precision = _lib.PRECISIONS[precision]
        s = _lib.Stats()
        _check(_lib.load().rr_pgo_analyze_g2o(str(file_path).encode(), C.byref(opt), C.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.Stats._fields_ if k != "reserved"}

    def profile(self, iters):
        ms = np.zeros(_lib.NUM_KCLASS)
        n = np.zeros(_lib.NUM_KCLASS, np.int64)
        _check(_lib.load().rr_pgo_profile(self._h, iters, _dp(ms), n.ctypes.data_as(C.POINTER(C.c_int64)), _lib.NUM_KCLASS))
        return {name: (float(ms[i]), int(n[i])) for i, name in enumerate(_lib.KCLASS_NAMES)}


def parse_g2o_arrays(file_path):
    """parse_g2o (g2o.rs:35-143) through the library's loader, returned as the flat arrays `from_arrays` takes
    (needs a device: the loader entry point builds a handle)."""
    return PoseGraph.new(file_path).graph_arrays()


def synthetic_grid_arrays(width, height, n_edges=0, seed_meas=42, seed_init=43):
    L = _lib.load()
    s = C.c_void_p()
    d = _lib.GraphDesc()
    _check(L.rr_pgo_synth_grid(width, height, n_edges, seed_meas, seed_init, C.byref(s), C.byref(d)))
    try:
        n, m = d.n_nodes, d.n_edges
        out = (np.ctypeslib.as_array(d.node_kind, (n,)).copy(), np.ctypeslib.as_array(d.node_state, (3 * n,)).copy(),
               np.ctypeslib.as_array(d.edge_kind, (m,)).copy(), np.ctypeslib.as_array(d.edge_from, (m,)).copy(),
               np.ctypeslib.as_array(d.edge_to, (m,)).copy(), np.ctypeslib.as_array(d.edge_meas, (3 * m,)).copy(),
               np.ctypeslib.as_array(d.edge_info, (6 * m,)).copy())
    finally:
        L.rr_pgo_synth_free(s)
    return out
