"""CPU reference for truncated least squares and the graduated non-convexity driver (include/rr_pgo.h,
rr_pgo_set_robust_tls / rr_pgo_optimize_gnc), built on RobustReference and so on the unchanged oracle.

The formulas are restated here from the header, not imported from the package.  With c = delta, s = e^T Omega e, mu > 0,
lo = mu / (mu + 1) c^2 and hi = (mu + 1) / mu c^2:
    s <= lo (and s < 0)   w = 1                               rho = s
    lo < s < hi           w = c sqrt(mu (mu + 1) / s) - mu    rho = 2 c sqrt(s mu (mu + 1)) - mu (c^2 + s)
    s >= hi               w = 0                               rho = c^2
gnc() is the loop of rr_pgo_optimize_gnc, statement by statement.
"""
import numpy as np

from robust_reference import RobustReference


def tls_band(delta, mu):
    c2 = delta * delta
    return mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2


def tls_weight(s, delta, mu):
    s = np.asarray(s, np.float64)
    lo, hi = tls_band(delta, mu)
    band = (s > lo) & (s < hi)
    inner = delta * np.sqrt(mu * (mu + 1.0) / np.where(band, s, 1.0)) - mu
    return np.where(s <= lo, 1.0, np.where(s >= hi, 0.0, inner))


def tls_rho(s, delta, mu):
    s = np.asarray(s, np.float64)
    lo, hi = tls_band(delta, mu)
    band = (s > lo) & (s < hi)
    c2 = delta * delta
    inner = 2.0 * delta * np.sqrt(np.where(band, s, 1.0) * mu * (mu + 1.0)) - mu * (c2 + s)
    return np.where(s <= lo, s, np.where(s >= hi, c2, inner))


class GncReference(RobustReference):
    """RobustReference under the truncated-least-squares kernel (delta, mu); `mu` may be changed between calls."""

    def __init__(self, arrays, delta, mu=1.0, mask=None):
        super().__init__(arrays, "tls", delta, mask)
        self.mu = float(mu)

    def weights(self, s):
        return np.where(self.mask, tls_weight(s, self.delta, self.mu), 1.0)

    def cost_terms(self, s):
        return np.where(self.mask, tls_rho(s, self.delta, self.mu), s)

    def scan(self):
        """(r2_max, n_fractional, n_rejected, sum rho, s) at the current state and the current mu"""
        s = self.edge_s()
        w = self.weights(s)
        r2_max = max(float(s[self.mask].max()), 0.0) if self.mask.any() else 0.0
        frac = int(np.sum(self.mask & (w > 0.0) & (w < 1.0)))
        rej = int(np.sum(self.mask & (w == 0.0)))
        return r2_max, frac, rej, float(np.sum(self.cost_terms(s))), s


def gnc(ref, mu_factor=1.4, max_stages=100, inner_iterations=1, final_iterations=20, lm=False):
    """rr_pgo_optimize_gnc on GncReference `ref` (its delta and mask).  Returns the result fields, stage_mu, stage_cost, and
    per stage the s of every edge at the stage's end (stage_s) for the tests of the band margins."""
    c2 = ref.delta * ref.delta
    ref.mu = 1.0
    r2_max, _, _, _, _ = ref.scan()                                            # 1.
    mu0 = c2 / (2.0 * r2_max - c2) if 2.0 * r2_max > c2 else 1.0               # 2.
    out = {"r2_max": r2_max, "mu0": mu0, "converged": 0, "final_iterations_run": 0}
    stage_mu, stage_cost, stage_s = [], [], []
    mu, t = mu0, 0
    while True:                                                                # 3.
        ref.mu = mu
        ref.optimize(inner_iterations, lm=lm)
        _, frac, rej, cost, s = ref.scan()
        stage_mu.append(mu)
        stage_cost.append(cost)
        stage_s.append(s)
        if frac == 0:
            out["converged"] = 1
            break
        if t + 1 == max_stages:
            break
        mu *= mu_factor
        t += 1
    if final_iterations > 0:                                                   # 4.
        errors, _ = ref.optimize(final_iterations, lm=lm)
        out["final_iterations_run"] = len(errors) - 1
        _, frac, rej, cost, s = ref.scan()
    out.update(n_stages=len(stage_mu), mu_last=mu, n_rejected=rej, n_fractional=frac, cost_last=cost,
               stage_mu=np.array(stage_mu), stage_cost=np.array(stage_cost), stage_s=stage_s)
    return out
