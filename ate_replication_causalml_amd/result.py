"""Estimator result record (the ``data.frame(Method, ATE, lower_ci, upper_ci)``
every reference estimator returns, e.g. ``ate_functions.R:20,38,62``) plus an
explicit ``se`` and a diagnostics dict."""
from __future__ import annotations

import json
import math
from dataclasses import asdict, dataclass, field

Z = 1.96  # hard-coded in every reference estimator (ate_functions.R:17-18 etc.)


@dataclass
class AteResult:
    method: str
    ate: float
    se: float                      # NaN when the reference reports no SE (LASSO, Q4)
    lower_ci: float
    upper_ci: float
    diagnostics: dict = field(default_factory=dict)

    @classmethod
    def make(cls, method, ate, se, **diag):
        ate = float(ate)
        if se is None or (isinstance(se, float) and math.isnan(se)):
            return cls(method, ate, float("nan"), ate, ate, diag)
        se = float(se)
        return cls(method, ate, se, ate - Z * se, ate + Z * se, diag)

    def row(self):
        return {"Method": self.method, "ATE": self.ate, "lower_ci": self.lower_ci,
                "upper_ci": self.upper_ci, "se": self.se}

    def to_json(self):
        d = asdict(self)
        d["diagnostics"] = {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v))
                            for k, v in d["diagnostics"].items()}
        return json.dumps(d)


def boot_rank(level: float, n_boot: int) -> int:
    """The order statistic that is the bootstrap critical value: the ceil(level * n_boot)-th
    smallest replicate (1-based; a product within 1e-9 of an integer counts as that integer,
    so 0.95 * 200 is 190 whatever its last bit)."""
    if not 0.0 < level < 1.0:
        raise ValueError(f"level must be in (0, 1), got {level}")
    return min(max(int(math.ceil(level * n_boot - 1e-9)), 1), int(n_boot))


@dataclass
class GateResult:
    """Group average treatment effects with pointwise and simultaneous (multiplier
    bootstrap) confidence bounds; ``overall`` is the ATE over the grouped rows."""
    method: str
    labels: list                   # group labels, in the order of every per-group list
    n: list                        # rows per group
    ate: list
    se: list
    lower_ci: list                 # pointwise: ate -/+ Z se
    upper_ci: list
    lower_joint: list              # simultaneous over the groups: ate -/+ crit se
    upper_joint: list
    crit: float
    n_boot: int
    level: float
    overall: AteResult
    diagnostics: dict = field(default_factory=dict)
    boot: dict | None = None       # keep_boot: the raw replicate sums "A", "Z" [n_boot, G]

    @classmethod
    def make(cls, method, labels, n, ate, se, crit, n_boot, level, overall, **diag):
        ate = [float(v) for v in ate]
        se = [float(v) for v in se]
        crit = float(crit)
        labels = [v.item() if hasattr(v, "item") else v for v in labels]
        n = [int(round(float(v))) if math.isfinite(float(v)) else -1 for v in n]
        return cls(method, labels, n, ate, se,
                   [a - Z * s for a, s in zip(ate, se)], [a + Z * s for a, s in zip(ate, se)],
                   [a - crit * s for a, s in zip(ate, se)],
                   [a + crit * s for a, s in zip(ate, se)], crit, int(n_boot), float(level),
                   overall, diag)

    def rows(self):
        return [{"group": self.labels[g], "n": self.n[g], "ATE": self.ate[g], "se": self.se[g],
                 "lower_ci": self.lower_ci[g], "upper_ci": self.upper_ci[g],
                 "lower_joint": self.lower_joint[g], "upper_joint": self.upper_joint[g]}
                for g in range(len(self.labels))]

    def table(self) -> str:
        lines = [f"{self.method}: joint {self.level:.0%} band, crit {self.crit:.4f} "
                 f"({self.n_boot} multiplier draws)",
                 f"{'group':>12s} {'n':>9s} {'ATE':>9s} {'SE':>9s} {'lower_ci':>9s} "
                 f"{'upper_ci':>9s} {'lower_jt':>9s} {'upper_jt':>9s}"]
        for r in self.rows():
            lines.append(f"{str(r['group']):>12s} {r['n']:9d} {r['ATE']:9.4f} {r['se']:9.4f} "
                         f"{r['lower_ci']:9.4f} {r['upper_ci']:9.4f} {r['lower_joint']:9.4f} "
                         f"{r['upper_joint']:9.4f}")
        o = self.overall
        lines.append(f"{'all':>12s} {sum(self.n):9d} {o.ate:9.4f} {o.se:9.4f} "
                     f"{o.lower_ci:9.4f} {o.upper_ci:9.4f}")
        return "\n".join(lines)

    def to_json(self):
        keep = lambda d: {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v))
                          for k, v in d.items()}
        return json.dumps({"method": self.method, "groups": self.rows(), "crit": self.crit,
                           "n_boot": self.n_boot, "level": self.level,
                           "overall": json.loads(self.overall.to_json()),
                           "diagnostics": keep(self.diagnostics)}, default=str)


def bspline_row(x: float, knots, degree: int) -> list:
    """The B-spline basis values [df] at one point of a clamped knot vector, by the textbook
    recursive Cox-de Boor definition (0 / 0 := 0; spans half-open, the last one closed on
    the right) -- float64 on the host, an algorithm of its own beside the kernels'
    span-local recurrence."""
    t = [float(v) for v in knots]
    q = int(degree)
    d = len(t) - q - 1
    x = float(x)

    def b(j, k):
        if k == 0:
            if t[j] <= x < t[j + 1]:
                return 1.0
            # the last non-empty span is closed on the right
            return 1.0 if (x == t[-1] and t[j] < t[j + 1] == t[-1]) else 0.0
        out = 0.0
        if t[j + k] > t[j]:
            out += (x - t[j]) / (t[j + k] - t[j]) * b(j, k - 1)
        if t[j + k + 1] > t[j + 1]:
            out += (t[j + k + 1] - x) / (t[j + k + 1] - t[j + 1]) * b(j + 1, k - 1)
        return out

    return [b(j, q) for j in range(d)]


@dataclass
class CateResult:
    """The conditional average treatment effect along one covariate as a B-spline curve on
    ``grid``, with pointwise and uniform (multiplier bootstrap) confidence bounds; ``coef``
    and ``cov`` are the projection's coefficients and their HC0 covariance, ``overall`` the
    ATE over the same rows."""
    method: str
    grid: list
    cate: list
    se: list
    lower_ci: list                 # pointwise: cate -/+ Z se
    upper_ci: list
    lower_joint: list              # uniform over the grid: cate -/+ crit se
    upper_joint: list
    crit: float
    coef: list                     # beta [df]
    cov: list                      # Omega [df][df]
    knots: list                    # clamped knot vector [df + degree + 1]
    degree: int
    n_boot: int
    level: float
    overall: AteResult
    diagnostics: dict = field(default_factory=dict)
    boot: dict | None = None       # keep_boot: "T" [n_boot, df], "M", "meat" [df, df]

    @classmethod
    def make(cls, method, grid, cate, se, crit, coef, cov, knots, degree, n_boot, level, overall,
             **diag):
        grid = [float(v) for v in grid]
        cate = [float(v) for v in cate]
        se = [float(v) for v in se]
        crit = float(crit)
        return cls(method, grid, cate, se,
                   [a - Z * s for a, s in zip(cate, se)], [a + Z * s for a, s in zip(cate, se)],
                   [a - crit * s for a, s in zip(cate, se)],
                   [a + crit * s for a, s in zip(cate, se)], crit, [float(v) for v in coef],
                   [[float(v) for v in row] for row in cov], [float(v) for v in knots],
                   int(degree), int(n_boot), float(level), overall, diag)

    @property
    def df(self) -> int:
        return len(self.coef)

    def predict(self, x):
        """(cate, se) at new points inside [min x, max x], on the host (no GPU work)."""
        import numpy as np
        pts = np.asarray(x, dtype=np.float64).reshape(-1)
        if len(pts) and (pts.min() < self.knots[0] or pts.max() > self.knots[-1]):
            raise ValueError(f"points must lie inside [{self.knots[0]}, {self.knots[-1]}]")
        G = np.array([bspline_row(v, self.knots, self.degree) for v in pts]).reshape(len(pts), self.df)
        cov = np.asarray(self.cov)
        return G @ np.asarray(self.coef), np.sqrt(np.maximum(((G @ cov) * G).sum(axis=1), 0.0))

    def rows(self):
        return [{"x": self.grid[j], "CATE": self.cate[j], "se": self.se[j],
                 "lower_ci": self.lower_ci[j], "upper_ci": self.upper_ci[j],
                 "lower_joint": self.lower_joint[j], "upper_joint": self.upper_joint[j]}
                for j in range(len(self.grid))]

    def table(self) -> str:
        lines = [f"{self.method}: df {self.df}, degree {self.degree}, uniform {self.level:.0%} "
                 f"band, crit {self.crit:.4f} ({self.n_boot} multiplier draws)",
                 f"{'x':>12s} {'CATE':>9s} {'SE':>9s} {'lower_ci':>9s} {'upper_ci':>9s} "
                 f"{'lower_jt':>9s} {'upper_jt':>9s}"]
        for r in self.rows():
            lines.append(f"{r['x']:12.4f} {r['CATE']:9.4f} {r['se']:9.4f} {r['lower_ci']:9.4f} "
                         f"{r['upper_ci']:9.4f} {r['lower_joint']:9.4f} {r['upper_joint']:9.4f}")
        o = self.overall
        lines.append(f"{'all':>12s} {o.ate:9.4f} {o.se:9.4f} {o.lower_ci:9.4f} {o.upper_ci:9.4f}")
        return "\n".join(lines)

    def to_json(self):
        keep = lambda d: {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v))
                          for k, v in d.items()}
        return json.dumps({"method": self.method, "curve": self.rows(), "crit": self.crit,
                           "coef": self.coef, "cov": self.cov, "knots": self.knots,
                           "degree": self.degree, "n_boot": self.n_boot, "level": self.level,
                           "overall": json.loads(self.overall.to_json()),
                           "diagnostics": keep(self.diagnostics)}, default=str)


def _policy_values(row, names):
    """One evaluation set of a policy tree from its finalised row [20] (estimators/policy.py
    ``policy_finalize``): value, treat_all and advantage with SE and 1.96 SE bounds, the share
    treated, n and the leaf table of the structural leaves ``names`` ((slot, label) pairs)."""
    v = [float(x) for x in row]
    out = {}
    for k, name in enumerate(("value", "treat_all", "advantage")):
        a, s = v[2 * k], v[2 * k + 1]
        out.update({name: a, f"{name}_se": s, f"{name}_lower_ci": a - Z * s,
                    f"{name}_upper_ci": a + Z * s})
    out["share_treated"] = v[6]
    out["n"] = int(round(v[7])) if math.isfinite(v[7]) else -1
    out["leaves"] = [{"leaf": label, "n": int(round(v[8 + 3 * s])) if math.isfinite(v[8 + 3 * s]) else -1,
                      "action": act, "mean": v[9 + 3 * s], "se": v[10 + 3 * s]}
                     for s, label, act in names]
    return out


@dataclass
class PolicyTreeResult:
    """An exact policy tree of depth <= 2 on per-row scores r = psi - cost: whom to treat.
    ``nodes``: root, left and right child, each with the column of X it splits (``feature``,
    None for a leaf), the bin ``t`` and the ``threshold`` (rows with x < threshold go left).
    ``in_sample`` / ``held_out``: value = mean(pi r), treat_all = mean(r), advantage = value -
    treat_all, each with SE and bounds, the share treated and the leaf table (n, action, mean
    r, SE). The in-sample values are optimistic: the tree was chosen on those rows."""
    method: str
    nodes: list
    actions: list                  # leaf actions LL, LR, RL, RR (a leaf node repeats its own)
    in_sample: dict
    held_out: dict | None
    value_q: int                   # the training value in fixed-point units (S q of treated leaves)
    n_train: int
    features: list                 # columns of X, the index space of nodes[.]["feature"]
    edges: list                    # per feature: the ascending split points
    cost: float
    depth: int
    diagnostics: dict = field(default_factory=dict)

    @classmethod
    def make(cls, method, rec, fin, features, edges, cost, depth, held_out=False, **diag):
        rec = [int(v) for v in rec]
        edges = [[float(v) for v in ed] for ed in edges]
        nan = not math.isfinite(float(fin[0][0]))
        if nan:                    # a NaN fit never yields a tree that looks learned (the
            rec = [-1] * 6 + [0] * 4 + [0, rec[11]]     # device path masks its record too)
        nodes = []
        for k, name in enumerate(("root", "left", "right")):
            j, t = rec[2 * k], rec[2 * k + 1]
            nodes.append({"node": name, "feature": features[j] if j >= 0 else None,
                          "bin": t if j >= 0 else None,
                          "threshold": edges[j][t] if j >= 0 else None})
        acts = rec[6:10]
        if rec[0] < 0:
            names = [(0, "root", acts[0])]
        else:
            names = []
            for side, tag in ((0, "L"), (1, "R")):
                if rec[2 + 2 * side] < 0:
                    names.append((2 * side, tag, acts[2 * side]))
                else:
                    names += [(2 * side, tag + "L", acts[2 * side]),
                              (2 * side + 1, tag + "R", acts[2 * side + 1])]
        diag = {"honest": bool(held_out), "nan": nan, **diag}
        return cls(method, nodes, acts, _policy_values(fin[0], names),
                   _policy_values(fin[1], names) if held_out else None, rec[10], rec[11],
                   [int(f) for f in features], edges, float(cost), int(depth), diag)

    @property
    def value(self) -> float:
        """The held-out value when there is a held-out set, else the (optimistic) in-sample one."""
        return (self.held_out or self.in_sample)["value"]

    def predict(self, X):
        """The 0/1 action of every row of X (columns as in the fitted X), on the host."""
        import numpy as np
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] <= max(self.features):
            raise ValueError(f"X must be a matrix with more than {max(self.features)} columns")
        root, acts = self.nodes[0], np.asarray(self.actions, dtype=np.int64)
        if root["feature"] is None:
            return np.full(len(X), acts[0], dtype=np.int64)
        right = X[:, root["feature"]] >= root["threshold"]
        down = np.zeros(len(X), dtype=bool)
        for side in (0, 1):
            ch = self.nodes[1 + side]
            if ch["feature"] is not None:
                down |= (right == bool(side)) & (X[:, ch["feature"]] >= ch["threshold"])
        return acts[2 * right.astype(np.int64) + down.astype(np.int64)]

    def table(self) -> str:
        lines = [f"{self.method}: depth {self.depth}, cost {self.cost:g}, "
                 f"{self.n_train} training rows"]
        for nd in self.nodes:
            lines.append(f"{nd['node']:>6s}: " + ("leaf" if nd["feature"] is None else
                                                  f"x{nd['feature']} < {nd['threshold']:.6g}"))
        for name, ev in (("in-sample (optimistic)", self.in_sample), ("held-out", self.held_out)):
            if ev is None:
                continue
            lines.append(f"{name}: n {ev['n']}, share treated {ev['share_treated']:.4f}")
            for k in ("value", "treat_all", "advantage"):
                lines.append(f"{k:>12s} {ev[k]:9.4f} {ev[k + '_se']:9.4f} "
                             f"{ev[k + '_lower_ci']:9.4f} {ev[k + '_upper_ci']:9.4f}")
            lines.append(f"{'leaf':>12s} {'n':>9s} {'action':>6s} {'mean':>9s} {'SE':>9s}")
            for lf in ev["leaves"]:
                lines.append(f"{lf['leaf']:>12s} {lf['n']:9d} {lf['action']:6d} {lf['mean']:9.4f} "
                             f"{lf['se']:9.4f}")
        return "\n".join(lines)

    def to_json(self):
        keep = lambda d: {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v))
                          for k, v in d.items()}
        return json.dumps({"method": self.method, "nodes": self.nodes, "actions": self.actions,
                           "in_sample": self.in_sample, "held_out": self.held_out,
                           "value_q": self.value_q, "n_train": self.n_train,
                           "features": self.features, "edges": self.edges, "cost": self.cost,
                           "depth": self.depth, "diagnostics": keep(self.diagnostics)},
                          default=str)


# ------------------------------------------------------------ sensitivity to confounding
# the 14 moments of the sensitivity pass (estimators/sensitivity.py, csrc/irm.hip), with
# b = (y - g_w)^2, rr = w / e - (1 - w) / (1 - e), c = 2 (1 / e + 1 / (1 - e)) - rr^2
SENS_MOMENTS = ("S psi", "S psi^2", "n", "n_clipped", "S b", "S b^2", "S c", "S c^2", "S psi b",
                "S psi c", "S b c", "S y", "S y^2", "n_treated")
N_BENCHMARKS_MAX = 8


def check_scenario(cf_y, cf_d, rho=1.0, level=0.95):
    """A confounding scenario: 0 <= cf_y < 1, 0 <= cf_d < 1, |rho| <= 1, 0.5 < level < 1."""
    if not 0.0 <= cf_y < 1.0:
        raise ValueError(f"cf_y must be in [0, 1), got {cf_y}")
    if not 0.0 <= cf_d < 1.0:
        raise ValueError(f"cf_d must be in [0, 1), got {cf_d}")
    if not abs(rho) <= 1.0:
        raise ValueError(f"rho must be in [-1, 1], got {rho}")
    if not 0.5 < level < 1.0:
        raise ValueError(f"level must be in (0.5, 1), got {level}")


def check_benchmarks(benchmarks, p: int):
    """Benchmark covariate sets as a tuple of tuples of column indices into X: at most 8
    sets, each of distinct indices in [0, p) and not all of X. A flat list of integers is
    one set."""
    if benchmarks is None:
        return ()
    sets = list(benchmarks)
    if sets and all(isinstance(c, (int,)) or (hasattr(c, "ndim") and c.ndim == 0) for c in sets):
        sets = [sets]
    if len(sets) > N_BENCHMARKS_MAX:
        raise ValueError(f"at most {N_BENCHMARKS_MAX} benchmark sets per call, got {len(sets)}")
    out = []
    for cols in sets:
        cols = [c for c in cols]
        if any(int(c) != c for c in cols):
            raise ValueError(f"benchmark columns must be integers, got {cols}")
        cols = tuple(int(c) for c in cols)
        if not cols:
            raise ValueError("an empty benchmark set")
        if any(not 0 <= c < p for c in cols):
            raise ValueError(f"benchmark columns must index the {p} columns of X, got {cols}")
        if len(set(cols)) != len(cols):
            raise ValueError(f"benchmark columns must be distinct, got {cols}")
        if len(cols) == p:
            raise ValueError("a benchmark set must leave at least one column of X in the model")
        out.append(cols)
    return tuple(out)


def cf_of_strength(a: float) -> float:
    """The cf = cf_y = cf_d with cf / sqrt(1 - cf) = a >= 0:
    (-a^2 + sqrt(a^4 + 4 a^2)) / 2, in the form without cancellation."""
    if not a > 0.0:
        return 0.0 if a == 0.0 else float("nan")
    if math.isinf(a):
        return 1.0
    return 2.0 / (1.0 + math.sqrt(1.0 + 4.0 / (a * a)))


def normal_quantile(level: float) -> float:
    from statistics import NormalDist
    return NormalDist().inv_cdf(level)


@dataclass
class SensBounds:
    """One confounding scenario: the bounds on theta and their one-sided ``level`` CI."""
    cf_y: float
    cf_d: float
    rho: float
    level: float
    theta_lower: float
    theta_upper: float
    se_lower: float
    se_upper: float
    ci_lower: float
    ci_upper: float


@dataclass
class SensBenchmark:
    """What leaving the covariate set ``columns`` out of the model does: the gains in
    explanatory power of the outcome regression (cf_y) and of the Riesz representer (cf_d)
    that these columns bring, raw and clipped to [0, 1], and the implied rho."""
    columns: tuple
    cf_y: float
    cf_d: float
    rho: float
    delta_theta: float
    cf_y_raw: float
    cf_d_raw: float
    theta_short: float
    sigma2_short: float
    nu2_short: float


def sens_plugins(mom):
    """(n, theta, sigma2, nu2, V11, V12, V22) from the 14 moments, float64 on the host.
    V11 = var(psi), V22 = var(pmb), V12 = cov(psi, pmb) with
    pmb = (sigma2 (c - nu2) + nu2 (b - sigma2)) / (2 S), S = sqrt(sigma2 nu2): linear in
    (b, c), so all three come from the 3x3 covariance of (psi, b, c); the n - 1, centred
    convention and the operation order of ``estimators.irm.irm_finalize``."""
    m = [float(v) for v in mom]
    if len(m) != len(SENS_MOMENTS):
        raise ValueError(f"{len(SENS_MOMENTS)} moments expected, got {len(m)}")
    n = m[2]
    theta, sigma2, nu2 = m[0] / n, m[4] / n, m[6] / n
    if not (sigma2 > 0.0 and nu2 > 0.0):
        from .utils.guards import NumericalError
        raise NumericalError(f"sensitivity analysis needs sigma2 > 0 and nu2 > 0, got "
                             f"sigma2 = {sigma2}, nu2 = {nu2}")

    def cov(suv, su, sv):
        return (suv - su * sv / n) / (n - 1)

    v11 = max(cov(m[1], m[0], m[0]), 0.0)
    vb, vc, cbc = max(cov(m[5], m[4], m[4]), 0.0), max(cov(m[7], m[6], m[6]), 0.0), \
        cov(m[10], m[4], m[6])
    cpb, cpc = cov(m[8], m[0], m[4]), cov(m[9], m[0], m[6])
    s = math.sqrt(sigma2 * nu2)
    ab, ac = nu2 / (2.0 * s), sigma2 / (2.0 * s)
    v22 = max(ab * ab * vb + ac * ac * vc + 2.0 * ab * ac * cbc, 0.0)
    v12 = ab * cpb + ac * cpc
    return n, theta, sigma2, nu2, v11, v12, v22


def sens_bounds(mom, cf_y, cf_d, rho=1.0, level=0.95) -> SensBounds:
    check_scenario(cf_y, cf_d, rho, level)
    n, theta, sigma2, nu2, v11, v12, v22 = sens_plugins(mom)
    s = math.sqrt(sigma2 * nu2)
    k = abs(rho) * math.sqrt(cf_y) * math.sqrt(cf_d / (1.0 - cf_d))
    z = normal_quantile(level)
    lo, hi = theta - s * k, theta + s * k
    se_lo = math.sqrt(max(v11 - 2.0 * k * v12 + k * k * v22, 0.0) / n)
    se_hi = math.sqrt(max(v11 + 2.0 * k * v12 + k * k * v22, 0.0) / n)
    return SensBounds(float(cf_y), float(cf_d), float(rho), float(level), lo, hi, se_lo, se_hi,
                      lo - z * se_lo, hi + z * se_hi)


def sens_robustness(mom, rho=1.0, level=0.95, null=0.0):
    """(RV, RVa): the cf = cf_y = cf_d at which the bound on the side of ``null`` (RVa: its
    confidence bound) reaches it. RVa is 0 when the CI at strength 0 covers the null."""
    check_scenario(0.0, 0.0, rho, level)
    n, theta, sigma2, nu2, v11, v12, v22 = sens_plugins(mom)
    s = math.sqrt(sigma2 * nu2)
    d = abs(theta - null)
    r = abs(rho)
    rv = cf_of_strength(d / (r * s)) if r > 0 else (1.0 if d > 0 else 0.0)
    z = normal_quantile(level)
    sgn = 1.0 if theta >= null else -1.0       # lower bound above, upper bound below the null
    if d - z * math.sqrt(v11 / n) <= 0.0:
        return rv, 0.0
    # the smallest k in [0, D / S] with D - S k = z se(k), se(k)^2 = (V11 - 2 sgn k V12 +
    # k^2 V22) / n: squared, A k^2 + B k + C = 0 with C > 0 here. D - S k - z se(k) is
    # concave in k, positive at 0 and <= 0 at D / S: one root in the interval
    zz = z * z / n
    A = s * s - zz * v22
    B = -2.0 * d * s + 2.0 * sgn * zz * v12
    C = d * d - zz * v11
    kmax = d / s
    roots = []
    if A == 0.0:
        if B != 0.0:
            roots.append(-C / B)
    else:
        disc = B * B - 4.0 * A * C
        if disc >= 0.0:
            q = -0.5 * (B + math.copysign(math.sqrt(disc), B))
            roots += [q / A] + ([C / q] if q != 0.0 else [])
    roots = [k for k in roots if 0.0 <= k <= kmax * (1.0 + 1e-12)]
    if roots:
        k = min(roots)
    else:                                      # bisection on the unsquared equation
        f = lambda k: d - s * k - z * math.sqrt(max(v11 - 2.0 * sgn * k * v12 + k * k * v22,
                                                    0.0) / n)
        a, b = 0.0, kmax
        for _ in range(200):
            k = 0.5 * (a + b)
            a, b = (k, b) if f(k) > 0.0 else (a, k)
        k = 0.5 * (a + b)
    rva = cf_of_strength(k / r) if r > 0 else 1.0
    return rv, rva


def sens_benchmark(columns, mom_long, mom_short) -> SensBenchmark:
    nl, th_l, s2_l, nu_l = sens_plugins(mom_long)[:4]
    ns, th_s, s2_s, nu_s = sens_plugins(mom_short)[:4]
    ml = [float(v) for v in mom_long]
    var_y = ml[12] / nl - (ml[11] / nl) ** 2
    r2_long, r2_short = 1.0 - s2_l / var_y, 1.0 - s2_s / var_y
    cf_y_raw = (r2_long - r2_short) / (1.0 - r2_long)
    cf_d_raw = (nu_l - nu_s) / nu_s
    delta = th_s - th_l
    var_g, var_riesz = s2_s - s2_l, nu_l - nu_s
    if var_g > 0.0 and var_riesz > 0.0:
        rho = math.copysign(min(abs(delta) / math.sqrt(var_g * var_riesz), 1.0), delta) \
            if delta != 0.0 else 0.0
    else:
        rho = float("nan")
    clip01 = lambda v: min(max(v, 0.0), 1.0)
    return SensBenchmark(tuple(int(c) for c in columns), clip01(cf_y_raw), clip01(cf_d_raw), rho,
                         delta, cf_y_raw, cf_d_raw, th_s, s2_s, nu_s)


@dataclass
class SensitivityResult:
    """Sensitivity of the cross-fitted IRM's ATE to unobserved confounding (Chernozhukov,
    Cinelli, Newey, Sharma & Syrgkanis 2022; DoubleML ``sensitivity_analysis`` /
    ``sensitivity_benchmark``): the bounds of the default scenario, the robustness values
    and the covariate benchmarks. Everything is a function of ``moments`` (SENS_MOMENTS), so
    ``bounds()`` evaluates any further scenario on the host."""
    method: str
    moments: list
    theta: float
    se: float
    sigma2: float
    nu2: float
    scenario: SensBounds           # the call's (cf_y, cf_d, rho, level)
    null: float
    rv: float
    rva: float
    benchmarks: list = field(default_factory=list)    # SensBenchmark per covariate set
    diagnostics: dict = field(default_factory=dict)

    @classmethod
    def from_moments(cls, method, moments, cf_y=0.03, cf_d=0.03, rho=1.0, level=0.95, null=0.0,
                     short=(), **diag):
        """``short``: (columns, moments of the model without them) per benchmark set."""
        mom = [float(v) for v in moments]
        n, theta, sigma2, nu2, v11 = sens_plugins(mom)[:5]
        rv, rva = sens_robustness(mom, rho, level, null)
        return cls(method, mom, theta, math.sqrt(v11 / n), sigma2, nu2,
                   sens_bounds(mom, cf_y, cf_d, rho, level), float(null), rv, rva,
                   [sens_benchmark(cols, mom, ms) for cols, ms in short], diag)

    @property
    def ate(self):
        return self.theta

    def bounds(self, cf_y, cf_d, rho=1.0, level=0.95) -> SensBounds:
        """The bounds and their CI under another scenario (no GPU work)."""
        return sens_bounds(self.moments, cf_y, cf_d, rho, level)

    def table(self) -> str:
        s = self.scenario
        lines = [f"{self.method}: theta {self.theta:.4f}, SE {self.se:.4f}, sigma2 "
                 f"{self.sigma2:.4f}, nu2 {self.nu2:.4f}",
                 f"{'cf_y':>9s} {'cf_d':>9s} {'rho':>9s} {'ci_lower':>9s} {'th_lower':>9s} "
                 f"{'theta':>9s} {'th_upper':>9s} {'ci_upper':>9s}",
                 f"{s.cf_y:9.4f} {s.cf_d:9.4f} {s.rho:9.4f} {s.ci_lower:9.4f} "
                 f"{s.theta_lower:9.4f} {self.theta:9.4f} {s.theta_upper:9.4f} {s.ci_upper:9.4f}",
                 f"robustness to null {self.null:g} at level {s.level:g}: RV {self.rv:.4%}, "
                 f"RVa {self.rva:.4%}"]
        if self.benchmarks:
            lines.append(f"{'benchmark':>20s} {'cf_y':>9s} {'cf_d':>9s} {'rho':>9s} "
                         f"{'d_theta':>9s} {'cf_y_raw':>10s} {'cf_d_raw':>10s}")
            for b in self.benchmarks:
                name = ",".join(str(c) for c in b.columns)
                name = name if len(name) <= 20 else name[:17] + "..."
                lines.append(f"{name:>20s} {b.cf_y:9.4f} {b.cf_d:9.4f} {b.rho:9.4f} "
                             f"{b.delta_theta:9.4f} {b.cf_y_raw:10.3e} {b.cf_d_raw:10.3e}")
        return "\n".join(lines)

    def to_json(self):
        keep = lambda d: {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v))
                          for k, v in d.items()}
        return json.dumps({"method": self.method, "theta": self.theta, "se": self.se,
                           "sigma2": self.sigma2, "nu2": self.nu2, "null": self.null,
                           "scenario": asdict(self.scenario), "rv": self.rv, "rva": self.rva,
                           "benchmarks": [asdict(b) for b in self.benchmarks],
                           "moments": self.moments, "diagnostics": keep(self.diagnostics)})


# ------------------------------------------------------------ target populations (ATE / ATT / ATC)
# the 12 moments of the target pass (estimators/targets.py, csrc/irm.hip), with e the clipped
# propensity, q1 = w (y - g1) / e, q0 = (1 - w)(y - g0) / (1 - e),
# a = w (y - g0) - e q0, c = -(1 - w)(y - g1) + (1 - e) q1 and psi = a + c
TARGET_MOMENTS = ("S psi", "S psi^2", "n", "n_clipped", "S a", "S a^2", "S a w", "S c", "S c^2",
                  "S c (1-w)", "S a c", "n_treated")
TARGETS = ("all", "treated", "control")      # the order of every per-target list and of cov


def check_targets(targets) -> tuple:
    """Target populations as a tuple of distinct names from ``TARGETS``, at least one. A
    single name is one target."""
    if isinstance(targets, str):
        targets = (targets,)
    try:
        out = tuple(targets)
    except TypeError:
        raise ValueError(f"targets must be a sequence of names from {TARGETS}") from None
    if not out:
        raise ValueError(f"at least one target of {TARGETS} is needed")
    for t in out:
        if t not in TARGETS:
            raise ValueError(f"unknown target {t!r}: pick from {TARGETS}")
    if len(set(out)) != len(out):
        raise ValueError(f"targets must be distinct, got {out}")
    return out


def target_estimates(mom):
    """(theta [3], cov [3][3]) in the order of ``TARGETS`` from the 12 moments, float64 on the
    host. With n1 = n_treated, n0 = n - n1, p1 = n1 / n, p0 = n0 / n:

        theta_all = S psi / n      theta_treated = S a / n1      theta_control = S c / n0
        phi_all = psi - theta_all
        phi_trt = (a - theta_treated w) / p1         (the ATTE score of DoubleML's IRM)
        phi_ctl = (c - theta_control (1 - w)) / p0
        cov[j][k] = S phi_j phi_k / (n - 1) / n      (the n - 1 rule of irm.mean_se)

    in closed form: S psi a = S a^2 + S a c, S psi c = S c^2 + S a c, S a (1 - w) = S a -
    S a w, S c w = S c - S c (1 - w), w (1 - w) = 0, and phi_trt and phi_ctl sum to 0.
    cov[0][0] has the operation order of ``estimators.irm.irm_finalize``."""
    m = [float(v) for v in mom]
    if len(m) != len(TARGET_MOMENTS):
        raise ValueError(f"{len(TARGET_MOMENTS)} moments expected, got {len(m)}")
    s_psi, s_psi2, n, _, s_a, s_a2, s_aw, s_c, s_c2, s_cv, s_ac, n1 = m
    nan = float("nan")
    n0 = n - n1
    if not (math.isfinite(n) and n > 1 and 0 < n1 < n):
        return [nan] * 3, [[nan] * 3 for _ in range(3)]
    p1, p0 = n1 / n, n0 / n
    th, t1, t0 = s_psi / n, s_a / n1, s_c / n0
    ss = [[0.0] * 3 for _ in range(3)]
    ss[0][0] = s_psi2 - s_psi * s_psi / n
    ss[1][1] = (s_a2 - 2.0 * t1 * s_aw + t1 * t1 * n1) / (p1 * p1)
    ss[2][2] = (s_c2 - 2.0 * t0 * s_cv + t0 * t0 * n0) / (p0 * p0)
    ss[0][1] = (s_a2 + s_ac - t1 * (s_aw + (s_c - s_cv))) / p1
    ss[0][2] = (s_c2 + s_ac - t0 * ((s_a - s_aw) + s_cv)) / p0
    ss[1][2] = (s_ac - t0 * (s_a - s_aw) - t1 * (s_c - s_cv)) / (p1 * p0)
    cov = [[0.0] * 3 for _ in range(3)]
    for j in range(3):
        for k in range(j, 3):
            v = ss[j][k] / (n - 1) / n
            cov[j][k] = cov[k][j] = max(v, 0.0) if j == k else v
    return [th, t1, t0], cov


@dataclass
class TargetContrast:
    """The difference ``a`` minus ``b`` of two target populations' effects, with its SE from
    the joint covariance, the 1.96 SE bounds and the two-sided normal p-value of no
    difference."""
    a: str
    b: str
    diff: float
    se: float
    lower_ci: float
    upper_ci: float
    p_value: float


@dataclass
class TargetResult:
    """The average effect of the cross-fitted interactive model over three target
    populations -- everyone ("all", the ATE), the treated ("treated", the ATT; DoubleML
    IRM(score="ATTE"), grf ``target.sample = "treated"``) and the controls ("control", the
    ATC) -- with their joint covariance. Everything is a function of ``moments``
    (TARGET_MOMENTS). A target that was not requested has NaN in its row and in its row and
    column of ``cov``: its nuisances were not fitted."""
    method: str
    moments: list
    targets: tuple                 # the requested targets, in the order of TARGETS
    estimates: dict                # target -> AteResult, all three keys
    cov: list                      # [3][3] in the order all, treated, control
    diagnostics: dict = field(default_factory=dict)

    @classmethod
    def from_moments(cls, method, mom, targets=TARGETS, **diag):
        mom = [float(v) for v in mom]
        return cls.from_estimates(method, *target_estimates(mom), targets, moments=mom, **diag)

    @classmethod
    def from_estimates(cls, method, theta, cov, targets=TARGETS, moments=(), **diag):
        """From (theta [3], cov [3][3]) in the order of TARGETS (the row-by-row reference)."""
        req = check_targets(targets)
        nan = float("nan")
        on = [t in req for t in TARGETS]
        theta = [float(v) if k else nan for v, k in zip(theta, on)]
        cov = [[float(cov[j][k]) if on[j] and on[k] else nan for k in range(3)] for j in range(3)]
        est = {}
        for j, t in enumerate(TARGETS):
            se = math.sqrt(cov[j][j]) if cov[j][j] >= 0.0 else nan
            est[t] = AteResult(f"{method}: {t}", theta[j], se, theta[j] - Z * se, theta[j] + Z * se)
        return cls(method, [float(v) for v in moments], tuple(t for t in TARGETS if t in req),
                   est, cov, diag)

    def __getitem__(self, target) -> AteResult:
        return self.estimates[target]

    def contrast(self, a="treated", b="control") -> TargetContrast:
        """The effect on ``a`` minus the effect on ``b`` (no GPU work): "does the effect on
        the treated differ from the effect on the controls?" is ``contrast().p_value``."""
        for t in (a, b):
            if t not in TARGETS:
                raise ValueError(f"unknown target {t!r}: pick from {TARGETS}")
        if a == b:
            raise ValueError("a contrast needs two different targets")
        j, k = TARGETS.index(a), TARGETS.index(b)
        d = self.estimates[a].ate - self.estimates[b].ate
        var = self.cov[j][j] + self.cov[k][k] - 2.0 * self.cov[j][k]
        se = math.sqrt(max(var, 0.0)) if var == var else float("nan")
        from statistics import NormalDist
        pv = 2.0 * (1.0 - NormalDist().cdf(abs(d) / se)) if se > 0.0 else float("nan")
        return TargetContrast(a, b, d, se, d - Z * se, d + Z * se, pv)

    def rows(self):
        return [{"target": t, "ATE": r.ate, "se": r.se, "lower_ci": r.lower_ci,
                 "upper_ci": r.upper_ci} for t, r in self.estimates.items()]

    def table(self) -> str:
        d = self.diagnostics
        lines = [f"{self.method}: n {d.get('n', '?')}, treated {d.get('n_treated', '?')}, "
                 f"clipped {d.get('n_clipped', '?')}",
                 f"{'target':>12s} {'effect':>9s} {'SE':>9s} {'lower_ci':>9s} {'upper_ci':>9s}"]
        for r in self.rows():
            lines.append(f"{r['target']:>12s} {r['ATE']:9.4f} {r['se']:9.4f} "
                         f"{r['lower_ci']:9.4f} {r['upper_ci']:9.4f}")
        if "treated" in self.targets and "control" in self.targets:
            c = self.contrast()
            lines.append(f"{'trt - ctl':>12s} {c.diff:9.4f} {c.se:9.4f} {c.lower_ci:9.4f} "
                         f"{c.upper_ci:9.4f}  p = {c.p_value:.4g}")
        return "\n".join(lines)

    def to_json(self):
        keep = lambda d: {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v))
                          for k, v in d.items()}
        return json.dumps({"method": self.method, "targets": list(self.targets),
                           "estimates": self.rows(), "cov": self.cov, "moments": self.moments,
                           "diagnostics": keep(self.diagnostics)})


# ------------------------------------------------------------ LATE (interactive IV model)
# the 15 moments of the LATE pass (estimators/late.py, csrc/iivm.hip), with e the clipped
# instrument propensity, b the AIPW score of Y and a the AIPW score of the treatment taken D,
# both split by the instrument z
LATE_MOMENTS = ("S b", "S b^2", "n", "n_clipped", "S a", "S a^2", "S a b", "S z", "S z d",
                "S (1-z) d", "S z (y-g1)^2", "S (1-z)(y-g0)^2", "S z (d-r1)^2",
                "S (1-z)(d-r0)^2", "S (z-m)^2")


def _mean_se(s1, s2, n):
    """(mean, SE) by the n - 1 rule, the host form of ``estimators.irm.mean_se``."""
    return s1 / n, math.sqrt(max((s2 - s1 * s1 / n) / (n - 1) / n, 0.0))


def late_estimates(mom):
    """(late, se, itt, itt_se, first_stage, first_stage_se, cov_itt_first_stage) from the 15
    moments, float64 on the host:

        theta = S b / S a
        SE^2  = [S b^2 - 2 theta S a b + theta^2 S a^2] / (n - 1) / n / (S a / n)^2

    (the influence values (b - theta a) / mean(a) sum to zero; the n - 1 rule of
    ``irm.mean_se``), the ITT ``mean_se(S b, S b^2, n)``, the first stage ``mean_se(S a,
    S a^2, n)`` and their covariance ``(S a b - S a S b / n) / (n - 1) / n``."""
    m = [float(v) for v in mom]
    if len(m) != len(LATE_MOMENTS):
        raise ValueError(f"{len(LATE_MOMENTS)} moments expected, got {len(m)}")
    sb, sbb, n, _, sa, saa, sab = m[:7]
    if not (math.isfinite(n) and n > 1 and all(math.isfinite(v) for v in m[:7])):
        return (float("nan"),) * 7
    itt, itt_se = _mean_se(sb, sbb, n)
    fs, fs_se = _mean_se(sa, saa, n)
    cov = (sab - sa * sb / n) / (n - 1) / n
    if sa == 0.0:
        return float("nan"), float("nan"), itt, itt_se, fs, fs_se, cov
    th = sb / sa
    var = (sbb - 2.0 * th * sab + th * th * saa) / (n - 1) / n / (sa / n) ** 2
    return th, math.sqrt(max(var, 0.0)), itt, itt_se, fs, fs_se, cov


@dataclass
class ArSet:
    """The Anderson-Rubin confidence set of the LATE. kind "interval": [lower, upper];
    "two_rays": (-inf, lower] and [upper, inf) (a weak first stage: one of the two may be
    infinite when the set is a single ray); "all": the whole line (lower = -inf, upper =
    inf)."""
    kind: str
    lower: float
    upper: float
    level: float

    def __contains__(self, theta) -> bool:
        if self.kind == "interval":
            return self.lower <= theta <= self.upper
        return self.kind == "all" or theta <= self.lower or theta >= self.upper


@dataclass
class LateResult:
    """The local average treatment effect of the cross-fitted interactive IV model (DoubleML
    ``DoubleMLIIVM``): the effect of the treatment taken on those whose take-up follows the
    binary instrument. ``late`` = ITT / first stage, where ``itt`` is the AIPW effect of the
    instrument on Y and ``first_stage`` its AIPW effect on the treatment taken (each an
    AteResult), with their 2x2 covariance ``cov`` (order itt, first stage). Everything is a
    function of ``moments`` (LATE_MOMENTS)."""
    method: str
    late: float
    se: float
    lower_ci: float
    upper_ci: float
    itt: AteResult
    first_stage: AteResult
    first_stage_t: float
    cov: list
    moments: list
    diagnostics: dict = field(default_factory=dict)

    @classmethod
    def from_moments(cls, method, mom, **diag):
        """From the 15 moments; the counts and held-out RMSEs of the diagnostics (n_clipped,
        n_z1, the four compliance cells n_z{z}_d{d}, rmse_g0 .. rmse_m) come from them too,
        ``diag`` adds n and hipgraph."""
        mom = [float(v) for v in mom]
        th, se, itt, itt_se, fs, fs_se, cov = late_estimates(mom)
        n, nz1 = mom[2], mom[7]
        nz0 = n - nz1
        cnt = lambda x: int(round(x)) if math.isfinite(x) else -1
        rm = lambda s, k: math.sqrt(s / k) if k > 0 and s >= 0 else float("nan")
        d = dict(n_clipped=cnt(mom[3]), n_z1=cnt(nz1), n_z0_d0=cnt(nz0 - mom[9]),
                 n_z0_d1=cnt(mom[9]), n_z1_d0=cnt(nz1 - mom[8]), n_z1_d1=cnt(mom[8]),
                 rmse_g0=rm(mom[11], nz0), rmse_g1=rm(mom[10], nz1), rmse_r0=rm(mom[13], nz0),
                 rmse_r1=rm(mom[12], nz1), rmse_m=rm(mom[14], n))
        d.update(diag)
        d.setdefault("n", cnt(n))
        return cls(method, th, se, th - Z * se, th + Z * se,
                   AteResult.make(f"{method}: ITT", itt, itt_se),
                   AteResult.make(f"{method}: first stage", fs, fs_se),
                   fs / fs_se if fs_se > 0 else float("nan"),
                   [[itt_se * itt_se, cov], [cov, fs_se * fs_se]], mom, d)

    def anderson_rubin(self, level=0.95) -> ArSet:
        """The weak-instrument-robust confidence set {theta : n mean(phi)^2 / var(phi) <=
        chi2_1(level)}, phi = b - theta a, var by the n - 1 rule. With k = chi2 / (n - 1) it
        is the quadratic inequality A theta^2 + B theta + C <= 0,

            A = (1 + k) (S a)^2 / n - k S a^2
            B = -2 (1 + k) S a S b / n + 2 k S a b
            C = (1 + k) (S b)^2 / n - k S b^2,

        solved in closed form on the host. A > 0 (a first stage away from zero at this
        level): an interval; A < 0: two rays, or the whole line when there is no real root.
        theta-hat = S b / S a has mean(phi) = 0 and is always inside."""
        if not 0.0 < level < 1.0:
            raise ValueError("level must be in (0, 1)")
        sb, sbb, n, _, sa, saa, sab = self.moments[:7]
        inf = float("inf")
        k = normal_quantile(0.5 + level / 2.0) ** 2 / (n - 1)
        A = (1 + k) * sa * sa / n - k * saa
        B = -2 * (1 + k) * sa * sb / n + 2 * k * sab
        C = (1 + k) * sb * sb / n - k * sbb
        if A == 0.0:                                    # B theta + C <= 0
            if B == 0.0:
                return ArSet("all", -inf, inf, level)
            return ArSet("two_rays", -C / B, inf, level) if B > 0 else \
                ArSet("two_rays", -inf, -C / B, level)
        disc = B * B - 4 * A * C
        if disc <= 0.0 and A < 0:
            return ArSet("all", -inf, inf, level)
        r = math.sqrt(max(disc, 0.0))
        # the root of larger magnitude without cancellation, the other from the product
        q = -0.5 * (B + math.copysign(r, B))
        roots = sorted((q / A, C / q)) if q != 0.0 else [0.0, 0.0]
        return ArSet("interval" if A > 0 else "two_rays", roots[0], roots[1], level)

    def table(self) -> str:
        d = self.diagnostics
        ar = self.anderson_rubin()
        row = lambda name, r: (f"{name:>12s} {r.ate:9.4f} {r.se:9.4f} {r.lower_ci:9.4f} "
                               f"{r.upper_ci:9.4f}")
        shape = {"interval": f"[{ar.lower:.4f}, {ar.upper:.4f}]", "all": "the whole line",
                 "two_rays": f"(-inf, {ar.lower:.4f}] and [{ar.upper:.4f}, inf)"}[ar.kind]
        return "\n".join([
            f"{self.method}: n {d.get('n', '?')}, Z=1 {d.get('n_z1', '?')}, clipped "
            f"{d.get('n_clipped', '?')}, cells (z,d) 00 {d.get('n_z0_d0', '?')} 01 "
            f"{d.get('n_z0_d1', '?')} 10 {d.get('n_z1_d0', '?')} 11 {d.get('n_z1_d1', '?')}",
            f"{'':>12s} {'effect':>9s} {'SE':>9s} {'lower_ci':>9s} {'upper_ci':>9s}",
            row("LATE", AteResult("", self.late, self.se, self.lower_ci, self.upper_ci)),
            row("ITT", self.itt), row("first stage", self.first_stage) +
            f"  t = {self.first_stage_t:.2f}",
            f"Anderson-Rubin 95% set: {shape}"])

    def json(self) -> str:
        keep = lambda d: {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v))
                          for k, v in d.items()}
        ar = self.anderson_rubin()
        est = lambda r: {"estimate": r.ate, "se": r.se, "lower_ci": r.lower_ci,
                         "upper_ci": r.upper_ci}
        return json.dumps({"method": self.method, "late": self.late, "se": self.se,
                           "lower_ci": self.lower_ci, "upper_ci": self.upper_ci,
                           "itt": est(self.itt), "first_stage": est(self.first_stage),
                           "first_stage_t": self.first_stage_t, "cov": self.cov,
                           "anderson_rubin": asdict(ar), "moments": self.moments,
                           "diagnostics": keep(self.diagnostics)})

    to_json = json


# ------------------------------------------------------------- RATE of a priority rule
@dataclass
class RateStat:
    """One rank-weighted average (AUTOC or QINI): estimate, half-sample bootstrap SE, normal
    interval at the result's level and the two-sided normal p-value of estimate = 0."""
    estimate: float
    se: float
    lower_ci: float
    upper_ci: float
    p_value: float

    @classmethod
    def make(cls, estimate, se, z):
        estimate, se = float(estimate), float(se)
        p = math.erfc(abs(estimate) / se / math.sqrt(2.0)) if se > 0 else float("nan")
        return cls(estimate, se, estimate - z * se, estimate + z * se, p)


@dataclass
class RateResult:
    """The rank-weighted average treatment effect of a treatment-priority rule
    (estimators/rate.py): AUTOC, the Qini coefficient and the TOC curve on the grid ``u``
    with pointwise (normal) and uniform (bootstrap maximum) ``level`` bounds. ``toc`` holds
    per-point lists: u, entered (rows treated at u, whole runs of ties), estimate, se,
    lower_ci, upper_ci, lower_joint, upper_joint."""
    method: str
    autoc: RateStat
    qini: RateStat
    toc: dict
    crit: float
    ate: float                     # the mean score over the evaluation rows
    n: int                         # evaluation rows
    n_runs: int                    # distinct priorities among them
    n_boot: int
    level: float
    diagnostics: dict = field(default_factory=dict)
    boot: object = None            # keep_boot: the raw [n_boot + 1, 5 + 2 Q] walk buffer

    @classmethod
    def make(cls, method, u, entered, fin, n, n_runs, n_boot, level, **diag):
        """``fin``: the flat vector of estimators.rate.rate_finalize."""
        fin = [float(x) for x in fin]
        Q = len(u)
        z = normal_quantile(0.5 + 0.5 * level)
        ate, a, sa, qn, sq, crit = fin[:6]
        est, se = fin[7:7 + Q], fin[7 + Q:7 + 2 * Q]
        toc = {"u": [float(x) for x in u], "entered": [int(x) for x in entered],
               "estimate": est, "se": se,
               "lower_ci": [e - z * s for e, s in zip(est, se)],
               "upper_ci": [e + z * s for e, s in zip(est, se)],
               "lower_joint": [e - crit * s for e, s in zip(est, se)],
               "upper_joint": [e + crit * s for e, s in zip(est, se)]}
        return cls(method, RateStat.make(a, sa, z), RateStat.make(qn, sq, z), toc, crit, ate,
                   int(n), int(n_runs), int(n_boot), float(level), diag)

    def rows(self):
        t = self.toc
        return [{k: t[k][j] for k in t} for j in range(len(t["u"]))]

    def table(self) -> str:
        lines = [f"{self.method}: n {self.n}, {self.n_runs} distinct priorities, ATE "
                 f"{self.ate:.4f}, {self.n_boot} half samples, {self.level:.0%} bounds, "
                 f"uniform crit {self.crit:.4f}",
                 f"{'':>8s} {'estimate':>9s} {'SE':>9s} {'lower_ci':>9s} {'upper_ci':>9s} "
                 f"{'p':>9s}"]
        for name, r in (("AUTOC", self.autoc), ("QINI", self.qini)):
            lines.append(f"{name:>8s} {r.estimate:9.4f} {r.se:9.4f} {r.lower_ci:9.4f} "
                         f"{r.upper_ci:9.4f} {r.p_value:9.4g}")
        lines.append(f"{'u':>8s} {'entered':>9s} {'TOC':>9s} {'SE':>9s} {'lower_ci':>9s} "
                     f"{'upper_ci':>9s} {'lower_un':>9s} {'upper_un':>9s}")
        for r in self.rows():
            lines.append(f"{r['u']:8.3f} {r['entered']:9d} {r['estimate']:9.4f} {r['se']:9.4f} "
                         f"{r['lower_ci']:9.4f} {r['upper_ci']:9.4f} {r['lower_joint']:9.4f} "
                         f"{r['upper_joint']:9.4f}")
        return "\n".join(lines)

    def json(self) -> str:
        keep = lambda d: {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v))
                          for k, v in d.items()}
        return json.dumps({"method": self.method, "autoc": asdict(self.autoc),
                           "qini": asdict(self.qini), "toc": self.rows(), "crit": self.crit,
                           "ate": self.ate, "n": self.n, "n_runs": self.n_runs,
                           "n_boot": self.n_boot, "level": self.level,
                           "diagnostics": keep(self.diagnostics)})

    to_json = json


# ------------------------------------------- potential outcomes of a multi-valued treatment
APO_MIN_LEVELS, APO_MAX_LEVELS = 2, 8
APO_LEVEL_MOMENTS = ("n_c", "n_clipped_c", "S 1{D=c}(y-g_c)^2", "S 1{D=c}/e_c")


@dataclass(frozen=True)
class ApoLayout:
    """Where the moments of the potential-outcome pass live for L levels (the host twin of
    csrc/apo.hip ``apo_n`` and its header): ``n`` at 0, ``S psi_c`` at ``psi + c``,
    ``S psi_c psi_c'`` (c <= c') at ``tri(c, c')``, and per level c the four sums of
    APO_LEVEL_MOMENTS at ``level + 4 c + q``. ``size``: 14 at L = 2, 77 at L = 8."""
    L: int

    def __post_init__(self):
        if not APO_MIN_LEVELS <= self.L <= APO_MAX_LEVELS:
            raise ValueError(f"the potential-outcome pass takes {APO_MIN_LEVELS} to "
                             f"{APO_MAX_LEVELS} treatment levels, got {self.L}")

    @property
    def psi(self) -> int:
        return 1

    @property
    def cross(self) -> int:
        return 1 + self.L

    @property
    def level(self) -> int:
        return 1 + self.L + self.L * (self.L + 1) // 2

    @property
    def size(self) -> int:
        return self.level + 4 * self.L

    def tri(self, c: int, c2: int) -> int:
        """The index of S psi_c psi_c2: row-major over the upper triangle."""
        c, c2 = (c, c2) if c <= c2 else (c2, c)
        return self.cross + c * self.L - c * (c - 1) // 2 + (c2 - c)

    def names(self) -> list:
        L = self.L
        return (["n"] + [f"S psi_{c}" for c in range(L)] +
                [f"S psi_{c} psi_{d}" for c in range(L) for d in range(c, L)] +
                [m for c in range(L) for m in (f"n_{c}", f"n_clipped_{c}",
                                               f"S 1{{D={c}}}(y-g_{c})^2", f"S 1{{D={c}}}/e_{c}")])


def apo_layout(L: int) -> ApoLayout:
    return ApoLayout(int(L))


def apo_levels_of(n_moments: int) -> int:
    """L from the length of a moment vector."""
    for L in range(APO_MIN_LEVELS, APO_MAX_LEVELS + 1):
        if ApoLayout(L).size == n_moments:
            return L
    raise ValueError(f"{n_moments} is not the moment count of any number of levels in "
                     f"{APO_MIN_LEVELS}..{APO_MAX_LEVELS}")


def apo_estimates(mom):
    """(theta [L], cov [L][L]) from the moments, float64 on the host: theta_c = S psi_c / n and
    cov_cc' = (S psi_c psi_c' - S psi_c S psi_c' / n) / (n - 1) / n, the n - 1 rule of
    ``irm.mean_se`` (its square on the diagonal)."""
    m = [float(v) for v in mom]
    lay = ApoLayout(apo_levels_of(len(m)))
    L, n = lay.L, m[0]
    nan = float("nan")
    head = m[:lay.level]
    if not (math.isfinite(n) and n > 1 and all(math.isfinite(v) for v in head)):
        return [nan] * L, [[nan] * L for _ in range(L)]
    s = m[lay.psi:lay.psi + L]
    cov = [[(m[lay.tri(c, d)] - s[c] * s[d] / n) / (n - 1) / n for d in range(L)] for c in range(L)]
    return [v / n for v in s], cov


def _chol_psd(A):
    """The lower Cholesky factor of a symmetric positive semidefinite matrix (lists), with a
    zero column where a pivot is not positive (a degenerate direction draws nothing)."""
    k = len(A)
    Lc = [[0.0] * k for _ in range(k)]
    for j in range(k):
        d = A[j][j] - sum(Lc[j][q] ** 2 for q in range(j))
        if not d > 1e-14 * max(abs(A[j][j]), 1e-300):
            continue
        Lc[j][j] = math.sqrt(d)
        for i in range(j + 1, k):
            Lc[i][j] = (A[i][j] - sum(Lc[i][q] * Lc[j][q] for q in range(j))) / Lc[j][j]
    return Lc


def _chi2_sf(x: float, df: int) -> float:
    """P(chi2_df > x): the regularised upper incomplete gamma function Q(df / 2, x / 2), by
    its series below a + 1 and its continued fraction above (Numerical Recipes 6.2)."""
    if not (x == x) or df < 1:
        return float("nan")
    if x <= 0.0:
        return 1.0
    a, x = df / 2.0, x / 2.0
    lg = math.lgamma(a)
    if x < a + 1.0:
        term = tot = 1.0 / a
        for k in range(1, 10000):
            term *= x / (a + k)
            tot += term
            if abs(term) < abs(tot) * 1e-16:
                break
        return max(0.0, 1.0 - tot * math.exp(-x + a * math.log(x) - lg))
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for k in range(1, 10000):
        an = -k * (k - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return h * math.exp(-x + a * math.log(x) - lg)


def contrast_cov(cov, r: int):
    """The covariance [L-1][L-1] of the contrasts theta_c - theta_r, c != r in ascending
    order: V_cd + V_rr - V_cr - V_dr."""
    idx = [c for c in range(len(cov)) if c != r]
    return [[cov[c][d] + cov[r][r] - cov[c][r] - cov[d][r] for d in idx] for c in idx]


def band_crit(ccov, seed: int, level: float = 0.95, n_boot: int = 999) -> float:
    """The critical value of a simultaneous ``level`` band over contrasts with covariance
    ``ccov``. The maximal |t| of a Gaussian multiplier bootstrap of the scores is, given the
    data, exactly max |N(0, R)| with R the contrasts' correlation matrix, so the value is the
    ``boot_rank(level, n_boot)``-th smallest of n_boot such maxima: draw b is ``chol(R) z_b``
    with z_b[j] the first Box-Muller normal of Philox (seed, P_BAND, stream j, index b). A pure
    function of (ccov, seed, level, n_boot). One contrast: the two-sided normal quantile, no
    draws. A contrast of zero variance takes no part."""
    rank = boot_rank(level, int(n_boot))
    k = len(ccov)
    if any(not (v == v) for row in ccov for v in row):
        return float("nan")
    if k <= 1:
        return normal_quantile(0.5 + level / 2.0)
    import numpy as np
    from .parallel import rng
    sd = [math.sqrt(ccov[j][j]) if ccov[j][j] > 0.0 else 0.0 for j in range(k)]
    R = [[ccov[i][j] / (sd[i] * sd[j]) if sd[i] > 0 and sd[j] > 0 else 0.0 for j in range(k)]
         for i in range(k)]
    A = np.asarray(_chol_psd(R), dtype=np.float64)
    b = np.arange(int(n_boot), dtype=np.uint64)
    z = np.stack([rng.normal_pair(int(seed), rng.P_BAND, j, b)[0] for j in range(k)])   # [k, B]
    tmax = np.abs(A @ z).max(axis=0)
    return float(np.sort(tmax)[rank - 1])


@dataclass
class ApoContrast:
    """theta_level - theta_reference with its SE from the joint covariance, the pointwise
    1.96 SE bounds and the simultaneous bounds over all contrasts against that reference."""
    level: object
    reference: object
    effect: float
    se: float
    lower_ci: float
    upper_ci: float
    lower_joint: float
    upper_joint: float


@dataclass
class WaldTest:
    stat: float
    df: int
    p_value: float


@dataclass
class ApoResult:
    """The mean potential outcomes of a multi-valued treatment under the cross-fitted
    interactive model (DoubleML ``DoubleMLAPOS``): ``apo[c]`` the mean outcome had everybody
    received level ``levels[c]``, ``cov`` their joint covariance, :meth:`contrasts` every
    level's effect against a reference with a simultaneous band (``crit``: its critical
    value for ``reference``), :meth:`wald` the test that all means are equal. Everything is
    a function of ``moments`` (:class:`ApoLayout`), ``seed`` and ``level``."""
    method: str
    levels: list                   # the original treatment values, ascending
    reference: object              # one of ``levels``
    apo: list                      # L AteResult
    cov: list                      # [L][L]
    moments: list
    crit: float
    n_boot: int
    level: float
    seed: int
    diagnostics: dict = field(default_factory=dict)
    scores: object = None          # keep_scores (the row-by-row reference): psi [n, L]

    @classmethod
    def from_moments(cls, method, mom, levels, reference=None, seed=1991, n_boot=999,
                     level=0.95, **diag):
        """From the moment vector; the per-level diagnostics (n_c, n_clipped_c, rmse_g_c,
        ipw_c = S 1{D=c}/e_c / n, near 1 for a calibrated propensity) come from it too,
        ``diag`` adds n and hipgraph."""
        mom = [float(v) for v in mom]
        levels = [v.item() if hasattr(v, "item") else v for v in levels]
        lay = ApoLayout(len(levels))
        if len(mom) != lay.size:
            raise ValueError(f"{lay.size} moments expected for {lay.L} levels, got {len(mom)}")
        reference = levels[0] if reference is None else reference
        if reference not in levels:
            raise ValueError(f"reference {reference!r} is not a treatment level: {levels}")
        reference = levels[levels.index(reference)]
        theta, cov = apo_estimates(mom)
        return cls._build(method, levels, reference, theta, cov, mom, seed, n_boot, level,
                          cls._level_diag(mom, lay), diag)

    @classmethod
    def from_scores(cls, method, psi, levels, reference=None, seed=1991, n_boot=999, level=0.95,
                    **diag):
        """From the per-row scores psi [n][L] (the row-by-row reference): the means and the
        covariance ``phi.T @ phi / (n - 1) / n`` of the centred scores."""
        import numpy as np
        psi = np.asarray(psi, dtype=np.float64)
        n = len(psi)
        levels = [v.item() if hasattr(v, "item") else v for v in levels]
        reference = levels[0] if reference is None else reference
        if reference not in levels:
            raise ValueError(f"reference {reference!r} is not a treatment level: {levels}")
        theta = psi.mean(0)
        phi = psi - theta
        cov = (phi.T @ phi / (n - 1) / n).tolist()
        return cls._build(method, levels, levels[levels.index(reference)], theta.tolist(), cov,
                          [], seed, n_boot, level, {}, diag)

    @classmethod
    def _build(cls, method, levels, reference, theta, cov, mom, seed, n_boot, level, ldiag, diag):
        nan = float("nan")
        apo = []
        for c, t in enumerate(theta):
            se = math.sqrt(cov[c][c]) if cov[c][c] >= 0.0 else nan
            apo.append(AteResult(f"{method}: Y({levels[c]})", t, se, t - Z * se, t + Z * se))
        crit = band_crit(contrast_cov(cov, levels.index(reference)), seed, level, n_boot)
        d = dict(ldiag)
        d.update(diag)
        if mom:
            d.setdefault("n", int(round(mom[0])) if math.isfinite(mom[0]) else -1)
        return cls(method, levels, reference, apo, cov, mom, crit, int(n_boot), float(level),
                   int(seed), d)

    @staticmethod
    def _level_diag(mom, lay):
        cnt = lambda x: int(round(x)) if math.isfinite(x) else -1
        n = mom[0]
        lv = [mom[lay.level + 4 * c:lay.level + 4 * c + 4] for c in range(lay.L)]
        return dict(n_c=[cnt(v[0]) for v in lv], n_clipped_c=[cnt(v[1]) for v in lv],
                    rmse_g_c=[math.sqrt(v[2] / v[0]) if v[0] > 0 and v[2] >= 0 else float("nan")
                              for v in lv],
                    ipw_c=[v[3] / n if n > 0 else float("nan") for v in lv])

    def __getitem__(self, lev) -> AteResult:
        return self.apo[self.levels.index(lev)]

    def contrasts(self, reference=None) -> list:
        """The L - 1 effects theta_c - theta_reference (ascending c; no GPU work), each with
        its pointwise and its simultaneous bounds. ``reference``: one of ``levels`` (default:
        the result's own); another reference draws its own band from the same seed."""
        ref = self.reference if reference is None else reference
        if ref not in self.levels:
            raise ValueError(f"reference {ref!r} is not a treatment level: {self.levels}")
        r = self.levels.index(ref)
        ccov = contrast_cov(self.cov, r)
        crit = self.crit if self.levels[r] == self.reference else \
            band_crit(ccov, self.seed, self.level, self.n_boot)
        out = []
        for j, c in enumerate(c for c in range(len(self.levels)) if c != r):
            d = self.apo[c].ate - self.apo[r].ate
            var = ccov[j][j]
            se = math.sqrt(max(var, 0.0)) if var == var else float("nan")
            out.append(ApoContrast(self.levels[c], self.levels[r], d, se, d - Z * se, d + Z * se,
                                   d - crit * se, d + crit * se))
        return out

    def wald(self) -> WaldTest:
        """The chi-square test of "all L means are equal": delta' V^-1 delta over the L - 1
        contrasts against the reference (the statistic does not depend on which), with L - 1
        degrees of freedom. NaN when the contrasts' covariance is singular."""
        r = self.levels.index(self.reference)
        ccov = contrast_cov(self.cov, r)
        k = len(ccov)
        delta = [self.apo[c].ate - self.apo[r].ate for c in range(len(self.levels)) if c != r]
        nan = float("nan")
        if any(not (v == v) for row in ccov for v in row):
            return WaldTest(nan, k, nan)
        Lc = _chol_psd(ccov)
        if any(Lc[j][j] <= 0.0 for j in range(k)):
            return WaldTest(nan, k, nan)
        u = []
        for i in range(k):                              # forward solve L u = delta
            u.append((delta[i] - sum(Lc[i][q] * u[q] for q in range(i))) / Lc[i][i])
        stat = sum(v * v for v in u)
        return WaldTest(stat, k, _chi2_sf(stat, k))

    def rows(self):
        d = self.diagnostics
        get = lambda k, c: d[k][c] if k in d else None
        return [{"level": self.levels[c], "apo": r.ate, "se": r.se, "lower_ci": r.lower_ci,
                 "upper_ci": r.upper_ci, "n_c": get("n_c", c), "n_clipped_c": get("n_clipped_c", c),
                 "rmse_g_c": get("rmse_g_c", c), "ipw_c": get("ipw_c", c)}
                for c, r in enumerate(self.apo)]

    def table(self) -> str:
        d = self.diagnostics
        w = self.wald()
        lines = [f"{self.method}: n {d.get('n', '?')}, {len(self.levels)} levels, joint "
                 f"{self.level:.0%} band over the contrasts, crit {self.crit:.4f} "
                 f"({self.n_boot} draws)",
                 f"{'level':>12s} {'n_c':>8s} {'clipped':>8s} {'E[Y(c)]':>9s} {'SE':>9s} "
                 f"{'lower_ci':>9s} {'upper_ci':>9s} {'rmse_g':>8s} {'ipw/n':>7s}"]
        num = lambda v, f: format(v, f) if isinstance(v, (int, float)) else "?"
        for r in self.rows():
            lines.append(f"{str(r['level']):>12s} {num(r['n_c'], '8d')} "
                         f"{num(r['n_clipped_c'], '8d')} {r['apo']:9.4f} {r['se']:9.4f} "
                         f"{r['lower_ci']:9.4f} {r['upper_ci']:9.4f} {num(r['rmse_g_c'], '8.4f')} "
                         f"{num(r['ipw_c'], '7.3f')}")
        lines.append(f"{'contrast':>12s} {'effect':>9s} {'SE':>9s} {'lower_ci':>9s} "
                     f"{'upper_ci':>9s} {'lower_jt':>9s} {'upper_jt':>9s}")
        for c in self.contrasts():
            lines.append(f"{str(c.level) + ' - ' + str(c.reference):>12s} {c.effect:9.4f} "
                         f"{c.se:9.4f} {c.lower_ci:9.4f} {c.upper_ci:9.4f} {c.lower_joint:9.4f} "
                         f"{c.upper_joint:9.4f}")
        lines.append(f"all means equal: chi2({w.df}) = {w.stat:.3f}, p = {w.p_value:.4g}")
        return "\n".join(lines)

    def json(self) -> str:
        keep = lambda d: {k: (v if isinstance(v, (int, float, str, bool, list, type(None)))
                              else str(v)) for k, v in d.items()}
        return json.dumps({"method": self.method, "levels": self.levels,
                           "reference": self.reference, "apo": self.rows(), "cov": self.cov,
                           "contrasts": [asdict(c) for c in self.contrasts()],
                           "crit": self.crit, "n_boot": self.n_boot, "level": self.level,
                           "seed": self.seed, "wald": asdict(self.wald()),
                           "moments": self.moments, "diagnostics": keep(self.diagnostics)},
                          default=str)

    to_json = json


# ------------------------------------------------- partially linear IV model (DML-PLIV)
PLIV_MAX_INSTRUMENTS = 4
PLIV_RANK_TOL = 1e-12   # a Cholesky pivot of S z~z~' at or below this times its largest diagonal


@dataclass(frozen=True)
class PlivLayout:
    """Where the moments of the PLIV pass live for q instruments (the host twin of
    csrc/pliv.hip ``pliv_n`` and its header), with y~, d~, z~ the held-out residuals and
    T = q (q + 1) / 2: ``n`` at 0, S y~y~, S y~d~, S d~d~ at 1..3, S z~_i y~ at ``zy + i``,
    S z~_i d~ at ``zd + i``, S z~_i z~_j (i <= j) at ``zz + tri(i, j)`` and the fourth moments
    Q_yy, Q_yd, Q_dd = S z~_i z~_j {y~y~, y~d~, d~d~} at ``qyy`` / ``qyd`` / ``qdd + tri(i, j)``.
    ``size``: 10 / 20 / 34 / 52 for q = 1..4."""
    q: int

    def __post_init__(self):
        if not 1 <= self.q <= PLIV_MAX_INSTRUMENTS:
            raise ValueError(f"DML-PLIV takes 1 to {PLIV_MAX_INSTRUMENTS} instruments, got "
                             f"{self.q}")

    @property
    def T(self) -> int:
        return self.q * (self.q + 1) // 2

    @property
    def zy(self) -> int:
        return 4

    @property
    def zd(self) -> int:
        return 4 + self.q

    @property
    def zz(self) -> int:
        return 4 + 2 * self.q

    @property
    def qyy(self) -> int:
        return self.zz + self.T

    @property
    def qyd(self) -> int:
        return self.zz + 2 * self.T

    @property
    def qdd(self) -> int:
        return self.zz + 3 * self.T

    @property
    def size(self) -> int:
        return self.zz + 4 * self.T

    def tri(self, i: int, j: int) -> int:
        """The offset of entry (i, j): row-major over the upper triangle."""
        i, j = (i, j) if i <= j else (j, i)
        return i * self.q - i * (i - 1) // 2 + (j - i)

    def names(self) -> list:
        q = self.q
        pairs = [(i, j) for i in range(q) for j in range(i, q)]
        return (["n", "S yy", "S yd", "S dd"] + [f"S z{i} y" for i in range(q)] +
                [f"S z{i} d" for i in range(q)] + [f"S z{i} z{j}" for i, j in pairs] +
                [f"S z{i} z{j} {t}" for t in ("yy", "yd", "dd") for i, j in pairs])

    def pack(self, n, syy, syd, sdd, szy, szd, szz, qyy, qyd, qdd) -> list:
        """The moment vector from its parts (szz, qyy, qyd, qdd: q x q symmetric)."""
        q = self.q
        pairs = [(i, j) for i in range(q) for j in range(i, q)]
        return ([float(n), float(syy), float(syd), float(sdd)] + [float(v) for v in szy] +
                [float(v) for v in szd] +
                [float(M[i][j]) for M in (szz, qyy, qyd, qdd) for i, j in pairs])

    def unpack(self, mom) -> dict:
        """The parts of a moment vector: n, syy, syd, sdd, szy [q], szd [q] and the full
        symmetric q x q lists szz, qyy, qyd, qdd."""
        m = [float(v) for v in mom]
        if len(m) != self.size:
            raise ValueError(f"{self.size} moments expected at q = {self.q}, got {len(m)}")
        q = self.q
        sym = lambda o: [[m[o + self.tri(i, j)] for j in range(q)] for i in range(q)]
        return dict(n=m[0], syy=m[1], syd=m[2], sdd=m[3], szy=m[self.zy:self.zy + q],
                    szd=m[self.zd:self.zd + q], szz=sym(self.zz), qyy=sym(self.qyy),
                    qyd=sym(self.qyd), qdd=sym(self.qdd))


def pliv_layout(q: int) -> PlivLayout:
    return PlivLayout(int(q))


def pliv_instruments_of(n_moments: int) -> int:
    """q from the length of a moment vector."""
    for q in range(1, PLIV_MAX_INSTRUMENTS + 1):
        if PlivLayout(q).size == n_moments:
            return q
    raise ValueError(f"{n_moments} is not the moment count of any number of instruments in "
                     f"1..{PLIV_MAX_INSTRUMENTS}")


def _chol_solve_small(A, b, tol=0.0):
    """x with A x = b for a small symmetric positive definite A (lists) by Cholesky, in the
    operation order of csrc/pliv.hip ``pliv_finish_kernel``; None when a pivot is at or below
    ``tol`` times the largest diagonal entry."""
    k = len(A)
    dmax = max([0.0] + [A[i][i] for i in range(k)])
    if not dmax > 0.0:
        return None
    L = [[0.0] * k for _ in range(k)]
    for j in range(k):
        d = A[j][j]
        for c in range(j):
            d -= L[j][c] * L[j][c]
        if not d > tol * dmax:
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, k):
            t = A[i][j]
            for c in range(j):
                t -= L[i][c] * L[j][c]
            L[i][j] = t / L[j][j]
    f = [0.0] * k
    for i in range(k):
        t = b[i]
        for c in range(i):
            t -= L[i][c] * f[c]
        f[i] = t / L[i][i]
    x = [0.0] * k
    for i in range(k - 1, -1, -1):
        t = f[i]
        for c in range(i + 1, k):
            t -= L[c][i] * x[c]
        x[i] = t / L[i][i]
    return x


def pliv_finish(mom) -> list:
    """[theta, SE, pi' S z~d~, rank flag, pi_1..pi_q] from the PLIV moments, float64 on the
    host: the twin of the in-kernel finish of csrc/pliv.hip, operation by operation.

        pi    = (S z~z~')^-1 S z~d~                 (Cholesky; no intercept)
        theta = pi' S z~y~ / pi' S z~d~
        Omega = Q_yy - 2 theta Q_yd + theta^2 Q_dd
        SE    = sqrt(pi' Omega pi) / (pi' S z~d~)

    A pivot at or below PLIV_RANK_TOL times the largest diagonal entry of S z~z~' sets the
    flag (1.0) and makes every other entry NaN."""
    lay = PlivLayout(pliv_instruments_of(len(mom)))
    u = lay.unpack(mom)
    q = lay.q
    nan = float("nan")
    pi = _chol_solve_small(u["szz"], u["szd"], PLIV_RANK_TOL)
    if pi is None:
        return [nan, nan, nan, 1.0] + [nan] * q
    num = den = 0.0
    for i in range(q):
        num += pi[i] * u["szy"][i]
        den += pi[i] * u["szd"][i]
    # IEEE division, as on the device: x / 0 is an infinity or NaN, not an exception
    div = lambda a, b: a / b if b != 0.0 else (nan if a == 0.0 or a != a else math.copysign(
        float("inf"), a) * math.copysign(1.0, b))
    th = div(num, den)
    var = 0.0
    for i in range(q):
        for j in range(q):
            var += pi[i] * pi[j] * (u["qyy"][i][j] - 2.0 * th * u["qyd"][i][j]
                                    + th * th * u["qdd"][i][j])
    return [th, div(math.sqrt(var if var > 0.0 else 0.0), den), den, 0.0] + pi


def chi2_quantile(level: float, df: int) -> float:
    """x with P(chi2_df <= x) = level, by bisection of ``_chi2_sf`` (df = 1: the squared
    normal quantile of ``LateResult.anderson_rubin``)."""
    if not 0.0 < level < 1.0:
        raise ValueError("level must be in (0, 1)")
    if df == 1:
        return normal_quantile(0.5 + level / 2.0) ** 2
    lo, hi = 0.0, 1.0
    while _chi2_sf(hi, df) > 1.0 - level:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _chi2_sf(mid, df) > 1.0 - level:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@dataclass
class ArGridSet:
    """The Anderson-Rubin set of a PLIV fit with several instruments, on a grid of theta:
    ``inside[i]`` says whether ``grid[i]`` is accepted; lower / upper are the extreme accepted
    points (NaN when none is). kind "empty", "interval" (the accepted points are consecutive)
    or "union"; ``open_ended`` when an end point of the grid is accepted, so the set may go on
    beyond it."""
    kind: str
    lower: float
    upper: float
    level: float
    grid: list
    inside: list
    open_ended: bool

    def __contains__(self, theta) -> bool:
        if self.kind == "empty":
            return False
        near = min(range(len(self.grid)), key=lambda i: abs(self.grid[i] - theta))
        return bool(self.inside[near])


@dataclass
class PlivResult:
    """The effect of a real treatment D in the cross-fitted partially linear IV model
    (DoubleML ``DoubleMLPLIV``, partialling-out score) with q instruments: ``theta`` with its
    SE and CI, the first-stage weights ``pi`` of the instrument residuals, the homoskedastic
    first-stage partial F and the ``weak_instruments`` flag (F < 10). Everything is a host
    function of ``moments`` (PlivLayout); a cluster-robust fit replaces the SE
    (``from_moments(se=)``) and keeps the unclustered one in the diagnostics."""
    method: str
    theta: float
    se: float
    lower_ci: float
    upper_ci: float
    pi: list
    first_stage_F: float
    weak_instruments: bool
    rank_deficient: bool
    moments: list
    diagnostics: dict = field(default_factory=dict)

    @classmethod
    def from_moments(cls, method, mom, se=None, **diag):
        """From the moments; n_instruments and the held-out RMSE of l and r come from them
        too, ``diag`` adds n and hipgraph. se: a standard error that replaces the score's
        (the cluster-robust one); the score's goes to diagnostics["se_unclustered"] then."""
        mom = [float(v) for v in mom]
        lay = PlivLayout(pliv_instruments_of(len(mom)))
        q = lay.q
        fin = pliv_finish(mom)
        th, se0, den, flag = fin[:4]
        pi = fin[4:]
        n, syy, sdd = mom[0], mom[1], mom[3]
        rss = sdd - den
        F = (den / q) / (rss / (n - q)) if flag == 0.0 and rss > 0 and n > q else float("nan")
        rm = lambda s: math.sqrt(s / n) if n > 0 and s >= 0 else float("nan")
        d = dict(n_instruments=q, rmse_l=rm(syy), rmse_r=rm(sdd))
        if se is not None:
            d["se_unclustered"] = se0
        d.update(diag)
        d.setdefault("n", int(round(n)) if math.isfinite(n) else -1)
        s = se0 if se is None else float(se)
        return cls(method, th, s, th - Z * s, th + Z * s, pi, F, bool(F < 10.0), flag != 0.0,
                   mom, d)

    @property
    def layout(self) -> PlivLayout:
        return PlivLayout(pliv_instruments_of(len(self.moments)))

    # the record of every estimator table (AteResult.row)
    @property
    def ate(self) -> float:
        return self.theta

    def row(self):
        return {"Method": self.method, "ATE": self.theta, "lower_ci": self.lower_ci,
                "upper_ci": self.upper_ci, "se": self.se}

    def _g_omega(self, theta):
        u = self.layout.unpack(self.moments)
        q = self.layout.q
        g = [u["szy"][i] - theta * u["szd"][i] for i in range(q)]
        om = [[u["qyy"][i][j] - 2.0 * theta * u["qyd"][i][j] + theta * theta * u["qdd"][i][j]
               for j in range(q)] for i in range(q)]
        return g, om

    def ar_stat(self, theta) -> float:
        """The Anderson-Rubin statistic g' Omega(theta)^-1 g with g = S z~y~ - theta S z~d~
        and Omega(theta) = Q_yy - 2 theta Q_yd + theta^2 Q_dd: chi2 with q degrees of freedom
        under H0: theta_0 = theta, however weak the instruments. NaN when Omega(theta) is not
        positive definite."""
        g, om = self._g_omega(float(theta))
        x = _chol_solve_small(om, g, 0.0)
        if x is None:
            return float("nan")
        return sum(a * b for a, b in zip(g, x))

    def anderson_rubin(self, level=0.95, grid=None):
        """The weak-instrument-robust confidence set {theta : ar_stat(theta) <=
        chi2_q(level)}. q = 1: in closed form, the quadratic inequality A theta^2 + B theta +
        C <= 0 with c = chi2_1(level),

            A = (S z~d~)^2 - c Q_dd     B = -2 S z~y~ S z~d~ + 2 c Q_yd     C = (S z~y~)^2 - c Q_yy

        and the cases of ``LateResult.anderson_rubin`` (A > 0: an interval; A < 0: two rays,
        or the whole line without a real root) -> ``ArSet``. q > 1: over ``grid`` (default:
        401 points over theta +- 10 SE) -> ``ArGridSet``."""
        crit = chi2_quantile(level, self.layout.q)
        if self.layout.q == 1:
            u = self.layout.unpack(self.moments)
            sy, sd = u["szy"][0], u["szd"][0]
            qyy, qyd, qdd = u["qyy"][0][0], u["qyd"][0][0], u["qdd"][0][0]
            inf = float("inf")
            A = sd * sd - crit * qdd
            B = -2.0 * sy * sd + 2.0 * crit * qyd
            C = sy * sy - crit * qyy
            if A == 0.0:                                    # B theta + C <= 0
                if B == 0.0:
                    return ArSet("all", -inf, inf, level)
                return ArSet("two_rays", -C / B, inf, level) if B > 0 else \
                    ArSet("two_rays", -inf, -C / B, level)
            disc = B * B - 4 * A * C
            if disc <= 0.0 and A < 0:
                return ArSet("all", -inf, inf, level)
            r = math.sqrt(max(disc, 0.0))
            qq = -0.5 * (B + math.copysign(r, B))
            roots = sorted((qq / A, C / qq)) if qq != 0.0 else [0.0, 0.0]
            return ArSet("interval" if A > 0 else "two_rays", roots[0], roots[1], level)
        if grid is None:
            if not (math.isfinite(self.theta) and math.isfinite(self.se) and self.se > 0):
                raise ValueError("a grid= of theta values is needed: theta or SE is not finite")
            grid = [self.theta + self.se * (k - 200) / 20.0 for k in range(401)]
        grid = sorted(float(t) for t in grid)
        if not grid:
            raise ValueError("grid must hold at least one theta")
        inside = [bool(self.ar_stat(t) <= crit) for t in grid]
        hit = [i for i, v in enumerate(inside) if v]
        if not hit:
            return ArGridSet("empty", float("nan"), float("nan"), level, grid, inside, False)
        kind = "interval" if hit[-1] - hit[0] + 1 == len(hit) else "union"
        return ArGridSet(kind, grid[hit[0]], grid[hit[-1]], level, grid, inside,
                         inside[0] or inside[-1])

    def _ar_text(self, ar) -> str:
        if isinstance(ar, ArGridSet):
            if ar.kind == "empty":
                return "empty on the grid"
            tail = " (reaches the end of the grid)" if ar.open_ended else ""
            return f"{ar.kind} within [{ar.lower:.4f}, {ar.upper:.4f}]{tail}"
        return {"interval": f"[{ar.lower:.4f}, {ar.upper:.4f}]", "all": "the whole line",
                "two_rays": f"(-inf, {ar.lower:.4f}] and [{ar.upper:.4f}, inf)"}[ar.kind]

    def table(self) -> str:
        d = self.diagnostics
        lines = [
            f"{self.method}: n {d.get('n', '?')}, instruments {self.layout.q}, first-stage F "
            f"{self.first_stage_F:.2f}{' (WEAK: F < 10)' if self.weak_instruments else ''}, "
            f"rmse l {d.get('rmse_l', float('nan')):.4f} r {d.get('rmse_r', float('nan')):.4f}",
            f"{'':>12s} {'effect':>9s} {'SE':>9s} {'lower_ci':>9s} {'upper_ci':>9s}",
            f"{'theta':>12s} {self.theta:9.4f} {self.se:9.4f} {self.lower_ci:9.4f} "
            f"{self.upper_ci:9.4f}",
            "pi: " + " ".join(f"{v:.4f}" for v in self.pi)]
        if "n_clusters" in d:
            lines.append(f"clusters {d['n_clusters']}, largest {d.get('max_cluster', '?')}, "
                         f"unclustered SE {d.get('se_unclustered', float('nan')):.4f}")
        if not self.rank_deficient:
            lines.append(f"Anderson-Rubin 95% set: {self._ar_text(self.anderson_rubin())}")
        return "\n".join(lines)

    def json(self) -> str:
        keep = lambda d: {k: (v if isinstance(v, (int, float, str, bool, type(None))) else str(v))
                          for k, v in d.items()}
        out = {"method": self.method, "theta": self.theta, "se": self.se,
               "lower_ci": self.lower_ci, "upper_ci": self.upper_ci, "pi": self.pi,
               "first_stage_F": self.first_stage_F, "weak_instruments": self.weak_instruments,
               "rank_deficient": self.rank_deficient, "moments": self.moments,
               "diagnostics": keep(self.diagnostics)}
        if not self.rank_deficient:
            ar = self.anderson_rubin()
            a = asdict(ar)
            a.pop("grid", None)
            a.pop("inside", None)
            out["anderson_rubin"] = a
        return json.dumps(out)

    to_json = json


def results_frame(results):
    import pandas as pd
    return pd.DataFrame([r.row() for r in results])


def format_table(results) -> str:
    lines = [f"{'Method':45s} {'ATE':>9s} {'SE':>9s} {'lower_ci':>9s} {'upper_ci':>9s}"]
    for r in results:
        se = "" if math.isnan(r.se) else f"{r.se:9.4f}"
        lines.append(f"{r.method:45s} {r.ate:9.4f} {se:>9s} {r.lower_ci:9.4f} {r.upper_ci:9.4f}")
    return "\n".join(lines)
