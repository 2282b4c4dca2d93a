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


def results_frame(results):
    import pandas as pd
    return pd.DataFrame([r.row() for r in results])


def format_table(results) -> str:
    lines = [f"{'Method':45s} {'ATE':>9s} {'SE':>9s} {'lower_ci':>9s} {'upper_ci':>9s}"]
    for r in results:
        se = "" if math.isnan(r.se) else f"{r.se:9.4f}"
        lines.append(f"{r.method:45s} {r.ate:9.4f} {se:>9s} {r.lower_ci:9.4f} {r.upper_ci:9.4f}")
    return "\n".join(lines)
