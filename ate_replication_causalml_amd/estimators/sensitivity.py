"""Sensitivity of the cross-fitted interactive model's ATE to unobserved confounding (the
``sensitivity_analysis`` / ``sensitivity_benchmark`` of DoubleML's IRM; Chernozhukov,
Cinelli, Newey, Sharma & Syrgkanis 2022, "Long story short").

With psi the AIPW score of ``estimators/irm.py``, e the clipped propensity and, per held-out
row,

    b  = (y - g_w)^2                         g_w = g1 on treated rows, g0 on control rows
    rr = w / e - (1 - w) / (1 - e)           the Riesz representer
    c  = 2 (1 / e + 1 / (1 - e)) - rr^2

the plug-ins are theta = mean(psi), sigma2 = mean(b), nu2 = mean(c), S = sqrt(sigma2 nu2). A
confounder that explains a share cf_y of the outcome's residual variance and raises the
precision of the Riesz representer by cf_d / (1 - cf_d), with correlation rho between the two
biases, moves theta by at most S k, k = |rho| sqrt(cf_y) sqrt(cf_d / (1 - cf_d)). The bounds
theta -/+ S k, their standard errors (from the 3x3 covariance of (psi, b, c)), the robustness
values and the covariate benchmarks are all functions of 14 fp64 sums over the rows
(``result.SENS_MOMENTS``): the fit is that of ``irm_phases``, one more instantiation of the
fused score pass (``irm.irm_sens_moments``, csrc/irm.hip) accumulates them, and everything
after it happens on the host (``result.SensitivityResult``).

A benchmark refits the model without a set of covariates on the same folds. Its Gram is a
sub-block of the fold Gram stack already in HBM, so it costs one more path launch on the
same stack (``cv_enet_gaussian`` with the kept columns) and one more 14-moment pass with
zeros on the dropped columns.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops.devconst import const
from ..ops.enet import cv_enet_gaussian
from ..result import SENS_MOMENTS, SensitivityResult, check_benchmarks, check_scenario
from .common import as_np
from .irm import (arm_split_panel, comm_counts, fit_problems, irm_fit_phases,  # noqa: F401
                  irm_sens_moments, run_body, run_phases)
from .lasso import global_seg_counts

N_SENS = len(SENS_MOMENTS)   # 14


def sens_phases(pan, folds: int, lambda_rule="min", clip=0.01, benchmarks=(), comm=None,
                seg_counts=None):
    """The sensitivity step as phases for utils.graphs.SegmentedStep: those of ``irm_phases``
    up to the fitted coefficients, then

    B'  the 14 sensitivity moments of the long model (csrc/irm.hip)           device
    B*  per benchmark set: CV-LASSO paths of the 3 K nuisances without its
        columns, on the same Gram stack (one path launch), the picked
        coefficients scattered to [K, 3, p+1], and their 14 moments          device
    C06 all-reduce of the [1 + sets, 14] moments                              collective (world > 1)

    The result state holds "mom" [1 + sets, 14] (row 0: the long model), "coef", "cv" and
    per set "coef_short"."""
    K = folds
    p = len(pan.xcols)
    benchmarks = check_benchmarks(benchmarks, p)
    if seg_counts is None:
        dist = comm is not None and comm.world_size > 1
        seg_counts = global_seg_counts(pan, comm) if dist else np.asarray(pan.seg_nreal)
    phases, reduce = irm_fit_phases(pan, K, lambda_rule, comm, seg_counts)
    counts3, full_sets, full_y, ycols = fit_problems(pan, K, seg_counts)

    def phase_long(st):
        return {**st, "moms": [irm_sens_moments(pan, st["coef"], clip, 2)], "coef_short": []}

    def phase_short(cols):
        drop = set(cols)
        kept = [j for j in range(p) if j not in drop]
        xkept = [pan.xcols[j] for j in kept]
        slots = const([0] + [1 + j for j in kept], torch.int64, pan.device)

        def f(st):
            G = st["G"]
            G3 = st["G3"] if "G3" in st else torch.cat([G, G[0::2] + G[1::2]])
            cv = cv_enet_gaussian(G3, pan, xkept, ycols, full_sets=full_sets,
                                  seg_counts=counts3, full_y=full_y)
            short = (cv.coef_min if lambda_rule == "min" else cv.coef_1se).reshape(K, 3, -1)
            coef = torch.zeros(K, 3, p + 1, dtype=torch.float64, device=short.device)
            coef.index_copy_(2, slots, short.double())
            return {**st, "G3": G3, "coef_short": st["coef_short"] + [coef],
                    "moms": st["moms"] + [irm_sens_moments(pan, coef, clip, 2)]}
        return f

    def phase_stack(st):
        mom = torch.stack(st["moms"])
        return {**{k: v for k, v in st.items() if k not in ("moms", "G3")}, "mom": mom}

    phases.append(phase_long)
    phases += [phase_short(cols) for cols in benchmarks]
    phases.append(phase_stack)
    if reduce is not None:
        phases.append(reduce("mom"))
    return phases


def irm_sens_panel(pan, folds: int, lambda_rule="min", clip=0.01, benchmarks=(), comm=None,
                   seg_counts=None):
    """The sensitivity moments on an arm-split fold panel (the layout of
    ``irm.irm_crossfit_panel``) -> (mom [1 + sets, 14], cv of the long model). Row 0: the
    model with every covariate; row 1 + j: the model without benchmark set j. Device tensors,
    no host sync (capturable); ``result.SensitivityResult.from_moments`` finishes on the
    host."""
    st = run_phases(sens_phases(pan, folds, lambda_rule, clip, benchmarks, comm, seg_counts))
    return st["mom"], st.get("cv")


def _sens_body(pan, folds, lambda_rule, clip, benchmarks, dist=None, counts=None):
    """The whole call as one device function (GraphCache captures it): the flat moments
    ``cat([long, short_1, ...])``."""
    comm, seg_counts = comm_counts(dist, counts)
    mom, _ = irm_sens_panel(pan, folds, lambda_rule, clip, benchmarks, comm=comm,
                            seg_counts=seg_counts)
    return mom.reshape(-1)


def dml_irm_sensitivity(Y, W, X, cf_y=0.03, cf_d=0.03, rho=1.0, level=0.95, null=0.0,
                        benchmarks=None, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                        method="DML-IRM sensitivity (LASSO)", device=None, dtype="f64",
                        dist=None, graph=True) -> SensitivityResult:
    """Sensitivity analysis of ``irm.dml_irm_lasso`` (same folds, same nuisances, same score,
    same theta and SE): bounds on the ATE and their one-sided ``level`` CI under a confounder
    of strength (cf_y, cf_d, rho), the robustness values RV / RVa against ``null``, and for
    each covariate set of ``benchmarks`` (lists of column indices into X; at most 8) the
    strength that set has, from a refit without it. Matches
    reference.estimators.dml_irm_sensitivity.

    graph: as ``dml_irm_lasso``, one captured hipGraph on a GPU; the benchmark sets are part
    of the cache key. Every further scenario is ``result.bounds(cf_y, cf_d, rho, level)``."""
    check_scenario(cf_y, cf_d, rho, level)
    bench = check_benchmarks(benchmarks, as_np(X).shape[1])
    pan, counts, _, n, _ = arm_split_panel(Y, W, X, folds, seed, dtype, device, dist)
    out, g = run_body("dml_irm_sens", _sens_body, (pan,), folds, lambda_rule, float(clip), bench,
                      dist, tuple(counts.tolist()), graph=graph, dist=dist)
    v = out.detach().double().cpu().numpy().reshape(1 + len(bench), N_SENS)
    mom = v[0]
    fin = lambda x: int(round(x)) if np.isfinite(x) else -1
    return SensitivityResult.from_moments(
        method, mom, cf_y, cf_d, rho, level, null,
        short=[(cols, v[1 + j]) for j, cols in enumerate(bench)],
        n=n, n_clipped=fin(mom[3]), n_treated=fin(mom[13]), hipgraph=g)
