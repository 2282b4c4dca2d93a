"""The average effect of the cross-fitted interactive model over other target populations:
the treated (ATT; DoubleML ``DoubleMLIRM(score="ATTE")``, grf
``average_treatment_effect(target.sample = "treated")``) and the controls (ATC,
``target.sample = "control"``), beside everyone (the ATE of ``estimators/irm.py``), with the
joint covariance of the three.

With e the clipped propensity and the two quotients the AIPW score psi is made of,

    q1 = w (y - g1) / e                q0 = (1 - w)(y - g0) / (1 - e)
    a  = w (y - g0) - e q0             (needs g0 and m only)
    c  = -(1 - w)(y - g1) + (1 - e) q1 (needs g1 and m only)
    psi = g1 - g0 + q1 - q0 = a + c    (algebraically)

and over the n held-out rows, n1 = S w, n0 = n - n1, p1 = n1 / n, p0 = n0 / n:

    theta_all = S psi / n      theta_treated = S a / n1      theta_control = S c / n0
    phi_all = psi - theta_all
    phi_trt = (a - theta_treated w) / p1        (the ATTE score: psi_a theta + psi_b, J = -1)
    phi_ctl = (c - theta_control (1 - w)) / p0
    Cov[j, k] = S phi_j phi_k / (n - 1) / n     (the n - 1 rule of ``irm.mean_se``)

All of it follows from 12 fp64 sums over the rows (``result.TARGET_MOMENTS``): the fit is
that of ``irm_fit_phases``, one more instantiation of the fused score pass
(``irm.irm_target_moments``, csrc/irm.hip) accumulates them with no division beside the two
of psi, and everything after it happens on the host (``result.TargetResult``). Because the
three estimands share one set of sums, "does the effect on the treated differ from the effect
on the controls?" is ``result.contrast("treated", "control")``.

Only the nuisances the requested targets need are fitted: "treated" needs g0 and m,
"control" g1 and m, "all" all three -- an ATT-only call solves 2 K K path problems instead of
3 K K (per nuisance: K outer folds x (1 full + K - 1 inner CV paths), ``cv_problem_count``).

Out of scope: repeated cross-fitting of these targets (the multi-split score kernel keeps 4
splits per pass on a measured register budget; 12 accumulators per split would need that
budget measured again), and group, curve and policy versions of the ATT (ratio estimators per
group).
"""
from __future__ import annotations

import numpy as np

from ..result import TARGET_MOMENTS, TARGETS, TargetResult, check_targets
from .irm import (arm_split_panel, check_logit_scope, comm_counts, irm_fit_phases,
                  irm_target_moments, propensity_args, propensity_link, run_body,
                  run_phases)

N_TARGET = len(TARGET_MOMENTS)   # 12
# the rows (0: g0, 1: g1, 2: m) of a coefficient block a target's moments read
TARGET_NUISANCES = {"all": (0, 1, 2), "treated": (0, 2), "control": (1, 2)}


def target_nuisances(targets) -> tuple:
    """The nuisances (0: g0, 1: g1, 2: m), ascending, that ``targets`` need between them."""
    return tuple(sorted({r for t in check_targets(targets) for r in TARGET_NUISANCES[t]}))


def target_phases(pan, folds: int, targets=TARGETS, lambda_rule="min", clip=0.01, comm=None,
                  seg_counts=None, propensity="linear"):
    """The target step as phases for utils.graphs.SegmentedStep: those of ``irm_phases`` up
    to the fitted coefficients, with only the nuisances ``targets`` need in the path launch
    (``irm_fit_phases(nuisances=)``), then

    B'  the 12 target moments (csrc/irm.hip ``ate_irm_target_moments``)      device
    C06 one all-reduce of the 12 moments                                     collective (world > 1)

    The result state holds "mom" [12], "coef" [K, 3, p+1] (zero rows for the nuisances that
    were not fitted) and "cv"."""
    phases, reduce = irm_fit_phases(pan, folds, lambda_rule, comm, seg_counts,
                                    nuisances=target_nuisances(targets), propensity=propensity)
    link = propensity_link(propensity)

    def phase_moments(st):
        return {**st, "mom": irm_target_moments(pan, st["coef"], clip, 2, link=link)}

    phases.append(phase_moments)
    if reduce is not None:
        phases.append(reduce("mom"))
    return phases


def irm_targets_panel(pan, folds: int, targets=TARGETS, lambda_rule="min", clip=0.01, comm=None,
                      seg_counts=None, propensity="linear"):
    """The target moments on an arm-split fold panel (the layout of
    ``irm.irm_crossfit_panel``) -> (mom [12], cv). Device tensors, no host sync (capturable);
    ``result.TargetResult.from_moments(method, mom, targets)`` finishes on the host."""
    st = run_phases(target_phases(pan, folds, targets, lambda_rule, clip, comm, seg_counts,
                                  propensity))
    return st["mom"], st.get("cv")


def _targets_body(pan, folds, targets, lambda_rule, clip, dist=None, counts=None,
                  propensity="linear"):
    """The whole call as one device function (GraphCache captures it): the 12 moments."""
    comm, seg_counts = comm_counts(dist, counts)
    mom, _ = irm_targets_panel(pan, folds, targets, lambda_rule, clip, comm=comm,
                               seg_counts=seg_counts, propensity=propensity)
    return mom


def dml_irm_targets(Y, W, X, targets=TARGETS, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                    method="DML-IRM target populations (LASSO)", device=None, dtype="f64",
                    dist=None, graph=True, repeats=1, propensity="linear") -> TargetResult:
    """The average effect over everyone ("all"), on the treated ("treated") and on the
    controls ("control") from one cross-fit of ``irm.dml_irm_lasso`` (same folds, same
    nuisances, same score; the "all" row is its theta and SE), with their joint covariance
    (``result.cov``, ``result.contrast(a, b)``). Only the nuisances that ``targets`` need are
    fitted; the rows of the other targets are NaN. W must be exactly {0, 1}. Matches
    reference.estimators.dml_irm_targets.

    graph: as ``dml_irm_lasso``, one captured hipGraph on a GPU; ``targets`` is part of the
    cache key. diagnostics: n, n_treated, n_clipped, hipgraph.

    Not supported (ValueError): ``repeats`` other than 1 -- repeated cross-fitting of these
    targets is out of scope (see the module docstring), as are their group, curve and policy
    versions."""
    targets = check_targets(targets)
    check_logit_scope(propensity, X, folds, dtype, dist, repeats)
    if repeats != 1:
        raise ValueError("repeated cross-fitting is not available for the target populations: "
                         "repeats must be 1")
    # the order of TARGETS: one cache entry per set of targets
    targets = tuple(t for t in TARGETS if t in targets)
    pan, counts, _, n, _ = arm_split_panel(Y, W, X, folds, seed, dtype, device, dist)
    out, g = run_body("dml_irm_targets", _targets_body, (pan,), folds, targets, lambda_rule,
                      float(clip), dist, tuple(counts.tolist()), *propensity_args(propensity),
                      graph=graph, dist=dist)
    mom = out.detach().double().cpu().numpy()
    fin = lambda x: int(round(x)) if np.isfinite(x) else -1
    extra = {} if propensity == "linear" else {"propensity": propensity}
    return TargetResult.from_moments(method, mom, targets, n=n, n_treated=fin(mom[11]),
                                     n_clipped=fin(mom[3]), hipgraph=g, **extra)
