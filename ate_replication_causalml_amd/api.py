"""Public API: one function per reference estimator, each taking
``(Y, W, X, ...)`` arrays and returning an :class:`AteResult`, plus ``replicate()``
which runs the driver ``ate_replication.Rmd`` end to end (14 rows, same labels).

``run=RunConfig(backend=...)`` selects the execution path:

* ``"gpu"``  — hand-written gfx950 kernels (libatehip.so), the default when a GPU
  is visible;
* ``"cpu"``  — the same device orchestration on host tensors (CPU Gram / solver
  fallbacks, host C++ forest engine);
* ``"reference"`` — the float64 numpy T-ref (reference/), the parity oracle.

Reference function -> API name:
naive_ate -> ate_naive; ate_condmean_ols -> ate_ols; prop_score_weight -> ate_ipw;
prop_score_ols -> ate_ipw_wls; ate_condmean_lasso -> ate_lasso_single; ate_lasso ->
ate_lasso; prop_score_lasso -> propensity_lasso; doubly_robust -> ate_aipw_rf;
doubly_robust_glm -> ate_aipw_glm; belloni -> ate_belloni; double_ml ->
ate_double_ml; residual_balance_ATE -> ate_residual_balance; grf::causal_forest +
estimate_average_effect -> ate_causal_forest; K-fold DML-PLR -> ate_dml; K-fold DML-IRM
(cross-fitted AIPW, LASSO nuisances) -> ate_dml_irm; its group effects with a joint
multiplier-bootstrap band (DoubleML gate / bootstrap / confint(joint=True)) -> ate_dml_irm_gate;
its effect curve along one covariate on a B-spline basis with a uniform band (DoubleML
cate(basis) / confint(joint=True)) -> ate_dml_irm_cate;
the exact depth-2 policy tree on its scores (DoubleML policy_tree, searched exactly as
policytree does) -> ate_dml_irm_policy;
the evaluation of a treatment-priority rule on its scores: AUTOC, Qini and the TOC curve with
half-sample bootstrap SEs (grf rank_average_treatment_effect) -> ate_dml_irm_rate;
its sensitivity to unobserved confounding (DoubleML sensitivity_analysis /
sensitivity_benchmark) -> ate_dml_irm_sensitivity;
its effect on the treated and on the controls with the joint covariance (DoubleML
IRM(score="ATTE"), grf average_treatment_effect(target.sample=)) -> ate_dml_irm_targets;
the LATE with a binary instrument under noncompliance (DoubleML DoubleMLIIVM) -> ate_dml_iivm;
the mean potential outcomes of a multi-valued treatment, their contrasts against a reference
level and a simultaneous band (DoubleML DoubleMLAPOS / causal_contrast, grf
multi_arm_causal_forest) -> ate_dml_apos;
the effect of a real treatment instrumented by 1 to 4 instruments in the partially linear IV
model (DoubleML DoubleMLPLIV) -> ate_dml_pliv.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from .config import METHODS, BalanceConfig, ReplicateConfig, RunConfig
from .result import (ApoResult, AteResult, CateResult, GateResult, LateResult, PlivResult, PolicyTreeResult, RateResult,
                     SensitivityResult,
                     TargetResult, format_table, results_frame)
from .utils import guards
from .utils.tracing import trace


def _run(run):
    return run if run is not None else RunConfig()


def _ref(run):
    return run.backend == "reference"


def _np(a):
    import torch
    if isinstance(a, torch.Tensor):
        return a.detach().double().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------ estimators
def ate_naive(Y, W, method="naive", run=None) -> AteResult:
    """E1 naive_ate (ate_functions.R:3-21)."""
    run = _run(run)
    with trace(f"ate_naive[{method}]"):
        if _ref(run):
            from .reference import estimators as R
            return R.naive(Y, W, method)
        from .estimators import linear as D
        return D.naive(Y, W, method, device=run.device())


def ate_ols(Y, W, X, method="Direct Method", run=None) -> AteResult:
    """E2 ate_condmean_ols (ate_functions.R:25-39)."""
    run = _run(run)
    with trace("ate_ols"):
        if _ref(run):
            from .reference import estimators as R
            return R.ols(Y, W, X, method)
        from .estimators import linear as D
        return D.ols(Y, W, X, method, device=run.device(), dtype=run.dtype)


def propensity_logistic(W, X, run=None) -> np.ndarray:
    """E16 glm(W ~ covariates, binomial) fitted values (ate_replication.Rmd:165-168)."""
    run = _run(run)
    with trace("propensity_logistic"):
        if _ref(run):
            from .reference import estimators as R
            return R.propensity_logistic(W, X)
        from .estimators import linear as D
        return _np(D.propensity_logistic(W, X, device=run.device(), dtype=run.dtype))


def propensity_lasso(W, X, nfolds=10, run=None) -> np.ndarray:
    """E7 prop_score_lasso (ate_functions.R:133-146): binomial cv.glmnet, lambda.1se."""
    run = _run(run)
    with trace("propensity_lasso"):
        if _ref(run):
            from .reference import estimators as R
            return R.propensity_lasso(W, X, seed=run.seed, nfolds=nfolds)
        from .estimators import linear as D
        dt = "f64" if run.dtype == "bf16" else run.dtype
        return _np(D.propensity_lasso(W, X, seed=run.seed, nfolds=nfolds, device=run.device(),
                                      dtype=dt))


def ate_ipw(Y, W, X, p, method="Propensity_Weighting", run=None) -> AteResult:
    """E3 prop_score_weight (ate_functions.R:44-63)."""
    run = _run(run)
    with trace(f"ate_ipw[{method}]"):
        if _ref(run):
            from .reference import estimators as R
            r = R.ipw(Y, W, X, p, method, compat=run.compat)
        else:
            from .estimators import linear as D
            r = D.ipw(Y, W, X, p, method, compat=run.compat, device=run.device(),
                      dtype="f64" if run.dtype == "bf16" else run.dtype)
    import torch
    r.diagnostics.update(guards.overlap_report(torch.as_tensor(_np(p)), torch.as_tensor(_np(W))))
    return r


def ate_ipw_wls(Y, W, p, method="Propensity_Regression", run=None) -> AteResult:
    """E4 prop_score_ols (ate_functions.R:67-86)."""
    run = _run(run)
    with trace("ate_ipw_wls"):
        if _ref(run):
            from .reference import estimators as R
            return R.ipw_wls(Y, W, p, method)
        from .estimators import linear as D
        return D.ipw_wls(Y, W, p, method, device=run.device(),
                         dtype="f64" if run.dtype == "bf16" else run.dtype)


def ate_lasso_single(Y, W, X, nfolds=10, method="Single-equation LASSO", run=None) -> AteResult:
    """E5 ate_condmean_lasso (ate_functions.R:89-108)."""
    run = _run(run)
    with trace("ate_lasso_single"):
        if _ref(run):
            from .reference import estimators as R
            return R.lasso_single(Y, W, X, seed=run.seed, nfolds=nfolds, method=method)
        from .estimators import lasso as DL
        return DL.lasso_single(Y, W, X, seed=run.seed, nfolds=nfolds, method=method,
                               device=run.device(), dtype=run.dtype)


def ate_lasso(Y, W, X, nfolds=10, method="Usual LASSO", run=None) -> AteResult:
    """E6 ate_lasso (ate_functions.R:111-130)."""
    run = _run(run)
    with trace("ate_lasso"):
        if _ref(run):
            from .reference import estimators as R
            return R.lasso_usual(Y, W, X, seed=run.seed, nfolds=nfolds, method=method)
        from .estimators import lasso as DL
        return DL.lasso_usual(Y, W, X, seed=run.seed, nfolds=nfolds, method=method,
                              device=run.device(), dtype=run.dtype)


def ate_aipw_rf(Y, W, X, num_trees=100, bootstrap_se=False, B=1000,
                method="Doubly Robust with Random Forest PS", run=None,
                splits="auto") -> AteResult:
    """E8 doubly_robust (ate_functions.R:149-207). ``splits``: "exact" = randomForest split
    semantics (every distinct value, midpoint thresholds), "binned" = 256-bin histograms,
    "auto" = exact up to 65536 rows (the tutorial's df_mod)."""
    run = _run(run)
    with trace("ate_aipw_rf", trees=num_trees):
        if _ref(run):
            from .reference import estimators as R
            return R.aipw_rf(Y, W, X, num_trees=num_trees, bootstrap_se=bootstrap_se, B=B,
                             seed=run.seed, compat=run.compat, method=method, splits=splits)
        from .estimators import forest as DF
        return DF.aipw_rf(Y, W, X, num_trees=num_trees, bootstrap_se=bootstrap_se, B=B,
                          seed=run.seed, compat=run.compat, method=method, device=run.device(),
                          splits=splits)


def ate_aipw_glm(Y, W, X, bootstrap_se=False, B=1000,
                 method="Doubly Robust with logistic regression PS", run=None) -> AteResult:
    """E9 doubly_robust_glm (ate_functions.R:211-264)."""
    run = _run(run)
    with trace("ate_aipw_glm"):
        if _ref(run):
            from .reference import estimators as R
            return R.aipw_glm(Y, W, X, bootstrap_se=bootstrap_se, B=B, seed=run.seed,
                              compat=run.compat, method=method)
        from .estimators import linear as D
        return D.aipw_glm(Y, W, X, bootstrap_se=bootstrap_se, B=B, seed=run.seed,
                          compat=run.compat, method=method, device=run.device(),
                          dtype="f64" if run.dtype == "bf16" else run.dtype)


def ate_belloni(Y, W, X, nfolds=10, method="Belloni et.al", run=None) -> AteResult:
    """E11 belloni (ate_functions.R:286-328)."""
    run = _run(run)
    with trace("ate_belloni"):
        if _ref(run):
            from .reference import estimators as R
            return R.belloni(Y, W, X, seed=run.seed, nfolds=nfolds, compat=run.compat,
                             method=method)
        from .estimators import lasso as DL
        return DL.belloni(Y, W, X, seed=run.seed, nfolds=nfolds, compat=run.compat,
                          method=method, device=run.device(), dtype=run.dtype)


def ate_double_ml(Y, W, X, num_trees=100, method="Double Machine Learning", run=None,
                  splits="auto") -> AteResult:
    """E12/E13 double_ml (ate_functions.R:332-389): two-half RF cross-fitting; ``splits``
    as in ate_aipw_rf."""
    run = _run(run)
    with trace("ate_double_ml", trees=num_trees):
        if _ref(run):
            from .reference import estimators as R
            return R.double_ml(Y, W, X, num_trees=num_trees, method=method, splits=splits)
        from .estimators import forest as DF
        return DF.double_ml(Y, W, X, num_trees=num_trees, method=method, device=run.device(),
                            splits=splits)


def ate_dml(Y, W, X, folds=5, lambda_rule="min", method="DML cross-fit (LASSO)",
            run=None, repeats=1, aggregate="median", clusters=None) -> AteResult:
    """K-fold cross-fit partially linear DML with CV-LASSO nuisances (north-star).
    ``repeats`` > 1: repeated cross-fitting over that many distinct K-fold partitions
    (Chernozhukov et al. 2018 §3.4), ``aggregate`` "median" (default) or "mean"; the
    partitions share one Gram pass (estimators/lasso.dml_repeated_phases).
    ``clusters``: an (n,) vector of labels (integers or strings) of dependent rows -- whole
    clusters are cross-fitted and the SE is cluster-robust (estimators/cluster.py; grf
    ``clusters=``, DoubleML ``DoubleMLClusterData``); diagnostics gain n_clusters,
    max_cluster, design_effect and se_unclustered. One-way clustering, ``repeats`` = 1."""
    run = _run(run)
    with trace("ate_dml", folds=folds, repeats=repeats):
        if clusters is not None:
            from .estimators import cluster as DC
            if _ref(run):
                from .reference import estimators as R
                lay = DC.cluster_layout(clusters, len(_np(Y)), folds, run.seed, repeats=repeats)
                return R.dml_plr_lasso(Y, W, X, folds=folds, seed=run.seed,
                                       lambda_rule=lambda_rule, method=method,
                                       clusters=lay.codes)
            return DC.dml_plr_lasso_cluster(Y, W, X, clusters, folds=folds, seed=run.seed,
                                            lambda_rule=lambda_rule, method=method,
                                            device=run.device(), dtype=run.dtype,
                                            repeats=repeats)
        if repeats > 1:
            if _ref(run):
                from .reference import estimators as R
                return R.dml_plr_lasso_repeated(Y, W, X, folds, repeats, run.seed, lambda_rule,
                                                aggregate)
            from .estimators import lasso as DL
            return DL.dml_plr_lasso_repeated(Y, W, X, folds, repeats, run.seed, lambda_rule,
                                             aggregate, device=run.device(), dtype=run.dtype)
        if _ref(run):
            from .reference import estimators as R
            return R.dml_plr_lasso(Y, W, X, folds=folds, seed=run.seed, lambda_rule=lambda_rule,
                                   method=method)
        from .estimators import lasso as DL
        return DL.dml_plr_lasso(Y, W, X, folds=folds, seed=run.seed, lambda_rule=lambda_rule,
                                method=method, device=run.device(), dtype=run.dtype)


def _linear_only(propensity, what):
    """``propensity`` of an estimator the binomial propensity fit does not reach."""
    from .estimators.irm import check_propensity
    if check_propensity(propensity) != "linear":
        raise ValueError(f'propensity="logit" is not available for {what}: only the '
                         'linear-probability propensity ("linear")')


def ate_dml_irm(Y, W, X, folds=5, lambda_rule="min", clip=0.01,
                method="DML-IRM cross-fit (LASSO)", run=None, repeats=1,
                aggregate="median", propensity="linear", clusters=None) -> AteResult:
    """K-fold cross-fitted AIPW for the interactive model (Chernozhukov et al. 2018 §5.1)
    with CV-LASSO nuisances: per-arm outcome regressions and the linear-probability
    propensity (clipped to [clip, 1 - clip]) on the fold Gram stack; the ATE under
    heterogeneous effects, doubly robust (estimators/irm.py). W must be binary.
    ``repeats`` > 1: repeated cross-fitting over that many K-fold partitions (at most
    ``folds``), ``aggregate`` "median" (default) or "mean", as ate_dml; the partitions share
    one Gram pass and one fused score pass (estimators/irm.irm_repeated_phases).
    ``propensity``: "linear" (default), or "logit" for the binomial CV-LASSO propensity
    (cv.glmnet(family="binomial"), all K * K fits in one launch, the score through the
    logistic link) -- as do ate_dml_irm_gate / _cate / _policy / _targets. Limits of "logit"
    (ValueError): ``repeats`` = 1, no row shards, an fp32 / fp64 panel, p <= 96, K <= 16; not
    available for ate_dml_irm_sensitivity and ate_dml_iivm.
    ``clusters``: an (n,) vector of labels of dependent rows -- whole clusters are
    cross-fitted and the SE is cluster-robust, as ate_dml(clusters=); either propensity,
    ``repeats`` = 1."""
    run = _run(run)
    with trace("ate_dml_irm", folds=folds, repeats=repeats):
        from .estimators.irm import check_logit_scope
        check_logit_scope(propensity, X, folds, repeats=repeats)
        if clusters is not None:
            from .estimators import cluster as DC
            if _ref(run):
                from .reference import estimators as R
                lay = DC.cluster_layout(clusters, len(_np(Y)), folds, run.seed, repeats=repeats)
                return R.dml_irm_lasso(Y, W, X, folds=folds, seed=run.seed,
                                       lambda_rule=lambda_rule, clip=clip, method=method,
                                       propensity=propensity, clusters=lay.codes)
            return DC.dml_irm_lasso_cluster(Y, W, X, clusters, folds=folds, seed=run.seed,
                                            lambda_rule=lambda_rule, clip=clip, method=method,
                                            device=run.device(), dtype=run.dtype,
                                            propensity=propensity, repeats=repeats)
        if repeats != 1:
            if _ref(run):
                from .reference import estimators as R
                return R.dml_irm_lasso_repeated(Y, W, X, folds, repeats, run.seed, lambda_rule,
                                                clip, aggregate)
            from .estimators import irm as DI
            return DI.dml_irm_lasso_repeated(Y, W, X, folds, repeats, run.seed, lambda_rule,
                                             clip, aggregate, device=run.device(),
                                             dtype=run.dtype)
        if _ref(run):
            from .reference import estimators as R
            return R.dml_irm_lasso(Y, W, X, folds=folds, seed=run.seed, lambda_rule=lambda_rule,
                                   clip=clip, method=method, propensity=propensity)
        from .estimators import irm as DI
        return DI.dml_irm_lasso(Y, W, X, folds=folds, seed=run.seed, lambda_rule=lambda_rule,
                                clip=clip, method=method, device=run.device(), dtype=run.dtype,
                                propensity=propensity)


def ate_dml_irm_gate(Y, W, X, groups, folds=5, lambda_rule="min", clip=0.01, n_boot=999,
                     level=0.95, method="DML-IRM group ATEs (LASSO)", run=None,
                     propensity="linear") -> GateResult:
    """Group average treatment effects of ate_dml_irm -- the mean AIPW score within each
    group of ``groups`` (an (n,) vector of labels; at most 64 groups) -- with pointwise and
    simultaneous ``level`` confidence bounds, the latter from ``n_boot`` Rademacher
    multiplier-bootstrap draws of the maximal t-statistic (estimators/gate.py)."""
    run = _run(run)
    with trace("ate_dml_irm_gate", folds=folds, n_boot=n_boot):
        if _ref(run):
            from .reference import estimators as R
            return R.dml_irm_gate(Y, W, X, groups, folds=folds, seed=run.seed,
                                  lambda_rule=lambda_rule, clip=clip, n_boot=n_boot, level=level,
                                  method=method, propensity=propensity)
        from .estimators import gate as DG
        return DG.dml_irm_gate_lasso(Y, W, X, groups, folds=folds, seed=run.seed,
                                     lambda_rule=lambda_rule, clip=clip, n_boot=n_boot,
                                     level=level, method=method, device=run.device(),
                                     dtype=run.dtype, propensity=propensity)


def ate_dml_irm_cate(Y, W, X, by, df=5, degree=3, knots=None, grid=None, folds=5,
                     lambda_rule="min", clip=0.01, n_boot=999, level=0.95,
                     method="DML-IRM CATE curve (LASSO)", run=None,
                     propensity="linear") -> CateResult:
    """The conditional average treatment effect of ate_dml_irm along one covariate ``by`` (a
    column index into X, or an (n,) vector): the projection of the AIPW score on a B-spline
    basis (``df`` <= 32 functions of ``degree`` 0..3, quantile knots unless ``knots`` is
    given) evaluated on ``grid`` (default: 100 points between the 5 % and 95 % order
    statistics), with pointwise and uniform ``level`` confidence bounds, the latter from
    ``n_boot`` Rademacher multiplier-bootstrap draws of the maximal t-statistic over the grid
    (estimators/cate.py). Further points: ``result.predict(x)``."""
    run = _run(run)
    with trace("ate_dml_irm_cate", folds=folds, n_boot=n_boot):
        if _ref(run):
            from .reference import estimators as R
            return R.dml_irm_cate(Y, W, X, by, df=df, degree=degree, knots=knots, grid=grid,
                                  n_boot=n_boot, level=level, folds=folds, seed=run.seed,
                                  lambda_rule=lambda_rule, clip=clip, method=method,
                                  propensity=propensity)
        from .estimators import cate as DC
        return DC.dml_irm_cate_lasso(Y, W, X, by, df=df, degree=degree, knots=knots, grid=grid,
                                     n_boot=n_boot, level=level, folds=folds, seed=run.seed,
                                     lambda_rule=lambda_rule, clip=clip, method=method,
                                     device=run.device(), dtype=run.dtype, propensity=propensity)


def ate_dml_irm_policy(Y, W, X, features, depth=2, bins=32, min_leaf=1, cost=0.0, train=None,
                       folds=5, lambda_rule="min", clip=0.01,
                       method="DML-IRM policy tree (LASSO)", run=None,
                       propensity="linear") -> PolicyTreeResult:
    """Whom to treat: the exact policy tree of depth <= 2 on the AIPW scores of ate_dml_irm
    less ``cost``, over the columns ``features`` of X (1..32) binned into at most ``bins``
    (2..64) bins, every split keeping ``min_leaf`` training rows on each side
    (estimators/policy.py). ``train``: a boolean mask of the rows the tree is learned on; the
    others give the held-out value. Without it only the in-sample value is reported, which is
    optimistic (``diagnostics["honest"]`` is False). New rows: ``result.predict(X)``."""
    run = _run(run)
    with trace("ate_dml_irm_policy", folds=folds, depth=depth):
        kw = dict(depth=depth, bins=bins, min_leaf=min_leaf, cost=cost, train=train, folds=folds,
                  seed=run.seed, lambda_rule=lambda_rule, clip=clip, method=method,
                  propensity=propensity)
        if _ref(run):
            from .reference import estimators as R
            return R.dml_irm_policy_tree(Y, W, X, features, **kw)
        from .estimators import policy as DP
        return DP.dml_irm_policy_lasso(Y, W, X, features, device=run.device(), dtype=run.dtype,
                                       **kw)


def ate_dml_irm_rate(Y, W, X, priority, q=None, subset=None, n_boot=200, level=0.95, folds=5,
                     lambda_rule="min", clip=0.01, run=None, propensity="linear",
                     clusters=None, repeats=1) -> RateResult:
    """Does treating in the order of ``priority`` (an (n,) vector, or a column index into X;
    higher = first, ties enter together) find the rows with large effects: the TOC curve on
    the grid ``q`` (default 0.1, ..., 1.0; at most 64 strictly increasing points in (0, 1]),
    its area AUTOC and the Qini coefficient of the AIPW scores of ate_dml_irm, with
    half-sample bootstrap standard errors from ``n_boot`` replicates, normal ``level``
    intervals, two-sided p-values and a uniform band over the curve (estimators/rate.py;
    grf's rank_average_treatment_effect). AUTOC / SE is the test for heterogeneity that the
    rule can exploit. ``subset``: a boolean mask of the evaluation rows (default: all).

    A priority fitted on the evaluation rows' own outcomes -- the tree of ate_dml_irm_policy
    or the curve of ate_dml_irm_cate from the same rows -- gives an optimistic RATE. Fit the
    rule on other rows and evaluate on the rest: ``ate_dml_irm_policy(train=mask)``, then
    ``subset=~mask`` here.

    ValueError: ``clusters``, ``repeats`` != 1, row shards, a non-finite priority on an
    evaluation row, fewer than 128 evaluation rows, a first grid point entering fewer than
    64 rows, 2^27 or more evaluation rows."""
    run = _run(run)
    with trace("ate_dml_irm_rate", folds=folds, n_boot=n_boot):
        from .estimators import rate as DR
        if clusters is not None:
            raise ValueError("ate_dml_irm_rate does not support clusters")
        if repeats != 1:
            raise ValueError("ate_dml_irm_rate does not support repeated cross-fitting")
        if _ref(run):
            from .reference import estimators as R
            return R.dml_irm_rate(Y, W, X, priority, q=q, subset=subset, n_boot=n_boot,
                                  level=level, folds=folds, seed=run.seed,
                                  lambda_rule=lambda_rule, clip=clip, propensity=propensity)
        return DR.dml_irm_rate_lasso(Y, W, X, priority, q=q, subset=subset, n_boot=n_boot,
                                     level=level, folds=folds, seed=run.seed,
                                     lambda_rule=lambda_rule, clip=clip, device=run.device(),
                                     dtype=run.dtype, propensity=propensity)


def ate_dml_irm_sensitivity(Y, W, X, cf_y=0.03, cf_d=0.03, rho=1.0, level=0.95, null=0.0,
                            benchmarks=None, folds=5, lambda_rule="min", clip=0.01,
                            run=None, propensity="linear") -> SensitivityResult:
    """Sensitivity of ate_dml_irm to unobserved confounding (Chernozhukov, Cinelli, Newey,
    Sharma & Syrgkanis 2022; DoubleML sensitivity_analysis / sensitivity_benchmark): bounds on
    the ATE and their one-sided ``level`` CI under a confounder of strength (cf_y, cf_d,
    rho), the robustness values RV / RVa against ``null``, and the strength of each covariate
    set of ``benchmarks`` (lists of column indices into X, at most 8), from a refit without
    it (estimators/sensitivity.py). Further scenarios: ``result.bounds(cf_y, cf_d, rho)``."""
    _linear_only(propensity, "ate_dml_irm_sensitivity")
    run = _run(run)
    with trace("ate_dml_irm_sensitivity", folds=folds):
        if _ref(run):
            from .reference import estimators as R
            return R.dml_irm_sensitivity(Y, W, X, cf_y, cf_d, rho, level, null, benchmarks,
                                         folds=folds, seed=run.seed, lambda_rule=lambda_rule,
                                         clip=clip)
        from .estimators import sensitivity as DS
        return DS.dml_irm_sensitivity(Y, W, X, cf_y, cf_d, rho, level, null, benchmarks,
                                      folds=folds, seed=run.seed, lambda_rule=lambda_rule,
                                      clip=clip, device=run.device(), dtype=run.dtype)


def ate_dml_irm_targets(Y, W, X, targets=("all", "treated", "control"), folds=5,
                        lambda_rule="min", clip=0.01, run=None, repeats=1,
                        propensity="linear") -> TargetResult:
    """The average effect of ate_dml_irm over other target populations: on the treated
    ("treated", the ATT; DoubleML IRM(score="ATTE"), grf target.sample = "treated") and on
    the controls ("control", the ATC), beside everyone ("all", the ATE of ate_dml_irm), with
    their joint covariance: ``result.contrast("treated", "control")`` tests whether the two
    effects differ (estimators/targets.py). Only the nuisances that ``targets`` need are
    fitted (the effect on the treated needs no g1, that on the controls no g0); the rows of
    the targets that were not requested are NaN. W must be binary. Repeated cross-fitting
    (``repeats`` other than 1) and group, curve and policy versions of these targets are not
    available."""
    run = _run(run)
    with trace("ate_dml_irm_targets", folds=folds):
        if _ref(run):
            from .reference import estimators as R
            return R.dml_irm_targets(Y, W, X, targets, folds=folds, seed=run.seed,
                                     lambda_rule=lambda_rule, clip=clip, repeats=repeats,
                                     propensity=propensity)
        from .estimators import targets as DT
        return DT.dml_irm_targets(Y, W, X, targets, folds=folds, seed=run.seed,
                                  lambda_rule=lambda_rule, clip=clip, device=run.device(),
                                  dtype=run.dtype, repeats=repeats, propensity=propensity)


def ate_dml_iivm(Y, W, Z, X, folds=5, lambda_rule="min", clip=0.01, always_takers=True,
                 never_takers=True, run=None, propensity="linear") -> LateResult:
    """The local average treatment effect (LATE) of the cross-fitted interactive IV model
    (DoubleML DoubleMLIIVM) with CV-LASSO nuisances: the effect of the treatment taken W on
    those whose take-up follows the binary instrument Z (the treatment assigned, e.g. an
    encouragement). The result carries the LATE, the ITT (the ate_dml_irm effect of Z on Y),
    the first stage with its t statistic, their covariance and the weak-instrument-robust
    ``result.anderson_rubin()`` set (estimators/late.py). W and Z must be binary.
    always_takers / never_takers: set False under one-sided noncompliance (DoubleML
    ``subgroups``); that nuisance is then fixed instead of fitted. Repeated cross-fitting,
    group / curve / policy / sensitivity versions and non-binary instruments are not
    available."""
    _linear_only(propensity, "ate_dml_iivm")
    run = _run(run)
    with trace("ate_dml_iivm", folds=folds):
        if _ref(run):
            from .reference import estimators as R
            return R.dml_iivm_lasso(Y, W, Z, X, folds=folds, seed=run.seed,
                                    lambda_rule=lambda_rule, clip=clip,
                                    always_takers=always_takers, never_takers=never_takers)
        from .estimators import late as DL
        return DL.dml_iivm_lasso(Y, W, Z, X, folds=folds, seed=run.seed, lambda_rule=lambda_rule,
                                 clip=clip, always_takers=always_takers,
                                 never_takers=never_takers, device=run.device(), dtype=run.dtype)


def ate_dml_apos(Y, D, X, reference=None, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                 n_boot=999, level=0.95, run=None, repeats=1, propensity="linear") -> ApoResult:
    """The mean potential outcomes of a treatment D with 2 to 8 distinct values under the
    cross-fitted interactive model (DoubleML DoubleMLAPOS, grf multi_arm_causal_forest) with
    CV-LASSO nuisances: per level c the outcome regression on the rows of that level and the
    one-vs-rest linear-probability propensity of 1{D = c}, clipped to [clip, 1 - clip]
    (estimators/apos.py). The result carries every level's mean with the joint covariance,
    ``result.contrasts(reference=)`` -- every level's effect against ``reference`` (a value of
    D; default the lowest) with pointwise bounds and a simultaneous ``level`` band from
    ``n_boot`` Gaussian draws -- and ``result.wald()``, the test that all means are equal.
    ``seed`` keys the folds and the band; ``run`` picks the backend, device and panel type.
    Repeated cross-fitting (``repeats`` other than 1), ``propensity="logit"`` and group, curve,
    policy and sensitivity versions are not available (ValueError)."""
    run = _run(run)
    with trace("ate_dml_apos", folds=folds):
        from .estimators import apos as DA
        DA.check_scope(repeats, propensity)
        if _ref(run):
            from .reference import estimators as R
            return R.dml_apos_lasso(Y, D, X, reference=reference, folds=folds, seed=seed,
                                    lambda_rule=lambda_rule, clip=clip, n_boot=n_boot, level=level)
        return DA.dml_apos_lasso(Y, D, X, reference=reference, folds=folds, seed=seed,
                                 lambda_rule=lambda_rule, clip=clip, n_boot=n_boot, level=level,
                                 device=run.device(), dtype=run.dtype)


def ate_dml_pliv(Y, D, Z, X, folds=5, seed=1991, lambda_rule="min", clusters=None, run=None,
                 repeats=1, nuisance="linear", form=None, dist=None,
                 method="DML-PLIV cross-fit (LASSO)") -> PlivResult:
    """The effect of a real treatment D (a dose, a price, a number of contacts) with an
    endogeneity problem, in the cross-fitted partially linear IV model (DoubleML
    DoubleMLPLIV, partialling-out score) with CV-LASSO nuisances E[Y|X], E[D|X] and E[Z_j|X]:
    Z is (n,) or (n, q) with 1 <= q <= 4 continuous or discrete instruments
    (estimators/pliv.py). The result carries theta with its SE and CI, the first-stage weights
    ``pi``, the homoskedastic first-stage partial F with a ``weak_instruments`` flag (F < 10),
    ``result.ar_stat(theta)`` and the weak-instrument-robust ``result.anderson_rubin()`` set.
    ``seed`` keys the folds, which are those of ate_dml; ``run`` picks the backend, device and
    panel type. ``clusters``: an (n,) vector of labels of dependent rows -- whole clusters are
    cross-fitted and the SE is cluster-robust, as ate_dml(clusters=).
    ValueError before any device work: more than 4 instruments, a constant instrument, row
    shards (``dist``), ``repeats`` other than 1, a logit ``nuisance``, a gate / cate / policy /
    sensitivity ``form``, more covariates than the pass stages in LDS; after the call:
    instruments that are collinear once X is partialled out."""
    run = _run(run)
    with trace("ate_dml_pliv", folds=folds):
        from .estimators import pliv as DP
        DP.check_scope(dist, repeats, nuisance, form)
        Zn = DP.check_instruments(Z, len(_np(Y)))
        DP.check_lds(_np(X).shape[1] if _np(X).ndim == 2 else 1, Zn.shape[1], run.dtype)
        if _ref(run):
            from .reference import estimators as R
            codes = None
            if clusters is not None:
                from .estimators import cluster as DC
                codes = DC.cluster_layout(clusters, len(Zn), folds, seed).codes
            return R.dml_pliv_lasso(Y, D, Zn, X, folds=folds, seed=seed, lambda_rule=lambda_rule,
                                    method=method, clusters=codes)
        if clusters is not None:
            return DP.dml_pliv_lasso_cluster(Y, D, Zn, X, clusters, folds=folds, seed=seed,
                                             lambda_rule=lambda_rule, method=method,
                                             device=run.device(), dtype=run.dtype)
        return DP.dml_pliv_lasso(Y, D, Zn, X, folds=folds, seed=seed, lambda_rule=lambda_rule,
                                 method=method, device=run.device(), dtype=run.dtype)


def ate_residual_balance(Y, W, X, balance: BalanceConfig | None = None,
                         method="residual_balancing", run=None) -> AteResult:
    """E14 residual_balance_ATE (ate_functions.R:393-405) -> balanceHD::residualBalance.ate."""
    run = _run(run)
    bc = balance or BalanceConfig()
    with trace("ate_residual_balance"):
        if _ref(run):
            from .reference.balance import residual_balance_ate
            return residual_balance_ate(Y, W, X, zeta=bc.zeta, alpha=bc.alpha, seed=run.seed,
                                        scale_x=bc.scale_x,
                                        allow_negative=bc.allow_negative_weights, method=method)
        from .estimators.balance import residual_balance
        return residual_balance(Y, W, X, zeta=bc.zeta, alpha=bc.alpha, seed=run.seed,
                                scale_x=bc.scale_x, method=method, device=run.device(),
                                dtype="f64" if run.dtype == "bf16" else run.dtype,
                                allow_negative=bc.allow_negative_weights)


def ate_causal_forest(Y, W, X, num_trees=2000, seed=12345, method="Causal Forest(GRF)",
                      run=None) -> AteResult:
    """E15 grf::causal_forest + estimate_average_effect (ate_replication.Rmd:250-272)."""
    run = _run(run)
    with trace("ate_causal_forest", trees=num_trees):
        if _ref(run):
            from .reference import estimators as R
            return R.causal_forest_ate(Y, W, X, num_trees=num_trees, seed=seed, method=method)
        from .estimators import forest as DF
        return DF.causal_forest_ate(Y, W, X, num_trees=num_trees, seed=seed, method=method,
                                    device=run.device(), compat=run.compat)


def ate_aipw_crossfit(Y, W, X, folds=5, learner="rf", num_trees=500, run=None, comm=None,
                      **kw) -> AteResult:
    """K-fold cross-fitted AIPW (textbook signs) with rf / glm / gbdt nuisances
    (BASELINE config 3); ``comm`` shards the forests' trees over ranks."""
    run = _run(run)
    with trace("ate_aipw_crossfit", learner=learner, folds=folds):
        from .estimators.crossfit import aipw_crossfit
        return aipw_crossfit(Y, W, X, folds=folds, learner=learner, num_trees=num_trees,
                             seed=run.seed, device=run.device() if not _ref(run) else "cpu",
                             comm=comm, **kw)


def ate_causal_forest_bootstrap(Y, W, X, num_trees=2000, B=1000, seed=12345, run=None,
                                comm=None) -> AteResult:
    """Causal-forest ATE with a B-replicate bootstrap SE sharded over ranks (config 4)."""
    run = _run(run)
    with trace("ate_causal_forest_bootstrap", trees=num_trees, B=B):
        from .estimators.crossfit import causal_forest_bootstrap
        return causal_forest_bootstrap(Y, W, X, num_trees=num_trees, B=B, seed=seed,
                                       boot_seed=run.seed,
                                       device=run.device() if not _ref(run) else "cpu",
                                       comm=comm, compat=run.compat)


# ------------------------------------------------------------------ driver
@dataclass
class Replication:
    results: list
    n_dropped: int
    n_mod: int
    tau_true: float
    seconds: dict = field(default_factory=dict)

    def frame(self):
        return results_frame(self.results)

    def table(self):
        return format_table(self.results)


def _result_arrays(r: AteResult) -> dict:
    import json
    return {"method": np.array(r.method), "vals": np.array([r.ate, r.se, r.lower_ci, r.upper_ci]),
            "diag": np.array(json.dumps(r.diagnostics, default=str))}


def _result_from(d: dict) -> AteResult:
    import json
    v = d["vals"]
    return AteResult(str(d["method"]), float(v[0]), float(v[1]), float(v[2]), float(v[3]),
                     json.loads(str(d["diag"])))


def replicate(data=None, config: ReplicateConfig | None = None, log_path=None, plot_path=None,
              verbose=False, checkpoint_dir=None) -> Replication:
    """ate_replication.Rmd end to end: oracle on the RCT sample, selection bias
    (pt=pc=0.85), then the 13 estimators on df_mod in the driver's order.

    ``checkpoint_dir``: every finished row is saved there (utils/checkpoint.py, keyed by
    the config and a fingerprint of the data); a rerun loads finished rows and computes
    only the missing ones — identical results, since every random draw is keyed by seed."""
    from .data.dgp import make_tutorial_data
    from .data.selection import apply_selection_bias
    cfg = config or ReplicateConfig()
    run = cfg.run
    if data is None:
        data = make_tutorial_data(cfg.n_obs, run.seed)
    mod, drop = apply_selection_bias(data, cfg.pt, cfg.pc, cfg.selection_compat)
    Y, W, X = mod.Y, mod.W, mod.X
    want = set(cfg.include) if cfg.include else set(METHODS)
    results, secs = [], {}
    ck, dkey = None, ""
    if checkpoint_dir is not None:
        from .utils.checkpoint import Checkpoint, fingerprint
        ck = Checkpoint(checkpoint_dir, cfg.to_dict())
        dkey = fingerprint(Y, W, X, data.Y, data.W)

    def add(label, fn):
        if label not in want:
            return None
        t0 = time.perf_counter()
        if ck is not None and ck.has(label, dkey):
            r = _result_from(ck.load(label, dkey))
        else:
            r = fn()
            if ck is not None:
                ck.save(label, dkey, **_result_arrays(r))
        secs[label] = time.perf_counter() - t0
        if verbose:
            print(f"{label:45s} {r.ate:9.4f}  ({secs[label]:.2f}s)", flush=True)
        results.append(r)
        return r

    add("oracle", lambda: ate_naive(data.Y, data.W, method="oracle", run=run))
    add("naive", lambda: ate_naive(Y, W, run=run))
    add("Direct Method", lambda: ate_ols(Y, W, X, run=run))
    cache = {}

    def p_log():
        if "log" not in cache:
            t0 = time.perf_counter()
            cache["log"] = propensity_logistic(W, X, run=run)
            secs["propensity_logistic"] = time.perf_counter() - t0
        return cache["log"]

    def p_las():
        if "las" not in cache:
            t0 = time.perf_counter()
            cache["las"] = propensity_lasso(W, X, run=run)
            secs["propensity_lasso"] = time.perf_counter() - t0
        return cache["las"]

    add("Propensity_Weighting", lambda: ate_ipw(Y, W, X, p_log(), run=run))
    add("Propensity_Regression", lambda: ate_ipw_wls(Y, W, p_log(), run=run))
    add("Propensity_Weighting_LASSOPS",
        lambda: ate_ipw(Y, W, X, p_las(), method="Propensity_Weighting_LASSOPS", run=run))
    add("Single-equation LASSO", lambda: ate_lasso_single(Y, W, X, run=run))
    add("Usual LASSO", lambda: ate_lasso(Y, W, X, run=run))
    add("Doubly Robust with Random Forest PS",
        lambda: ate_aipw_rf(Y, W, X, num_trees=cfg.dr_trees, bootstrap_se=cfg.bootstrap_se,
                            B=cfg.B, run=run))
    add("Doubly Robust with logistic regression PS",
        lambda: ate_aipw_glm(Y, W, X, bootstrap_se=cfg.bootstrap_se, B=cfg.B, run=run))
    add("Belloni et.al", lambda: ate_belloni(Y, W, X, run=run))
    add("Double Machine Learning", lambda: ate_double_ml(Y, W, X, num_trees=cfg.dml_trees, run=run))
    add("residual_balancing", lambda: ate_residual_balance(Y, W, X, cfg.balance, run=run))
    add("Causal Forest(GRF)",
        lambda: ate_causal_forest(Y, W, X, num_trees=cfg.cf_trees, seed=cfg.cf_seed, run=run))
    rep = Replication(results, len(drop), len(Y), data.tau_true, secs)
    if log_path:
        from .utils.logging import write_jsonl
        write_jsonl(log_path, results, backend=run.backend, n_obs=cfg.n_obs, n_mod=len(Y),
                    n_dropped=len(drop), seconds=secs)
    if plot_path:
        from .utils.logging import pointrange_plot
        pointrange_plot(results, plot_path, title="ATE by method (df_mod)")
    return rep


__all__ = [
    "ate_naive", "ate_ols", "propensity_logistic", "propensity_lasso", "ate_ipw", "ate_ipw_wls",
    "ate_lasso_single", "ate_lasso", "ate_aipw_rf", "ate_aipw_glm", "ate_belloni",
    "ate_double_ml", "ate_dml", "ate_dml_irm", "ate_dml_irm_gate", "ate_dml_irm_cate", "ate_dml_irm_policy", "ate_dml_irm_sensitivity", "ate_dml_irm_targets", "ate_dml_iivm", "ate_dml_apos", "ate_residual_balance", "ate_causal_forest", "replicate",
    "ate_aipw_crossfit", "ate_causal_forest_bootstrap",
    "Replication", "ApoResult", "AteResult", "CateResult", "GateResult", "PolicyTreeResult", "SensitivityResult", "TargetResult", "LateResult", "RunConfig", "ReplicateConfig", "BalanceConfig",
]
