"""Float64 CPU reference (T-ref) of every estimator in ``ate_functions.R``.

This is the parity oracle for the GPU path (R is not available here; SURVEY.md
§7.4.1). Every function takes ``(Y, W, X)`` numpy arrays and returns an
:class:`~ate_replication_causalml_amd.result.AteResult`. Reference quirks
 are reproduced under ``compat="reference"`` (default);
``compat="textbook"`` gives the intended estimator.
"""
from __future__ import annotations

import numpy as np

from ..parallel import rng
from ..result import AteResult
from . import glmnet as gn
from .linear import glm_logit, glm_predict, lm_fit


def _arr(a):
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------- E1 naive
def naive(Y, W, method="naive"):
    """``naive_ate`` (ate_functions.R:3-21): diff in means; SE uses var/(n-1) (Q2)."""
    Y, W = _arr(Y), _arr(W)
    se2 = 0.0
    means = {}
    for g in (0.0, 1.0):
        yg = Y[W == g]
        means[g] = yg.mean()
        se2 += yg.var(ddof=1) / (len(yg) - 1)
    return AteResult.make(method, means[1.0] - means[0.0], np.sqrt(se2),
                          n1=int((W == 1).sum()), n0=int((W == 0).sum()))


# ---------------------------------------------------------------- E2 OLS
def ols(Y, W, X, method="Direct Method"):
    """``ate_condmean_ols`` (ate_functions.R:25-39): lm(Y ~ covariates + W)."""
    fit = lm_fit(np.column_stack([_arr(X), _arr(W)]), _arr(Y))
    return AteResult.make(method, fit.coef[-1], fit.se[-1], rank=fit.rank)


# ---------------------------------------------------------------- E16 / E7 propensities
def propensity_logistic(W, X):
    """glm(W ~ covariates, binomial) fitted values (ate_replication.Rmd:165-168)."""
    return glm_logit(_arr(X), _arr(W)).fitted


def propensity_lasso(W, X, seed=1991, nfolds=10, fold_stream=7):
    """``prop_score_lasso`` (ate_functions.R:133-146): binomial cv.glmnet,
    predicted response at lambda.1se (Q5)."""
    cv = gn.cv_glmnet(_arr(X), _arr(W), family="binomial", nfolds=nfolds, seed=seed,
                      fold_stream=fold_stream)
    return cv.predict(_arr(X), s="lambda.1se", type="response")


# ---------------------------------------------------------------- E3 IPW
def ipw_design(Y, W, X, p, compat="reference"):
    """Regressor matrix of the SE projection in ``prop_score_weight``.

    Reference quirk (Q25): the function's ``covariates`` formal is never
    supplied by the driver (ate_replication.Rmd:169,184), so
    ``wyp_df[,covariates]`` selects *every* column of the augmented frame
    [covariates, Y, W, p, tau_hat, ps_er] (ate_functions.R:45-50), each
    multiplied by ps_er. ``compat="textbook"`` uses the covariates only."""
    Y, W, X, p = _arr(Y), _arr(W), _arr(X), _arr(p)
    ps = W - p
    tau = (W - p) * Y / (p * (1 - p))
    if compat == "reference":
        frame = np.column_stack([X, Y, W, p, tau, ps])
    else:
        frame = X
    return frame * ps[:, None], tau


def ipw(Y, W, X, p, method="Propensity_Weighting", compat="reference"):
    """``prop_score_weight`` (ate_functions.R:44-63). SE = sqrt(mean(e^2))/sqrt(N) (Q22)."""
    d, tau = ipw_design(Y, W, X, p, compat)
    e = lm_fit(d, tau).residuals
    n = len(tau)
    return AteResult.make(method, tau.mean(), np.sqrt(np.mean(e ** 2)) / np.sqrt(n))


# ---------------------------------------------------------------- E4 PS-WLS
def ipw_wls(Y, W, p, method="Propensity_Regression"):
    """``prop_score_ols`` (ate_functions.R:67-86): WLS Y ~ W, weights W/p + (1-W)/(1-p)."""
    Y, W, p = _arr(Y), _arr(W), _arr(p)
    wts = W / p + (1 - W) / (1 - p)
    fit = lm_fit(W[:, None], Y, weights=wts)
    return AteResult.make(method, fit.coef[1], fit.se[1])


# ---------------------------------------------------------------- E5 / E6 LASSO
def lasso_single(Y, W, X, seed=1991, nfolds=10, fold_stream=5, method="Single-equation LASSO"):
    """``ate_condmean_lasso`` (ate_functions.R:89-108): W unpenalised; no SE (Q4)."""
    Xw = np.column_stack([_arr(X), _arr(W)])
    pf = np.r_[np.ones(Xw.shape[1] - 1), 0.0]
    cv = gn.cv_glmnet(Xw, _arr(Y), penalty_factor=pf, nfolds=nfolds, seed=seed,
                      fold_stream=fold_stream)
    return AteResult.make(method, cv.coef()[1][-1], None, lambda_1se=cv.lambda_1se)


def lasso_usual(Y, W, X, seed=1991, nfolds=10, fold_stream=6, method="Usual LASSO"):
    """``ate_lasso`` (ate_functions.R:111-130): W penalised; no SE (Q4)."""
    Xw = np.column_stack([_arr(X), _arr(W)])
    cv = gn.cv_glmnet(Xw, _arr(Y), nfolds=nfolds, seed=seed, fold_stream=fold_stream)
    return AteResult.make(method, cv.coef()[1][-1], None, lambda_1se=cv.lambda_1se)


# ---------------------------------------------------------------- AIPW pieces (E8/E9/E10)
def aipw_point(w, y, p, mu0, mu1, compat="reference"):
    """tau_hat as written (ate_functions.R:184-186): '+' on the control term (Q7);
    ``mean(est1, na.rm=TRUE)`` drops NaN (Q23)."""
    sign = 1.0 if compat == "reference" else -1.0
    est1 = w * (y - mu1) / p + sign * (1 - w) * (y - mu0) / (1 - p)
    est2 = mu1 - mu0
    return np.nanmean(est1) + np.mean(est2)


def aipw_sandwich_se(w, y, p, mu0, mu1, tau):
    """Sandwich SE (ate_functions.R:198-199): textbook IF with '-' sign."""
    ii = (w * y) / p - mu1 * (w - p) / p - (((1 - w) * y / (1 - p)) + (mu0 * (w - p) / (1 - p))) - tau
    n = len(ii)
    return np.sqrt(np.sum(ii ** 2) * n ** -2.0)


def bootstrap_counts_matrix(n, B, seed, stream0=0):
    """(B, n) resample counts; replicate b draws rows randint(seed, P_BOOT, b, j, n)."""
    out = np.empty((B, n), dtype=np.int64)
    for b in range(B):
        out[b] = rng.bootstrap_counts(n, seed, rng.P_BOOT, stream0 + b)
    return out


def aipw_bootstrap(w, y, p, mu0, mu1, B=1000, seed=1991, compat="reference"):
    """E10 ``tau_hat_dr_est`` x B (ate_functions.R:188-195, 267-283): resample the
    FIXED nuisance predictions (no refit, Q21); SE = sd(tau_b) (n-1)."""
    sign = 1.0 if compat == "reference" else -1.0
    est1 = w * (y - mu1) / p + sign * (1 - w) * (y - mu0) / (1 - p)
    est2 = mu1 - mu0
    ok = ~np.isnan(est1)
    e1 = np.where(ok, est1, 0.0)
    n = len(w)
    taus = np.empty(B)
    for b in range(B):
        c = rng.bootstrap_counts(n, seed, rng.P_BOOT, b).astype(np.float64)
        taus[b] = (c @ e1) / (c @ ok) + (c @ est2) / n
    return float(np.std(taus, ddof=1)), taus


def _aipw_result(method, w, y, p, mu0, mu1, bootstrap_se, B, seed, compat, **diag):
    tau = aipw_point(w, y, p, mu0, mu1, compat)
    if bootstrap_se:
        se, _ = aipw_bootstrap(w, y, p, mu0, mu1, B=B, seed=seed, compat=compat)
    else:
        se = aipw_sandwich_se(w, y, p, mu0, mu1, tau)
    return AteResult.make(method, tau, se, **diag)


def outcome_logit_mu(Y, W, X, counterfactual_quirk):
    """Outcome GLM Y ~ covariates + W (Q24) and mu1/mu0 predictions.
    ``counterfactual_quirk`` (Q6): ``mutate_("W = 1")`` adds a column named
    "W = 1" and leaves W untouched, so mu1 = mu0 = mu(x, W_observed)."""
    X, W, Y = _arr(X), _arr(W), _arr(Y)
    fit = glm_logit(np.column_stack([X, W]), Y)
    if counterfactual_quirk:
        mu = glm_predict(fit, np.column_stack([X, W]))
        return mu, mu.copy()
    mu1 = glm_predict(fit, np.column_stack([X, np.ones_like(W)]))
    mu0 = glm_predict(fit, np.column_stack([X, np.zeros_like(W)]))
    return mu0, mu1


def clip_propensity(p):
    """ate_functions.R:181-182: exact 0 -> min positive, exact 1 -> max below 1."""
    p = p.copy()
    pos = p[p > 0]
    below = p[p < 1]
    if pos.size:
        p = np.where(p == 0, pos.min(), p)
    if below.size:
        p = np.where(p == 1, below.max(), p)
    return p


def aipw_glm(Y, W, X, bootstrap_se=False, B=1000, seed=1991, compat="reference",
             method="Doubly Robust with logistic regression PS"):
    """``doubly_robust_glm`` (ate_functions.R:211-264): logistic outcome and
    propensity models, no clipping (Q9)."""
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    mu0, mu1 = outcome_logit_mu(Y, W, X, counterfactual_quirk=False)
    p = propensity_logistic(W, X)
    return _aipw_result(method, W, Y, p, mu0, mu1, bootstrap_se, B, seed, compat)


def aipw_rf(Y, W, X, num_trees=100, bootstrap_se=False, B=1000, seed=1991, forest_seed=12325,
            compat="reference", method="Doubly Robust with Random Forest PS", splits="auto"):
    """``doubly_robust`` (ate_functions.R:149-207): logistic outcome model,
    random-forest OOB propensity (clipped, Q9), counterfactual quirk Q6 under
    ``compat="reference"``. ``splits``: models/forest.resolve_splits."""
    from ..models.forest import resolve_splits
    from .forest import rf_classifier_fit
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    mu0, mu1 = outcome_logit_mu(Y, W, X, counterfactual_quirk=(compat == "reference"))
    rf = rf_classifier_fit(X, W, num_trees=num_trees, seed=forest_seed,
                           splits=resolve_splits(splits, len(Y), X.shape[1]))
    p = clip_propensity(rf.oob_proba())
    return _aipw_result(method, W, Y, p, mu0, mu1, bootstrap_se, B, seed, compat,
                        n_oob_nan=int(np.isnan(rf.oob_proba()).sum()))


# ---------------------------------------------------------------- E11 Belloni
def interaction_expand(X):
    """All ordered pairwise products incl. squares (ate_functions.R:289-296, Q10)."""
    X = _arr(X)
    n, p = X.shape
    prods = (X[:, :, None] * X[:, None, :]).reshape(n, p * p)
    return np.column_stack([X, prods])


def lambda_interp(lambdas, s):
    """glmnet's ``lambda.interp`` (linear interpolation in lambda)."""
    lam = np.asarray(lambdas, float)
    k = len(lam)
    if k == 1:
        return 0, 0, 1.0
    sfrac = (lam[0] - s) / (lam[0] - lam[k - 1])
    ln = (lam[0] - lam) / (lam[0] - lam[k - 1])
    sfrac = min(max(sfrac, ln.min()), ln.max())
    coord = np.interp(sfrac, ln, np.arange(k))
    left, right = int(np.floor(coord)), int(np.ceil(coord))
    if left == right or abs(ln[left] - ln[right]) < np.finfo(float).eps:
        return left, right, 1.0
    frac = (sfrac - ln[right]) / (ln[left] - ln[right])
    return left, right, float(frac)


def coef_at(path, s):
    left, right, frac = lambda_interp(path.lambdas, s)
    a0 = path.a0[left] * frac + path.a0[right] * (1 - frac)
    b = path.beta[left] * frac + path.beta[right] * (1 - frac)
    return a0, b


def belloni_select(Xint, W, Y, seed=1991, nfolds=10, compat="reference"):
    cw = gn.cv_glmnet(Xint, W, nfolds=nfolds, seed=seed, fold_stream=8)
    cy = gn.cv_glmnet(Xint, Y, nfolds=nfolds, seed=seed, fold_stream=9)
    s = cw.lambda_min
    _, bw = coef_at(cw.fit, s)
    _, by = coef_at(cy.fit, s if compat == "reference" else cy.lambda_min)   # Q11
    if compat == "reference":
        sw = np.flatnonzero(bw > 0) + 1                     # 1-based, positive only (Q12)
        sy = np.flatnonzero(by > 0) + 1
        union = []
        for v in np.concatenate([sw, sy]):
            if v not in union:
                union.append(int(v))
        shifted = [v - 1 for v in union]                    # Q13: '- 1' shift
        cols = [v - 1 for v in shifted if v >= 1]           # R drops index 0; to 0-based
    else:
        cols = sorted(set(np.flatnonzero(bw != 0)) | set(np.flatnonzero(by != 0)))
    return cols, cw, cy


def belloni(Y, W, X, seed=1991, nfolds=10, compat="reference", method="Belloni et.al"):
    """``belloni`` (ate_functions.R:286-328): post-double-selection on 462 features."""
    Y, W = _arr(Y), _arr(W)
    Xint = interaction_expand(X)
    cols, cw, cy = belloni_select(Xint, W, Y, seed, nfolds, compat)
    fit = lm_fit(np.column_stack([Xint[:, cols], W]), Y)
    return AteResult.make(method, fit.coef[-1], fit.se[-1], n_selected=len(cols),
                          rank=fit.rank)


# ---------------------------------------------------------------- E12/E13 DML (compat)
def chernozhukov(Y, W, X, idx1, idx2, num_trees, seed=123, splits="auto"):
    """One DML half (ate_functions.R:332-369, Q14/Q15); bins from all rows."""
    from ..models import forest as F
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    splits = F.resolve_splits(splits, len(Y), X.shape[1])
    edges = F.exact_bins(X) if splits == "exact" else F.bin_edges(X)
    rf1 = F.fit_forest(X[idx1], F.KIND_CLASS, y=W[idx1], ntree=num_trees, seed=seed,
                       backend="cpu", edges=edges, splits=splits)
    rf2 = F.fit_forest(X[idx2], F.KIND_CLASS, y=Y[idx2], ntree=num_trees, seed=seed + 1,
                       backend="cpu", edges=edges, splits=splits)
    ew = rf1.predict_proba(X)
    ey = rf2.predict_proba(X)
    return resid_on_resid(Y - ey, W - ew)


def resid_on_resid(yr, wr):
    """lm(Y_resid ~ 0 + W_resid): tau, classical SE."""
    sww = wr @ wr
    tau = (wr @ yr) / sww
    rss = np.sum((yr - tau * wr) ** 2)
    se = np.sqrt(rss / (len(yr) - 1) / sww)
    return tau, se


def double_ml(Y, W, X, num_trees=100, seed=123, method="Double Machine Learning",
              splits="auto"):
    """``double_ml`` (ate_functions.R:372-389): positional 2-way split, average tau and SE."""
    n = len(Y)
    h = n // 2
    idx1, idx2 = np.arange(h), np.arange(h, n)
    t1, s1 = chernozhukov(Y, W, X, idx1, idx2, num_trees, seed, splits)
    t2, s2 = chernozhukov(Y, W, X, idx2, idx1, num_trees, seed + 2, splits)
    return AteResult.make(method, (t1 + t2) / 2, (s1 + s2) / 2)


# ---------------------------------------------------------------- E15 causal forest
def causal_forest_ate(Y, W, X, num_trees=2000, seed=12345, method="Causal Forest(GRF)",
                      nuisance_trees=None):
    """grf causal forest + AIPW ATE (ate_replication.Rmd:250-272) on the host engine."""
    from ..models import forest as F
    cf = F.causal_forest(_arr(X), _arr(Y), _arr(W), num_trees=num_trees, seed=seed,
                         nuisance_trees=nuisance_trees, backend="cpu")
    est, se = F.average_treatment_effect(cf)
    return AteResult.make(method, est, se, ate_bad=float(np.nanmean(cf.tau_oob)),
                          se_bad=float(np.sqrt(np.nanmean(cf.var_oob))))


# ---------------------------------------------------------------- cluster-robust inference
def cluster_codes(clusters):
    """(codes, J): the labels of ``clusters`` as integers 0..J-1 in sorted label order."""
    labels, codes = np.unique(np.asarray(clusters), return_inverse=True)
    return codes.reshape(-1).astype(np.int64), len(labels)


def cluster_fold_ids(clusters, folds, seed):
    """The fold of every row when whole clusters are cross-fitted: cluster j (sorted label
    order) goes to fold ``rng.fold_ids(J, folds, seed, 0)[j]`` and each of its rows with it
    (balanced over clusters, not rows; singleton clusters give the row-level folds)."""
    codes, J = cluster_codes(clusters)
    return rng.fold_ids(J, folds, seed, stream=0)[codes]


def cluster_se(a, b, theta, codes, correction):
    """The cluster-robust SE of the solution theta of sum_i (a_i - theta b_i) = 0 (b None:
    b == 1): with t_j = sum_{i in j} (a_i - theta b_i), Var = sum_j t_j^2 / (sum_i b_i)^2,
    times J / (J - 1) when ``correction`` is set (the n - 1 rule of the mean)."""
    a = _arr(a)
    b = np.ones_like(a) if b is None else _arr(b)
    codes = np.asarray(codes, dtype=np.int64)
    J = int(codes.max()) + 1
    A, B = np.zeros(J), np.zeros(J)
    np.add.at(A, codes, a)
    np.add.at(B, codes, b)
    t = A - theta * B
    var = (t * t).sum() / B.sum() ** 2
    if correction:
        var *= J / (J - 1)
    return float(np.sqrt(var))


def _cluster_diag(codes, J, se_unclustered):
    nj = np.bincount(codes, minlength=J).astype(np.float64)
    return dict(n_clusters=J, max_cluster=int(nj.max()),
                design_effect=float((nj * nj).sum() / len(codes)),
                se_unclustered=float(se_unclustered))


# ---------------------------------------------------------------- K-fold DML (north star)
def dml_plr_lasso(Y, W, X, folds=5, seed=1991, lambda_rule="min",
                  method="DML cross-fit (LASSO)", fold_ids=None, clusters=None):
    """Partially-linear DML with K-fold cross-fitting and CV-LASSO nuisances.

    For held-out fold k the nuisances E[Y|X], E[W|X] are gaussian LASSO fits on
    the other K-1 folds, with lambda chosen by (K-1)-fold CV over those same
    folds (so every Gram the GPU needs is a sum of per-fold Grams). ``fold_ids``:
    an explicit fold of every row (default: the Philox assignment). ``clusters``: (n,)
    labels -- whole clusters are cross-fitted (:func:`cluster_fold_ids`) and the SE is the
    cluster-robust one (:func:`cluster_se`, no correction)."""
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    if clusters is not None:
        fold_ids = cluster_fold_ids(clusters, folds, seed)
    fid = rng.fold_ids(len(Y), folds, seed, stream=0) if fold_ids is None else \
        np.asarray(fold_ids, dtype=np.int64)
    yr = np.empty_like(Y)
    wr = np.empty_like(W)
    for k in range(folds):
        tr = fid != k
        te = ~tr
        inner = fid[tr]
        inner = np.where(inner > k, inner - 1, inner)
        for target, out in ((Y, yr), (W, wr)):
            cv = gn.cv_glmnet(X[tr], target[tr], foldid=inner)
            s = "lambda.min" if lambda_rule == "min" else "lambda.1se"
            out[te] = target[te] - cv.predict(X[te], s=s)
    r = dml_from_residuals(yr, wr, method)
    if clusters is None:
        return r
    codes, J = cluster_codes(clusters)
    se = cluster_se(wr * yr, wr * wr, r.ate, codes, correction=False)
    return AteResult.make(method, r.ate, se, n=len(Y), **_cluster_diag(codes, J, r.se))


def _pliv_residuals(Y, D, Z, X, folds, seed, lambda_rule, fold_ids=None):
    """The held-out residuals (y~ [n], d~ [n], z~ [n, q]) of the cross-fitted partially linear
    IV model: for held-out fold k, l = E[Y|X], r = E[D|X] and m_j = E[Z_j|X] are gaussian
    LASSO fits on the other K - 1 folds with lambda chosen by (K-1)-fold CV over those folds
    (the nuisance code of dml_plr_lasso)."""
    fid = rng.fold_ids(len(Y), folds, seed, stream=0) if fold_ids is None else \
        np.asarray(fold_ids, dtype=np.int64)
    s = "lambda.min" if lambda_rule == "min" else "lambda.1se"
    targets = np.column_stack([Y, D, Z])
    res = np.empty_like(targets)
    for k in range(folds):
        tr = fid != k
        te = ~tr
        inner = fid[tr]
        inner = np.where(inner > k, inner - 1, inner)
        for c in range(targets.shape[1]):
            cv = gn.cv_glmnet(X[tr], targets[tr, c], foldid=inner)
            res[te, c] = targets[te, c] - cv.predict(X[te], s=s)
    return res[:, 0], res[:, 1], res[:, 2:]


def pliv_moments_from_residuals(yr, dr, zr):
    """The moment vector of result.PlivLayout from per-row residuals (zr: [n, q])."""
    from ..result import pliv_layout
    q = zr.shape[1]
    w = lambda a, b: (zr * (a * b)[:, None]).T @ zr
    return pliv_layout(q).pack(len(yr), yr @ yr, yr @ dr, dr @ dr, zr.T @ yr, zr.T @ dr,
                               zr.T @ zr, w(yr, yr), w(yr, dr), w(dr, dr))


def dml_pliv_lasso(Y, D, Z, X, folds=5, seed=1991, lambda_rule="min",
                   method="DML-PLIV cross-fit (LASSO)", fold_ids=None, clusters=None):
    """The cross-fitted partially linear IV estimate (Chernozhukov et al. 2018 §4.2, DoubleML
    DoubleMLPLIV, partialling-out score) with CV-LASSO nuisances, row by row in float64, the
    twin of estimators.pliv.dml_pliv_lasso: D any real treatment, Z (n,) or (n, q) instruments
    with 1 <= q <= 4. With the held-out residuals y~, d~, z~: pi = (S z~z~')^-1 S z~d~,
    v = z~ pi, theta = S v y~ / S v d~, SE = sqrt(S v^2 (y~ - theta d~)^2) / S v d~ -- taken
    from the moments of result.PlivLayout, summed over the per-row arrays here. ``clusters``:
    (n,) labels -- whole clusters are cross-fitted (:func:`cluster_fold_ids`) and the SE is
    the cluster-robust one of psi = v y~ - theta v d~ (:func:`cluster_se`, no correction)."""
    from ..result import PLIV_MAX_INSTRUMENTS, PlivResult
    Y, D, X = _arr(Y), _arr(D), _arr(X)
    Z = _arr(Z)
    Z = Z[:, None] if Z.ndim == 1 else Z
    if Z.ndim != 2 or len(Z) != len(Y) or not 1 <= Z.shape[1] <= PLIV_MAX_INSTRUMENTS:
        raise ValueError(f"Z must be (n,) or (n, q) with 1 <= q <= {PLIV_MAX_INSTRUMENTS}, got "
                         f"shape {tuple(Z.shape)}")
    for j in range(Z.shape[1]):
        if np.ptp(Z[:, j]) == 0.0:
            raise ValueError(f"instrument {j} is constant: it cannot move the treatment")
    if clusters is not None:
        fold_ids = cluster_fold_ids(clusters, folds, seed)
    yr, dr, zr = _pliv_residuals(Y, D, Z, X, folds, seed, lambda_rule, fold_ids)
    mom = pliv_moments_from_residuals(yr, dr, zr)
    r = PlivResult.from_moments(method, mom, n=len(Y), hipgraph=False)
    if r.rank_deficient:
        raise ValueError(f"the {Z.shape[1]} instrument residuals are collinear after "
                         "partialling out X")
    if clusters is None:
        return r
    codes, J = cluster_codes(clusters)
    v = zr @ np.asarray(r.pi)
    se = cluster_se(v * yr, v * dr, r.theta, codes, correction=False)
    diag = _cluster_diag(codes, J, r.se)
    diag.pop("se_unclustered")
    return PlivResult.from_moments(method, mom, se=se, n=len(Y), hipgraph=False, **diag)


PROPENSITIES = ("linear", "logit")


def check_propensity(propensity) -> str:
    """The propensity fit of the interactive model: "linear" (the linear-probability gaussian
    LASSO, clipped) or "logit" (the binomial LASSO, cv.glmnet(family="binomial"))."""
    if propensity not in PROPENSITIES:
        raise ValueError(f"propensity must be one of {PROPENSITIES}, got {propensity!r}")
    return propensity


def _irm_scores(Y, W, X, folds, seed, lambda_rule, clip, fold_ids=None, propensity="linear"):
    """The held-out nuisances and per-row AIPW scores of the cross-fitted interactive model
    (validated inputs as float64 arrays): (psi, g0, g1, m), m before clipping. propensity
    "logit": m is the predicted response of the binomial LASSO on the same training rows and
    inner folds."""
    logit = check_propensity(propensity) == "logit"
    if not np.isin(W, (0.0, 1.0)).all():
        raise ValueError("DML-IRM needs a binary treatment: W must be exactly 0 or 1")
    fid = rng.fold_ids(len(Y), folds, seed, stream=0) if fold_ids is None else \
        np.asarray(fold_ids, dtype=np.int64)
    for k in range(folds):
        for a in (0, 1):
            if not np.any((fid == k) & (W == a)):
                raise ValueError(f"empty (fold, arm) cell: fold {k}, arm W={a} has no rows")
    s = "lambda.min" if lambda_rule == "min" else "lambda.1se"
    g0 = np.empty_like(Y)
    g1 = np.empty_like(Y)
    m = np.empty_like(Y)
    for k in range(folds):
        te = fid == k
        inner = np.where(fid > k, fid - 1, fid)
        for rows, target, out in (((~te) & (W == 0), Y, g0), ((~te) & (W == 1), Y, g1),
                                  (~te, W, m)):
            family = "binomial" if logit and out is m else "gaussian"
            cv = gn.cv_glmnet(X[rows], target[rows], family=family, foldid=inner[rows])
            out[te] = cv.predict(X[te], s=s)
    e = np.clip(m, clip, 1 - clip)
    psi = g1 - g0 + W * (Y - g1) / e - (1 - W) * (Y - g0) / (1 - e)
    return psi, g0, g1, m


def dml_irm_lasso(Y, W, X, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                  method="DML-IRM cross-fit (LASSO)", fold_ids=None, propensity="linear",
                  clusters=None):
    """Cross-fitted AIPW for the interactive model (Chernozhukov et al. 2018 §5.1) with
    CV-LASSO nuisances, row by row in float64: for held-out fold k, g0 and g1 are gaussian
    LASSO fits of Y on the training rows of each arm and m is the linear-probability LASSO of
    W on all training rows, each with lambda chosen by (K-1)-fold CV over the training folds
    (as dml_plr_lasso). Score (textbook signs): psi = g1 - g0 + W (Y - g1) / m
    - (1 - W)(Y - g0) / (1 - m) with m clipped to [clip, 1 - clip]; theta = mean(psi),
    SE = sd(psi) / sqrt(n). ``clusters``: (n,) labels -- whole clusters are cross-fitted
    (:func:`cluster_fold_ids`) and the SE is the cluster-robust one (:func:`cluster_se` with
    the J / (J - 1) correction)."""
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    if clusters is not None:
        fold_ids = cluster_fold_ids(clusters, folds, seed)
    psi, g0, g1, m = _irm_scores(Y, W, X, folds, seed, lambda_rule, clip, fold_ids, propensity)
    n = len(Y)
    nt = W.sum()
    extra = {} if propensity == "linear" else {"propensity": propensity}
    se = psi.std(ddof=1) / np.sqrt(n)
    if clusters is not None:
        codes, J = cluster_codes(clusters)
        extra.update(_cluster_diag(codes, J, se))
        se = cluster_se(psi, None, psi.mean(), codes, correction=True)
    return AteResult.make(method, psi.mean(), se, n=n, **extra,
                          n_clipped=int(((m < clip) | (m > 1 - clip)).sum()),
                          n_treated=int(nt),
                          rmse_g0=float(np.sqrt(((1 - W) * (Y - g0) ** 2).sum() / (n - nt))),
                          rmse_g1=float(np.sqrt((W * (Y - g1) ** 2).sum() / nt)),
                          rmse_m=float(np.sqrt(((W - m) ** 2).mean())))


def gate_from_scores(psi, codes, n_groups, n_boot=999, level=0.95, seed=1991, row_ids=None):
    """Group means of per-row scores with the multiplier-bootstrap critical value of their
    simultaneous band, in float64: theta_g = mean, SE_g = sd / sqrt(n_g), and with Rademacher
    multipliers xi (rng.rademacher, keyed by ``row_ids``, default 0..n-1)
    t[b, g] = S_{i in g} xi_i^b (psi_i - theta_g) / (n_g SE_g), crit = the
    ceil(level n_boot)-th smallest of max_g |t[b, .]|.
    Returns (n_g, theta, se, crit, A [B, G], Z [B, G]) with A = S xi psi, Z = S xi."""
    from ..result import boot_rank
    psi = np.asarray(psi, dtype=np.float64)
    codes = np.asarray(codes, dtype=np.int64)
    G, B = int(n_groups), int(n_boot)
    rows = np.arange(len(psi)) if row_ids is None else np.asarray(row_ids)
    xi = rng.rademacher(seed, rows, B)
    ng = np.zeros(G)
    theta = np.zeros(G)
    se = np.zeros(G)
    A = np.zeros((B, G))
    Z = np.zeros((B, G), dtype=np.int64)
    t = np.zeros((B, G))
    for g in range(G):
        in_g = codes == g
        pg = psi[in_g]
        ng[g] = len(pg)
        theta[g] = pg.mean()
        se[g] = pg.std(ddof=1) / np.sqrt(len(pg))
        xg = xi[in_g].astype(np.float64)
        A[:, g] = pg @ xg
        Z[:, g] = xi[in_g].astype(np.int64).sum(axis=0)
        t[:, g] = ((pg - theta[g]) @ xg) / (ng[g] * se[g])
    crit = np.sort(np.abs(t).max(axis=1))[boot_rank(level, B) - 1]
    return ng, theta, se, float(crit), A, Z


def dml_irm_gate(Y, W, X, groups, folds=5, seed=1991, lambda_rule="min", clip=0.01, n_boot=999,
                 level=0.95, method="DML-IRM group ATEs (LASSO)", fold_ids=None,
                 keep_boot=False, propensity="linear"):
    """Group average treatment effects of the cross-fitted interactive model with a
    simultaneous confidence band (the float64 twin of estimators.gate.dml_irm_gate_lasso):
    the scores of dml_irm_lasso, averaged within the groups of ``groups`` (one per distinct
    label), and the Rademacher multiplier bootstrap of gate_from_scores."""
    from ..result import GateResult, boot_rank
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    gl = np.asarray(groups)
    if gl.ndim != 1 or len(gl) != len(Y):
        raise ValueError(f"groups must be a vector with one label per row ({len(Y)}), "
                         f"got shape {gl.shape}")
    if int(n_boot) != n_boot or not 1 <= int(n_boot) <= 4096:
        raise ValueError(f"n_boot must be an integer in [1, 4096], got {n_boot}")
    boot_rank(level, int(n_boot))
    labels, codes = np.unique(gl, return_inverse=True)
    if len(labels) > 64:
        raise ValueError(f"at most 64 groups are supported, got {len(labels)}")
    for g, c in enumerate(np.bincount(codes, minlength=len(labels))):
        if c < 2:
            raise ValueError(f"group {g} has {int(c)} row(s): every group needs at least 2")
    psi, _, _, _ = _irm_scores(Y, W, X, folds, seed, lambda_rule, clip, fold_ids, propensity)
    ng, theta, se, crit, A, Z = gate_from_scores(psi, codes, len(labels), n_boot, level, seed)
    n = len(Y)
    overall = AteResult.make("DML-IRM cross-fit (LASSO)", psi.mean(),
                             psi.std(ddof=1) / np.sqrt(n), n=n)
    res = GateResult.make(method, labels, ng, theta, se, crit, int(n_boot), level, overall)
    if keep_boot:
        res.boot = {"A": A, "Z": Z}
    return res


def _rate_grid(q):
    g = np.arange(1, 11) / 10.0 if q is None else np.asarray(q, dtype=np.float64).reshape(-1)
    if not 1 <= len(g) <= 64:
        raise ValueError(f"q must hold between 1 and 64 points, got {len(g)}")
    if not (np.isfinite(g).all() and g[0] > 0.0 and g[-1] <= 1.0 and np.all(np.diff(g) > 0)):
        raise ValueError("q must be strictly increasing in (0, 1]")
    return g


def _rate_of_sample(psi, priority, thresholds):
    """(AUTOC, QINI, TOC at the threshold priorities) of one sample, by its own tie groups:
    the distinct priorities descending, the cumulative mean of psi down to each, and the
    group-size-weighted averages of (cumulative mean - overall mean)."""
    vals, inv, cnt = np.unique(-priority, return_inverse=True, return_counts=True)
    n = len(psi)
    csum = np.cumsum(np.bincount(inv, weights=psi, minlength=len(vals)))
    k = np.cumsum(cnt)
    theta = csum[-1] / n
    gain = csum / k - theta
    autoc = (cnt * gain).sum() / n
    qini = (cnt * (k / n) * gain).sum() / n
    # rows with priority >= threshold: the groups with -priority <= -threshold
    upto = np.searchsorted(vals, -np.asarray(thresholds), side="right")
    toc = np.where(upto > 0, gain[np.maximum(upto, 1) - 1], -theta)
    return autoc, qini, toc


def rate_from_scores(psi, priority, include, q=None, level=0.95):
    """AUTOC, the Qini coefficient and the TOC curve of per-row scores under a priority rule
    (higher = first, ties enter together), with half-sample bootstrap SEs, in float64 and
    sample by sample: ``include`` [n, B] in {0, 1} picks each replicate's rows
    (rng.half_sample). A replicate takes its rows, groups them by their own distinct
    priorities, forms the cumulative means over those groups, and reads the TOC grid at the
    full sample's threshold priorities -- the ceil(u n)-th largest. SE: the sd over the
    replicates (ddof 1); crit: the ceil(level B)-th smallest of max_j |TOC_b - TOC| / SE over
    the grid points with SE > 0. Returns a dict: autoc, qini, toc [Q], entered [Q], their
    ``*_b`` replicates, ``*_se``, crit, ate, n, n_runs."""
    from ..result import boot_rank
    psi = np.asarray(psi, dtype=np.float64)
    pr = np.asarray(priority, dtype=np.float64)
    inc = np.asarray(include).astype(bool)
    g = _rate_grid(q)
    n, B = len(psi), inc.shape[1]
    desc = np.sort(pr)[::-1]
    kpos = np.clip(np.ceil(g * n - 1e-9).astype(np.int64), 1, n)
    thr = desc[kpos - 1]
    autoc, qini, toc = _rate_of_sample(psi, pr, thr)
    ab, qb, tb = np.zeros(B), np.zeros(B), np.zeros((B, len(g)))
    for b in range(B):
        rows = inc[:, b]
        ab[b], qb[b], tb[b] = _rate_of_sample(psi[rows], pr[rows], thr)
    sd = lambda x: x.std(axis=0, ddof=1) if B > 1 else np.full(x.shape[1:], np.nan)
    se_t = sd(tb)
    live = se_t > 0
    t = np.abs(tb[:, live] - toc[live]) / se_t[live]
    crit = float(np.sort(t.max(axis=1))[boot_rank(level, B) - 1]) if live.any() else 0.0
    return dict(autoc=autoc, qini=qini, toc=toc, autoc_b=ab, qini_b=qb, toc_b=tb,
                autoc_se=float(sd(ab)), qini_se=float(sd(qb)), toc_se=se_t, crit=crit,
                entered=np.array([(pr >= v).sum() for v in thr]), ate=psi.mean(), n=n,
                n_runs=len(np.unique(pr)))


def dml_irm_rate(Y, W, X, priority, q=None, subset=None, n_boot=200, level=0.95, folds=5,
                 seed=1991, lambda_rule="min", clip=0.01, method="DML-IRM RATE (LASSO)",
                 fold_ids=None, keep_boot=False, propensity="linear"):
    """The RATE of a priority rule on the scores of dml_irm_lasso (the float64 twin of
    estimators.rate.dml_irm_rate_lasso): the scores of every row, then rate_from_scores on
    the evaluation rows ``subset`` with the half samples of rng.half_sample keyed by the
    row number."""
    from ..result import RateResult
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    g = _rate_grid(q)
    if int(n_boot) != n_boot or not 1 <= int(n_boot) <= 4096:
        raise ValueError(f"n_boot must be an integer in [1, 4096], got {n_boot}")
    if np.ndim(priority) == 0:
        priority = X[:, int(priority)]
    pr = _arr(priority).reshape(-1)
    mask = np.ones(len(Y), dtype=bool) if subset is None else np.asarray(subset, dtype=bool)
    if len(pr) != len(Y) or mask.shape != (len(Y),):
        raise ValueError("priority and subset must have one entry per row")
    if mask.sum() < 128:
        raise ValueError(f"RATE needs at least 128 evaluation rows, got {int(mask.sum())}")
    if not np.isfinite(pr[mask]).all():
        raise ValueError("the priority must be finite on every evaluation row")
    psi, _, _, _ = _irm_scores(Y, W, X, folds, seed, lambda_rule, clip, fold_ids, propensity)
    rows = np.flatnonzero(mask)
    r = rate_from_scores(psi[rows], pr[rows], rng.half_sample(seed, rows, int(n_boot)), g, level)
    if r["entered"][0] < 64:
        raise ValueError(f"the first grid point q = {g[0]} enters {r['entered'][0]} rows: at "
                         "least 64 are needed")
    fin = np.concatenate([[r["ate"], r["autoc"], r["autoc_se"], r["qini"], r["qini_se"],
                           r["crit"], r["n"]], r["toc"], r["toc_se"]])
    res = RateResult.make(method, g, r["entered"], fin, r["n"], r["n_runs"], int(n_boot), level)
    if propensity != "linear":
        res.diagnostics["propensity"] = propensity
    if keep_boot:
        res.boot = {k: r[k] for k in ("autoc_b", "qini_b", "toc_b")}
    return res


def bspline_design(x, knots, degree):
    """The B-spline design matrix [n, df] of the points x on a clamped knot vector, point by
    point from the textbook recursive Cox-de Boor definition (result.bspline_row)."""
    from ..result import bspline_row
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    d = len(knots) - int(degree) - 1
    return np.array([bspline_row(v, knots, degree) for v in x]).reshape(len(x), d)


def _check_cate_basis(df, degree):
    if int(degree) != degree or not 0 <= int(degree) <= 3:
        raise ValueError(f"degree must be an integer in 0..3, got {degree}")
    if int(df) != df or not int(degree) + 1 <= int(df) <= 32:
        raise ValueError(f"df must be an integer in [degree + 1, 32] = [{int(degree) + 1}, 32], "
                         f"got {df}")


def _check_cate_knots(knots, degree):
    t = np.asarray(knots, dtype=np.float64).reshape(-1)
    _check_cate_basis(len(t) - degree - 1, degree)
    q = int(degree)
    d = len(t) - q - 1
    if not np.isfinite(t).all() or np.any(t[:q + 1] != t[0]) or np.any(t[d:] != t[-1]):
        raise ValueError("the knot vector must be finite and clamped: the boundary knots "
                         f"repeated degree + 1 = {q + 1} times")
    if not np.all(np.diff(t[q:d + 1]) > 0):
        raise ValueError("the knots are not strictly increasing (too few distinct values of "
                         f"the covariate for df = {d}, degree = {q}?): {t[q:d + 1].tolist()}")
    return t


def cate_from_scores(psi, x, knots, degree, grid, n_boot=999, level=0.95, seed=1991,
                     row_ids=None):
    """The projection of per-row scores on a B-spline basis of x with the multiplier-bootstrap
    critical value of the curve's uniform band, in float64 (the twin of estimators/cate.py):
    beta = (S b b')^-1 S b psi, the HC0 covariance Omega = M^-1 (S e^2 b b') M^-1 with
    e = psi - b' beta, cate = g' beta and se = sqrt(g' Omega g) at the grid's basis rows g,
    and with Rademacher multipliers xi (rng.rademacher, keyed by ``row_ids``, default 0..n-1)
    t[b, j] = g_j' M^-1 S xi^b e b / se_j, crit = the ceil(level n_boot)-th smallest of
    max_j |t[b, .]|. Returns a dict: cate, se, crit, beta, cov, M, meat, T [B, df],
    span_counts."""
    from ..result import boot_rank
    psi = np.asarray(psi, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(knots, dtype=np.float64)
    q, B = int(degree), int(n_boot)
    d = len(t) - q - 1
    Bm = bspline_design(x, t, q)
    G = bspline_design(grid, t, q)
    rows = np.arange(len(psi)) if row_ids is None else np.asarray(row_ids)
    M = Bm.T @ Bm
    beta = np.linalg.solve(M, Bm.T @ psi)
    EB = Bm * (psi - Bm @ beta)[:, None]
    meat = EB.T @ EB
    Minv = np.linalg.inv(M)
    cov = Minv @ meat @ Minv
    cate = G @ beta
    se = np.sqrt(np.einsum("jk,kl,jl->j", G, cov, G))
    T = np.zeros((B, d))
    for i0 in range(0, len(psi), 8192):
        sl = slice(i0, i0 + 8192)
        T += rng.rademacher(seed, rows[sl], B).T.astype(np.float64) @ EB[sl]
    tstat = (T @ Minv @ G.T) / se
    crit = np.sort(np.abs(tstat).max(axis=1))[boot_rank(level, B) - 1]
    span = np.searchsorted(t[q + 1:d], x, side="right")
    return dict(cate=cate, se=se, crit=float(crit), beta=beta, cov=cov, M=M, meat=meat, T=T,
                span_counts=np.bincount(span, minlength=d - q))


def dml_irm_cate(Y, W, X, by, df=5, degree=3, knots=None, grid=None, n_boot=999, level=0.95,
                 folds=5, seed=1991, lambda_rule="min", clip=0.01,
                 method="DML-IRM CATE curve (LASSO)", fold_ids=None, keep_boot=False,
                 propensity="linear"):
    """The CATE curve of the cross-fitted interactive model along one covariate with a uniform
    confidence band (the float64 twin of estimators.cate.dml_irm_cate_lasso): the scores of
    dml_irm_lasso projected on a B-spline basis of ``by`` (a column index into X, or an (n,)
    vector) by cate_from_scores. Default knots: the order statistics at rank k n / (df -
    degree) between min and max; default grid: 100 equally spaced points between the 5 % and
    95 % order statistics."""
    from ..result import CateResult, boot_rank
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    if int(n_boot) != n_boot or not 1 <= int(n_boot) <= 4096:
        raise ValueError(f"n_boot must be an integer in [1, 4096], got {n_boot}")
    boot_rank(level, int(n_boot))
    if np.ndim(by) == 0:
        if int(by) != by or not 0 <= int(by) < X.shape[1]:
            raise ValueError(f"by must index the {X.shape[1]} columns of X, got {by}")
        x = X[:, int(by)].copy()
    else:
        x = _arr(by).reshape(-1)
        if len(x) != len(Y):
            raise ValueError(f"by must be a vector with one value per row ({len(Y)}), "
                             f"got shape {np.shape(by)}")
    xs = np.sort(x)
    n = len(x)
    if knots is None:
        _check_cate_basis(df, degree)
        q = int(degree)
        bins = int(df) - q
        inner = xs[[(k * n) // bins for k in range(1, bins)]]
        knots = np.concatenate([[xs[0]] * (q + 1), inner, [xs[-1]] * (q + 1)])
    t = _check_cate_knots(knots, degree)
    q = int(degree)
    d = len(t) - q - 1
    if xs[0] < t[0] or xs[-1] > t[-1]:
        raise ValueError(f"the boundary knots [{t[0]}, {t[-1]}] must contain every x "
                         f"([{xs[0]}, {xs[-1]}])")
    if grid is None:
        grid = np.linspace(xs[(5 * n) // 100], xs[min((95 * n) // 100, n - 1)], 100)
    grid = np.asarray(grid, dtype=np.float64).reshape(-1)
    if not 1 <= len(grid) <= 512:
        raise ValueError(f"the grid must have between 1 and 512 points, got {len(grid)}")
    if not (np.isfinite(grid).all() and grid.min() >= t[0] and grid.max() <= t[-1]):
        raise ValueError(f"grid points must lie inside [min x, max x] = [{t[0]}, {t[-1]}]")
    for s, c in enumerate(np.bincount(np.searchsorted(t[q + 1:d], x, side="right"),
                                      minlength=d - q)):
        if c < 2:
            raise ValueError(f"span {s} of the knot vector has {int(c)} row(s): every span "
                             "needs at least 2")
    psi, _, _, _ = _irm_scores(Y, W, X, folds, seed, lambda_rule, clip, fold_ids, propensity)
    r = cate_from_scores(psi, x, t, q, grid, n_boot, level, seed)
    overall = AteResult.make("DML-IRM cross-fit (LASSO)", psi.mean(),
                             psi.std(ddof=1) / np.sqrt(n), n=n)
    res = CateResult.make(method, grid, r["cate"], r["se"], r["crit"], r["beta"], r["cov"], t, q,
                          int(n_boot), level, overall,
                          span_counts=[int(c) for c in r["span_counts"]])
    if keep_boot:
        res.boot = {"T": r["T"], "M": r["M"], "meat": r["meat"]}
    return res


def policy_tree_from_scores(r, Xf, edges, train=None, depth=2, min_leaf=1):
    """The exact policy tree of depth <= 2 on per-row scores r over the feature columns Xf
    (n, d) with split points ``edges`` (per feature, ascending), by brute force over row
    masks -- written from the definitions of estimators/policy.py, sharing no code with its
    histogram / prefix-sum search. The scores are quantised to integers q = rint(r 2^e)
    (e = min(30, 61 - bit_length(n) - x), max|r| = m 2^x), a leaf with sum S is worth
    max(S, 0) and treats iff S > 0, a node takes the best of staying a leaf and every split
    (j, t) (x_j < edges[j][t] goes left) that keeps ``min_leaf`` training rows on each side;
    the first best candidate in the order leaf, (j, t) ascending wins.
    Returns (rec [16] ints as the kernels' tree record, fin [2][20] as policy_finalize, e)."""
    import math
    r = np.asarray(r, dtype=np.float64)
    Xf = np.asarray(Xf, dtype=np.float64).reshape(len(r), -1)
    n, d = Xf.shape
    tr = np.ones(n, dtype=bool) if train is None else np.asarray(train, dtype=bool)
    ok = np.isfinite(r)
    e = min(30, 61 - n.bit_length() - math.frexp(np.abs(r[ok]).max() if ok.any() else 0.0)[1])
    q = np.rint(np.ldexp(np.where(ok, r, 0.0), e)).astype(np.int64)
    goes_left = {(j, t): Xf[:, j] < edges[j][t] for j in range(d) for t in range(len(edges[j]))}

    def best(rows, k):
        S = int(q[rows].sum())
        value, tree = max(S, 0), {"split": None, "action": int(S > 0)}
        if k == 0:
            return value, tree
        for (j, t), lt in goes_left.items():          # insertion order: (j, t) ascending
            lo, hi = rows & lt, rows & ~lt
            if lo.sum() < min_leaf or hi.sum() < min_leaf:
                continue
            vl, tl = best(lo, k - 1)
            vh, th = best(hi, k - 1)
            if vl + vh > value:
                value, tree = vl + vh, {"split": (j, t), "lo": tl, "hi": th}
        return value, tree

    value, tree = best(tr, int(depth))
    rec = [-1] * 6 + [0] * 4 + [value, int(tr.sum()), 0, 0, 0, 0]
    pi = np.zeros(n, dtype=np.int64)
    slot = np.zeros(n, dtype=np.int64)
    if tree["split"] is None:
        rec[6:10] = [tree["action"]] * 4
        pi[:] = tree["action"]
    else:
        rec[0:2] = tree["split"]
        right = ~goes_left[tree["split"]]
        for side, sub in enumerate((tree["lo"], tree["hi"])):
            here = right == bool(side)
            if sub["split"] is None:
                rec[6 + 2 * side:8 + 2 * side] = [sub["action"]] * 2
                pi[here] = sub["action"]
                slot[here] = 2 * side
            else:
                rec[2 + 2 * side:4 + 2 * side] = sub["split"]
                up = ~goes_left[sub["split"]]
                for cs, leaf in enumerate((sub["lo"], sub["hi"])):
                    rec[6 + 2 * side + cs] = leaf["action"]
                    pi[here & (up == bool(cs))] = leaf["action"]
                    slot[here & (up == bool(cs))] = 2 * side + cs

    def mean_se(v):
        if len(v) == 0:
            return [np.nan, np.nan]
        return [v.mean(), v.std(ddof=1) / np.sqrt(len(v)) if len(v) > 1 else np.nan]

    fin = []
    for rows in (tr, ~tr):
        rr, pp = r[rows], pi[rows]
        row = mean_se(pp * rr) + mean_se(rr) + mean_se((pp - 1) * rr)
        row += [pp.mean() if len(pp) else np.nan, float(len(rr))]
        for s in range(4):
            v = rr[slot[rows] == s]
            row += [float(len(v))] + mean_se(v)
        fin.append(row)
    fin = np.asarray(fin, dtype=np.float64)
    if not ok.all():
        fin[:] = np.nan
    return rec, fin, e


def dml_irm_policy_tree(Y, W, X, features, depth=2, bins=32, min_leaf=1, cost=0.0, train=None,
                        folds=5, seed=1991, lambda_rule="min", clip=0.01,
                        method="DML-IRM policy tree (LASSO)", fold_ids=None,
                        propensity="linear"):
    """The exact policy tree on the AIPW scores of the cross-fitted interactive model (the
    float64 twin of estimators.policy.dml_irm_policy_lasso): the scores of dml_irm_lasso less
    ``cost``, the columns ``features`` of X cut at every distinct value but the smallest (at
    most ``bins`` distinct values) or at the order statistics of rank k n / bins, and the
    brute-force search of policy_tree_from_scores."""
    from ..result import PolicyTreeResult
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    if depth not in (0, 1, 2):
        raise ValueError(f"depth must be 0, 1 or 2, got {depth}")
    if int(bins) != bins or not 2 <= int(bins) <= 64:
        raise ValueError(f"bins must be an integer in [2, 64], got {bins}")
    if int(min_leaf) != min_leaf or int(min_leaf) < 1:
        raise ValueError(f"min_leaf must be an integer >= 1, got {min_leaf}")
    f = np.asarray(features).reshape(-1)
    if not 1 <= len(f) <= 32:
        raise ValueError(f"between 1 and 32 features are supported, got {len(f)}")
    if not np.all(f == np.floor(f)) or f.min() < 0 or f.max() >= X.shape[1]:
        raise ValueError(f"features must index the {X.shape[1]} columns of X, got {list(f)}")
    f = [int(v) for v in f]
    if len(set(f)) != len(f):
        raise ValueError(f"features must be distinct, got {f}")
    n = len(Y)
    tr = None
    if train is not None:
        tr = np.asarray(train)
        if tr.shape != (n,) or tr.dtype != np.bool_:
            raise ValueError(f"train must be a boolean mask with one entry per row ({n})")
        if not tr.any():
            raise ValueError("the train mask leaves no training rows")
    edges = []
    for j in f:
        u = np.unique(X[:, j])
        if len(u) <= bins:
            edges.append(u[1:])
        else:
            xs = np.sort(X[:, j])
            edges.append(np.unique([xs[(k * n) // int(bins)] for k in range(1, int(bins))]))
    psi, _, _, _ = _irm_scores(Y, W, X, folds, seed, lambda_rule, clip, fold_ids, propensity)
    rec, fin, e = policy_tree_from_scores(psi - float(cost), X[:, f], edges, tr, depth, min_leaf)
    return PolicyTreeResult.make(method, rec, fin, f, edges, float(cost), int(depth),
                                 held_out=train is not None, hipgraph=False, e=int(e),
                                 min_leaf=int(min_leaf), bins=int(bins))


def sensitivity_from_rows(psi, b, c, cf_y=0.03, cf_d=0.03, rho=1.0, level=0.95, null=0.0):
    """The sensitivity figures of per-row (psi, b, c), row by row in float64 -- written
    independently of the moment route of result.SensitivityResult: the SEs are
    np.std(ddof=1) of the bound's influence function psi - theta -/+ k pmb, and RV / RVa
    are found by bisection on cf. Returns (theta, se, sigma2, nu2, SensBounds, rv, rva)."""
    from statistics import NormalDist
    from ..result import SensBounds, check_scenario
    from ..utils.guards import NumericalError
    check_scenario(cf_y, cf_d, rho, level)
    psi, b, c = (np.asarray(v, dtype=np.float64) for v in (psi, b, c))
    n = len(psi)
    theta, sigma2, nu2 = psi.mean(), b.mean(), c.mean()
    if not (sigma2 > 0 and nu2 > 0):
        raise NumericalError(f"sensitivity analysis needs sigma2 > 0 and nu2 > 0, got "
                             f"sigma2 = {sigma2}, nu2 = {nu2}")
    S = np.sqrt(sigma2 * nu2)
    pmb = (sigma2 * (c - nu2) + nu2 * (b - sigma2)) / (2 * S)
    z = NormalDist().inv_cdf(level)

    def at(cy, cd, r=rho):
        k = abs(r) * np.sqrt(cy) * np.sqrt(cd / (1 - cd))
        lo, hi = theta - S * k, theta + S * k
        se_lo = (psi - theta - k * pmb).std(ddof=1) / np.sqrt(n)
        se_hi = (psi - theta + k * pmb).std(ddof=1) / np.sqrt(n)
        return SensBounds(float(cy), float(cd), float(r), float(level), float(lo), float(hi),
                          float(se_lo), float(se_hi), float(lo - z * se_lo),
                          float(hi + z * se_hi))

    up = theta >= null

    def gap(cf, ci):
        """Signed distance from the (confidence) bound on the null's side to the null."""
        s = at(cf, cf)
        if up:
            return (s.ci_lower if ci else s.theta_lower) - null
        return null - (s.ci_upper if ci else s.theta_upper)

    def root(ci):
        if gap(0.0, ci) <= 0:
            return 0.0
        lo, hi = 0.0, 1.0 - 2.0 ** -40
        if gap(hi, ci) > 0:
            return 1.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if gap(mid, ci) > 0 else (lo, mid)
        return 0.5 * (lo + hi)

    return (float(theta), float(psi.std(ddof=1) / np.sqrt(n)), float(sigma2), float(nu2),
            at(cf_y, cf_d), root(False), root(True))


def _sens_rows(Y, W, X, folds, seed, lambda_rule, clip, fold_ids=None):
    """(psi, b, c, m) per row of the cross-fitted interactive model, m before clipping."""
    psi, g0, g1, m = _irm_scores(Y, W, X, folds, seed, lambda_rule, clip, fold_ids)
    e = np.clip(m, clip, 1 - clip)
    b = (Y - np.where(W == 1, g1, g0)) ** 2
    rr = W / e - (1 - W) / (1 - e)
    c = 2 * (1 / e + 1 / (1 - e)) - rr ** 2
    return psi, b, c, m


def dml_irm_sensitivity(Y, W, X, cf_y=0.03, cf_d=0.03, rho=1.0, level=0.95, null=0.0,
                        benchmarks=None, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                        method="DML-IRM sensitivity (LASSO)", fold_ids=None):
    """Sensitivity of the cross-fitted IRM's ATE to unobserved confounding (Chernozhukov,
    Cinelli, Newey, Sharma & Syrgkanis 2022), the float64 twin of
    estimators.sensitivity.dml_irm_sensitivity: per-row arrays from _irm_scores,
    sensitivity_from_rows for the bounds and robustness values, and for every benchmark set
    a second _irm_scores run on the other columns (same folds, same clip)."""
    from ..result import SensBenchmark, SensitivityResult, check_benchmarks, check_scenario
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    check_scenario(cf_y, cf_d, rho, level)
    bench = check_benchmarks(benchmarks, X.shape[1])
    psi, b, c, m = _sens_rows(Y, W, X, folds, seed, lambda_rule, clip, fold_ids)
    theta, se, sigma2, nu2, scen, rv, rva = sensitivity_from_rows(psi, b, c, cf_y, cf_d, rho,
                                                                  level, null)
    n = len(Y)
    rows = []
    var_y = Y.var()
    for cols in bench:
        kept = [j for j in range(X.shape[1]) if j not in cols]
        ps, bs, cs, _ = _sens_rows(Y, W, X[:, kept], folds, seed, lambda_rule, clip, fold_ids)
        th_s, s2_s, nu_s = ps.mean(), bs.mean(), cs.mean()
        r2_long, r2_short = 1 - sigma2 / var_y, 1 - s2_s / var_y
        cy_raw = (r2_long - r2_short) / (1 - r2_long)
        cd_raw = (nu2 - nu_s) / nu_s
        delta = th_s - theta
        var_g, var_riesz = s2_s - sigma2, nu2 - nu_s
        r = float(np.sign(delta) * min(abs(delta) / np.sqrt(var_g * var_riesz), 1.0)) \
            if var_g > 0 and var_riesz > 0 else float("nan")
        rows.append(SensBenchmark(cols, float(np.clip(cy_raw, 0, 1)), float(np.clip(cd_raw, 0, 1)),
                                  r, float(delta), float(cy_raw), float(cd_raw), float(th_s),
                                  float(s2_s), float(nu_s)))
    one = np.ones(n)
    out = ((m < clip) | (m > 1 - clip)).astype(np.float64)
    mom = [v.sum() for v in (psi, psi * psi, one, out, b, b * b, c, c * c, psi * b, psi * c,
                             b * c, Y, Y * Y, W)]
    diag = dict(n=n, n_clipped=int(out.sum()), n_treated=int(W.sum()))
    return SensitivityResult(method, [float(v) for v in mom], theta, se, sigma2, nu2, scen,
                             float(null), rv, rva, rows, diag)


def targets_from_rows(y, w, g0, g1, m, clip):
    """The effects over everyone, on the treated and on the controls with their joint
    covariance from per-row held-out nuisances (m before clipping), row by row in float64 --
    written independently of the moment route of result.TargetResult: per-row influence
    vectors and ``phi @ phi.T``, no closed forms. Returns (theta [3], cov [3, 3]) in the
    order (all, treated, control). With e the clipped propensity:

        a = w (y - g0) - e (1 - w)(y - g0) / (1 - e)        theta_treated = sum(a) / n1
        c = -(1 - w)(y - g1) + (1 - e) w (y - g1) / e       theta_control = sum(c) / n0
        psi = g1 - g0 + w (y - g1) / e - (1 - w)(y - g0) / (1 - e)   theta_all = mean(psi)
        phi = [psi - theta_all, (a - theta_treated w) / p1, (c - theta_control (1 - w)) / p0]
        cov = phi phi' / (n - 1) / n

    (the ATTE score of DoubleML's IRM: psi_a theta + psi_b with J = -1; p1 = n1 / n)."""
    y, w, g0, g1, m = (np.asarray(v, dtype=np.float64) for v in (y, w, g0, g1, m))
    n = len(y)
    n1 = w.sum()
    n0 = n - n1
    e = np.clip(m, clip, 1 - clip)
    psi = g1 - g0 + w * (y - g1) / e - (1 - w) * (y - g0) / (1 - e)
    a = w * (y - g0) - e * ((1 - w) * (y - g0) / (1 - e))
    c = -(1 - w) * (y - g1) + (1 - e) * (w * (y - g1) / e)
    theta = np.array([psi.mean(), a.sum() / n1, c.sum() / n0])
    phi = np.stack([psi - theta[0], (a - theta[1] * w) / (n1 / n),
                    (c - theta[2] * (1 - w)) / (n0 / n)])
    return theta, phi @ phi.T / (n - 1) / n


def dml_irm_targets(Y, W, X, targets=("all", "treated", "control"), folds=5, seed=1991,
                    lambda_rule="min", clip=0.01, method="DML-IRM target populations (LASSO)",
                    fold_ids=None, repeats=1, propensity="linear"):
    """The average effect of the cross-fitted interactive model over everyone, on the
    treated (ATT) and on the controls (ATC) with their joint covariance, the float64 twin of
    estimators.targets.dml_irm_targets: per-row nuisances from _irm_scores (all three are
    always fitted here), targets_from_rows for the estimates. The rows of the targets that
    were not requested are NaN. Repeated cross-fitting of these targets is out of scope."""
    from ..result import TargetResult, check_targets
    targets = check_targets(targets)
    if repeats != 1:
        raise ValueError("repeated cross-fitting is not available for the target populations: "
                         "repeats must be 1")
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    _, g0, g1, m = _irm_scores(Y, W, X, folds, seed, lambda_rule, clip, fold_ids, propensity)
    theta, cov = targets_from_rows(Y, W, g0, g1, m, clip)
    return TargetResult.from_estimates(method, theta, cov, targets, n=len(Y),
                                       n_treated=int(W.sum()),
                                       n_clipped=int(((m < clip) | (m > 1 - clip)).sum()),
                                       hipgraph=False)


def _iivm_scores(Y, D, Z, X, folds, seed, lambda_rule, clip, always_takers, never_takers,
                 fold_ids=None):
    """The held-out nuisances and the two per-row AIPW scores of the cross-fitted interactive
    IV model (validated inputs as float64 arrays), in the shape of _irm_scores with the
    instrument Z splitting the rows: (b, a, g0, g1, r0, r1, m), m before clipping. Without
    always-takers r0 = 0, without never-takers r1 = 1: fixed, not fitted."""
    for name, v in (("treatment W", D), ("instrument Z", Z)):
        if not np.isin(v, (0.0, 1.0)).all():
            raise ValueError(f"DML-IIVM needs a binary {name}: it must be exactly 0 or 1")
    fid = rng.fold_ids(len(Y), folds, seed, stream=0) if fold_ids is None else \
        np.asarray(fold_ids, dtype=np.int64)
    for k in range(folds):
        for z in (0, 1):
            if not np.any((fid == k) & (Z == z)):
                raise ValueError(f"empty (fold, arm) cell: fold {k}, arm W={z} has no rows")
    for z, (flag, name) in enumerate(((always_takers, "always_takers"),
                                      (never_takers, "never_takers"))):
        for k in range(folds):
            cell = D[(fid == k) & (Z == z)]
            if not flag:
                if np.any(cell == 1 - z):
                    raise ValueError(f"{name}=False needs D = {z} wherever Z = {z}: fold {k} has "
                                     f"{int((cell == 1 - z).sum())} rows with Z={z}, D={1 - z}; "
                                     f"set {name}=True")
                continue
            for d in (0, 1):
                if not np.any(cell == d):
                    raise ValueError(f"empty (fold, Z, D) cell: fold {k}, Z={z}, D={d} has no "
                                     f"rows, so r{z} = E[D|Z={z},X] cannot be fitted; set "
                                     f"{name}=False if D = {z} wherever Z = {z}")
    s = "lambda.min" if lambda_rule == "min" else "lambda.1se"
    g0, g1, m = np.empty_like(Y), np.empty_like(Y), np.empty_like(Y)
    r0, r1 = np.zeros_like(Y), np.ones_like(Y)
    for k in range(folds):
        te = fid == k
        inner = np.where(fid > k, fid - 1, fid)
        fits = [((~te) & (Z == 0), Y, g0), ((~te) & (Z == 1), Y, g1), (~te, Z, m)]
        if always_takers:
            fits.append(((~te) & (Z == 0), D, r0))
        if never_takers:
            fits.append(((~te) & (Z == 1), D, r1))
        for rows, target, out in fits:
            cv = gn.cv_glmnet(X[rows], target[rows], foldid=inner[rows])
            out[te] = cv.predict(X[te], s=s)
    e = np.clip(m, clip, 1 - clip)
    b = g1 - g0 + Z * (Y - g1) / e - (1 - Z) * (Y - g0) / (1 - e)
    a = r1 - r0 + Z * (D - r1) / e - (1 - Z) * (D - r0) / (1 - e)
    return b, a, g0, g1, r0, r1, m


def dml_iivm_lasso(Y, W, Z, X, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                   always_takers=True, never_takers=True,
                   method="DML-IIVM cross-fit LATE (LASSO)", fold_ids=None):
    """The LATE of the cross-fitted interactive IV model (Chernozhukov et al. 2018 §5.2,
    DoubleML DoubleMLIIVM) with CV-LASSO nuisances, row by row in float64, the twin of
    estimators.late.dml_iivm_lasso: W is the treatment taken, Z the binary instrument. For
    held-out fold k, g_z and r_z are gaussian LASSO fits of Y and of W on the training rows
    with Z = z and m is the linear-probability LASSO of Z on all training rows, each with
    lambda chosen by (K-1)-fold CV over the training folds (as dml_irm_lasso). With b the
    AIPW score of Y and a that of W, both split by Z over the clipped m: theta = sum(b) /
    sum(a), SE = sd((b - theta a) / mean(a)) / sqrt(n). The 15 sums of result.LATE_MOMENTS
    are taken over the per-row arrays here."""
    from ..result import LateResult
    Y, D, Z, X = _arr(Y), _arr(W), _arr(Z), _arr(X)
    b, a, g0, g1, r0, r1, m = _iivm_scores(Y, D, Z, X, folds, seed, lambda_rule, clip,
                                           bool(always_takers), bool(never_takers), fold_ids)
    n = len(Y)
    mom = [b.sum(), (b * b).sum(), float(n), float(((m < clip) | (m > 1 - clip)).sum()),
           a.sum(), (a * a).sum(), (a * b).sum(), Z.sum(), (Z * D).sum(), ((1 - Z) * D).sum(),
           (Z * (Y - g1) ** 2).sum(), ((1 - Z) * (Y - g0) ** 2).sum(),
           (Z * (D - r1) ** 2).sum(), ((1 - Z) * (D - r0) ** 2).sum(), ((Z - m) ** 2).sum()]
    return LateResult.from_moments(method, mom, n=n, hipgraph=False)


def _apos_scores(Y, D, X, folds, seed, lambda_rule, clip, fold_ids=None):
    """The held-out nuisances and the per-row potential-outcome scores of a multi-valued
    treatment (validated inputs as float64 arrays), in the shape of _irm_scores: (psi [n, L],
    values [L], level [n], g [n, L], m [n, L]), m before clipping. g_c is fitted on the
    training rows with D = values[c], m_c on all training rows with the target 1{D = c}."""
    if not np.isfinite(D).all():
        raise ValueError("DML-APOS needs a finite treatment: D has NaN or infinite values")
    values, level = np.unique(D, return_inverse=True)
    level = level.reshape(-1)
    L = len(values)
    if not 2 <= L <= 8:
        raise ValueError(f"DML-APOS needs between 2 and 8 treatment levels, D has {L} distinct "
                         f"value{'' if L == 1 else 's'}")
    fid = rng.fold_ids(len(Y), folds, seed, stream=0) if fold_ids is None else \
        np.asarray(fold_ids, dtype=np.int64)
    for k in range(folds):
        for c in range(L):
            if not np.any((fid == k) & (level == c)):
                raise ValueError(f"empty (fold, level) cell: fold {k}, level D={values[c]:g} has "
                                 "no rows")
    s = "lambda.min" if lambda_rule == "min" else "lambda.1se"
    n = len(Y)
    g, m = np.empty((n, L)), np.empty((n, L))
    for k in range(folds):
        te = fid == k
        inner = np.where(fid > k, fid - 1, fid)
        for c in range(L):
            rows = (~te) & (level == c)
            cv = gn.cv_glmnet(X[rows], Y[rows], foldid=inner[rows])
            g[te, c] = cv.predict(X[te], s=s)
            cv = gn.cv_glmnet(X[~te], (level[~te] == c).astype(np.float64), foldid=inner[~te])
            m[te, c] = cv.predict(X[te], s=s)
    own = np.arange(n)
    e = np.clip(m[own, level], clip, 1 - clip)
    psi = g.copy()
    psi[own, level] += (Y - g[own, level]) / e
    return psi, values, level, g, m


def dml_apos_lasso(Y, D, X, reference=None, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                   n_boot=999, level=0.95, method="DML-APOS cross-fit (LASSO)", fold_ids=None,
                   keep_scores=False):
    """The mean potential outcomes of a treatment with 2 to 8 distinct values under the
    cross-fitted interactive model (DoubleML DoubleMLAPOS) with CV-LASSO nuisances, row by row
    in float64, the twin of estimators.apos.dml_apos_lasso: psi_c = g_c + 1{D = c}(Y - g_c) /
    clip(m_c), theta = the column means of psi [n, L], Cov = phi' phi / (n - 1) / n with phi
    the centred scores. The per-level diagnostics are taken over the per-row arrays here;
    ``keep_scores`` leaves psi in the result's ``scores``."""
    from ..result import ApoResult
    Y, D, X = _arr(Y), _arr(D), _arr(X)
    psi, values, lev, g, m = _apos_scores(Y, D, X, folds, seed, lambda_rule, clip, fold_ids)
    n, L = psi.shape
    own = np.arange(n)
    m_own, g_own = m[own, lev], g[own, lev]
    out = (m_own < clip) | (m_own > 1 - clip)
    e = np.clip(m_own, clip, 1 - clip)
    n_c = np.bincount(lev, minlength=L)
    res = ApoResult.from_scores(
        method, psi, [float(v) for v in values], reference=reference, seed=seed, n_boot=n_boot,
        level=level, n=n, hipgraph=False, n_c=[int(v) for v in n_c],
        n_clipped_c=[int(v) for v in np.bincount(lev, weights=out, minlength=L)],
        rmse_g_c=[float(v) for v in np.sqrt(np.bincount(lev, weights=(Y - g_own) ** 2,
                                                        minlength=L) / n_c)],
        ipw_c=[float(v) for v in np.bincount(lev, weights=1.0 / e, minlength=L) / n])
    if keep_scores:
        res.scores = psi
    return res


def dml_plr_lasso_repeated(Y, W, X, folds=5, repeats=3, seed=1991, lambda_rule="min",
                           aggregate="median", method="DML cross-fit (LASSO, repeated)"):
    """Repeated cross-fitting (Chernozhukov et al. 2018 §3.4, median method): S = repeats
    K-fold partitions built from K*K micro-groups (group m = K a + b of a balanced Philox
    assignment; partition s puts it in fold (a + s b) mod K), one DML fit per partition,
    theta = median(theta_s), SE^2 = median(SE_s^2 + (theta_s - theta)^2) ("mean": means)."""
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    micro = rng.fold_ids(len(Y), folds * folds, seed, stream=0)
    a, b = np.divmod(micro, folds)
    th, se = [], []
    for s in range(repeats):
        r = dml_plr_lasso(Y, W, X, folds, seed, lambda_rule, method, fold_ids=(a + s * b) % folds)
        th.append(r.ate)
        se.append(r.se)
    th, se = np.array(th), np.array(se)
    agg = np.median if aggregate == "median" else np.mean
    t = float(agg(th))
    return AteResult.make(method, t, float(np.sqrt(agg(se * se + (th - t) ** 2))),
                          n=len(Y), repeats=repeats, splits=np.stack([th, se], 1).tolist())


def dml_irm_lasso_repeated(Y, W, X, folds=5, repeats=3, seed=1991, lambda_rule="min", clip=0.01,
                           aggregate="median", method="DML-IRM cross-fit (LASSO, repeated)"):
    """Repeated cross-fitting of the interactive model: S = repeats calls of the row-by-row
    dml_irm_lasso on the partitions of dml_plr_lasso_repeated (K*K micro-groups, partition s
    puts group m = K a + b in fold (a + s b) mod K), aggregated in the same way."""
    Y, W, X = _arr(Y), _arr(W), _arr(X)
    if not 1 <= repeats <= folds:
        raise ValueError(f"repeats must be in 1..{folds} (distinct partitions of K*K micro-groups)")
    micro = rng.fold_ids(len(Y), folds * folds, seed, stream=0)
    a, b = np.divmod(micro, folds)
    rs = []
    for s in range(repeats):
        try:
            rs.append(dml_irm_lasso(Y, W, X, folds, seed, lambda_rule, clip, method,
                                    fold_ids=(a + s * b) % folds))
        except ValueError as e:
            if "empty (fold, arm) cell" not in str(e):
                raise
            raise ValueError(str(e).replace("cell:", f"cell in partition {s}:")) from None
    th, se = np.array([r.ate for r in rs]), np.array([r.se for r in rs])
    agg = np.median if aggregate == "median" else np.mean
    t = float(agg(th))
    return AteResult.make(method, t, float(np.sqrt(agg(se * se + (th - t) ** 2))), n=len(Y),
                          repeats=repeats, aggregate=aggregate,
                          splits=np.stack([th, se], 1).tolist(),
                          n_clipped=[r.diagnostics["n_clipped"] for r in rs],
                          n_treated=rs[0].diagnostics["n_treated"])


def dml_from_residuals(yr, wr, method):
    """Orthogonal-score combine: theta = sum(wr yr)/sum(wr^2); SE from the
    Neyman score psi = (yr - theta wr) wr, J = mean(wr^2)."""
    n = len(yr)
    j = np.mean(wr * wr)
    theta = np.mean(wr * yr) / j
    psi = (yr - theta * wr) * wr
    se = np.sqrt(np.mean(psi * psi) / (j * j) / n)
    return AteResult.make(method, theta, se, n=n)
