"""The effect of a REAL treatment with an endogeneity problem in the cross-fitted partially
linear IV model (DML-PLIV, Chernozhukov et al. 2018 §4.2; DoubleML ``DoubleMLPLIV``,
partialling-out score) with CV-LASSO nuisances on the fold Gram stack: a dose, a price or a
number of contacts D, instrumented by q = 1..4 continuous or discrete instruments Z. PLR
(``estimators/lasso.py``) is biased under an unobserved confounder of D and Y; the LATE of
``estimators/late.py`` needs D and Z binary.

The held-out nuisances are gaussian CV-LASSO fits with the inner CV of ``lasso.dml_plr_lasso``:

    l = E[Y|X]   r = E[D|X]   m_j = E[Z_j|X]
    y~ = y - l   d~ = d - r   z~ = z - m   (a q-vector)
    pi    = (S z~ z~')^-1 S z~ d~         v_i = z~_i' pi   (no intercept; pi treated as fixed)
    theta = pi' S z~y~ / pi' S z~d~
    Omega = Q_yy - 2 theta Q_yd + theta^2 Q_dd,   Q_ab[i,j] = S z~_i z~_j a b
    SE    = sqrt(pi' Omega pi) / (pi' S z~d~)

the convention of ``stats.dml_finalize("plr")``: with q = 1 and Z = D, pi = 1 and theta, SE are
PLR's. Layout: the plain K-fold panel of ``dml_plr_lasso`` (segment k = fold k, the folds
``_fold_ids(n, K, seed, 0, None)``) with D in column ``W`` and the instruments in target
columns ``Z0 .. Z{q-1}``; its one Gram pass already includes them; the (2 + q) K nuisances
(that many times K path problems) run in as few ``ate_enet_path`` launches as hold them; one
fused pass over the panel (csrc/pliv.hip ``ate_pliv_moments``) accumulates the moments
``result.PlivLayout`` and its summing launch also finishes (a q x q Cholesky in one lane), so
the captured call needs no ``torch.linalg`` and no host sync. Everything reported follows from
the moments on the host (``result.PlivResult``).

Clusters (``dml_pliv_lasso_cluster``): whole clusters go into folds
(``cluster.cluster_layout``), theta is the unclustered pass's, and the SE is
sqrt(sum_j t_j^2) / (pi' S z~d~) with t_j the within-cluster sum of a - theta b, a = v y~,
b = v d~ (csrc/pliv.hip ``ate_pliv_terms``, then csrc/cluster.hip); no J / (J - 1) factor, as
for PLR, so singleton clusters reproduce the unclustered SE.

Out of scope: more than 4 instruments, row shards, repeated cross-fitting, the robust
first-stage F (it needs fourth moments of z~ alone), two-step GMM and the Hansen J test,
DoubleML's ``IV-type`` score, group / curve / policy / sensitivity versions, and an instrument
in the device data generator.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..ops.devconst import const
from ..ops.enet import (MAX_PATH_PROBLEMS, cv_enet_gaussian, cv_problem_count,
                        default_lambda_min_ratio)
from ..ops.panel import build_panel, dtype_code
from ..result import PLIV_MAX_INSTRUMENTS, PlivResult, pliv_finish, pliv_layout
from .apos import path_launches
from .common import as_np, resolve_device
from .irm import gram_phases, run_body, run_phases
from .lasso import _fold_ids

PLIV_LDS_MAX = 64 * 1024 - 8192    # csrc/pliv.hip PLIV_LDS_MAX (ate_pliv_lds_max)


def instrument_names(q: int) -> list:
    return [f"Z{j}" for j in range(q)]


def _target_columns(pan, q: int) -> list:
    """[(first, second)] columns of the 2 + q targets the pass reads, Y, D (column ``W``),
    Z0..: bf16 panels carry them as hi + lo pairs, the others as one column (second = -1)."""
    names = ["Y", "W"] + instrument_names(q)
    for k in names:
        if k not in pan.cols:
            raise ValueError(f"the PLIV pass needs a panel with the columns {names}: "
                             "build_panel(X, D, Y, targets={'Z0': ...}); it has no " + repr(k))
    if pan.dtype == torch.bfloat16:
        return [(pan.cols[f"{k}_hi"], pan.cols[f"{k}_lo"]) for k in names]
    return [(pan.cols[k], -1) for k in names]


def check_lds(p: int, q: int, dtype) -> None:
    """The 2 + q coefficient vectors and the column list of one segment are staged in LDS:
    (2 + q)(p + 1) esz + 4 p bytes (esz: 4 on a bf16 panel, 8 otherwise) must fit what the
    kernel's static part leaves (csrc/pliv.hip; the bound of the LATE pass for its five)."""
    esz = 4 if dtype in (torch.bfloat16, "bf16") else 8
    need = (2 + q) * (p + 1) * esz + 4 * p
    if need > PLIV_LDS_MAX:
        raise ValueError(f"{p} covariates with {q} instruments need {need} bytes of LDS for the "
                         f"coefficient block of the PLIV pass, more than the {PLIV_LDS_MAX} it "
                         "has")


def _pliv_args(pan, coef, q):
    """The argument checks of the pass; returns p, the number of covariates."""
    lay = pliv_layout(q)
    p = len(pan.xcols)
    if coef.dim() != 3 or tuple(coef.shape) != (pan.nseg, 2 + lay.q, p + 1):
        raise ValueError(f"coef must be [{pan.nseg}, {2 + lay.q}, {p + 1}] (one block per "
                         f"segment), got {tuple(coef.shape)}")
    check_lds(p, lay.q, pan.dtype)
    return p


def _pliv_rows(pan, coef, q):
    """The float64 CPU twin of the row pass (the kernel's oracle): per segment
    ``(rows, res [2 + q, n_s])`` over its real rows -- the panel rows and the residuals
    y~, d~, z~_0.. ."""
    _pliv_args(pan, coef, q)
    tc = _target_columns(pan, q)
    X = pan.colmajor().double()
    c = coef.double().cpu()
    for s in range(pan.nseg):
        r0, r1 = (int(v) for v in pan.seg_bounds[s])
        Xs = X[:, r0:r1]
        v = Xs[pan.cols["one"]] != 0
        xs = Xs[pan.xcols][:, v]
        res = torch.stack([Xs[a][v] + (Xs[b][v] if b >= 0 else 0.0) - (c[s, t, 0] + c[s, t, 1:] @ xs)
                           for t, (a, b) in enumerate(tc)])
        yield r0 + torch.nonzero(v).reshape(-1), res


def pliv_moments_twin(pan, coef: torch.Tensor, q: int):
    """(moments, sum |term|): the float64 torch twin of csrc/pliv.hip ``ate_pliv_moments`` on
    a host panel, and per moment the sum of the absolute values of its per-row terms -- the
    denominator of the kernel tests' relative bound (the signed cross moments cancel)."""
    lay = pliv_layout(q)
    mom = torch.zeros(lay.size, dtype=torch.float64)
    ab = torch.zeros(lay.size, dtype=torch.float64)
    for _, res in _pliv_rows(pan, coef, q):
        ry, rd, rz = res[0], res[1], res[2:]
        terms = [torch.ones_like(ry), ry * ry, ry * rd, rd * rd]
        terms += [rz[i] * ry for i in range(q)] + [rz[i] * rd for i in range(q)]
        pairs = [(i, j) for i in range(q) for j in range(i, q)]
        terms += [rz[i] * rz[j] for i, j in pairs]
        for w in (ry * ry, ry * rd, rd * rd):
            terms += [rz[i] * rz[j] * w for i, j in pairs]
        t = torch.stack(terms)
        mom += t.sum(1)
        ab += t.abs().sum(1)
    return mom, ab


def default_nbx(pan, q: int) -> int:
    """Workgroups per segment of the pass: enough for the LARGEST segment to give every
    workgroup one trip of rows (2048 on a bf16 panel; 256 x 4 rows per thread up to q = 2,
    256 x 2 beyond), at most the grid of ``lasso.dml_residual_moments`` (512 / 256): a partial
    is up to 52 doubles, so a grid sized by the cap would mostly write and then sum zeros."""
    bf = pan.dtype == torch.bfloat16
    rows = 2048 if bf else 256 * (4 if q <= 2 else 2)
    b = np.asarray(pan.seg_bounds, dtype=np.int64)
    longest = int((b[:, 1] - b[:, 0]).max()) if len(b) else 1
    return max(1, min(512 if bf else 256, -(-longest // rows)))


def _launch_args(pan, coef, q, nbx):
    p = _pliv_args(pan, coef, q)
    dev = pan.device
    xc = const(pan.xcols, torch.int32, dev)
    segs = const(np.asarray(pan.seg_bounds, dtype=np.int64), torch.int64, dev)
    tc = const(np.asarray(_target_columns(pan, q), dtype=np.int32).reshape(-1), torch.int32, dev)
    if nbx is None:
        nbx = default_nbx(pan, q)
    c = coef.double().contiguous()
    cs, bs = pan.strides()
    head = (dtype_code(pan.data), pan.data.data_ptr(), cs, bs, xc.data_ptr(), p, segs.data_ptr(),
            pan.nseg, q, c.data_ptr(), tc.data_ptr(), pan.cols["one"], int(nbx))
    return head, (xc, segs, tc, c)


def pliv_moments(pan, coef: torch.Tensor, q: int, nbx: int | None = None, finish: bool = False):
    """The fused held-out PLIV pass -> the fp64 moments of ``result.PlivLayout`` (10 / 20 / 34
    / 52 at q = 1..4); ``finish``: (moments, res [4 + q]) with res = [theta, SE, pi' S z~d~,
    rank flag, pi] of the same launch sequence.

    pan: a K-fold panel (segment k = fold k) with D in column ``W`` and the instruments in
    ``Z0 .. Z{q-1}``. coef: [nseg, 2 + q, p+1] fp64, rows (l, r, m_0..m_{q-1}), intercept
    first. GPU: csrc/pliv.hip ``ate_pliv_moments`` (``nbx`` blocks per segment, default
    :func:`default_nbx`; per-workgroup partials and a fixed-order sum: equal bits run to run).
    CPU: the float64 torch twin :func:`pliv_moments_twin` and :func:`pliv_finalize`."""
    q = pliv_layout(q).q
    if not pan.data.is_cuda:
        mom = pliv_moments_twin(pan, coef, q)[0]
        return (mom, pliv_finalize(mom)) if finish else mom
    head, keep = _launch_args(pan, coef, q, nbx)
    dev = pan.device
    N = pliv_layout(q).size
    mom = torch.empty(N, dtype=torch.float64, device=dev)
    res = torch.empty(4 + q, dtype=torch.float64, device=dev)
    partial = torch.empty(pan.nseg * head[-1] * N, dtype=torch.float64, device=dev)
    _native.call("ate_pliv_moments", *head, partial.data_ptr(), mom.data_ptr(), res.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    del keep
    return (mom, res) if finish else mom


def pliv_terms(pan, coef: torch.Tensor, q: int, pi: torch.Tensor, nbx: int | None = None):
    """The per-row terms (a, b) = (v y~, v d~), v = z~' pi, of the PLIV score psi = a - theta b
    [ld] (fp64, panel row order, 0 on padding rows): the row pass of :func:`pliv_moments` --
    same arguments, same residuals -- writing the terms instead of summing moments. pi: [q]
    fp64, read on the device (no host sync: capturable). GPU: csrc/pliv.hip
    ``ate_pliv_terms``; CPU: the float64 torch twin."""
    q = pliv_layout(q).q
    if pi.numel() != q or pi.dtype != torch.float64:
        raise ValueError(f"pi must hold {q} fp64 weights")
    if not pan.data.is_cuda:
        ta = torch.zeros(pan.ld, dtype=torch.float64)
        tb = torch.zeros(pan.ld, dtype=torch.float64)
        w = pi.double().cpu().reshape(-1)
        for rows, res in _pliv_rows(pan, coef, q):
            v = (res[2:] * w[:, None]).sum(0)
            ta[rows] = v * res[0]
            tb[rows] = v * res[1]
        return ta, tb
    bounds = np.asarray(pan.seg_bounds, dtype=np.int64)
    if bounds[0, 0] != 0 or bounds[-1, 1] != pan.ld or np.any(bounds[1:, 0] != bounds[:-1, 1]):
        raise ValueError("the panel's segments must tile [0, ld): every row gets its terms")
    head, keep = _launch_args(pan, coef, q, nbx)
    dev = pan.device
    ta = torch.empty(pan.ld, dtype=torch.float64, device=dev)
    tb = torch.empty(pan.ld, dtype=torch.float64, device=dev)
    pi = pi.contiguous()
    _native.call("ate_pliv_terms", *head, pi.data_ptr(), ta.data_ptr(), tb.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    del keep
    return ta, tb


def pliv_finalize(mom: torch.Tensor) -> torch.Tensor:
    """[theta, SE, pi' S z~d~, rank flag, pi_0..pi_{q-1}] from the moments: the CPU twin of the
    in-kernel finish (``result.pliv_finish``, the module docstring's formulas, a q x q
    Cholesky). Reads the moments on the host."""
    return torch.tensor(pliv_finish(mom.detach().double().cpu().tolist()), dtype=torch.float64)


# ---------------------------------------------------------------- the front end
def check_instruments(Z, n: int) -> np.ndarray:
    """Z as an (n, q) float64 array; ValueError for a wrong shape, more than 4 instruments,
    non-finite values or a constant instrument (its residual is the fit's noise)."""
    Zn = as_np(Z).astype(np.float64)
    if Zn.ndim == 1:
        Zn = Zn[:, None]
    if Zn.ndim != 2 or Zn.shape[0] != n or Zn.shape[1] < 1:
        raise ValueError(f"Z must be (n,) or (n, q) with n = {n}, got shape {tuple(Zn.shape)}")
    q = Zn.shape[1]
    if q > PLIV_MAX_INSTRUMENTS:
        raise ValueError(f"DML-PLIV takes at most {PLIV_MAX_INSTRUMENTS} instruments, Z has {q}")
    if not np.isfinite(Zn).all():
        raise ValueError("DML-PLIV needs finite instruments: Z has NaN or infinite values")
    for j in range(q):
        if np.ptp(Zn[:, j]) == 0.0:
            raise ValueError(f"instrument {j} is constant: it cannot move the treatment")
    return Zn


def check_scope(dist=None, repeats=1, nuisance="linear", form=None):
    """What DML-PLIV does not do, each a ValueError before any device work."""
    if dist is not None:
        raise ValueError("DML-PLIV does not support row-sharded calls (dist)")
    if repeats != 1:
        raise ValueError("repeated cross-fitting is not available for DML-PLIV: repeats must be 1")
    if nuisance != "linear":
        raise ValueError('DML-PLIV fits gaussian (linear) nuisances only: a logit nuisance is '
                         f'not available, got {nuisance!r}')
    if form is not None:
        raise ValueError(f"the {form!r} form is not available for DML-PLIV: no gate / cate / "
                         "policy / sensitivity versions")


def check_rank(flag, q: int):
    """The rank flag of a finished call: ValueError for instruments that are collinear after
    partialling out X (a z~ that is identically 0 -- Z a column of X -- included)."""
    if flag != 0.0:
        raise ValueError(f"the {q} instrument residual{'s are' if q > 1 else ' is'} collinear "
                         "after partialling out X (a pivot of S z~z~' at or below 1e-12 of its "
                         "largest diagonal entry): drop the redundant instrument, or one that "
                         "X already explains")


def pliv_problems(pan, K: int, q: int):
    """The (2 + q) K nuisance problems on the K-Gram stack as arguments of
    ``cv_enet_gaussian``: (full_sets, full_y, ycols), fold by fold, l, r, m_0..m_{q-1}; every
    nuisance of fold k trains on the other K - 1 folds. ycols: (Y, W, Z0 ..)."""
    full_sets, full_y = [], []
    for k in range(K):
        others = [s for s in range(K) if s != k]
        full_sets += [others] * (2 + q)
        full_y += list(range(2 + q))
    ycols = [pan.cols["Y"], pan.cols["W"]] + [pan.cols[z] for z in instrument_names(q)]
    return full_sets, full_y, ycols


def pliv_fit_phases(pan, folds: int, q: int, lambda_rule="min", head=None,
                    max_problems: int = MAX_PATH_PROBLEMS):
    """The Gram phases (``irm.gram_phases``; ``head``: another phase list that leaves "G",
    e.g. the first two of ``lasso.dml_phases``), then the CV-LASSO fit of the (2 + q) K
    nuisances with ``ycols = [Y, W, Z0 ..]`` on the K full sets, in the launches of
    ``apos.path_launches`` (``max_problems``: the cap of one launch; one launch holds them all
    up to K = 6 at q = 4). Every launch gets the lambda ratio of the whole fit, so a nuisance
    does not depend on what shares its launch. State: "G", "coef" [K, 2 + q, p+1], "cv" (the
    last launch's). ``ValueError`` before any device work when one nuisance with its folds
    exceeds a launch or the coefficient block exceeds the pass's LDS."""
    K, q = int(folds), pliv_layout(q).q
    if pan.nseg != K:
        raise ValueError(f"DML-PLIV needs {K} segments (segment k = fold k), the panel has "
                         f"{pan.nseg}")
    counts = np.asarray(pan.seg_nreal, dtype=np.float64)
    for s in np.flatnonzero(counts <= 0):
        raise ValueError(f"empty fold: fold {int(s)} has no rows")
    _target_columns(pan, q)
    p = len(pan.xcols)
    check_lds(p, q, pan.dtype)
    full_sets, full_y, ycols = pliv_problems(pan, K, q)
    per = cv_problem_count(K, full_sets[:1], len(ycols), full_y[:1])
    launches = path_launches(len(full_sets), per, max_problems)
    ratio = default_lambda_min_ratio(min(counts[list(fs)].sum() for fs in full_sets), p)

    def phase_fit(st):
        coefs, cv = [], None
        for a, b in launches:
            cv = cv_enet_gaussian(st["G"], pan, pan.xcols, ycols, full_sets=full_sets[a:b],
                                  seg_counts=counts, full_y=full_y[a:b], lambda_min_ratio=ratio)
            coefs.append(cv.coef_min if lambda_rule == "min" else cv.coef_1se)
        coef = torch.cat(coefs).reshape(K, 2 + q, -1).double().contiguous()
        return {**st, "cv": cv, "coef": coef}

    phases = list(head) if head is not None else gram_phases(pan, None)[0]
    phases.append(phase_fit)
    return phases


def pliv_phases(pan, folds: int, q: int, lambda_rule="min",
                max_problems: int = MAX_PATH_PROBLEMS):
    """The PLIV step as phases for utils.graphs.SegmentedStep: those of
    :func:`pliv_fit_phases`, then

    B'  the PLIV moments and, in their summing launch, theta / SE / pi     device
        (csrc/pliv.hip ``ate_pliv_moments``)

    The result state holds "res" [4 + q], "mom" [N(q)], "coef" [K, 2 + q, p+1] and "cv"."""
    phases = pliv_fit_phases(pan, folds, q, lambda_rule, max_problems=max_problems)

    def phase_moments(st):
        mom, res = pliv_moments(pan, st["coef"], q, finish=True)
        return {**st, "mom": mom, "res": res}

    phases.append(phase_moments)
    return phases


def pliv_panel(pan, folds: int, q: int, lambda_rule="min"):
    """DML-PLIV on a K-fold panel with D in column W and the instruments in Z0..
    (``build_panel(X, D, Y, folds=fold, targets={"Z0": ...})``). Returns (res [4 + q],
    mom [N(q)], coef [K, 2 + q, p+1]): device tensors, no host sync on a GPU (capturable)."""
    st = run_phases(pliv_phases(pan, folds, q, lambda_rule))
    return st["res"], st["mom"], st["coef"]


def _pliv_body(pan, q, folds, lambda_rule):
    """The whole call as one device function (GraphCache captures it, keyed by q): [res, mom]."""
    res, mom, _ = pliv_panel(pan, folds, q, lambda_rule)
    return torch.cat([res, mom])


def _build(Y, D, Zn, X, fid, dtype, dev, perm=None):
    Yn, Dn, Xn = as_np(Y), as_np(D), as_np(X)
    if perm is not None:
        Yn, Dn, Xn, Zn, fid = Yn[perm], Dn[perm], Xn[perm], Zn[perm], fid[perm]
    targets = {z: Zn[:, j] for j, z in enumerate(instrument_names(Zn.shape[1]))}
    return build_panel(Xn, Dn, Yn, folds=fid, dtype=dtype, device=dev, targets=targets)


def _check_inputs(Y, D, Z, X, folds, dtype, dist, repeats):
    check_scope(dist, repeats)
    Yn = as_np(Y)
    Zn = check_instruments(Z, len(Yn))
    Xn = as_np(X)
    q = Zn.shape[1]
    check_lds(Xn.shape[1] if Xn.ndim == 2 else 1, q, dtype)
    path_launches((2 + q) * folds, folds)        # a nuisance is 1 full + K - 1 fold problems
    return Zn, q


def dml_pliv_lasso(Y, D, Z, X, folds=5, seed=1991, lambda_rule="min",
                   method="DML-PLIV cross-fit (LASSO)", device=None, dtype="f64", dist=None,
                   graph=True, repeats=1) -> PlivResult:
    """K-fold cross-fitted partially linear IV estimate with CV-LASSO nuisances (the module
    docstring). Y: outcome; D: the treatment, any real values; Z: (n,) or (n, q) instruments,
    1 <= q <= 4; X: covariates. Folds are those of ``lasso.dml_plr_lasso``. Matches
    reference.estimators.dml_pliv_lasso.

    graph: as ``dml_plr_lasso``, one captured hipGraph on a GPU (graph name ``dml_pliv``); q is
    part of the cache key. ValueError before any device work: more than 4 instruments, a
    constant instrument, ``dist``, ``repeats`` other than 1, a coefficient block over the
    pass's LDS; after the call: instruments collinear after partialling out. diagnostics: n,
    n_instruments, rmse_l, rmse_r, hipgraph."""
    Zn, q = _check_inputs(Y, D, Z, X, folds, dtype, dist, repeats)
    dev = resolve_device(device)
    fid = np.asarray(_fold_ids(len(Zn), folds, seed, 0, None), dtype=np.int64)
    pan = _build(Y, D, Zn, X, fid, dtype, dev)
    out, g = run_body("dml_pliv", _pliv_body, (pan,), q, folds, lambda_rule, graph=graph)
    v = out.detach().double().cpu().numpy()
    check_rank(v[3], q)
    return PlivResult.from_moments(method, v[4 + q:], n=len(Zn), hipgraph=g)


def _pliv_cluster_body(pan, starts, order, q, folds, lambda_rule, J):
    """The clustered PLIV cross-fit as one device function: the unclustered phases (theta and
    its moments, same launches), the per-row terms, the cluster pass -> [res (4 + q), SE, the
    4 cluster moments, mom]."""
    from .cluster import cluster_finalize, cluster_moments
    st = run_phases(pliv_phases(pan, folds, q, lambda_rule))
    res, mom = st["res"], st["mom"]
    a, b = pliv_terms(pan, st["coef"], q, res[4:4 + q])
    out = cluster_moments(a, b, starts, order, J, res[:1])
    se = cluster_finalize(out, res[2], J, False)
    return torch.cat([res, se.reshape(1), out, mom])


def dml_pliv_lasso_cluster(Y, D, Z, X, clusters, folds=5, seed=1991, lambda_rule="min",
                           method="DML-PLIV cross-fit (LASSO)", device=None, dtype="f64",
                           dist=None, graph=True, repeats=1) -> PlivResult:
    """:func:`dml_pliv_lasso` with whole clusters cross-fitted and the cluster-robust SE (the
    module docstring; graph name ``dml_pliv_cluster``, whose replays carry new clusters of the
    same count). Matches reference.estimators.dml_pliv_lasso(clusters=). theta carries the
    bits of the unclustered estimator on the same folds. diagnostics: those of
    ``dml_pliv_lasso`` plus n_clusters, max_cluster, design_effect, se_unclustered."""
    from .cluster import _csr_tensors, cluster_layout
    Zn, q = _check_inputs(Y, D, Z, X, folds, dtype, dist, repeats)
    dev = resolve_device(device)
    lay = cluster_layout(clusters, len(Zn), folds, seed, dist, repeats)
    pan = _build(Y, D, Zn, X, lay.fid, dtype, dev, perm=lay.perm)
    starts, order = _csr_tensors(pan, lay)
    out, g = run_body("dml_pliv_cluster", _pliv_cluster_body, (pan, starts, order), q, folds,
                      lambda_rule, lay.J, graph=graph)
    v = out.detach().double().cpu().numpy()
    check_rank(v[3], q)
    cm = v[5 + q:9 + q]                           # sum t^2, sum t, sum n_j^2, max n_j
    n = len(Zn)
    return PlivResult.from_moments(
        method, v[9 + q:], se=v[4 + q], n=n, n_clusters=lay.J,
        max_cluster=int(round(cm[3])) if np.isfinite(cm[3]) else -1,
        design_effect=float(cm[2] / n), hipgraph=g)
