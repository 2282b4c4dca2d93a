"""Cross-fitted AIPW for the interactive regression model (DML-IRM, Chernozhukov et al.
2018 §5.1) with CV-LASSO nuisances on the fold Gram stack.

Where ``lasso.dml_plr_lasso`` estimates the one coefficient of the partially linear model
(the ATE only under a constant effect), this estimator fits the outcome regression per arm,
g0(X) = E[Y|X, W=0] and g1(X) = E[Y|X, W=1], and the linear-probability propensity
m(X) = E[W|X], all by gaussian CV-LASSO, and averages the doubly robust score

    psi = g1 - g0 + w (y - g1) / m - (1 - w)(y - g0) / (1 - m),   m clipped to [clip, 1-clip]

over held-out rows (textbook signs, as ``crossfit.aipw_score``).

``propensity="logit"`` replaces the linear-probability fit of m by the binomial CV-LASSO
(``cv.glmnet(family="binomial")`` on the same training rows and inner folds): g0 and g1 stay in
the gaussian launch, all K * K propensity problems run in ONE grouped binomial path launch
(``ops/lognet.cv_lognet_groups``), and the score pass takes the logit through a logistic link
(:func:`irm_fit_phases`, :func:`check_logit_scope` for its limits).

Layout: a 2K-segment panel, segment ``2k + a`` = the rows of fold k with W = a. One Gram
pass (K01) then yields per-(fold, arm) Grams; the fold Grams of the propensity problems are
their pairwise sums. All 3 K (K + 1) path problems (3 nuisances x K outer folds x (1 full +
K - 1 inner CV)) run in ONE ``ate_enet_path`` launch (``ops/enet.cv_enet_gaussian(full_y=)``),
and one fused pass over the panel (csrc/irm.hip) accumulates the 8 score moments.

Repeated cross-fitting (:func:`dml_irm_lasso_repeated`, :func:`irm_repeated_phases`): S
partitions built from K*K micro-groups on a 2 K*K-segment panel share one Gram pass and one
multi-split score pass (:func:`irm_score_moments_multi`), median-aggregated.

The estimators on the same score (gate, cate, policy, sensitivity, targets) share what lives
here: the score pass in its forms (:func:`irm_score_moments`, :func:`irm_sens_moments`,
:func:`irm_target_moments`, :func:`irm_scores` -- one CPU twin ``_score_terms``, one launcher
``_score_launch``), the
front end of every ``dml_irm_*`` function (:func:`arm_split_panel`, :func:`run_body`,
:func:`comm_counts`), the fit and score phases (:func:`irm_fit_phases`, :func:`phase_scores`,
:func:`run_phases`) and the n - 1 variance rule (:func:`mean_se`).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..ops.devconst import const
from ..ops.enet import (MAX_PATH_PROBLEMS, cv_enet_gaussian, cv_problem_count,
                        default_lambda_min_ratio)
from ..ops.gram import gram
from ..ops.panel import build_panel, dtype_code
from ..result import SENS_MOMENTS, TARGET_MOMENTS, AteResult
from ..utils.graphs import estimator_graphs
from .common import as_np, resolve_device
from .lasso import (_fold_ids, _tri_index, allreduce_sym_, global_seg_counts, median_aggregate,
                    micro_fold_map)

PROPENSITIES = ("linear", "logit")   # the fit of m: gaussian LASSO (clipped) | binomial LASSO
LINKS = ("identity", "logistic")     # what coefficient row 2 predicts: m | logit(m)
LOGIT_MAX_P, LOGIT_MAX_FOLDS = 96, 16   # ops/lognet: p <= 96, K * K <= 256 path problems


def check_propensity(propensity) -> str:
    if propensity not in PROPENSITIES:
        raise ValueError(f"propensity must be one of {PROPENSITIES}, got {propensity!r}")
    return propensity


def propensity_link(propensity) -> str:
    """The link of the score pass for a propensity fit."""
    return LINKS[PROPENSITIES.index(check_propensity(propensity))]


def check_logit_scope(propensity, p, folds, dtype=None, dist=None, repeats=1):
    """The limits of ``propensity="logit"`` (ValueError naming the one exceeded, before any
    device work): one partition, no row shards (the binomial path has no collective), an
    fp32 / fp64 panel, p <= 96 and K <= 16 (K * K path problems in one launch). p: the
    number of covariates, or the covariate matrix (looked at only for "logit")."""
    if check_propensity(propensity) == "linear":
        return
    p = int(p) if np.ndim(p) == 0 else np.shape(p)[1]       # p, or the covariate matrix
    if repeats != 1:
        raise ValueError('propensity="logit" supports repeats = 1 only (no repeated '
                         "cross-fitting of the binomial path)")
    if dist is not None:
        raise ValueError('propensity="logit" does not support row-sharded calls (dist): the '
                         "binomial path has no collective")
    if dtype in ("bf16", torch.bfloat16):
        raise ValueError('propensity="logit" needs an fp32 / fp64 panel, not bf16')
    if p > LOGIT_MAX_P:
        raise ValueError(f'propensity="logit" supports p <= {LOGIT_MAX_P} covariates, got {p}')
    if folds > LOGIT_MAX_FOLDS:
        raise ValueError(f'propensity="logit" supports K <= {LOGIT_MAX_FOLDS} folds, got {folds}')


N_MOMENTS = 8   # [S psi, S psi^2, n, n_clipped, S w(y-g1)^2, S (1-w)(y-g0)^2, S (w-m)^2, n_treated]


def _yw_columns(pan):
    """(y0, y1, w0, w1): the target columns the score pass reads; bf16 panels carry Y / W
    as hi + lo pairs (exact for binary targets), the others as one column (second = -1)."""
    if pan.dtype == torch.bfloat16:
        return pan.cols["Y_hi"], pan.cols["Y_lo"], pan.cols["W_hi"], pan.cols["W_lo"]
    return pan.cols["Y"], -1, pan.cols["W"], -1


def _score_args(pan, coef, segs_per_fold):
    """The argument checks of the score pass; returns p, the number of covariates."""
    nseg = pan.nseg
    nfold = coef.shape[0]
    if segs_per_fold < 1 or nfold * segs_per_fold < nseg:
        raise ValueError(f"{nseg} segments at {segs_per_fold} per fold need "
                         f"{-(-nseg // max(segs_per_fold, 1))} coefficient blocks, got {nfold}")
    p = len(pan.xcols)
    if tuple(coef.shape[1:]) != (3, p + 1):
        raise ValueError(f"coef must be [nfold, 3, {p + 1}], got {tuple(coef.shape)}")
    return p


def _score_terms(pan, coef, segs_per_fold, blk=None, link="identity"):
    """The float64 CPU twin of the score pass (the kernels' oracle): per segment
    ``(r0, r1, v, y, w, g0, g1, m)`` -- its row range, the mask of its real rows, and over
    those rows the targets, the two outcome regressions and the unclipped propensity
    (link "logistic": coefficient row 2 predicts its logit, m = 1 / (1 + exp(-eta))).
    blk [S, ngroups] (the multi-split pass): segment group g uses block ``blk[t][g]`` under
    split t, and g0, g1, m are lists of S tensors, each the expression of the single pass."""
    if blk is None:
        _score_args(pan, coef, segs_per_fold)
    logistic = _link_code(link, pan) == 1
    y0, y1, w0, w1 = _yw_columns(pan)
    X = pan.colmajor().double()
    c = coef.double()
    for s in range(pan.nseg):
        r0, r1 = (int(v) for v in pan.seg_bounds[s])
        Xs = X[:, r0:r1]
        v = Xs[pan.cols["one"]] != 0
        xs = Xs[pan.xcols][:, v]
        y = Xs[y0][v] + (Xs[y1][v] if y1 >= 0 else 0.0)
        w = Xs[w0][v] + (Xs[w1][v] if w1 >= 0 else 0.0)
        k = s // segs_per_fold
        if blk is not None:
            ks = [int(b[k]) for b in blk]
            yield (r0, r1, v, y, w, *([c[q, r, 0] + c[q, r, 1:] @ xs for q in ks]
                                      for r in range(3)))
            continue
        m = c[k, 2, 0] + c[k, 2, 1:] @ xs
        if logistic:
            m = 1.0 / (1.0 + torch.exp(-m))
        yield (r0, r1, v, y, w, c[k, 0, 0] + c[k, 0, 1:] @ xs, c[k, 1, 0] + c[k, 1, 1:] @ xs, m)


def _link_code(link, pan) -> int:
    """0 identity, 1 logistic; the logistic link exists for fp32 / fp64 panels only."""
    if link not in LINKS:
        raise ValueError(f"link must be one of {LINKS}, got {link!r}")
    if link == "logistic" and pan.dtype == torch.bfloat16:
        raise ValueError("the logistic link of the score pass needs an fp32 / fp64 panel")
    return LINKS.index(link)


_LINK_MODES = {"ate_irm_score_moments": 0, "ate_irm_scores": 1, "ate_irm_sens_moments": 2,
               "ate_irm_target_moments": 3}


def aipw_psi(y, w, g0, g1, e):
    """The AIPW score with the clipped propensity ``e`` (the module docstring's psi)."""
    return g1 - g0 + w * (y - g1) / e - (1.0 - w) * (y - g0) / (1.0 - e)


def _score_launch(name, pan, coef, clip, segs_per_fold, nbx, n_out, moments, blk=None,
                  link="identity"):
    """One instantiation of the fused score pass (csrc/irm.hip entry point ``name``) with
    ``nbx`` blocks per segment. ``moments``: the entry point sums ``n_out`` moments (a
    ``partial`` workspace, then the result); otherwise it writes ``n_out`` = ld row scores.
    blk [S, ngroups] (checked by the caller): the multi-split entry point, whose arguments
    add (nblk, blk, S) after ``coef``; ``n_out`` = S * 8 then. link "logistic": the same pass
    through ``ate_irm_score_link`` (mode of ``name``, link 1); "identity" keeps ``name``."""
    head = ()
    if _link_code(link, pan):
        if blk is not None:
            raise ValueError("the multi-split score pass has no logistic link")
        head, name = (_LINK_MODES[name], 1), "ate_irm_score_link"
    p = len(pan.xcols) if blk is not None else _score_args(pan, coef, segs_per_fold)
    y0, y1, w0, w1 = _yw_columns(pan)
    dev = pan.device
    xc = const(pan.xcols, torch.int32, dev)
    segs = const(np.asarray(pan.seg_bounds, dtype=np.int64), torch.int64, dev)
    if nbx is None:
        # bf16: 2048 rows per block; enough blocks per segment to fill 256 CUs several times
        nbx = 512 if pan.dtype == torch.bfloat16 else 256
    out = torch.empty(n_out, dtype=torch.float64, device=dev)
    bufs = (out,)
    if moments:
        bufs = (torch.empty(pan.nseg * nbx * n_out, dtype=torch.float64, device=dev), out)
    c = coef.double().contiguous()
    split = () if blk is None else (coef.shape[0], const(blk, torch.int32, dev).data_ptr(),
                                    blk.shape[0])
    cs, bs = pan.strides()
    ptrs = [b.data_ptr() for b in bufs]
    if head and not moments:
        ptrs.append(None)                        # the link entry point's unused `moments`
    _native.call(name, *head, dtype_code(pan.data), pan.data.data_ptr(), cs, bs, xc.data_ptr(), p,
                 segs.data_ptr(), pan.nseg, segs_per_fold, c.data_ptr(), *split, y0, y1, w0, w1,
                 pan.cols["one"], float(clip), nbx, *ptrs,
                 torch.cuda.current_stream().cuda_stream)
    return out


def irm_score_moments(pan, coef: torch.Tensor, clip: float = 0.01, segs_per_fold: int = 2,
                      nbx: int | None = None, link: str = "identity") -> torch.Tensor:
    """Fused held-out AIPW score pass -> the 8 fp64 moments (N_MOMENTS).

    coef: [nfold, 3, p+1] fp64, rows (g0, g1, m), intercept first; segment s of the panel
    uses block ``s // segs_per_fold`` (2: the arm-split layout; 1: a plain K-fold panel).
    W is read from the panel on every row. GPU: csrc/irm.hip (``nbx`` blocks per segment);
    CPU: the float64 torch twin (:func:`_score_terms`), the kernel's oracle.
    link "logistic": row m of coef holds logit coefficients (``propensity="logit"``); the
    sigmoid is taken in fp64 before the score, so n_clipped and S (w - m)^2 are about the
    probability (fp32 / fp64 panels; the same keyword on the three sibling passes)."""
    if pan.data.is_cuda:
        return _score_launch("ate_irm_score_moments", pan, coef, clip, segs_per_fold, nbx,
                             N_MOMENTS, True, link=link)
    mom = torch.zeros(N_MOMENTS, dtype=torch.float64)
    for _, _, _, y, w, g0, g1, m in _score_terms(pan, coef, segs_per_fold, link=link):
        mom += _segment_moments(y, w, g0, g1, m, clip)
    return mom


def _segment_moments(y, w, g0, g1, m, clip):
    """The 8 moments (N_MOMENTS) of one segment's rows in the float64 twin."""
    lo, hi = clip, 1.0 - clip
    psi = aipw_psi(y, w, g0, g1, m.clamp(lo, hi))
    one = torch.ones_like(psi)
    return torch.stack([psi.sum(), (psi * psi).sum(), one.sum(),
                        ((m < lo) | (m > hi)).double().sum(),
                        (w * (y - g1) ** 2).sum(), ((1.0 - w) * (y - g0) ** 2).sum(),
                        ((w - m) ** 2).sum(), w.sum()])


def score_multi_smax() -> int:
    """The most splits one pass of the multi-split score kernel serves (csrc/irm.hip)."""
    return int(_native.hip().ate_irm_score_multi_smax())


def irm_score_moments_multi(pan, coef: torch.Tensor, blk, clip: float = 0.01,
                            segs_per_fold: int = 2, nbx: int | None = None) -> torch.Tensor:
    """The pass of :func:`irm_score_moments` for S partitions of the same segments at once
    (repeated cross-fitting) -> [S, 8] fp64 moments.

    coef: [nblk, 3, p+1] fp64; blk: host integers [S, ngroups], ngroups = ceil(nseg /
    segs_per_fold): under split t, segment s uses block ``blk[t][s // segs_per_fold]``. Row t
    of the result carries the bits of ``irm_score_moments(pan, coef[blk[t]], ...)`` at the
    same ``nbx``. GPU: csrc/irm.hip ``ate_irm_score_moments_multi`` -- every column of the
    union of the splits' supports is read once for all splits, ``one``, Y and W once per row;
    the panel is read again only past :func:`score_multi_smax` splits. CPU: the float64 torch
    twin, one loop over the segments with S scores per row."""
    blk = np.ascontiguousarray(np.asarray(blk.cpu() if torch.is_tensor(blk) else blk),
                               dtype=np.int64)
    p = len(pan.xcols)
    ngroups = -(-pan.nseg // max(segs_per_fold, 1))
    if segs_per_fold < 1 or blk.ndim != 2 or blk.shape[0] < 1 or blk.shape[1] != ngroups:
        raise ValueError(f"blk must be [S, {ngroups}] ({pan.nseg} segments at {segs_per_fold} "
                         f"per group), got {tuple(blk.shape)}")
    if coef.dim() != 3 or tuple(coef.shape[1:]) != (3, p + 1):
        raise ValueError(f"coef must be [nblk, 3, {p + 1}], got {tuple(coef.shape)}")
    nblk, S = coef.shape[0], blk.shape[0]
    if blk.min() < 0 or blk.max() >= nblk:
        raise ValueError(f"blk entries must be coefficient blocks in [0, {nblk})")
    if not pan.data.is_cuda:
        mom = torch.zeros((S, N_MOMENTS), dtype=torch.float64)
        for _, _, _, y, w, g0, g1, m in _score_terms(pan, coef, segs_per_fold, blk):
            for t in range(S):
                mom[t] += _segment_moments(y, w, g0[t], g1[t], m[t], clip)
        return mom
    return _score_launch("ate_irm_score_moments_multi", pan, coef, clip, segs_per_fold, nbx,
                         S * N_MOMENTS, True, blk).view(S, N_MOMENTS)


def irm_sens_moments(pan, coef: torch.Tensor, clip: float = 0.01, segs_per_fold: int = 2,
                     nbx: int | None = None, link: str = "identity") -> torch.Tensor:
    """The pass of :func:`irm_score_moments` -- same arguments, same dot products, same psi --
    accumulating the 14 fp64 moments of the sensitivity analysis (``result.SENS_MOMENTS``;
    estimators/sensitivity.py). GPU: csrc/irm.hip ``ate_irm_sens_moments`` (for the same
    ``nbx`` S psi, S psi^2, n, n_clipped and n_treated carry the bits of
    ``irm_score_moments``); CPU: the float64 torch twin."""
    if pan.data.is_cuda:
        return _score_launch("ate_irm_sens_moments", pan, coef, clip, segs_per_fold, nbx,
                             len(SENS_MOMENTS), True, link=link)
    mom = torch.zeros(len(SENS_MOMENTS), dtype=torch.float64)
    lo, hi = clip, 1.0 - clip
    for _, _, _, y, w, g0, g1, m in _score_terms(pan, coef, segs_per_fold, link=link):
        e = m.clamp(lo, hi)
        psi = aipw_psi(y, w, g0, g1, e)
        b = torch.where(w != 0, (y - g1) ** 2, (y - g0) ** 2)
        rr = w / e - (1.0 - w) / (1.0 - e)
        cc = 2.0 * (1.0 / e + 1.0 / (1.0 - e)) - rr * rr
        one = torch.ones_like(psi)
        mom += torch.stack([psi.sum(), (psi * psi).sum(), one.sum(),
                            ((m < lo) | (m > hi)).double().sum(),
                            b.sum(), (b * b).sum(), cc.sum(), (cc * cc).sum(),
                            (psi * b).sum(), (psi * cc).sum(), (b * cc).sum(),
                            y.sum(), (y * y).sum(), w.sum()])
    return mom


def irm_target_moments(pan, coef: torch.Tensor, clip: float = 0.01, segs_per_fold: int = 2,
                       nbx: int | None = None, link: str = "identity") -> torch.Tensor:
    """The pass of :func:`irm_score_moments` -- same arguments, same dot products, same psi --
    accumulating the 12 fp64 moments of the three target populations (``result.TARGET_MOMENTS``;
    estimators/targets.py): with e the clipped propensity and the two quotients of psi,

        q1 = w (y - g1) / e                q0 = (1 - w)(y - g0) / (1 - e)
        a  = w (y - g0) - e q0             (the ATT numerator: g0 and m only)
        c  = -(1 - w)(y - g1) + (1 - e) q1 (the ATC numerator: g1 and m only)

    and psi = a + c algebraically. GPU: csrc/irm.hip ``ate_irm_target_moments`` (for the same
    ``nbx`` S psi, S psi^2, n, n_clipped and n_treated carry the bits of
    ``irm_score_moments``); CPU: the float64 torch twin. A zero coefficient row (a nuisance
    that was not fitted) is legal: the moments that involve it are finite and meaningless."""
    if pan.data.is_cuda:
        return _score_launch("ate_irm_target_moments", pan, coef, clip, segs_per_fold, nbx,
                             len(TARGET_MOMENTS), True, link=link)
    mom = torch.zeros(len(TARGET_MOMENTS), dtype=torch.float64)
    lo, hi = clip, 1.0 - clip
    for _, _, _, y, w, g0, g1, m in _score_terms(pan, coef, segs_per_fold, link=link):
        e = m.clamp(lo, hi)
        psi = aipw_psi(y, w, g0, g1, e)
        q1, q0 = w * (y - g1) / e, (1.0 - w) * (y - g0) / (1.0 - e)
        a = w * (y - g0) - e * q0
        c = -(1.0 - w) * (y - g1) + (1.0 - e) * q1
        one = torch.ones_like(psi)
        mom += torch.stack([psi.sum(), (psi * psi).sum(), one.sum(),
                            ((m < lo) | (m > hi)).double().sum(),
                            a.sum(), (a * a).sum(), (a * w).sum(),
                            c.sum(), (c * c).sum(), (c * (1.0 - w)).sum(), (a * c).sum(),
                            w.sum()])
    return mom


def irm_scores(pan, coef: torch.Tensor, clip: float = 0.01, segs_per_fold: int = 2,
               nbx: int | None = None, link: str = "identity") -> torch.Tensor:
    """The per-row AIPW scores psi [ld] (fp64, panel row order, 0 on padding rows): the pass
    of :func:`irm_score_moments` -- same arguments, same dot products, same psi -- writing
    every row's score instead of summing moments (csrc/irm.hip ``ate_irm_scores``; CPU: the
    float64 torch twin). Input of the estimators on the scores (gate, cate, policy)."""
    if pan.data.is_cuda:
        bounds = np.asarray(pan.seg_bounds, dtype=np.int64)
        if bounds[0, 0] != 0 or bounds[-1, 1] != pan.ld or np.any(bounds[1:, 0] != bounds[:-1, 1]):
            raise ValueError("the panel's segments must tile [0, ld): every row gets a score")
        return _score_launch("ate_irm_scores", pan, coef, clip, segs_per_fold, nbx, pan.ld, False,
                             link=link)
    psi = torch.zeros(pan.ld, dtype=torch.float64)
    for r0, r1, v, y, w, g0, g1, m in _score_terms(pan, coef, segs_per_fold, link=link):
        psi[r0:r1][v] = aipw_psi(y, w, g0, g1, m.clamp(clip, 1.0 - clip))
    return psi


def mean_se(s1, s2, n):
    """(mean, SE) from S x, S x^2 and n: SE^2 = the sample variance (the n - 1 rule) over n,
    clamped at 0. Device tensors in and out, no host sync (capturable)."""
    return s1 / n, torch.sqrt(((s2 - s1 * s1 / n) / (n - 1) / n).clamp(min=0))


def irm_finalize(mom: torch.Tensor) -> torch.Tensor:
    """[theta, SE] from the score moments: theta = S psi / n, SE by :func:`mean_se`."""
    return torch.stack(mean_se(mom[0], mom[1], mom[2]))


def check_cells(counts, folds: int):
    """Every (fold, arm) cell of the 2K-segment layout needs a row: the per-arm outcome fit
    of every other fold trains on it. ``counts``: (global) rows per segment."""
    c = np.asarray(counts)
    if len(c) != 2 * folds:
        raise ValueError(f"DML-IRM needs {2 * folds} segments (fold k, arm a -> 2k + a), "
                         f"the panel has {len(c)}")
    for s in np.flatnonzero(c <= 0):
        raise ValueError(f"empty (fold, arm) cell: fold {int(s) // 2}, arm W={int(s) % 2} "
                         "has no rows")


def irm_phases(pan, folds: int, lambda_rule="min", clip=0.01, comm=None, seg_counts=None,
               propensity="linear"):
    """The cross-fit DML-IRM step as phases for utils.graphs.SegmentedStep (as
    lasso.dml_phases):

    A  per-(fold, arm) Gram stack (K01): tile kernel, then slab reduce   device (two phases)
    C01 all-reduce of the Gram stack over row shards                     collective (world > 1)
    B  CV-LASSO paths for K folds x {g0, g1, m} + inner CV and the
       lambda selection, one path launch (K08/K09)                       device
    B' fused held-out AIPW score moments (csrc/irm.hip)                  device
    C06 all-reduce of the 8 score moments                                collective (world > 1)
    C  theta / SE (fp64, on device)                                      device

    Every rank solves every path (paths are not sharded over ranks). The result state holds
    "res" [2], "mom" [8], "coef" [K, 3, p+1] and "cv". propensity "logit": m by the grouped
    binomial path (:func:`irm_fit_phases`), scored through the logistic link."""
    phases, reduce = irm_fit_phases(pan, folds, lambda_rule, comm, seg_counts,
                                    propensity=propensity)
    link = propensity_link(propensity)

    def phase_score(st):
        return {**st, "mom": irm_score_moments(pan, st["coef"], clip, 2, link=link)}

    def phase_final(st):
        return {**st, "res": irm_finalize(st["mom"])}

    phases.append(phase_score)
    if reduce is not None:
        phases.append(reduce("mom"))
    phases.append(phase_final)
    return phases


NUISANCES = (0, 1, 2)   # rows of a coefficient block: g0, g1, m


def check_nuisances(nuisances) -> tuple:
    """A subset of :data:`NUISANCES` (0: g0, 1: g1, 2: m), distinct, ascending, not empty."""
    nu = tuple(int(r) for r in nuisances)
    if not nu or any(r not in NUISANCES for r in nu) or list(nu) != sorted(set(nu)):
        raise ValueError(f"nuisances must be an ascending, non-empty subset of {NUISANCES} "
                         f"(g0, g1, m), got {tuple(nuisances)}")
    return nu


def fit_problems(pan, K: int, counts, nuisances=NUISANCES):
    """The 3 K nuisance problems on the 3K-Gram stack ``cat([G, G[0::2] + G[1::2]])`` as
    arguments of ``cv_enet_gaussian``: (seg_counts, full_sets, full_y, ycols). Segments of
    the stack: 2s + a = (fold s, arm a); 2K + s = fold s, both arms. ``counts``: (global)
    rows per panel segment. nuisances: the subset of (0: g0, 1: g1, 2: m) to fit -- only its
    ``len(nuisances) K`` problems are named, fold by fold in that order."""
    nuisances = check_nuisances(nuisances)
    counts = np.asarray(counts, dtype=np.float64)
    counts3 = np.concatenate([counts, counts[0::2] + counts[1::2]])
    full_sets, full_y = [], []
    for k in range(K):
        others = [s for s in range(K) if s != k]
        sets = [[2 * s for s in others], [2 * s + 1 for s in others],
                [2 * K + s for s in others]]
        full_sets += [sets[r] for r in nuisances]
        full_y += [(0, 0, 1)[r] for r in nuisances]   # g0, g1: target Y; m: target W
    return counts3, full_sets, full_y, [pan.cols["Y"], pan.cols["W"]]


def gram_phases(pan, comm=None):
    """The head of every IRM phase list: the per-segment Gram stack (K01: tile kernel, slab
    reduce; state "G") and, at world > 1, its symmetric all-reduce over row shards (C01).
    Returns (phases, reduce): ``reduce(name)`` makes an all-reduce phase of a state tensor
    (None at world 1)."""
    from ..utils.graphs import Collective
    dist = comm is not None and comm.world_size > 1

    def phase_gram(_):
        return {"G": gram(pan, stage="tiles")}

    def phase_gram_reduce(st):
        return {"G": gram(pan, stage="reduce", out=st["G"])}

    cap = bool(getattr(comm, "capturable", False))

    def reduce(name):
        def f(st):
            comm.all_reduce_(st[name])
            return st
        return Collective(f, capturable=cap)     # RCCL: captured inside the step's graph

    phases = [phase_gram, phase_gram_reduce]
    if dist:
        _tri_index(pan.P, pan.device)            # built here, never inside a capture

        def reduce_g(st):
            allreduce_sym_(comm, st["G"])
            return st
        phases.append(Collective(reduce_g, capturable=cap))
    return phases, (reduce if dist else None)


def logit_fold_sets(K: int):
    """The K cross-validated binomial fits of the logit propensity as ``full_sets`` of
    ``ops.lognet.cv_lognet_groups``: group k trains on every fold but k, its CV folds are the
    other folds in ascending order, fold j = the two arm segments (2j, 2j + 1)."""
    return [[(2 * j, 2 * j + 1) for j in range(K) if j != k] for k in range(K)]


def irm_fit_phases(pan, folds: int, lambda_rule="min", comm=None, seg_counts=None,
                   nuisances=NUISANCES, propensity="linear"):
    """The phases of :func:`irm_phases` up to the fitted coefficients (A, C01, B; state "G",
    "cv", "coef"), shared with the group-effect estimator (estimators/gate.py), and the
    factory ``reduce(name)`` of an all-reduce phase of a state tensor (None at world 1).

    nuisances: the subset of (0: g0, 1: g1, 2: m) to fit (estimators/targets.py: the effect
    on the treated needs no g1, the effect on the controls no g0). Only those
    ``len(nuisances) K K`` problems go into the one path launch; the picked
    coefficients are scattered into "coef" [K, 3, p+1], whose other rows are zero. The launch
    keeps the lambda ratio of the whole fit (``default_lambda_min_ratio`` over the training
    sets of all three nuisances), so a nuisance does not depend on which others are fitted
    beside it. The default fits all three with today's call.

    propensity "logit": the gaussian launch names only the requested ones of g0 and g1 (the
    subset path above: their coefficients carry the bits of the linear fit), and ONE grouped
    binomial launch (``ops.lognet.cv_lognet_groups``: the K outer training sets, then their
    K (K - 1) inner folds) fits m; row 2 of "coef" then holds logit coefficients, for the
    logistic link of the score pass. State "cv_m": the binomial fit. Limits:
    :func:`check_logit_scope`."""
    dist = comm is not None and comm.world_size > 1
    K = folds
    logit = check_propensity(propensity) == "logit"
    check_logit_scope(propensity, len(pan.xcols), K, pan.dtype, comm)
    if seg_counts is None:
        seg_counts = global_seg_counts(pan, comm) if dist else np.asarray(pan.seg_nreal)
    counts = np.asarray(seg_counts, dtype=np.float64)
    check_cells(counts, K)
    if pan.nseg != 2 * K:
        raise ValueError(f"DML-IRM needs {2 * K} segments, this shard's panel has {pan.nseg}")
    nuisances = check_nuisances(nuisances)
    fit_m = logit and 2 in nuisances
    if logit:
        nuisances = tuple(r for r in nuisances if r != 2)
    if not nuisances:
        raise ValueError('propensity="logit" needs an outcome regression (g0 or g1) among the '
                         "nuisances")
    counts3, full_sets, full_y, ycols = fit_problems(pan, K, counts, nuisances)
    subset = nuisances != NUISANCES
    ratio = None
    if subset:
        _, sets_all, _, _ = fit_problems(pan, K, counts)
        ratio = default_lambda_min_ratio(min(counts3[list(fs)].sum() for fs in sets_all),
                                         len(pan.xcols))
        slots = const(nuisances, torch.int64, pan.device)

    def phase_fit(st):
        G = st["G"]
        G3 = torch.cat([G, G[0::2] + G[1::2]])
        cv = cv_enet_gaussian(G3, pan, pan.xcols, ycols, full_sets=full_sets,
                              seg_counts=counts3, full_y=full_y, lambda_min_ratio=ratio)
        coef = (cv.coef_min if lambda_rule == "min" else cv.coef_1se)
        if subset:
            some = coef.reshape(K, len(nuisances), -1).double()
            coef = torch.zeros(K, 3, some.shape[2], dtype=torch.float64, device=some.device)
            coef.index_copy_(1, slots, some)
            if fit_m:
                from ..ops.lognet import cv_lognet_groups
                cvm = cv_lognet_groups(pan, pan.xcols, pan.cols["W"], logit_fold_sets(K))
                coef[:, 2] = cvm.coef_min if lambda_rule == "min" else cvm.coef_1se
                return {**st, "cv": cv, "cv_m": cvm, "coef": coef}
            return {**st, "cv": cv, "coef": coef}
        return {**st, "cv": cv, "coef": coef.reshape(K, 3, -1).double().contiguous()}

    phases, reduce = gram_phases(pan, comm)
    phases.append(phase_fit)
    return phases, reduce


def phase_scores(pan, clip, link="identity"):
    """The phase after :func:`irm_fit_phases` of every estimator on the per-row scores:
    state "psi" [ld] (csrc/irm.hip ``ate_irm_scores``; link: that of the propensity fit,
    :func:`propensity_link`)."""
    def f(st):
        return {**st, "psi": irm_scores(pan, st["coef"], clip, 2, link=link)}
    return f


def run_phases(phases) -> dict:
    """Run a phase list eagerly to its final state."""
    st = None
    for ph in phases:
        st = ph(st)
    return st


def irm_crossfit_panel(pan, folds: int, lambda_rule="min", clip=0.01, comm=None,
                       seg_counts=None, propensity="linear"):
    """DML-IRM on an arm-split fold panel (segment 2k + a = fold k, W = a; from host arrays
    ``build_panel(X, W, Y, folds=2 * fold + W)``, at scale
    ``data.device_dgp.synthetic_panel(arm_split=True)``). Returns (res[2], mom[8], cv).

    comm: optional parallel.comm.Communicator -- each rank holds a row shard of every
    segment; the Gram stack and the score moments are all-reduced. seg_counts: global rows
    per segment (one all-reduce when omitted). A truncated CV fold path NaN-poisons the
    picked coefficients (ops/enet), and through them res."""
    st = run_phases(irm_phases(pan, folds, lambda_rule, clip, comm, seg_counts, propensity))
    return st["res"], st["mom"], st.get("cv")


# ---------------------------------------------------------------- repeated cross-fitting
def check_partition_cells(counts, folds: int, repeats: int):
    """The sibling of :func:`check_cells` for the micro layout (segment 2m + a = micro-group
    m, arm a; K*K micro-groups): every (fold, arm) cell of every used partition
    (``lasso.micro_fold_map``) needs a row. A micro-group with an empty arm is legal."""
    K = folds
    c = np.asarray(counts, dtype=np.float64)
    if len(c) != 2 * K * K:
        raise ValueError(f"repeated DML-IRM needs 2*K*K = {2 * K * K} segments (micro-group m, "
                         f"arm a -> 2m + a), the panel has {len(c)}")
    for s in range(repeats):
        fold = micro_fold_map(K, s)
        for a in (0, 1):
            cell = np.bincount(fold, weights=c[a::2], minlength=K)
            for k in np.flatnonzero(cell <= 0):
                raise ValueError(f"empty (fold, arm) cell in partition {s}: fold {int(k)}, "
                                 f"arm W={a} has no rows")


def _path_launches(ratios, cap):
    """Consecutive partitions grouped into as few path launches as possible: at most ``cap``
    partitions per launch, evenly filled, and only partitions with the same lambda ratio
    share one (``cv_enet_gaussian`` picks one ratio per launch: a partition keeps the ratio,
    and so the bits, of its own solve). Returns [(first, last + 1), ...]."""
    out, s, S = [], 0, len(ratios)
    while s < S:
        e = s
        while e < S and ratios[e] == ratios[s]:
            e += 1
        n = e - s
        nl = -(-n // cap)
        for i in range(nl):
            out.append((s + i * n // nl, s + (i + 1) * n // nl))
        s = e
    return out


def irm_repeated_phases(pan, folds: int, repeats: int, lambda_rule="min", clip=0.01, comm=None,
                        seg_counts=None, aggregate="median"):
    """Repeated K-fold cross-fitting of DML-IRM (Chernozhukov et al. 2018 §3.4): ``repeats``
    = S partitions of the rows, one cross-fitted AIPW fit per partition, median-aggregated
    (``lasso.median_aggregate``). The panel holds 2*K*K segments, segment 2m + a = micro-group
    m, arm a; partition s puts micro-group m = K a' + b in fold (a' + s b) mod K
    (``lasso.micro_fold_map``). As for ``ate_dml(repeats=)`` the partitions are built from ONE
    assignment to K*K micro-groups, so they are correlated (two partitions share one
    micro-group per fold pair), and there are at most K of them: 1 <= repeats <= K. Phases
    (utils.graphs.SegmentedStep captures them, one graph at world 1):

    A  the 2 K*K micro-arm Gram stack (K01): tile kernel, slab reduce, ONCE   device
    C01 symmetric all-reduce of the stack over row shards                     collective
    B  per partition the 2K fold-arm Grams (a 0/1 matrix times the stack, fp64) and their K
       arm sums: the 3K-segment stack of :func:`fit_problems`; all partitions' problems in
       as few path launches as ``ate_enet_path`` admits (256 co-resident problems), each
       holding whole partitions with segment ids offset per partition                device
    B' ONE fused score pass for all S partitions (csrc/irm.hip
       ``ate_irm_score_moments_multi``), blk[s][m] = s K + fold of m under s        device
    C06 one all-reduce of the [S, 8] moments                                   collective
    C  theta / SE per split, the aggregate                                      device

    A partition's coefficients carry the bits of solving that partition alone: its problems
    name only its own 3K segments. The result state holds "res" [2] (the aggregate), "splits"
    [S, 2], "mom" [S, 8] and "coef" [S K, 3, p+1]. Raises ValueError, before any device work,
    when one partition alone exceeds the path launch (large K)."""
    K, Sn = folds, repeats
    if pan.nseg != 2 * K * K:
        raise ValueError(f"repeated DML-IRM needs 2*K*K = {2 * K * K} micro-arm segments, the "
                         f"panel has {pan.nseg}")
    if not 1 <= Sn <= K:
        raise ValueError(f"repeats must be in 1..{K} (distinct partitions of K*K micro-groups)")
    dist = comm is not None and comm.world_size > 1
    if seg_counts is None:
        seg_counts = global_seg_counts(pan, comm) if dist else np.asarray(pan.seg_nreal)
    counts = np.asarray(seg_counts, dtype=np.float64)
    check_partition_cells(counts, K, Sn)
    dev, P, p = pan.device, pan.P, len(pan.xcols)
    maps = [micro_fold_map(K, s) for s in range(Sn)]
    # partition s: fold-arm segment 2k + a = the sum of the micro-arm segments 2m + a, m in k
    M = np.zeros((Sn, 2 * K, 2 * K * K))
    for s, fold in enumerate(maps):
        for a in (0, 1):
            M[s, 2 * fold + a, 2 * np.arange(K * K) + a] = 1.0
    cell_counts = M @ counts                                              # [Sn, 2K]
    probs = [fit_problems(pan, K, cc) for cc in cell_counts]             # per partition
    _, sets1, full_y1, ycols = probs[0]
    per = cv_problem_count(3 * K, sets1, len(ycols), full_y1)
    if per > MAX_PATH_PROBLEMS:
        raise ValueError(f"one partition of K = {K} folds is {per} path problems, more than "
                         f"the {MAX_PATH_PROBLEMS} one path launch holds")
    Mall = const(M.reshape(Sn * 2 * K, 2 * K * K), torch.float64, dev)
    # the lambda ratio cv_enet_gaussian picks for the partition alone
    ratios = [default_lambda_min_ratio(min(c3[list(fs)].sum() for fs in sets1), p)
              for c3, *_ in probs]
    launches = _path_launches(ratios, MAX_PATH_PROBLEMS // per)
    blk = np.stack([s * K + maps[s] for s in range(Sn)])                 # [Sn, K*K]

    def phase_fit(st):
        Gfa = (Mall @ st["G"].view(2 * K * K, P * P)).view(Sn, 2 * K, P, P)
        G3 = torch.cat([Gfa, Gfa[:, 0::2] + Gfa[:, 1::2]], 1)           # [Sn, 3K, P, P]
        coefs = []
        for s0, s1 in launches:
            n = s1 - s0
            cv = cv_enet_gaussian(
                G3[s0:s1].reshape(n * 3 * K, P, P), pan, pan.xcols, ycols,
                full_sets=[[i * 3 * K + q for q in fs] for i in range(n) for fs in sets1],
                seg_counts=np.concatenate([probs[s][0] for s in range(s0, s1)]),
                full_y=full_y1 * n, lambda_min_ratio=ratios[s0])
            coefs.append((cv.coef_min if lambda_rule == "min" else cv.coef_1se)
                         .reshape(n * K, 3, -1))
        return {**st, "coef": torch.cat(coefs).double().contiguous()}

    def phase_score(st):
        return {**st, "mom": irm_score_moments_multi(pan, st["coef"], blk, clip, 2)}

    def phase_final(st):
        res = torch.stack([irm_finalize(st["mom"][s]) for s in range(Sn)])
        return {**st, "splits": res, "res": median_aggregate(res[:, 0], res[:, 1], aggregate)}

    phases, reduce = gram_phases(pan, comm)
    phases += [phase_fit, phase_score]
    if reduce is not None:
        phases.append(reduce("mom"))
    phases.append(phase_final)
    return phases


def irm_repeated_panel(pan, folds: int, repeats: int, lambda_rule="min", clip=0.01, comm=None,
                       seg_counts=None, aggregate="median"):
    """Eager run of :func:`irm_repeated_phases` on a micro-arm panel (from host arrays
    ``build_panel(folds=2 * micro + W)``, at scale ``synthetic_panel(folds=K * K,
    arm_split=True)``): (aggregate [2], splits [S, 2], mom [S, 8])."""
    st = run_phases(irm_repeated_phases(pan, folds, repeats, lambda_rule, clip, comm,
                                        seg_counts, aggregate))
    return st["res"], st["splits"], st["mom"]


# ---------------------------------------------------------------- the shared front end
def arm_split_panel(Y, W, X, folds, seed, dtype, device, dist=None, extra_counts=None,
                    check_extra=None, cells=check_cells, targets=None, fold_ids=None):
    """The prologue of every ``dml_irm_*`` estimator: the binary-W check, the fold ids, the
    (global) rows per (fold, arm) cell and the arm-split panel (segment 2k + a = fold k,
    W = a) on ``device``. Returns (pan, counts [2K], extra, n_total, rid).

    extra_counts: further local counts of the caller (rows per group, per span, ...). Over
    row shards they are summed in the one all-reduce that sums the cell counts, come back as
    ``extra`` and are handed to ``check_extra`` before the panel is built. rid: the rows'
    global ids in panel row order (the key of the bootstrap multipliers), -1 on padding.
    cells: the check of the cell counts, ``cells(counts, folds)`` (repeated cross-fitting
    passes its own: its K*K micro-groups may have an empty arm). targets: further named
    target columns of the panel (``build_panel(targets=)``; estimators/late.py: the treatment
    taken D beside the instrument in column W). fold_ids: an explicit fold of every row
    (estimators/cluster.py: whole clusters per fold) instead of the Philox assignment."""
    dev = resolve_device(device)
    Yn, Wn, Xn = as_np(Y), as_np(W), as_np(X)
    if not np.isin(Wn, (0.0, 1.0)).all():
        raise ValueError("DML-IRM needs a binary treatment: W must be exactly 0 or 1")
    fid = _fold_ids(len(Yn), folds, seed, 0, dist) if fold_ids is None else fold_ids
    seg = 2 * np.asarray(fid, dtype=np.int64) + Wn.astype(np.int64)
    counts = np.bincount(seg, minlength=2 * folds).astype(np.float64)
    extra = None if extra_counts is None else np.asarray(extra_counts, dtype=np.float64)
    if dist is not None and dist.world > 1:
        t = torch.as_tensor(counts if extra is None else np.concatenate([counts, extra])).to(dev)
        dist.sum_(t)
        t = t.cpu().numpy()
        counts, extra = t[:2 * folds], None if extra is None else t[2 * folds:]
    if check_extra is not None:
        check_extra(extra)
    cells(counts, folds)
    pan = build_panel(Xn, Wn, Yn, folds=seg, dtype=dtype, device=dev, nseg=2 * folds,
                      targets=targets)
    rid = torch.where(pan.row_index >= 0,
                      pan.row_index + (dist.row_offset if dist is not None else 0),
                      torch.full_like(pan.row_index, -1))
    return pan, counts, extra, (dist.n_total if dist is not None else len(Yn)), rid


def comm_counts(dist, counts):
    """(comm, seg_counts) of a ``*_panel`` call from a body's trailing (dist, counts)."""
    return (dist.comm if dist is not None else None,
            None if counts is None else np.asarray(counts))


def run_body(name, body, tensors, *args, graph=True, dist=None):
    """``body(*tensors, *args)`` as one captured hipGraph (``estimator_graphs`` entry
    ``name``: first call of a layout eager, captured on the second, replayed after) when
    ``graph`` is set, the panel ``tensors[0]`` is on a GPU and the collectives of ``dist`` can
    be captured; otherwise a direct call. Returns (out, replayed)."""
    if graph and (dist is None or dist.capturable) and tensors[0].data.is_cuda:
        return estimator_graphs.run(name, body, tensors, *args)
    return body(*tensors, *args), False


def propensity_args(propensity) -> tuple:
    """The trailing static argument of a graph body for the propensity fit: none for the
    default (its cache key and call stay what they were), the name otherwise."""
    return () if check_propensity(propensity) == "linear" else (propensity,)


def _irm_body(pan, folds, lambda_rule, clip, dist=None, counts=None, propensity="linear"):
    """The whole cross-fit as one device function (GraphCache captures it): [res, mom]."""
    comm, seg_counts = comm_counts(dist, counts)
    res, mom, _ = irm_crossfit_panel(pan, folds, lambda_rule, clip, comm=comm,
                                     seg_counts=seg_counts, propensity=propensity)
    return torch.cat([res, mom])


def dml_irm_lasso(Y, W, X, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                  method="DML-IRM cross-fit (LASSO)", device=None, dtype="f64", dist=None,
                  graph=True, propensity="linear"):
    """K-fold cross-fitted AIPW (interactive model) with CV-LASSO nuisances: per-arm
    outcome regressions and the linear-probability propensity, each with an inner CV over
    the other K-1 folds (the fold stream of dml_plr_lasso). W must be exactly {0, 1}.
    Matches reference.estimators.dml_irm_lasso.

    graph: on a GPU (alone, or row-sharded over RCCL) the estimator runs as one captured
    hipGraph (first call of a panel layout eager, captured on the second, replayed after).
    diagnostics: n, n_clipped (propensities outside [clip, 1-clip]), n_treated, the held-out
    RMSE of the three nuisances, hipgraph.

    propensity: "linear" (default) or "logit": m by the binomial CV-LASSO
    (cv.glmnet(family="binomial") on the same training rows and inner folds; all K * K fits
    in one launch), the score through the logistic link; diagnostics gain ``propensity``.
    Limits of "logit": one partition, no ``dist``, an fp32 / fp64 panel, p <= 96, K <= 16."""
    check_logit_scope(propensity, X, folds, dtype, dist)
    pan, counts, _, n, _ = arm_split_panel(Y, W, X, folds, seed, dtype, device, dist)
    out, g = run_body("dml_irm", _irm_body, (pan,), folds, lambda_rule, float(clip), dist,
                      tuple(counts.tolist()), *propensity_args(propensity), graph=graph,
                      dist=dist)
    v = out.detach().double().cpu().numpy()
    mom = v[2:]
    nt = mom[7]
    diag = dict(n=n, n_clipped=int(round(mom[3])) if np.isfinite(mom[3]) else -1,
                n_treated=int(round(nt)) if np.isfinite(nt) else -1,
                rmse_g0=float(np.sqrt(mom[5] / (mom[2] - nt))),
                rmse_g1=float(np.sqrt(mom[4] / nt)), rmse_m=float(np.sqrt(mom[6] / mom[2])),
                hipgraph=g)
    if propensity != "linear":
        diag["propensity"] = propensity
    return AteResult.make(method, v[0], v[1], **diag)


def _irm_repeated_body(pan, folds, repeats, lambda_rule, clip, aggregate, dist=None,
                       counts=None):
    """The whole repeated cross-fit as one device function: [res, splits, mom] flattened."""
    comm, seg_counts = comm_counts(dist, counts)
    res, splits, mom = irm_repeated_panel(pan, folds, repeats, lambda_rule, clip, comm,
                                          seg_counts, aggregate)
    return torch.cat([res, splits.reshape(-1), mom.reshape(-1)])


def dml_irm_lasso_repeated(Y, W, X, folds=5, repeats=3, seed=1991, lambda_rule="min",
                           clip=0.01, aggregate="median",
                           method="DML-IRM cross-fit (LASSO, repeated)", device=None,
                           dtype="f64", dist=None, graph=True):
    """``repeats`` = S K-fold cross-fitted AIPW fits on S partitions of the rows, aggregated
    by the median rule (:func:`irm_repeated_phases`; "mean": the means). Rows go to K*K
    micro-groups by the balanced Philox assignment of ``dml_plr_lasso_repeated`` (stream 0);
    partition s is ``micro_fold_map(K, s)``, so 1 <= repeats <= K and the partitions are
    correlated. One Gram pass and one fused score pass serve all partitions; on a GPU the
    call is one captured hipGraph. Matches reference.estimators.dml_irm_lasso_repeated.
    diagnostics: n, repeats, aggregate, splits (the S (ATE, SE) pairs), n_clipped per split,
    n_treated, hipgraph."""
    K = folds
    if not 1 <= repeats <= K:
        raise ValueError(f"repeats must be in 1..{K} (distinct partitions of K*K micro-groups)")
    pan, counts, _, n, _ = arm_split_panel(
        Y, W, X, K * K, seed, dtype, device, dist,
        cells=lambda c, _: check_partition_cells(c, K, repeats))
    out, g = run_body("dml_irm_repeated", _irm_repeated_body, (pan,), K, repeats, lambda_rule,
                      float(clip), aggregate, dist, tuple(counts.tolist()), graph=graph,
                      dist=dist)
    v = out.detach().double().cpu().numpy()
    splits = v[2:2 + 2 * repeats].reshape(repeats, 2)
    mom = v[2 + 2 * repeats:].reshape(repeats, N_MOMENTS)

    def count(x):
        return int(round(x)) if np.isfinite(x) else -1
    return AteResult.make(method, v[0], v[1], n=n, repeats=repeats, aggregate=aggregate,
                          splits=splits.tolist(), n_clipped=[count(x) for x in mom[:, 3]],
                          n_treated=count(mom[0, 7]), hipgraph=g)
