"""Cross-fitted AIPW for the interactive regression model (DML-IRM, Chernozhukov et al.
2018 §5.1) with CV-LASSO nuisances on the fold Gram stack.

Where ``lasso.dml_plr_lasso`` estimates the one coefficient of the partially linear model
(the ATE only under a constant effect), this estimator fits the outcome regression per arm,
g0(X) = E[Y|X, W=0] and g1(X) = E[Y|X, W=1], and the linear-probability propensity
m(X) = E[W|X], all by gaussian CV-LASSO, and averages the doubly robust score

    psi = g1 - g0 + w (y - g1) / m - (1 - w)(y - g0) / (1 - m),   m clipped to [clip, 1-clip]

over held-out rows (textbook signs, as ``crossfit.aipw_score``).

Layout: a 2K-segment panel, segment ``2k + a`` = the rows of fold k with W = a. One Gram
pass (K01) then yields per-(fold, arm) Grams; the fold Grams of the propensity problems are
their pairwise sums. All 3 K (K + 1) path problems (3 nuisances x K outer folds x (1 full +
K - 1 inner CV)) run in ONE ``ate_enet_path`` launch (``ops/enet.cv_enet_gaussian(full_y=)``),
and one fused pass over the panel (csrc/irm.hip) accumulates the 8 score moments.

The estimators on the same score (gate, cate, policy, sensitivity) share what lives here: the
score pass in its three forms (:func:`irm_score_moments`, :func:`irm_sens_moments`,
:func:`irm_scores` -- one CPU twin ``_score_terms``, one launcher ``_score_launch``), the
front end of every ``dml_irm_*`` function (:func:`arm_split_panel`, :func:`run_body`,
:func:`comm_counts`), the fit and score phases (:func:`irm_fit_phases`, :func:`phase_scores`,
:func:`run_phases`) and the n - 1 variance rule (:func:`mean_se`).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..ops.devconst import const
from ..ops.enet import cv_enet_gaussian
from ..ops.gram import gram
from ..ops.panel import build_panel, dtype_code
from ..result import SENS_MOMENTS, AteResult
from ..utils.graphs import estimator_graphs
from .common import as_np, resolve_device
from .lasso import _fold_ids, _tri_index, allreduce_sym_, global_seg_counts

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


def _score_terms(pan, coef, segs_per_fold):
    """The float64 CPU twin of the score pass (the kernels' oracle): per segment
    ``(r0, r1, v, y, w, g0, g1, m)`` -- its row range, the mask of its real rows, and over
    those rows the targets, the two outcome regressions and the unclipped propensity."""
    _score_args(pan, coef, segs_per_fold)
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
        yield (r0, r1, v, y, w, c[k, 0, 0] + c[k, 0, 1:] @ xs, c[k, 1, 0] + c[k, 1, 1:] @ xs,
               c[k, 2, 0] + c[k, 2, 1:] @ xs)


def aipw_psi(y, w, g0, g1, e):
    """The AIPW score with the clipped propensity ``e`` (the module docstring's psi)."""
    return g1 - g0 + w * (y - g1) / e - (1.0 - w) * (y - g0) / (1.0 - e)


def _score_launch(name, pan, coef, clip, segs_per_fold, nbx, n_out, moments):
    """One instantiation of the fused score pass (csrc/irm.hip entry point ``name``) with
    ``nbx`` blocks per segment. ``moments``: the entry point sums ``n_out`` moments (a
    ``partial`` workspace, then the result); otherwise it writes ``n_out`` = ld row scores."""
    p = _score_args(pan, coef, segs_per_fold)
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
    cs, bs = pan.strides()
    _native.call(name, dtype_code(pan.data), pan.data.data_ptr(), cs, bs, xc.data_ptr(), p,
                 segs.data_ptr(), pan.nseg, segs_per_fold, c.data_ptr(), y0, y1, w0, w1,
                 pan.cols["one"], float(clip), nbx, *(b.data_ptr() for b in bufs),
                 torch.cuda.current_stream().cuda_stream)
    return out


def irm_score_moments(pan, coef: torch.Tensor, clip: float = 0.01, segs_per_fold: int = 2,
                      nbx: int | None = None) -> torch.Tensor:
    """Fused held-out AIPW score pass -> the 8 fp64 moments (N_MOMENTS).

    coef: [nfold, 3, p+1] fp64, rows (g0, g1, m), intercept first; segment s of the panel
    uses block ``s // segs_per_fold`` (2: the arm-split layout; 1: a plain K-fold panel).
    W is read from the panel on every row. GPU: csrc/irm.hip (``nbx`` blocks per segment);
    CPU: the float64 torch twin (:func:`_score_terms`), the kernel's oracle."""
    if pan.data.is_cuda:
        return _score_launch("ate_irm_score_moments", pan, coef, clip, segs_per_fold, nbx,
                             N_MOMENTS, True)
    mom = torch.zeros(N_MOMENTS, dtype=torch.float64)
    lo, hi = clip, 1.0 - clip
    for _, _, _, y, w, g0, g1, m in _score_terms(pan, coef, segs_per_fold):
        psi = aipw_psi(y, w, g0, g1, m.clamp(lo, hi))
        one = torch.ones_like(psi)
        mom += torch.stack([psi.sum(), (psi * psi).sum(), one.sum(),
                            ((m < lo) | (m > hi)).double().sum(),
                            (w * (y - g1) ** 2).sum(), ((1.0 - w) * (y - g0) ** 2).sum(),
                            ((w - m) ** 2).sum(), w.sum()])
    return mom


def irm_sens_moments(pan, coef: torch.Tensor, clip: float = 0.01, segs_per_fold: int = 2,
                     nbx: int | None = None) -> torch.Tensor:
    """The pass of :func:`irm_score_moments` -- same arguments, same dot products, same psi --
    accumulating the 14 fp64 moments of the sensitivity analysis (``result.SENS_MOMENTS``;
    estimators/sensitivity.py). GPU: csrc/irm.hip ``ate_irm_sens_moments`` (for the same
    ``nbx`` S psi, S psi^2, n, n_clipped and n_treated carry the bits of
    ``irm_score_moments``); CPU: the float64 torch twin."""
    if pan.data.is_cuda:
        return _score_launch("ate_irm_sens_moments", pan, coef, clip, segs_per_fold, nbx,
                             len(SENS_MOMENTS), True)
    mom = torch.zeros(len(SENS_MOMENTS), dtype=torch.float64)
    lo, hi = clip, 1.0 - clip
    for _, _, _, y, w, g0, g1, m in _score_terms(pan, coef, segs_per_fold):
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


def irm_scores(pan, coef: torch.Tensor, clip: float = 0.01, segs_per_fold: int = 2,
               nbx: int | None = None) -> torch.Tensor:
    """The per-row AIPW scores psi [ld] (fp64, panel row order, 0 on padding rows): the pass
    of :func:`irm_score_moments` -- same arguments, same dot products, same psi -- writing
    every row's score instead of summing moments (csrc/irm.hip ``ate_irm_scores``; CPU: the
    float64 torch twin). Input of the estimators on the scores (gate, cate, policy)."""
    if pan.data.is_cuda:
        bounds = np.asarray(pan.seg_bounds, dtype=np.int64)
        if bounds[0, 0] != 0 or bounds[-1, 1] != pan.ld or np.any(bounds[1:, 0] != bounds[:-1, 1]):
            raise ValueError("the panel's segments must tile [0, ld): every row gets a score")
        return _score_launch("ate_irm_scores", pan, coef, clip, segs_per_fold, nbx, pan.ld, False)
    psi = torch.zeros(pan.ld, dtype=torch.float64)
    for r0, r1, v, y, w, g0, g1, m in _score_terms(pan, coef, segs_per_fold):
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


def irm_phases(pan, folds: int, lambda_rule="min", clip=0.01, comm=None, seg_counts=None):
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
    "res" [2], "mom" [8], "coef" [K, 3, p+1] and "cv"."""
    phases, reduce = irm_fit_phases(pan, folds, lambda_rule, comm, seg_counts)

    def phase_score(st):
        return {**st, "mom": irm_score_moments(pan, st["coef"], clip, 2)}

    def phase_final(st):
        return {**st, "res": irm_finalize(st["mom"])}

    phases.append(phase_score)
    if reduce is not None:
        phases.append(reduce("mom"))
    phases.append(phase_final)
    return phases


def fit_problems(pan, K: int, counts):
    """The 3 K nuisance problems on the 3K-Gram stack ``cat([G, G[0::2] + G[1::2]])`` as
    arguments of ``cv_enet_gaussian``: (seg_counts, full_sets, full_y, ycols). Segments of
    the stack: 2s + a = (fold s, arm a); 2K + s = fold s, both arms. ``counts``: (global)
    rows per panel segment."""
    counts = np.asarray(counts, dtype=np.float64)
    counts3 = np.concatenate([counts, counts[0::2] + counts[1::2]])
    full_sets, full_y = [], []
    for k in range(K):
        others = [s for s in range(K) if s != k]
        full_sets += [[2 * s for s in others], [2 * s + 1 for s in others],
                      [2 * K + s for s in others]]
        full_y += [0, 0, 1]                       # g0, g1: target Y; m: target W
    return counts3, full_sets, full_y, [pan.cols["Y"], pan.cols["W"]]


def irm_fit_phases(pan, folds: int, lambda_rule="min", comm=None, seg_counts=None):
    """The phases of :func:`irm_phases` up to the fitted coefficients (A, C01, B; state "G",
    "cv", "coef"), shared with the group-effect estimator (estimators/gate.py), and the
    factory ``reduce(name)`` of an all-reduce phase of a state tensor (None at world 1)."""
    from ..utils.graphs import Collective
    dist = comm is not None and comm.world_size > 1
    K = folds
    if seg_counts is None:
        seg_counts = global_seg_counts(pan, comm) if dist else np.asarray(pan.seg_nreal)
    counts = np.asarray(seg_counts, dtype=np.float64)
    check_cells(counts, K)
    if pan.nseg != 2 * K:
        raise ValueError(f"DML-IRM needs {2 * K} segments, this shard's panel has {pan.nseg}")
    counts3, full_sets, full_y, ycols = fit_problems(pan, K, counts)

    def phase_gram(_):
        return {"G": gram(pan, stage="tiles")}

    def phase_gram_reduce(st):
        return {"G": gram(pan, stage="reduce", out=st["G"])}

    def phase_fit(st):
        G = st["G"]
        G3 = torch.cat([G, G[0::2] + G[1::2]])
        cv = cv_enet_gaussian(G3, pan, pan.xcols, ycols, full_sets=full_sets,
                              seg_counts=counts3, full_y=full_y)
        coef = (cv.coef_min if lambda_rule == "min" else cv.coef_1se).reshape(K, 3, -1)
        return {**st, "cv": cv, "coef": coef.double().contiguous()}

    cap = bool(getattr(comm, "capturable", False))

    def reduce(name):
        def f(st):
            comm.all_reduce_(st[name])
            return st
        return Collective(f, capturable=cap)     # RCCL: captured inside the step's graph

    def reduce_sym(name):
        _tri_index(pan.P, pan.device)            # built here, never inside a capture

        def f(st):
            allreduce_sym_(comm, st[name])
            return st
        return Collective(f, capturable=cap)

    phases = [phase_gram, phase_gram_reduce]
    if dist:
        phases.append(reduce_sym("G"))
    phases.append(phase_fit)
    return phases, (reduce if dist else None)


def phase_scores(pan, clip):
    """The phase after :func:`irm_fit_phases` of every estimator on the per-row scores:
    state "psi" [ld] (csrc/irm.hip ``ate_irm_scores``)."""
    def f(st):
        return {**st, "psi": irm_scores(pan, st["coef"], clip, 2)}
    return f


def run_phases(phases) -> dict:
    """Run a phase list eagerly to its final state."""
    st = None
    for ph in phases:
        st = ph(st)
    return st


def irm_crossfit_panel(pan, folds: int, lambda_rule="min", clip=0.01, comm=None,
                       seg_counts=None):
    """DML-IRM on an arm-split fold panel (segment 2k + a = fold k, W = a; from host arrays
    ``build_panel(X, W, Y, folds=2 * fold + W)``, at scale
    ``data.device_dgp.synthetic_panel(arm_split=True)``). Returns (res[2], mom[8], cv).

    comm: optional parallel.comm.Communicator -- each rank holds a row shard of every
    segment; the Gram stack and the score moments are all-reduced. seg_counts: global rows
    per segment (one all-reduce when omitted). A truncated CV fold path NaN-poisons the
    picked coefficients (ops/enet), and through them res."""
    st = run_phases(irm_phases(pan, folds, lambda_rule, clip, comm, seg_counts))
    return st["res"], st["mom"], st.get("cv")


# ---------------------------------------------------------------- the shared front end
def arm_split_panel(Y, W, X, folds, seed, dtype, device, dist=None, extra_counts=None,
                    check_extra=None):
    """The prologue of every ``dml_irm_*`` estimator: the binary-W check, the fold ids, the
    (global) rows per (fold, arm) cell and the arm-split panel (segment 2k + a = fold k,
    W = a) on ``device``. Returns (pan, counts [2K], extra, n_total, rid).

    extra_counts: further local counts of the caller (rows per group, per span, ...). Over
    row shards they are summed in the one all-reduce that sums the cell counts, come back as
    ``extra`` and are handed to ``check_extra`` before the panel is built. rid: the rows'
    global ids in panel row order (the key of the bootstrap multipliers), -1 on padding."""
    dev = resolve_device(device)
    Yn, Wn, Xn = as_np(Y), as_np(W), as_np(X)
    if not np.isin(Wn, (0.0, 1.0)).all():
        raise ValueError("DML-IRM needs a binary treatment: W must be exactly 0 or 1")
    fid = _fold_ids(len(Yn), folds, seed, 0, dist)
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
    check_cells(counts, folds)
    pan = build_panel(Xn, Wn, Yn, folds=seg, dtype=dtype, device=dev)
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


def _irm_body(pan, folds, lambda_rule, clip, dist=None, counts=None):
    """The whole cross-fit as one device function (GraphCache captures it): [res, mom]."""
    comm, seg_counts = comm_counts(dist, counts)
    res, mom, _ = irm_crossfit_panel(pan, folds, lambda_rule, clip, comm=comm,
                                     seg_counts=seg_counts)
    return torch.cat([res, mom])


def dml_irm_lasso(Y, W, X, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                  method="DML-IRM cross-fit (LASSO)", device=None, dtype="f64", dist=None,
                  graph=True):
    """K-fold cross-fitted AIPW (interactive model) with CV-LASSO nuisances: per-arm
    outcome regressions and the linear-probability propensity, each with an inner CV over
    the other K-1 folds (the fold stream of dml_plr_lasso). W must be exactly {0, 1}.
    Matches reference.estimators.dml_irm_lasso.

    graph: on a GPU (alone, or row-sharded over RCCL) the estimator runs as one captured
    hipGraph (first call of a panel layout eager, captured on the second, replayed after).
    diagnostics: n, n_clipped (propensities outside [clip, 1-clip]), n_treated, the held-out
    RMSE of the three nuisances, hipgraph."""
    pan, counts, _, n, _ = arm_split_panel(Y, W, X, folds, seed, dtype, device, dist)
    out, g = run_body("dml_irm", _irm_body, (pan,), folds, lambda_rule, float(clip), dist,
                      tuple(counts.tolist()), graph=graph, dist=dist)
    v = out.detach().double().cpu().numpy()
    mom = v[2:]
    nt = mom[7]
    diag = dict(n=n, n_clipped=int(round(mom[3])) if np.isfinite(mom[3]) else -1,
                n_treated=int(round(nt)) if np.isfinite(nt) else -1,
                rmse_g0=float(np.sqrt(mom[5] / (mom[2] - nt))),
                rmse_g1=float(np.sqrt(mom[4] / nt)), rmse_m=float(np.sqrt(mom[6] / mom[2])),
                hipgraph=g)
    return AteResult.make(method, v[0], v[1], **diag)
