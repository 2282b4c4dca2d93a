"""Average potential outcomes of a MULTI-VALUED treatment under the cross-fitted interactive
model (DML-APOS: DoubleML ``DoubleMLAPO`` / ``DoubleMLAPOS`` with ``causal_contrast``, grf
``multi_arm_causal_forest``) with CV-LASSO nuisances on the fold Gram stack: the mean outcome
of every arm, every arm's effect against a reference arm with a joint covariance, and a band
that holds for all arms at once. The tutorial's mailing experiment has one control group and
four mailings; ``estimators/irm.py`` can look at one mailing at a time, this estimator at all.

D takes L distinct values, 2 <= L <= 8, coded to levels 0..L-1 in ascending order of value.
For held-out fold k and level c the nuisances are gaussian CV-LASSO fits with the inner CV of
``irm.dml_irm_lasso``:

    g_c(X) = E[Y | X, D = c]      on the training rows with D = c
    m_c(X) = P(D = c | X)         on all training rows, target 1{D = c} (one-vs-rest; the L
                                   propensities are fitted independently, as DoubleML APOS)

and a row of level d, with e = clip(m_d, clip, 1 - clip), scores

    psi_c = g_c(X) + 1{c = d} (Y - g_d(X)) / e            c = 0..L-1

theta_c = mean(psi_c); Cov(theta) from the second moments of psi under the n - 1 rule of
``irm.mean_se``; the contrast of level c against a reference r is theta_c - theta_r with
variance V_cc + V_rr - 2 V_cr.

Layout: the level-split fold panel, segment ``L k + c`` = the rows of fold k with D = c, with
the level in a target column ``D`` and the L indicators in ``I0 .. I{L-1}``
(:func:`level_split_panel`). One Gram pass gives the per-(fold, level) Grams, the fold Grams
of the propensity problems are their sums over the levels, the 2 L K K path problems run in
as few ``ate_enet_path`` launches as hold them (one up to L = 5 at K = 5), and one fused pass
over the panel (csrc/apo.hip ``ate_apo_moments``) accumulates the moments
``result.ApoLayout``; everything reported follows from them on the host (``result.ApoResult``).

Out of scope: repeated cross-fitting, the logistic propensity, and group, curve, policy and
sensitivity versions.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..ops.devconst import const
from ..ops.enet import (MAX_PATH_PROBLEMS, cv_enet_gaussian, cv_problem_count,
                        default_lambda_min_ratio)
from ..ops.panel import build_panel, dtype_code
from ..result import APO_MAX_LEVELS, APO_MIN_LEVELS, ApoResult, apo_layout
from .common import as_np, resolve_device
from .irm import comm_counts, gram_phases, run_body, run_phases
from .lasso import _fold_ids, global_seg_counts


def _yd_columns(pan):
    """(y0, y1, d0, d1): the target columns the pass reads; bf16 panels carry them as hi + lo
    pairs (a level is exact in the hi part), the others as one column (second = -1)."""
    if "D" not in pan.cols:
        raise ValueError("the potential-outcome pass needs a panel with a level column D: "
                         "build_panel(targets={'D': level, ...})")
    if pan.dtype == torch.bfloat16:
        return pan.cols["Y_hi"], pan.cols["Y_lo"], pan.cols["D_hi"], pan.cols["D_lo"]
    return pan.cols["Y"], -1, pan.cols["D"], -1


def _apo_args(pan, coef, levels):
    """The argument checks of the pass that the host can name; returns p."""
    L = int(levels)
    p = len(pan.xcols)
    nfold = -(-pan.nseg // max(L, 1))
    if coef.dim() != 3 or tuple(coef.shape) != (nfold, 2 * L, p + 1):
        raise ValueError(f"coef must be [{nfold}, {2 * L}, {p + 1}] ({pan.nseg} segments at {L} "
                         f"levels), got {tuple(coef.shape)}")
    return p


def _apo_terms(pan, coef, L):
    """The float64 CPU twin of the pass (the kernel's oracle), in the pattern of
    ``irm._score_terms``: per segment ``(lev, y, d, g [L], m)`` over its real rows -- its
    level, the targets, the L outcome regressions and the unclipped propensity of ITS level."""
    _apo_args(pan, coef, L)
    y0, y1, d0, d1 = _yd_columns(pan)
    X = pan.colmajor().double()
    c = coef.double()
    for s in range(pan.nseg):
        r0, r1 = (int(v) for v in pan.seg_bounds[s])
        Xs = X[:, r0:r1]
        v = Xs[pan.cols["one"]] != 0
        xs = Xs[pan.xcols][:, v]
        y = Xs[y0][v] + (Xs[y1][v] if y1 >= 0 else 0.0)
        d = Xs[d0][v] + (Xs[d1][v] if d1 >= 0 else 0.0)
        k, lev = divmod(s, L)
        g = [c[k, q, 0] + c[k, q, 1:] @ xs for q in range(L)]
        yield lev, y, d, g, c[k, L + lev, 0] + c[k, L + lev, 1:] @ xs


def default_nbx(pan, levels: int) -> int:
    """Workgroups per segment of the pass: enough for the LARGEST segment to give every
    workgroup one trip of rows (2048 on a bf16 panel; 256 x 4 rows per thread up to L = 4, 256 x
    2 beyond), at most the grid of ``irm._score_launch`` (512 / 256). Arms are rarely balanced
    and a partial is N(L) doubles, so a grid sized by the cap would mostly write and then sum
    zeros (profiles/apos/README.md)."""
    bf = pan.dtype == torch.bfloat16
    rows = 2048 if bf else 256 * (4 if levels <= 4 else 2)
    b = np.asarray(pan.seg_bounds, dtype=np.int64)
    longest = int((b[:, 1] - b[:, 0]).max()) if len(b) else 1
    return max(1, min(512 if bf else 256, -(-longest // rows)))


def apo_moments(pan, coef: torch.Tensor, levels: int, clip: float = 0.01,
                nbx: int | None = None) -> torch.Tensor:
    """The fused held-out potential-outcome pass -> the fp64 moments of ``result.ApoLayout``
    (14 at L = 2, 77 at L = 8).

    pan: a level-split panel (segment ``L k + c`` = fold k, level c) with the level in column
    ``D``. coef: [nseg / L, 2 L, p+1] fp64, rows g_0..g_{L-1}, m_0..m_{L-1}, intercept first.
    GPU: csrc/apo.hip ``ate_apo_moments`` (``nbx`` blocks per segment, default
    :func:`default_nbx`; at L = 2 and the same
    ``nbx`` the per-level residual sums, n and n_1 carry the bits of
    ``irm.irm_score_moments`` [5], [4], [2], [7] with rows (g_0, g_1, m_1)); an argument the
    entry point refuses (L outside 2..8, segments no multiple of L, clip outside [0, 0.5), too
    many covariates for the LDS) is a ``NativeError``. CPU: the float64 torch twin, the
    kernel's oracle."""
    L = int(levels)
    if pan.data.is_cuda:
        y0, y1, d0, d1 = _yd_columns(pan)
        p = len(pan.xcols)
        dev = pan.device
        xc = const(pan.xcols, torch.int32, dev)
        segs = const(np.asarray(pan.seg_bounds, dtype=np.int64), torch.int64, dev)
        if nbx is None:
            nbx = default_nbx(pan, L)
        if APO_MIN_LEVELS <= L <= APO_MAX_LEVELS and pan.nseg % L == 0:
            _apo_args(pan, coef, L)          # what the entry point cannot see: coef's extent
        N = 1 + L + L * (L + 1) // 2 + 4 * L
        out = torch.empty(N, dtype=torch.float64, device=dev)
        partial = torch.empty(pan.nseg * nbx * N, dtype=torch.float64, device=dev)
        c = coef.double().contiguous()
        cs, bs = pan.strides()
        _native.call("ate_apo_moments", dtype_code(pan.data), pan.data.data_ptr(), cs, bs,
                     xc.data_ptr(), p, segs.data_ptr(), pan.nseg, L, c.data_ptr(), y0, y1, d0,
                     d1, pan.cols["one"], float(clip), nbx, partial.data_ptr(), out.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
        return out
    lay = apo_layout(L)
    if pan.nseg % L:
        raise ValueError(f"{pan.nseg} segments are no multiple of {L} levels")
    mom = torch.zeros(lay.size, dtype=torch.float64)
    lo, hi = clip, 1.0 - clip
    for lev, y, d, g, m in _apo_terms(pan, coef, L):
        ind = (d == lev).double()
        r = y - g[lev]
        ie = 1.0 / m.clamp(lo, hi)
        psi = [g[c] + ind * (r * ie) if c == lev else g[c] for c in range(L)]
        seg = torch.zeros_like(mom)
        seg[0] = float(len(y))
        for c in range(L):
            seg[lay.psi + c] = psi[c].sum()
            for c2 in range(c, L):
                seg[lay.tri(c, c2)] = (psi[c] * psi[c2]).sum()
        b = lay.level + 4 * lev
        seg[b] = ind.sum()
        seg[b + 1] = (ind * ((m < lo) | (m > hi)).double()).sum()
        seg[b + 2] = (ind * (r * r)).sum()
        seg[b + 3] = (ind * ie).sum()
        mom += seg
    return mom


def apo_finalize(mom: torch.Tensor, L: int) -> torch.Tensor:
    """[theta_0 .. theta_{L-1}, SE_0 .. SE_{L-1}] from the moments (``irm.mean_se`` per level).
    Device tensors in and out, no host sync (capturable)."""
    lay = apo_layout(L)
    n = mom[0]
    s1 = mom[lay.psi:lay.psi + L]
    s2 = torch.stack([mom[lay.tri(c, c)] for c in range(L)])
    return torch.cat([s1 / n, torch.sqrt(((s2 - s1 * s1 / n) / (n - 1) / n).clamp(min=0))])


# ---------------------------------------------------------------- the front end
def code_levels(D):
    """(values [L], level [n] int64): the distinct values of D in ascending order and every
    row's level 0..L-1. ValueError for a non-finite D or a number of values outside 2..8."""
    Dn = as_np(D).astype(np.float64).reshape(-1)
    if not np.isfinite(Dn).all():
        raise ValueError("DML-APOS needs a finite treatment: D has NaN or infinite values")
    values, level = np.unique(Dn, return_inverse=True)
    if not APO_MIN_LEVELS <= len(values) <= APO_MAX_LEVELS:
        raise ValueError(f"DML-APOS needs between {APO_MIN_LEVELS} and {APO_MAX_LEVELS} treatment "
                         f"levels, D has {len(values)} distinct value"
                         f"{'' if len(values) == 1 else 's'}")
    return values, level.astype(np.int64).reshape(-1)


def check_level_cells(counts, folds: int, values):
    """Every (fold, level) cell of the L K-segment layout needs a row: the outcome fit of that
    level for every other fold trains on it. ``counts``: (global) rows per segment."""
    L = len(values)
    c = np.asarray(counts)
    if len(c) != L * folds:
        raise ValueError(f"DML-APOS needs {L * folds} segments (fold k, level c -> {L} k + c), "
                         f"the panel has {len(c)}")
    for s in np.flatnonzero(c <= 0):
        raise ValueError(f"empty (fold, level) cell: fold {int(s) // L}, level D="
                         f"{values[int(s) % L]:g} has no rows")


def level_split_panel(Y, D, X, folds, seed, dtype, device, dist=None):
    """The prologue of :func:`dml_apos_lasso`, the L-level sibling of ``irm.arm_split_panel``:
    the level coding of D, the fold ids (the stream of ``dml_irm_lasso``), the (global) rows
    per (fold, level) cell, their check, and the level-split panel on ``device``: segment
    ``L k + c`` = fold k, level c, target columns ``D`` (the level) and ``I0 .. I{L-1}`` (the
    indicators 1{D = c}, the propensity targets). Returns (pan, values [L], level [n], fid [n],
    counts [L K], n_total)."""
    dev = resolve_device(device)
    Yn, Xn = as_np(Y), as_np(X)
    values, level = code_levels(D)
    L = len(values)
    fid = np.asarray(_fold_ids(len(Yn), folds, seed, 0, dist), dtype=np.int64)
    seg = L * fid + level
    counts = np.bincount(seg, minlength=L * folds).astype(np.float64)
    if dist is not None and dist.world > 1:
        t = torch.as_tensor(counts).to(dev)
        dist.sum_(t)
        counts = t.cpu().numpy()
    check_level_cells(counts, folds, values)
    targets = {"D": level.astype(np.float64)}
    for c in range(L):
        targets[f"I{c}"] = (level == c).astype(np.float64)
    pan = build_panel(Xn, None, Yn, folds=seg, dtype=dtype, device=dev, nseg=L * folds,
                      targets=targets)
    return pan, values, level, fid, counts, (dist.n_total if dist is not None else len(Yn))


def apos_problems(pan, K: int, L: int, counts):
    """The 2 L K nuisance problems on the (L K + K)-Gram stack ``cat([G, G.view(K, L, P,
    P).sum(1)])`` as arguments of ``cv_enet_gaussian``: (seg_counts, full_sets, full_y, ycols),
    fold by fold, g_0..g_{L-1} then m_0..m_{L-1}. Segments of the stack: L s + c = (fold s,
    level c); L K + s = fold s, all levels. ycols: (Y, I0 .. I{L-1})."""
    counts = np.asarray(counts, dtype=np.float64)
    counts2 = np.concatenate([counts, counts.reshape(K, L).sum(1)])
    full_sets, full_y = [], []
    for k in range(K):
        others = [s for s in range(K) if s != k]
        full_sets += [[L * s + c for s in others] for c in range(L)]
        full_y += [0] * L
        full_sets += [[L * K + s for s in others] for _ in range(L)]
        full_y += [1 + c for c in range(L)]
    ycols = [pan.cols["Y"]] + [pan.cols[f"I{c}"] for c in range(L)]
    return counts2, full_sets, full_y, ycols


def path_launches(n_sets: int, per_set: int, cap: int = MAX_PATH_PROBLEMS):
    """``n_sets`` full sets of ``per_set`` path problems each (a full set with its CV folds)
    grouped, whole and in order, into as few launches of at most ``cap`` problems as hold
    them, evenly filled: [(first, last + 1), ...]. ValueError when one full set alone exceeds
    the cap."""
    if per_set > cap:
        raise ValueError(f"one nuisance with its CV folds is {per_set} path problems, more than "
                         f"the {cap} one path launch holds")
    nl = -(-n_sets // (cap // per_set))
    return [(i * n_sets // nl, (i + 1) * n_sets // nl) for i in range(nl)]


def apos_fit_phases(pan, folds: int, levels: int, lambda_rule="min", comm=None, seg_counts=None,
                    max_problems: int = MAX_PATH_PROBLEMS):
    """``irm.gram_phases`` on the L K-segment panel, then the CV-LASSO fit of the 2 L K
    nuisances (2 L K K path problems) on the stack of :func:`apos_problems`, in the launches of
    :func:`path_launches` (``max_problems``: the cap of one launch). Every launch gets the
    same explicit lambda ratio, ``default_lambda_min_ratio`` over the training sets of all 2 L
    nuisances (the rule of ``irm.irm_fit_phases(nuisances=)``), so a nuisance's coefficients do
    not depend on what shares its launch. State: "G", "coef" [K, 2L, p+1], "cv" (the last
    launch's). Returns (phases, reduce) as ``irm.irm_fit_phases``; ``ValueError`` before any
    device work when one full set with its folds exceeds a launch."""
    dist = comm is not None and comm.world_size > 1
    K, L = int(folds), int(levels)
    apo_layout(L)
    if seg_counts is None:
        seg_counts = global_seg_counts(pan, comm) if dist else np.asarray(pan.seg_nreal)
    counts = np.asarray(seg_counts, dtype=np.float64)
    check_level_cells(counts, K, np.arange(L))
    if pan.nseg != L * K:
        raise ValueError(f"DML-APOS needs {L * K} segments, this shard's panel has {pan.nseg}")
    _yd_columns(pan)
    counts2, full_sets, full_y, ycols = apos_problems(pan, K, L, counts)
    per = cv_problem_count(L * K + K, full_sets[:1], len(ycols), full_y[:1])
    launches = path_launches(len(full_sets), per, max_problems)
    p, P = len(pan.xcols), pan.P
    ratio = default_lambda_min_ratio(min(counts2[list(fs)].sum() for fs in full_sets), p)

    def phase_fit(st):
        G = st["G"]
        G2 = torch.cat([G, G.view(K, L, P, P).sum(1)])
        coefs, cv = [], None
        for a, b in launches:
            cv = cv_enet_gaussian(G2, pan, pan.xcols, ycols, full_sets=full_sets[a:b],
                                  seg_counts=counts2, full_y=full_y[a:b], lambda_min_ratio=ratio)
            coefs.append(cv.coef_min if lambda_rule == "min" else cv.coef_1se)
        coef = torch.cat(coefs).reshape(K, 2 * L, -1).double().contiguous()
        return {**st, "cv": cv, "coef": coef}

    phases, reduce = gram_phases(pan, comm)
    phases.append(phase_fit)
    return phases, reduce


def apos_phases(pan, folds: int, levels: int, lambda_rule="min", clip=0.01, comm=None,
                seg_counts=None, max_problems: int = MAX_PATH_PROBLEMS):
    """The APOS step as phases for utils.graphs.SegmentedStep: those of
    :func:`apos_fit_phases`, then

    B'  the potential-outcome moments (csrc/apo.hip ``ate_apo_moments``)      device
    C06 one all-reduce of the moments                                         collective (world > 1)
    C   theta_c / SE_c (:func:`apo_finalize`, fp64, on device)                device

    The result state holds "res" [2L], "mom" [N(L)], "coef" [K, 2L, p+1] and "cv"."""
    L = int(levels)
    phases, reduce = apos_fit_phases(pan, folds, L, lambda_rule, comm, seg_counts, max_problems)

    def phase_moments(st):
        return {**st, "mom": apo_moments(pan, st["coef"], L, clip)}

    def phase_final(st):
        return {**st, "res": apo_finalize(st["mom"], L)}

    phases.append(phase_moments)
    if reduce is not None:
        phases.append(reduce("mom"))
    phases.append(phase_final)
    return phases


def apos_panel(pan, folds: int, levels: int, lambda_rule="min", clip=0.01, comm=None,
               seg_counts=None, max_problems: int = MAX_PATH_PROBLEMS):
    """DML-APOS on a level-split fold panel (:func:`level_split_panel`). Returns (res [2L],
    mom [N(L)], coef [K, 2L, p+1]): device tensors, no host sync (capturable). comm,
    seg_counts: as ``irm.irm_crossfit_panel``."""
    st = run_phases(apos_phases(pan, folds, levels, lambda_rule, clip, comm, seg_counts,
                                max_problems))
    return st["res"], st["mom"], st["coef"]


def _apos_body(pan, levels, folds, lambda_rule, clip, dist=None, counts=None):
    """The whole call as one device function (GraphCache captures it, keyed by L): [res, mom]."""
    comm, seg_counts = comm_counts(dist, counts)
    res, mom, _ = apos_panel(pan, folds, levels, lambda_rule, clip, comm, seg_counts)
    return torch.cat([res, mom])


def check_scope(repeats=1, propensity="linear"):
    """What DML-APOS does not do, each a ValueError before any device work."""
    if repeats != 1:
        raise ValueError("repeated cross-fitting is not available for DML-APOS: repeats must be 1")
    if propensity != "linear":
        raise ValueError('DML-APOS fits linear-probability propensities only: propensity must be '
                         f'"linear", got {propensity!r}')


def check_reference(reference, values):
    """The reference level's index among ``values`` (default: the lowest level)."""
    if reference is None:
        return 0
    hit = np.flatnonzero(np.asarray(values, dtype=np.float64) == reference) \
        if isinstance(reference, (int, float, np.number)) else []
    if len(hit) != 1:
        raise ValueError(f"reference {reference!r} is not a treatment level: "
                         f"{[float(v) for v in values]}")
    return int(hit[0])


def dml_apos_lasso(Y, D, X, reference=None, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                   n_boot=999, level=0.95, method="DML-APOS cross-fit (LASSO)", device=None,
                   dtype="f64", dist=None, graph=True, repeats=1,
                   propensity="linear") -> ApoResult:
    """K-fold cross-fitted mean potential outcomes of a treatment D with 2 to 8 distinct
    values and CV-LASSO nuisances (the module docstring). Y: outcome; D: the treatment, any
    finite values, coded to levels in ascending order; X: covariates. reference: the value of
    D the contrasts are taken against (default: the lowest). Folds are those of
    ``irm.dml_irm_lasso``. Matches reference.estimators.dml_apos_lasso.

    graph: as ``dml_irm_lasso``, one captured hipGraph on a GPU; L is part of the cache key.
    n_boot, level: the simultaneous band over the L - 1 contrasts (``result.band_crit``, drawn
    on the host from ``seed``). diagnostics: n, per level n_c, n_clipped_c, rmse_g_c and ipw_c
    (the mean inverse-propensity weight S 1{D=c}/e_c / n, near 1 when m_c is calibrated),
    hipgraph. ``repeats`` and ``propensity`` exist to say what is out of scope."""
    check_scope(repeats, propensity)
    values, _ = code_levels(D)
    ref = check_reference(reference, values)
    L = len(values)
    path_launches(2 * L * folds, folds)      # a nuisance is 1 full + K - 1 fold problems
    pan, values, _, _, counts, n = level_split_panel(Y, D, X, folds, seed, dtype, device, dist)
    out, g = run_body("dml_apos", _apos_body, (pan,), L, folds, lambda_rule, float(clip), dist,
                      tuple(counts.tolist()), graph=graph, dist=dist)
    v = out.detach().double().cpu().numpy()
    return ApoResult.from_moments(method, v[2 * L:], [float(x) for x in values],
                                  reference=float(values[ref]), seed=seed, n_boot=n_boot,
                                  level=level, n=n, hipgraph=g)
