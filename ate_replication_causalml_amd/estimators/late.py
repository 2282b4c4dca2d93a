"""The local average treatment effect (LATE) of the cross-fitted interactive IV model
(DML-IIVM, Chernozhukov et al. 2018 §5.2; DoubleML ``DoubleMLIIVM``) with CV-LASSO nuisances
on the fold Gram stack: the answer to "what is the effect on those who complied?" when the
treatment assigned (a binary instrument Z) is not the treatment taken (D in {0, 1}).

The held-out nuisances are gaussian CV-LASSO fits, as in ``estimators/irm.py``:

    g0 = E[Y|Z=0,X]   g1 = E[Y|Z=1,X]   r0 = E[D|Z=0,X]   r1 = E[D|Z=1,X]   m = E[Z|X]
    e  = clip(m, clip, 1 - clip)
    b  = g1 - g0 + z (y - g1) / e - (1 - z)(y - g0) / (1 - e)     (the ITT score)
    a  = r1 - r0 + z (d - r1) / e - (1 - z)(d - r0) / (1 - e)     (the first-stage score)
    theta = S b / S a
    SE^2  = [S b^2 - 2 theta S a b + theta^2 S a^2] / (n - 1) / n / (S a / n)^2

two AIPW scores (``irm.aipw_psi``) over one propensity, split by the instrument. With the
instrument in the panel's ``W`` column the layout of DML-IRM carries over: the arm-split fold
panel (segment 2k + z), its one Gram pass, ONE path launch for the 5 K K problems on the 3K
stack with targets (Y, D, Z), and one fused pass over the panel (csrc/iivm.hip
``ate_iivm_moments``) that accumulates the 15 moments ``result.LATE_MOMENTS``; the ITT, the
first stage, their covariance and the Anderson-Rubin set follow from them on the host
(``result.LateResult``).

One-sided noncompliance (DoubleML ``subgroups``): ``always_takers=False`` states D = 0
wherever Z = 0 and fixes r0 = 0; ``never_takers=False`` states D = 1 wherever Z = 1 and fixes
r1 = 1. A fixed nuisance is not fitted (K K path problems fewer each) and its coefficient row
is zero (r1: intercept 1).

Out of scope: repeated cross-fitting; group, curve, policy and sensitivity versions of the
LATE; instruments or treatments that are not binary (a real treatment with one or several
real instruments is the partially linear IV model, ``estimators/pliv.py``); and an instrument
in the device data generator (``data.device_dgp``) -- panels come from host arrays
(``data.dgp.make_late_data``).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..ops.devconst import const
from ..ops.enet import default_lambda_min_ratio
from ..ops.panel import dtype_code
from ..result import LATE_MOMENTS, LateResult
from . import irm
from .common import as_np
from .irm import (aipw_psi, arm_split_panel, check_cells, comm_counts, gram_phases, run_body,
                  run_phases)
from .lasso import _fold_ids, global_seg_counts

N_LATE = len(LATE_MOMENTS)   # 15
NUISANCES = ("g0", "g1", "r0", "r1", "m")   # rows of a coefficient block


def _ydz_columns(pan):
    """(y0, y1, d0, d1, z0, z1): the target columns the pass reads (the instrument lives in
    column W); bf16 panels carry them as hi + lo pairs, the others as one column (-1)."""
    if "D" not in pan.cols:
        raise ValueError("the LATE pass needs a panel with a D column: "
                         "build_panel(targets={'D': ...})")
    if pan.dtype == torch.bfloat16:
        return tuple(pan.cols[f"{k}_{h}"] for k in "YDW" for h in ("hi", "lo"))
    return pan.cols["Y"], -1, pan.cols["D"], -1, pan.cols["W"], -1


def _late_args(pan, coef, segs_per_fold):
    """The argument checks of the pass; returns p, the number of covariates."""
    nseg, nfold = pan.nseg, coef.shape[0]
    if segs_per_fold < 1 or nfold * segs_per_fold < nseg:
        raise ValueError(f"{nseg} segments at {segs_per_fold} per fold need "
                         f"{-(-nseg // max(segs_per_fold, 1))} coefficient blocks, got {nfold}")
    p = len(pan.xcols)
    if coef.dim() != 3 or tuple(coef.shape[1:]) != (5, p + 1):
        raise ValueError(f"coef must be [nfold, 5, {p + 1}], got {tuple(coef.shape)}")
    return p


def _late_terms(pan, coef, segs_per_fold):
    """The float64 CPU twin of the pass (the kernel's oracle), in the pattern of
    ``irm._score_terms``: per segment ``(y, d, z, g0, g1, r0, r1, m)`` over its real rows,
    m before clipping."""
    _late_args(pan, coef, segs_per_fold)
    cols = _ydz_columns(pan)
    X = pan.colmajor().double()
    c = coef.double()
    for s in range(pan.nseg):
        r0, r1 = (int(v) for v in pan.seg_bounds[s])
        Xs = X[:, r0:r1]
        v = Xs[pan.cols["one"]] != 0
        xs = Xs[pan.xcols][:, v]
        y, d, z = (Xs[cols[2 * q]][v] + (Xs[cols[2 * q + 1]][v] if cols[2 * q + 1] >= 0 else 0.0)
                   for q in range(3))
        k = s // segs_per_fold
        yield (y, d, z, *(c[k, r, 0] + c[k, r, 1:] @ xs for r in range(5)))


def iivm_moments(pan, coef: torch.Tensor, clip: float = 0.01, segs_per_fold: int = 2,
                 nbx: int | None = None) -> torch.Tensor:
    """The fused held-out LATE pass -> the 15 fp64 moments (``result.LATE_MOMENTS``).

    pan: an arm-split panel with the instrument in column ``W`` and the treatment taken in
    column ``D``. coef: [nfold, 5, p+1] fp64, rows (g0, g1, r0, r1, m), intercept first;
    segment s uses block ``s // segs_per_fold``. GPU: csrc/iivm.hip ``ate_iivm_moments``
    (``nbx`` blocks per segment; at the same ``nbx`` moments [0,1,2,3,7,10,11,14] carry the
    bits of ``irm.irm_score_moments`` [0,1,2,3,7,4,5,6] with rows (g0, g1, m), and moments
    [4,5,12,13] those of ``irm_score_moments`` [0,1,4,5] with rows (r0, r1, m) on a panel
    whose Y column holds D). CPU: the float64 torch twin, the kernel's oracle."""
    if pan.data.is_cuda:
        p = _late_args(pan, coef, segs_per_fold)
        cols = _ydz_columns(pan)
        dev = pan.device
        xc = const(pan.xcols, torch.int32, dev)
        segs = const(np.asarray(pan.seg_bounds, dtype=np.int64), torch.int64, dev)
        if nbx is None:                      # the geometry of irm._score_launch
            nbx = 512 if pan.dtype == torch.bfloat16 else 256
        out = torch.empty(N_LATE, dtype=torch.float64, device=dev)
        partial = torch.empty(pan.nseg * nbx * N_LATE, dtype=torch.float64, device=dev)
        c = coef.double().contiguous()
        cs, bs = pan.strides()
        _native.call("ate_iivm_moments", dtype_code(pan.data), pan.data.data_ptr(), cs, bs,
                     xc.data_ptr(), p, segs.data_ptr(), pan.nseg, segs_per_fold, c.data_ptr(),
                     *cols, pan.cols["one"], float(clip), nbx, partial.data_ptr(),
                     out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return out
    mom = torch.zeros(N_LATE, dtype=torch.float64)
    lo, hi = clip, 1.0 - clip
    for y, d, z, g0, g1, r0, r1, m in _late_terms(pan, coef, segs_per_fold):
        e = m.clamp(lo, hi)
        b = aipw_psi(y, z, g0, g1, e)
        a = aipw_psi(d, z, r0, r1, e)
        one = torch.ones_like(b)
        mom += torch.stack([b.sum(), (b * b).sum(), one.sum(),
                            ((m < lo) | (m > hi)).double().sum(),
                            a.sum(), (a * a).sum(), (a * b).sum(), z.sum(),
                            (z * d).sum(), ((1.0 - z) * d).sum(),
                            (z * (y - g1) ** 2).sum(), ((1.0 - z) * (y - g0) ** 2).sum(),
                            (z * (d - r1) ** 2).sum(), ((1.0 - z) * (d - r0) ** 2).sum(),
                            ((z - m) ** 2).sum()])
    return mom


def late_finalize(mom: torch.Tensor) -> torch.Tensor:
    """[theta, SE] from the 15 moments (the module docstring's formulas). Device tensors in
    and out, no host sync (capturable)."""
    sb, sbb, n, sa, saa, sab = mom[0], mom[1], mom[2], mom[4], mom[5], mom[6]
    th = sb / sa
    fs = sa / n
    var = (sbb - 2.0 * th * sab + th * th * saa) / (n - 1) / n / (fs * fs)
    return torch.stack([th, torch.sqrt(var.clamp(min=0))])


def fitted_nuisances(always_takers=True, never_takers=True) -> tuple:
    """The rows of a coefficient block (0: g0, 1: g1, 2: r0, 3: r1, 4: m) that are fitted:
    all but r0 without always-takers and r1 without never-takers."""
    return tuple(r for r in range(5) if not (r == 2 and not always_takers) and
                 not (r == 3 and not never_takers))


def late_problems(pan, K: int, counts, always_takers=True, never_takers=True):
    """The nuisance problems on the 3K-Gram stack ``cat([G, G[0::2] + G[1::2]])`` as arguments
    of ``cv_enet_gaussian``: (seg_counts, full_sets, full_y, ycols), fold by fold in the order
    of :func:`fitted_nuisances`. Segments of the stack as ``irm.fit_problems``: 2s + z =
    (fold s, Z = z); 2K + s = fold s. ycols: (Y, D, Z)."""
    counts = np.asarray(counts, dtype=np.float64)
    counts3 = np.concatenate([counts, counts[0::2] + counts[1::2]])
    fit = fitted_nuisances(always_takers, never_takers)
    full_sets, full_y = [], []
    for k in range(K):
        others = [s for s in range(K) if s != k]
        z0, z1 = [2 * s for s in others], [2 * s + 1 for s in others]
        sets = [z0, z1, z0, z1, [2 * K + s for s in others]]
        full_sets += [sets[r] for r in fit]
        full_y += [(0, 0, 1, 1, 2)[r] for r in fit]
    return counts3, full_sets, full_y, [pan.cols["Y"], pan.cols["D"], pan.cols["W"]]


def late_fit_phases(pan, folds: int, lambda_rule="min", comm=None, seg_counts=None,
                    always_takers=True, never_takers=True):
    """``irm.gram_phases``, then ONE ``cv_enet_gaussian`` launch for every fitted nuisance
    of every fold (5 K K path problems; K K fewer per fixed nuisance) on the 3K stack with
    ``ycols = [Y, D, W]``. The lambda ratio is always that of the whole five-nuisance fit,
    so a nuisance does not depend on which others are fitted beside it. State: "G", "cv",
    "coef" [K, 5, p+1] (a fixed r0 row is zero, a fixed r1 row is the intercept 1). Returns
    (phases, reduce) as ``irm.irm_fit_phases``."""
    dist = comm is not None and comm.world_size > 1
    K = folds
    if seg_counts is None:
        seg_counts = global_seg_counts(pan, comm) if dist else np.asarray(pan.seg_nreal)
    counts = np.asarray(seg_counts, dtype=np.float64)
    check_cells(counts, K)
    if pan.nseg != 2 * K:
        raise ValueError(f"DML-IIVM needs {2 * K} segments, this shard's panel has {pan.nseg}")
    _ydz_columns(pan)
    fit = fitted_nuisances(always_takers, never_takers)
    counts3, full_sets, full_y, ycols = late_problems(pan, K, counts, always_takers, never_takers)
    _, sets_all, _, _ = late_problems(pan, K, counts)
    p = len(pan.xcols)
    ratio = default_lambda_min_ratio(min(counts3[list(fs)].sum() for fs in sets_all), p)
    slots = const(fit, torch.int64, pan.device)
    fixed = np.zeros((K, 5, p + 1))
    if not never_takers:
        fixed[:, 3, 0] = 1.0
    fixed = const(fixed, torch.float64, pan.device)

    def phase_fit(st):
        G = st["G"]
        G3 = torch.cat([G, G[0::2] + G[1::2]])
        cv = irm.cv_enet_gaussian(G3, pan, pan.xcols, ycols, full_sets=full_sets,
                                  seg_counts=counts3, full_y=full_y, lambda_min_ratio=ratio)
        some = (cv.coef_min if lambda_rule == "min" else cv.coef_1se)
        coef = fixed.clone()
        coef.index_copy_(1, slots, some.reshape(K, len(fit), -1).double())
        return {**st, "cv": cv, "coef": coef}

    phases, reduce = gram_phases(pan, comm)
    phases.append(phase_fit)
    return phases, reduce


def late_phases(pan, folds: int, lambda_rule="min", clip=0.01, comm=None, seg_counts=None,
                always_takers=True, never_takers=True):
    """The LATE step as phases for utils.graphs.SegmentedStep: those of
    :func:`late_fit_phases`, then

    B'  the 15 LATE moments (csrc/iivm.hip ``ate_iivm_moments``)             device
    C06 one all-reduce of the 15 moments                                     collective (world > 1)
    C   theta / SE (:func:`late_finalize`, fp64, on device)                  device

    The result state holds "res" [2], "mom" [15], "coef" [K, 5, p+1] and "cv"."""
    phases, reduce = late_fit_phases(pan, folds, lambda_rule, comm, seg_counts, always_takers,
                                     never_takers)

    def phase_moments(st):
        return {**st, "mom": iivm_moments(pan, st["coef"], clip, 2)}

    def phase_final(st):
        return {**st, "res": late_finalize(st["mom"])}

    phases.append(phase_moments)
    if reduce is not None:
        phases.append(reduce("mom"))
    phases.append(phase_final)
    return phases


def late_panel(pan, folds: int, lambda_rule="min", clip=0.01, comm=None, seg_counts=None,
               always_takers=True, never_takers=True):
    """DML-IIVM on an arm-split fold panel with the instrument in column W and the treatment
    taken in column D (``build_panel(X, Z, Y, folds=2 * fold + Z, targets={"D": D})``).
    Returns (res [2], mom [15], cv): device tensors, no host sync (capturable). comm,
    seg_counts: as ``irm.irm_crossfit_panel``."""
    st = run_phases(late_phases(pan, folds, lambda_rule, clip, comm, seg_counts, always_takers,
                                never_takers))
    return st["res"], st["mom"], st.get("cv")


def _late_body(pan, folds, lambda_rule, clip, always_takers, never_takers, dist=None,
               counts=None):
    """The whole call as one device function (GraphCache captures it): [res, mom]."""
    comm, seg_counts = comm_counts(dist, counts)
    res, mom, _ = late_panel(pan, folds, lambda_rule, clip, comm, seg_counts, always_takers,
                             never_takers)
    return torch.cat([res, mom])


def check_compliance_cells(cells, folds: int, always_takers=True, never_takers=True):
    """``cells``: the (global) rows per (fold k, Z = z, D = d) cell at index 4k + 2z + d. A
    fixed nuisance needs its statement to hold (no row with Z = 0, D = 1 without
    always-takers; none with Z = 1, D = 0 without never-takers); a fitted r_z needs both
    values of D in every (fold, Z = z) cell, or its training target is constant."""
    c = np.asarray(cells).reshape(folds, 2, 2)
    check_cells(c.sum(axis=2).ravel(), folds)      # an empty (fold, Z) cell: said as such
    for z, (flag, name) in enumerate(((always_takers, "always_takers"),
                                      (never_takers, "never_takers"))):
        for k in range(folds):
            if not flag:
                if c[k, z, 1 - z] > 0:
                    raise ValueError(f"{name}=False needs D = {z} wherever Z = {z}: fold {k} has "
                                     f"{int(c[k, z, 1 - z])} rows with Z={z}, D={1 - z}; set "
                                     f"{name}=True")
                continue
            for d in (0, 1):
                if c[k, z, d] <= 0:
                    raise ValueError(f"empty (fold, Z, D) cell: fold {k}, Z={z}, D={d} has no "
                                     f"rows, so r{z} = E[D|Z={z},X] cannot be fitted; set "
                                     f"{name}=False if D = {z} wherever Z = {z}")


def check_binary(**named):
    for name, v in named.items():
        if not np.isin(v, (0.0, 1.0)).all():
            raise ValueError(f"DML-IIVM needs a binary {name}: it must be exactly 0 or 1")


def dml_iivm_lasso(Y, W, Z, X, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                   always_takers=True, never_takers=True,
                   method="DML-IIVM cross-fit LATE (LASSO)", device=None, dtype="f64", dist=None,
                   graph=True) -> LateResult:
    """K-fold cross-fitted LATE of the interactive IV model with CV-LASSO nuisances (the
    module docstring). Y: outcome; W: the treatment TAKEN, exactly {0, 1}; Z: the instrument
    (the treatment assigned), exactly {0, 1}; X: covariates. Folds are those of
    ``irm.dml_irm_lasso(Y, Z, X)``, whose theta is this result's ITT. Matches
    reference.estimators.dml_iivm_lasso.

    always_takers / never_takers: set False under one-sided noncompliance (nobody takes the
    treatment unassigned / everybody assigned takes it): r0 = 0 / r1 = 1 is then fixed, not
    fitted, and the data must agree (ValueError otherwise). graph: as ``dml_irm_lasso``, one
    captured hipGraph on a GPU; the two flags are part of the cache key. diagnostics: n,
    n_clipped, n_z1, the four compliance cell counts, the held-out RMSE of the five
    nuisances, hipgraph."""
    always_takers, never_takers = bool(always_takers), bool(never_takers)
    Dn, Zn = as_np(W), as_np(Z)
    check_binary(**{"treatment W": Dn, "instrument Z": Zn})
    fid = np.asarray(_fold_ids(len(Dn), folds, seed, 0, dist), dtype=np.int64)
    cells = np.bincount(4 * fid + 2 * Zn.astype(np.int64) + Dn.astype(np.int64),
                        minlength=4 * folds)
    pan, counts, _, n, _ = arm_split_panel(
        Y, Zn, X, folds, seed, dtype, device, dist, extra_counts=cells,
        check_extra=lambda c: check_compliance_cells(c, folds, always_takers, never_takers),
        targets={"D": Dn})
    out, g = run_body("dml_iivm", _late_body, (pan,), folds, lambda_rule, float(clip),
                      always_takers, never_takers, dist, tuple(counts.tolist()), graph=graph,
                      dist=dist)
    v = out.detach().double().cpu().numpy()
    return LateResult.from_moments(method, v[2:], n=n, hipgraph=g)
