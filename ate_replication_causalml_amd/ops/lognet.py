"""Binomial elastic net + cv.glmnet on the device (csrc/lognet.hip).

``cv_lognet`` fits the full problem (all segments) and the K fold problems (all
segments but k, on the full problem's lambda sequence), evaluates held-out binomial
deviance per (fold, lambda), and applies the cv.glmnet selection rules
(``ate_cv_select``, shared with the gaussian path). Three launches + selection, no
host synchronisation. CPU tensors run reference/glmnet.py on the same folds.

``cv_lognet_groups`` runs several such cross-validated fits -- the K outer training sets of a
cross-fit with their inner folds, a fold being any set of segments -- in ONE path launch
(``ate_lognet_path_groups``), one held-out deviance launch over segment sets and one selection.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _native
from ..reference import glmnet as ref
from .devconst import const
from .panel import dtype_code

MAX_PATH_PROBLEMS = 256   # co-resident workgroups of one concurrent path launch
MAX_SEGMENTS = 64         # csrc/lognet.hip MAXSEG
MAX_P = 96


@dataclass
class LognetCvResult:
    lambdas: torch.Tensor    # [L] (NaN beyond nlam)
    nlam: torch.Tensor       # [1] int32
    cvm: torch.Tensor        # [L] (NaN beyond nlam, on the device as on the CPU)
    cvsd: torch.Tensor       # [L] (NaN beyond nlam)
    sel: torch.Tensor        # [2] (idx_min, idx_1se)
    coef_path: torch.Tensor  # [L, p+1] original scale, intercept first (NaN rows beyond nlam)
    coef_min: torch.Tensor   # [p+1]
    coef_1se: torch.Tensor
    npass: torch.Tensor      # [1 + K]: full fit, then the K fold fits (< 0: wait timed out)

    def check(self):
        """Raise NumericalError if a fold fit was truncated (its wait for the full fit's
        lambda timed out). Device outputs are NaN-poisoned in that case already."""
        bad = np.flatnonzero(self.npass.cpu().numpy()[1:] < 0).tolist()
        if bad:
            from ..utils.guards import NumericalError
            raise NumericalError(f"binomial CV fold fit(s) {bad} timed out waiting for the "
                                 "full fit's lambda sequence; selection is invalid")
        return self


def _rescale_vp(vp, p):
    vp = np.ones(p) if vp is None else np.maximum(np.asarray(vp, float), 0)
    return vp * p / vp.sum()


def cv_lognet(panel, xcols, ycol, penalty_factor=None, alpha=1.0, nlambda=100,
              lambda_min_ratio=None, thresh=1e-7, maxit=100000,
              concurrent=True) -> LognetCvResult:
    """cv.glmnet(x, y, family="binomial") with the panel's segments as the CV folds.

    ``concurrent``: full and fold fits in one launch (fold paths follow the full fit's
    lambdas through device flags); False = two launches, full fit then folds. Same bits.
    ``npass`` < 0 flags a fold whose wait for the full fit timed out."""
    K = panel.nseg
    p = len(xcols)
    n = int(np.sum(panel.seg_nreal))
    flmin = lambda_min_ratio if lambda_min_ratio is not None else (1e-4 if n > p else 1e-2)
    vp = _rescale_vp(penalty_factor, p)
    if not panel.data.is_cuda:
        return _cv_cpu(panel, xcols, ycol, vp, alpha, nlambda, flmin, thresh, maxit)
    if p > 96:
        raise ValueError("device lognet supports p <= 96")
    if panel.data.dtype not in (torch.float32, torch.float64):
        raise ValueError("device lognet needs an fp32/fp64 panel")
    dev = panel.device
    s = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    L = nlambda
    segs = np.stack([panel.seg_bounds[:, 0], panel.seg_bounds[:, 0] + panel.seg_nreal], 1)
    segs_t = torch.as_tensor(segs.astype(np.int64), device=dev)
    xc = torch.tensor(xcols, dtype=torch.int32, device=dev)
    vp_t = torch.tensor(vp, **f64)
    masks = np.ones((1 + K, K), dtype=np.uint8)
    for k in range(K):
        masks[1 + k, k] = 0
    masks_t = torch.from_numpy(masks).to(dev)
    nq = 1 + K
    a0 = torch.zeros((nq, L), **f64)
    beta = torch.zeros((nq, L, p), **f64)
    lam = torch.full((nq, L), float("nan"), **f64)
    devr = torch.zeros((nq, L), **f64)
    nlam = torch.zeros(nq, dtype=torch.int32, device=dev)
    npass = torch.zeros(nq, dtype=torch.int32, device=dev)
    dt = dtype_code(panel.data)
    X = panel.data
    off = lambda t: t.data_ptr() + t.element_size() * t.stride(0)
    if concurrent and L >= 3 and nq <= 256:
        # one launch: the full fit (problem 0) and the K fold fits run side by side, the
        # folds following the full fit's lambda sequence and stop through device flags
        progress = torch.zeros(2, dtype=torch.int32, device=dev)
        lampub = torch.zeros(L, **f64)
        _native.call("ate_lognet_path", dt, X.data_ptr(), panel.cm_ld, xc.data_ptr(), p, ycol,
                     segs_t.data_ptr(), K, masks_t.data_ptr(), nq, vp_t.data_ptr(), alpha,
                     flmin, thresh, maxit, 0, 0, L, a0.data_ptr(), beta.data_ptr(),
                     lam.data_ptr(), devr.data_ptr(), nlam.data_ptr(), npass.data_ptr(),
                     progress.data_ptr(), lampub.data_ptr(), s)
    else:
        # full problem: its own lambda sequence
        _native.call("ate_lognet_path", dt, X.data_ptr(), panel.cm_ld, xc.data_ptr(), p, ycol,
                     segs_t.data_ptr(), K, masks_t.data_ptr(), 1, vp_t.data_ptr(), alpha, flmin,
                     thresh, maxit, 0, 0, L, a0.data_ptr(), beta.data_ptr(), lam.data_ptr(),
                     devr.data_ptr(), nlam.data_ptr(), npass.data_ptr(), 0, 0, s)
        # fold problems on the full lambda sequence (count read on the device)
        _native.call("ate_lognet_path", dt, X.data_ptr(), panel.cm_ld, xc.data_ptr(), p, ycol,
                     segs_t.data_ptr(), K, off(masks_t), K, vp_t.data_ptr(), alpha, flmin,
                     thresh, maxit, lam.data_ptr(), nlam.data_ptr(), L, off(a0), off(beta),
                     off(lam), off(devr), nlam.data_ptr() + 4, npass.data_ptr() + 4, 0, 0, s)
    hold = torch.arange(K, dtype=torch.int32, device=dev)
    cvraw = torch.empty((K, L), **f64)
    _native.call("ate_lognet_cvloss", dt, X.data_ptr(), panel.cm_ld, xc.data_ptr(), p, ycol,
                 segs_t.data_ptr(), hold.data_ptr(), K, off(a0), off(beta),
                 nlam.data_ptr() + 4, L, cvraw.data_ptr(), s)
    fidx = torch.arange(K, dtype=torch.int32, device=dev)[None]
    nfold = torch.as_tensor(panel.seg_nreal.astype(np.float64), device=dev)[None]
    cvm = torch.empty((1, L), **f64)
    cvsd = torch.empty((1, L), **f64)
    sel = torch.empty((1, 2), dtype=torch.int32, device=dev)
    _native.call("ate_cv_select", cvraw.data_ptr(), fidx.data_ptr(), nfold.data_ptr(), K, 1,
                 nlam.data_ptr(), L, cvm.data_ptr(), cvsd.data_ptr(), sel.data_ptr(), None, 0,
                 s)
    coef = torch.cat([a0[0][:, None], beta[0]], 1)
    # rows the path never reached are NaN, as in the CPU twin (device-side, no host sync)
    past = torch.arange(L, device=dev)[:, None] >= nlam[0]
    coef = torch.where(past, torch.full((), float("nan"), **f64), coef)
    sl = sel[0].long()
    from .enet import poison_if_truncated
    cvm0, cvsd0, cmin, c1se = poison_if_truncated(npass[1:], cvm[0], cvsd[0], coef[sl[0]],
                                                  coef[sl[1]])
    return LognetCvResult(lam[0], nlam[:1], cvm0, cvsd0, sel[0], coef, cmin, c1se, npass)


def _cv_cpu(panel, xcols, ycol, vp, alpha, nlambda, flmin, thresh, maxit):
    X = panel.data.double()
    rows, fid = [], []
    for k, ((r0, _), nr) in enumerate(zip(panel.seg_bounds, panel.seg_nreal)):
        rows.append(np.arange(r0, r0 + nr))
        fid.append(np.full(nr, k))
    rows = np.concatenate(rows)
    fid = np.concatenate(fid)
    Xn = X[xcols][:, rows].T.numpy()
    yn = X[ycol][rows].numpy()
    cv = ref.cv_glmnet(Xn, yn, family="binomial", alpha=alpha, penalty_factor=vp, foldid=fid,
                       nlambda=nlambda, lambda_min_ratio=flmin, thresh=thresh, maxit=maxit)
    L = nlambda
    m = len(cv.lambdas)
    pad = lambda a: torch.as_tensor(np.r_[a, np.full(L - len(a), np.nan)])
    coef = np.column_stack([cv.fit.a0, cv.fit.beta])
    coef_t = torch.as_tensor(np.vstack([coef, np.full((L - m, coef.shape[1]), np.nan)]))
    sel = torch.tensor([cv.idx_min, cv.idx_1se], dtype=torch.int32)
    return LognetCvResult(pad(cv.lambdas), torch.tensor([m], dtype=torch.int32), pad(cv.cvm),
                          pad(cv.cvsd), sel, coef_t, coef_t[cv.idx_min], coef_t[cv.idx_1se],
                          torch.tensor([cv.fit.npasses]))


@dataclass
class LognetGroupsResult:
    """Per group g (one cross-validated binomial fit): the fields of LognetCvResult stacked."""
    lambdas: torch.Tensor    # [G, L] (NaN beyond nlam[g])
    nlam: torch.Tensor       # [G] int32
    cvm: torch.Tensor        # [G, L]
    cvsd: torch.Tensor       # [G, L]
    sel: torch.Tensor        # [G, 2] (idx_min, idx_1se)
    coef_min: torch.Tensor   # [G, p+1] original scale, intercept first
    coef_1se: torch.Tensor   # [G, p+1]
    npass: torch.Tensor      # [nprob]: the G full fits, then every group's fold fits (< 0:
                             # the wait for the group's full fit timed out)

    def check(self):
        """Raise NumericalError if a fold fit was truncated; the outputs are NaN already."""
        G = self.nlam.shape[0]
        bad = np.flatnonzero(self.npass.cpu().numpy()[G:] < 0).tolist()
        if bad:
            from ..utils.guards import NumericalError
            raise NumericalError(f"binomial CV fold fit(s) {bad} timed out waiting for their "
                                 "group's lambda sequence; selection is invalid")
        return self


def _group_folds(full_sets, nseg):
    """full_sets as a list (groups) of lists (folds) of segment tuples; an integer is a fold
    of one segment. A group's training set is the union of its folds."""
    groups = []
    for fs in full_sets:
        folds = [tuple(sorted({int(f)} if np.isscalar(f) else {int(x) for x in f})) for f in fs]
        flat = [x for f in folds for x in f]
        if len(folds) < 2 or any(not f for f in folds):
            raise ValueError("every group needs at least 2 non-empty folds")
        if len(set(flat)) != len(flat) or min(flat) < 0 or max(flat) >= nseg:
            raise ValueError(f"a group's folds must be disjoint sets of segments in [0, {nseg})")
        groups.append(folds)
    if not groups:
        raise ValueError("full_sets is empty")
    return groups


def cv_lognet_groups(panel, xcols, ycol, full_sets, penalty_factor=None, alpha=1.0, nlambda=100,
                     lambda_min_ratio=None, thresh=1e-7, maxit=100000) -> LognetGroupsResult:
    """G independent cv.glmnet(family="binomial") fits on one panel in one path launch.

    full_sets: per group the list of its CV folds, each a tuple of panel segments (the
    arm-split panel: fold j = segments (2j, 2j + 1)). Group g trains on the union of its
    folds with its own lambda sequence and ratio (glmnet's 1e-4 / 1e-2 rule on its own n vs
    p); its fold fits leave one fold out and follow that sequence through device flags
    (csrc/lognet.hip ``ate_lognet_path_groups``: problems 0..G-1 the full fits, then the fold
    fits group by group). The held-out deviance is one mean over the rows of a fold's
    segments (``ate_lognet_cvloss_set``); the selection is ``ate_cv_select``. No host
    synchronisation and no upload after the first call of a layout: capturable. CPU tensors
    run reference/glmnet.py per group on the same rows and folds.
    Limits (ValueError): p <= 96, an fp32/fp64 panel, <= 64 segments, <= 256 problems."""
    nseg = panel.nseg
    p = len(xcols)
    groups = _group_folds(full_sets, nseg)
    G = len(groups)
    nreal = np.asarray(panel.seg_nreal, dtype=np.int64)
    ntrain = [int(sum(nreal[list(f)].sum() for f in folds)) for folds in groups]
    flmin = [float(lambda_min_ratio) if lambda_min_ratio is not None else
             (1e-4 if n > p else 1e-2) for n in ntrain]
    vp = _rescale_vp(penalty_factor, p)
    L = int(nlambda)
    if not panel.data.is_cuda:
        return _cv_groups_cpu(panel, xcols, ycol, groups, vp, alpha, L, flmin, thresh, maxit)
    nprob = G + sum(len(folds) for folds in groups)
    if p > MAX_P:
        raise ValueError(f"device lognet supports p <= {MAX_P}, got {p}")
    if panel.data.dtype not in (torch.float32, torch.float64):
        raise ValueError("device lognet needs an fp32/fp64 panel")
    if nseg > MAX_SEGMENTS:
        raise ValueError(f"device lognet supports <= {MAX_SEGMENTS} segments, got {nseg}")
    if nprob > MAX_PATH_PROBLEMS:
        raise ValueError(f"{nprob} path problems, more than the {MAX_PATH_PROBLEMS} one "
                         "concurrent launch holds")
    if L < 3:
        raise ValueError("the concurrent path needs nlambda >= 3")
    dev = panel.device
    s = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    # problems: the G leaders, then every group's fold fits; hold: the fold fits' held-out sets
    nq = nprob - G
    masks = np.zeros((nprob, nseg), dtype=np.uint8)
    hold = np.zeros((nq, nseg), dtype=np.uint8)
    leader = np.arange(nprob, dtype=np.int32)
    Kmax = max(len(folds) for folds in groups)
    if any(len(folds) != Kmax for folds in groups):
        raise ValueError("every group needs the same number of folds")
    fidx = np.zeros((G, Kmax), dtype=np.int32)
    nfold = np.zeros((G, Kmax), dtype=np.float64)
    q = 0
    for g, folds in enumerate(groups):
        train = [x for f in folds for x in f]
        masks[g, train] = 1
        for i, f in enumerate(folds):
            masks[G + q, train] = 1
            masks[G + q, list(f)] = 0
            hold[q, list(f)] = 1
            leader[G + q] = g
            fidx[g, i] = q
            nfold[g, i] = nreal[list(f)].sum()
            q += 1
    segs = np.stack([panel.seg_bounds[:, 0], panel.seg_bounds[:, 0] + panel.seg_nreal], 1)
    segs_t = const(segs.astype(np.int64), torch.int64, dev)
    xc = const(np.asarray(xcols), torch.int32, dev)
    vp_t = const(vp, torch.float64, dev)
    masks_t = const(masks, torch.uint8, dev)
    hold_t = const(hold, torch.uint8, dev)
    leader_t = const(leader, torch.int32, dev)
    flmin_t = const(np.asarray(flmin), torch.float64, dev)
    fidx_t = const(fidx, torch.int32, dev)
    nfold_t = const(nfold, torch.float64, dev)
    a0 = torch.zeros((nprob, L), **f64)
    beta = torch.zeros((nprob, L, p), **f64)
    lam = torch.full((nprob, L), float("nan"), **f64)
    devr = torch.zeros((nprob, L), **f64)
    nlam = torch.zeros(nprob, dtype=torch.int32, device=dev)
    npass = torch.zeros(nprob, dtype=torch.int32, device=dev)
    progress = torch.zeros((G, 2), dtype=torch.int32, device=dev)   # zeroed on every call
    lampub = torch.zeros((G, L), **f64)
    dt = dtype_code(panel.data)
    X = panel.data
    _native.call("ate_lognet_path_groups", dt, X.data_ptr(), panel.cm_ld, xc.data_ptr(), p, ycol,
                 segs_t.data_ptr(), nseg, masks_t.data_ptr(), nprob, leader.ctypes.data,
                 leader_t.data_ptr(), vp_t.data_ptr(), alpha, flmin_t.data_ptr(), thresh, maxit,
                 L, a0.data_ptr(), beta.data_ptr(), lam.data_ptr(), devr.data_ptr(),
                 nlam.data_ptr(), npass.data_ptr(), progress.data_ptr(), lampub.data_ptr(), s)
    cvraw = torch.empty((nq, L), **f64)
    _native.call("ate_lognet_cvloss_set", dt, X.data_ptr(), panel.cm_ld, xc.data_ptr(), p, ycol,
                 segs_t.data_ptr(), nseg, hold_t.data_ptr(), nq, a0[G:].data_ptr(),
                 beta[G:].data_ptr(), nlam[G:].data_ptr(), L, cvraw.data_ptr(), s)
    cvm = torch.empty((G, L), **f64)
    cvsd = torch.empty((G, L), **f64)
    sel = torch.empty((G, 2), dtype=torch.int32, device=dev)
    _native.call("ate_cv_select", cvraw.data_ptr(), fidx_t.data_ptr(), nfold_t.data_ptr(), Kmax,
                 G, nlam.data_ptr(), L, cvm.data_ptr(), cvsd.data_ptr(), sel.data_ptr(),
                 npass[G:].data_ptr(), nq, s)
    coef = torch.cat([a0[:G, :, None], beta[:G]], 2)                 # [G, L, p+1]
    sl = sel.long()
    pick = lambda i: torch.gather(coef, 1, sl[:, i, None, None].expand(G, 1, p + 1))[:, 0]
    from .enet import poison_if_truncated
    cmin, c1se = poison_if_truncated(npass[G:], pick(0), pick(1))
    return LognetGroupsResult(lam[:G], nlam[:G], cvm, cvsd, sel, cmin, c1se, npass)


def _cv_groups_cpu(panel, xcols, ycol, groups, vp, alpha, L, flmin, thresh, maxit):
    X = panel.data.double()
    G, p = len(groups), len(xcols)
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64)
    lam, cvm, cvsd = nan(G, L), nan(G, L), nan(G, L)
    cmin, c1se = nan(G, p + 1), nan(G, p + 1)
    sel = torch.zeros((G, 2), dtype=torch.int32)
    nlam = torch.zeros(G, dtype=torch.int32)
    npass = torch.zeros(G, dtype=torch.int32)
    for g, folds in enumerate(groups):
        rows, fid = [], []
        for i, f in enumerate(folds):
            for sgm in f:
                r0, nr = int(panel.seg_bounds[sgm][0]), int(panel.seg_nreal[sgm])
                rows.append(np.arange(r0, r0 + nr))
                fid.append(np.full(nr, i))
        rows = np.concatenate(rows)
        cv = ref.cv_glmnet(X[xcols][:, rows].T.numpy(), X[ycol][rows].numpy(), family="binomial",
                           alpha=alpha, penalty_factor=vp, foldid=np.concatenate(fid), nlambda=L,
                           lambda_min_ratio=flmin[g], thresh=thresh, maxit=maxit)
        m = len(cv.lambdas)
        coef = np.column_stack([cv.fit.a0, cv.fit.beta])
        lam[g, :m] = torch.as_tensor(cv.lambdas)
        cvm[g, :m] = torch.as_tensor(cv.cvm)
        cvsd[g, :m] = torch.as_tensor(cv.cvsd)
        cmin[g] = torch.as_tensor(coef[cv.idx_min])
        c1se[g] = torch.as_tensor(coef[cv.idx_1se])
        sel[g, 0], sel[g, 1], nlam[g], npass[g] = cv.idx_min, cv.idx_1se, m, cv.fit.npasses
    return LognetGroupsResult(lam, nlam, cvm, cvsd, sel, cmin, c1se, npass)
