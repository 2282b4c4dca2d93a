"""Cluster-robust DML: cluster-level cross-fitting and cluster-robust standard errors for
the partially linear model (``ate_dml(clusters=)``) and the interactive model
(``ate_dml_irm(clusters=)``).

Rows that share a cluster (a household, a school, repeated observations of a person) are not
independent. Two things change against the row-level estimators:

* whole clusters go into folds (:func:`cluster_layout`): cluster j -- the j-th label in sorted
  order -- takes fold ``rng.fold_ids(J, K, seed, 0)[j]`` and each of its rows with it, so no
  nuisance is trained on rows of the cluster it predicts; the inner CV uses the outer folds
  and is cluster-respecting with them. ``clusters=np.arange(n)`` gives the row-level folds.
* the variance sums the scores within clusters first. Every score here is
  psi_i = a_i - theta b_i (IRM: a = the AIPW score, b = 1; PLR: a = wr yr, b = wr^2), and with
  t_j = sum_{i in j} psi_i

      IRM: Var = J / (J - 1) * sum_j t_j^2 / n^2        PLR: Var = sum_j t_j^2 / (sum_i b_i)^2

  (the factors mirror ``irm.mean_se`` and ``stats.dml_finalize("plr")``: singleton clusters
  give the unclustered SE algebraically). theta itself is the existing moment pass's.

The rows are stable-sorted by cluster before the panel is built, so a cluster is at most
``segs_per_fold`` contiguous runs of panel rows; a CSR over panel rows (:func:`cluster_csr`)
names them, and one deterministic segmented reduction (csrc/cluster.hip,
:func:`cluster_moments`) returns sum t^2, sum t, sum n_j^2 and max n_j. Its launch geometry
depends on n alone, so a call is one hipGraph (graph names ``dml_plr_cluster`` /
``dml_irm_cluster``) whose replays carry new clusters of the same count.

Out of scope: two-way clustering, row shards (``dist``), repeated cross-fitting, and the
gate / cate / policy / sensitivity / targets / IIVM / APOS estimators.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _native
from ..ops.devconst import const
from ..ops.panel import build_panel, dtype_code
from ..parallel import rng
from ..reference.estimators import cluster_codes
from ..result import AteResult
from .common import as_np, resolve_device

INT_MAX = 2 ** 31


@dataclass
class ClusterLayout:
    codes: np.ndarray   # (n,) cluster of every row, 0..J-1 in sorted label order
    J: int
    fid: np.ndarray     # (n,) fold of every row: that of its cluster
    perm: np.ndarray    # (n,) the stable sort of the rows by cluster


def cluster_layout(clusters, n: int, folds: int, seed: int, dist=None,
                   repeats: int = 1) -> ClusterLayout:
    """Codes, folds and row order of a clustered call; ValueError for what it does not
    serve: a wrong length, NaN / None labels, fewer than max(2, K) clusters, row shards,
    repeated cross-fitting, n or J at or above 2^31."""
    if dist is not None:
        raise ValueError("clusters= does not support row-sharded calls (dist)")
    if repeats != 1:
        raise ValueError("clusters= supports repeats = 1 only (no repeated cross-fitting)")
    lab = np.asarray(clusters.cpu() if torch.is_tensor(clusters) else clusters)
    if lab.ndim != 1 or len(lab) != n:
        raise ValueError(f"clusters must be an (n,) array of {n} labels, got shape "
                         f"{tuple(lab.shape)}")
    if lab.dtype == object:
        bad = any(v is None or (isinstance(v, float) and v != v) for v in lab)
    else:
        bad = lab.dtype.kind in "fc" and bool(np.isnan(lab).any())
    if bad:
        raise ValueError("clusters must not contain NaN or None labels")
    codes, J = cluster_codes(lab)
    if J < max(2, folds):
        raise ValueError(f"clusters= needs at least max(2, K) = {max(2, folds)} clusters, "
                         f"got {J}")
    if n >= INT_MAX or J >= INT_MAX:
        raise ValueError("clusters= supports n and J below 2^31")
    fid = rng.fold_ids(J, folds, seed, 0)[codes]
    return ClusterLayout(codes, J, fid, np.argsort(codes, kind="stable"))


def cluster_csr(row_index, codes: np.ndarray, J: int):
    """The CSR of the clusters over panel rows: (starts [J + 1], order [n]) int32 --
    ``order[starts[j]:starts[j + 1]]`` are the panel rows of cluster j, ascending; padding
    rows (``row_index`` < 0) never appear. row_index: the panel's original row per panel row;
    codes: the cluster of every original row."""
    ri = np.asarray(row_index.cpu() if torch.is_tensor(row_index) else row_index)
    rows = np.flatnonzero(ri >= 0)
    pc = np.asarray(codes)[ri[rows]]
    order = rows[np.argsort(pc, kind="stable")]
    starts = np.concatenate([[0], np.cumsum(np.bincount(pc, minlength=J))])
    return starts.astype(np.int32), order.astype(np.int32)


def cluster_chunk() -> int:
    """The positions of ``order`` one workgroup of the cluster pass owns; longer clusters are
    split into pieces of this size (csrc/cluster.hip)."""
    return int(_native.hip().ate_cluster_chunk())


def cluster_moments(a: torch.Tensor, b, starts: torch.Tensor, order: torch.Tensor, J: int,
                    theta: torch.Tensor) -> torch.Tensor:
    """[sum_j t_j^2, sum_j t_j, sum_j n_j^2, max_j n_j] (fp64) of t_j = A_j - theta B_j, the
    sums of a and b (None: b = 1) over the rows ``order[starts[j]:starts[j + 1]]``.

    a, b: [ld] fp64; starts [J + 1], order [n]: int32; theta: fp64, its first element read on
    the device (no host sync: capturable). GPU: csrc/cluster.hip ``ate_cluster_moments`` --
    two launches whose geometry depends on n alone, no floating-point atomics, equal bits run
    to run. CPU: the float64 torch twin."""
    n = order.numel()
    if J < 1 or starts.numel() != J + 1:
        raise ValueError(f"starts must hold J + 1 = {J + 1} entries, got {starts.numel()}")
    if starts.dtype != torch.int32 or order.dtype != torch.int32:
        raise ValueError("starts and order must be int32")
    if a.dtype != torch.float64 or (b is not None and (b.dtype != torch.float64
                                                       or b.numel() != a.numel())):
        raise ValueError("a and b must be fp64 vectors of one length")
    if not a.is_cuda:
        size = (starts[1:] - starts[:-1]).long()
        of = torch.repeat_interleave(torch.arange(J), size)
        rows = order.long()[:of.numel()]
        A = torch.zeros(J, dtype=torch.float64).index_add_(0, of, a[rows])
        B = size.double() if b is None else \
            torch.zeros(J, dtype=torch.float64).index_add_(0, of, b[rows])
        t = A - theta.reshape(-1)[0] * B
        sz = size.double()
        return torch.stack([(t * t).sum(), t.sum(), (sz * sz).sum(), sz.max()])
    lib = _native.hip()
    work = torch.empty(int(lib.ate_cluster_work(n)), dtype=torch.float64, device=a.device)
    out = torch.empty(4, dtype=torch.float64, device=a.device)
    a, starts, order = a.contiguous(), starts.contiguous(), order.contiguous()
    _native.call("ate_cluster_moments", a.data_ptr(),
                 None if b is None else b.contiguous().data_ptr(), a.numel(), starts.data_ptr(),
                 order.data_ptr(), n, J, theta.data_ptr(), work.data_ptr(), out.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    return out


def dml_resid_terms(pan, coef: torch.Tensor):
    """The per-row terms (a, b) = (wr yr, wr^2) of the PLR score [ld] (fp64, panel row order,
    0 on padding rows): the held-out residual pass of ``lasso.dml_residual_moments`` -- same
    arguments, same residuals -- writing the terms instead of summing moments (csrc/dml.hip
    ``ate_dml_resid_terms``; CPU: the float64 torch twin ``lasso.dml_residual_terms``)."""
    if not pan.data.is_cuda:
        from .lasso import dml_residual_terms
        t = dml_residual_terms(pan, coef.double())
        return t[:, 0].contiguous(), t[:, 1].contiguous()
    K = coef.shape[0]
    bounds = np.asarray(pan.seg_bounds[:K], dtype=np.int64)
    if K != pan.nseg or bounds[0, 0] != 0 or bounds[-1, 1] != pan.ld or \
            np.any(bounds[1:, 0] != bounds[:-1, 1]):
        raise ValueError("the coefficient blocks' segments must tile [0, ld): every row gets "
                         "its terms")
    dev = pan.device
    xc = const(pan.xcols, torch.int32, dev)
    segs = const(bounds, torch.int64, dev)
    bf = pan.dtype == torch.bfloat16
    y0, y1 = (pan.cols["Y_hi"], pan.cols["Y_lo"]) if bf else (pan.cols["Y"], -1)
    w0, w1 = (pan.cols["W_hi"], pan.cols["W_lo"]) if bf else (pan.cols["W"], -1)
    ta = torch.empty(pan.ld, dtype=torch.float64, device=dev)
    tb = torch.empty(pan.ld, dtype=torch.float64, device=dev)
    cs, bs = pan.strides()
    c = coef.double().contiguous()
    _native.call("ate_dml_resid_terms", dtype_code(pan.data), pan.data.data_ptr(), cs, bs,
                 xc.data_ptr(), len(pan.xcols), segs.data_ptr(), K, c.data_ptr(), y0, y1, w0, w1,
                 pan.cols["one"], 512 if bf else 256, ta.data_ptr(), tb.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    return ta, tb


def cluster_finalize(out: torch.Tensor, denom: torch.Tensor, J: int, correction: bool):
    """The cluster-robust SE from the cluster moments: sqrt(sum t^2) / denom (denom = n for
    IRM, sum b for PLR), with the J / (J - 1) factor when ``correction`` is set. Device
    tensors in and out (capturable)."""
    var = out[0] / (denom * denom)
    if correction:
        var = var * (J / (J - 1))
    return torch.sqrt(var.clamp(min=0))


def _csr_tensors(pan, lay):
    """The CSR over the rows of a panel built from the cluster-sorted rows."""
    starts, order = cluster_csr(pan.row_index, lay.codes[lay.perm], lay.J)
    return (torch.from_numpy(starts).to(pan.device), torch.from_numpy(order).to(pan.device))


def _diag(v, n, J, g):
    """n_clusters, max_cluster, design_effect = sum n_j^2 / n, se_unclustered from the tail
    [se_unclustered, sum t^2, sum t, sum n_j^2, max n_j] of a body's result."""
    return dict(n=n, n_clusters=J, max_cluster=int(round(v[4])) if np.isfinite(v[4]) else -1,
                design_effect=float(v[3] / n), se_unclustered=float(v[0]), hipgraph=g)


def _plr_cluster_body(pan, starts, order, folds, lambda_rule, J):
    """The clustered PLR cross-fit as one device function: the unclustered phases (theta and
    its moments, same launches), the per-row terms, the cluster pass ->
    [theta, SE, se_unclustered, the 4 cluster moments]."""
    from .lasso import dml_phases
    st = None
    for ph in dml_phases(pan, folds, lambda_rule):
        st = ph(st)
    cv = st["cv"]
    coef = (cv.coef_min if lambda_rule == "min" else cv.coef_1se).reshape(folds, 2, -1)
    a, b = dml_resid_terms(pan, coef.double().contiguous())
    res, mom = st["res"], st["mom"]
    out = cluster_moments(a, b, starts, order, J, res[:1])
    se = cluster_finalize(out, mom[1], J, False)
    return torch.cat([res[:1], se.reshape(1), res[1:2], out])


def dml_plr_lasso_cluster(Y, W, X, clusters, folds=5, seed=1991, lambda_rule="min",
                          method="DML cross-fit (LASSO)", device=None, dtype="f64", dist=None,
                          graph=True, repeats=1):
    """``lasso.dml_plr_lasso`` with whole clusters cross-fitted and the cluster-robust SE
    (module docstring). Matches reference.estimators.dml_plr_lasso(clusters=). theta carries
    the bits of the unclustered estimator on the same folds. diagnostics: n, n_clusters,
    max_cluster, design_effect, se_unclustered, hipgraph."""
    from .irm import run_body
    dev = resolve_device(device)
    Yn, Wn, Xn = as_np(Y), as_np(W), as_np(X)
    lay = cluster_layout(clusters, len(Yn), folds, seed, dist, repeats)
    q = lay.perm
    pan = build_panel(Xn[q], Wn[q], Yn[q], folds=lay.fid[q], dtype=dtype, device=dev)
    starts, order = _csr_tensors(pan, lay)
    out, g = run_body("dml_plr_cluster", _plr_cluster_body, (pan, starts, order), folds,
                      lambda_rule, lay.J, graph=graph)
    v = out.detach().double().cpu().numpy()
    return AteResult.make(method, v[0], v[1], **_diag(v[2:], len(Yn), lay.J, g))


def _irm_cluster_body(pan, starts, order, folds, lambda_rule, clip, J, counts,
                      propensity="linear"):
    """The clustered IRM cross-fit as one device function: the fit phases, the moment pass
    (theta: same launch as the unclustered estimator), the per-row scores, the cluster pass
    -> [theta, SE, se_unclustered, the 4 cluster moments, the 8 score moments]."""
    from .irm import (irm_finalize, irm_fit_phases, irm_score_moments, irm_scores,
                      propensity_link, run_phases)
    phases, _ = irm_fit_phases(pan, folds, lambda_rule, None, np.asarray(counts),
                               propensity=propensity)
    coef = run_phases(phases)["coef"]
    link = propensity_link(propensity)
    mom = irm_score_moments(pan, coef, clip, 2, link=link)
    res = irm_finalize(mom)
    psi = irm_scores(pan, coef, clip, 2, link=link)
    out = cluster_moments(psi, None, starts, order, J, res[:1])
    se = cluster_finalize(out, mom[2], J, True)
    return torch.cat([res[:1], se.reshape(1), res[1:2], out, mom])


def dml_irm_lasso_cluster(Y, W, X, clusters, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                          method="DML-IRM cross-fit (LASSO)", device=None, dtype="f64",
                          dist=None, graph=True, propensity="linear", repeats=1):
    """``irm.dml_irm_lasso`` with whole clusters cross-fitted and the cluster-robust SE (module
    docstring); either propensity. Matches reference.estimators.dml_irm_lasso(clusters=). The
    (fold, arm) cell check of the unclustered estimator applies. diagnostics: those of
    ``dml_irm_lasso`` plus n_clusters, max_cluster, design_effect, se_unclustered."""
    from .irm import (arm_split_panel, check_logit_scope, propensity_args, run_body)
    check_logit_scope(propensity, X, folds, dtype, dist)
    Yn, Wn, Xn = as_np(Y), as_np(W), as_np(X)
    lay = cluster_layout(clusters, len(Yn), folds, seed, dist, repeats)
    q = lay.perm
    pan, counts, _, n, _ = arm_split_panel(Yn[q], Wn[q], Xn[q], folds, seed, dtype, device,
                                           fold_ids=lay.fid[q])
    starts, order = _csr_tensors(pan, lay)
    out, g = run_body("dml_irm_cluster", _irm_cluster_body, (pan, starts, order), folds,
                      lambda_rule, float(clip), lay.J, tuple(counts.tolist()),
                      *propensity_args(propensity), graph=graph)
    v = out.detach().double().cpu().numpy()
    mom = v[7:]
    nt = mom[7]
    diag = _diag(v[2:7], n, lay.J, g)
    diag.update(n_clipped=int(round(mom[3])) if np.isfinite(mom[3]) else -1,
                n_treated=int(round(nt)) if np.isfinite(nt) else -1,
                rmse_g0=float(np.sqrt(mom[5] / (mom[2] - nt))),
                rmse_g1=float(np.sqrt(mom[4] / nt)), rmse_m=float(np.sqrt(mom[6] / mom[2])))
    if propensity != "linear":
        diag["propensity"] = propensity
    return AteResult.make(method, v[0], v[1], **diag)
