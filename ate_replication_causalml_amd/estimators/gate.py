"""Group average treatment effects (GATEs) of the cross-fitted interactive model with a
simultaneous confidence band from a multiplier bootstrap (the ``gate()`` / ``bootstrap()`` /
``confint(joint=True)`` of DoubleML's IRM; Chernozhukov et al. 2018 §5.1 for the score,
Chernozhukov, Chetverikov & Kato 2013 for the multiplier bootstrap of a maximum).

With psi the AIPW score of ``estimators/irm.py`` and disjoint covariate-defined groups g:

    theta_g = mean of psi over group g,   SE_g = sd of psi over g / sqrt(n_g)
    t[b, g] = S_{i in g} xi_i^b (psi_i - theta_g) / (n_g SE_g),   xi Rademacher
    crit    = the ceil(level B)-th smallest of max_g |t[b, .]|

so theta_g -/+ crit SE_g covers every group at once with probability ``level``, where
theta_g -/+ 1.96 SE_g covers one. The fit is that of ``irm_phases``; the score pass then
writes psi per row (csrc/irm.hip ``ate_irm_scores``) and one pass over (psi, group, row id)
accumulates all B x G replicate sums with the multipliers generated in registers
(csrc/gate.hip): A = S xi psi and Z = S xi, so S xi (psi - theta_g) = A - theta_g Z and no
group mean is needed inside the pass. Multipliers are keyed by the global row id
(parallel/rng.rademacher): the same draws at every world size and in every panel order.
The launch geometry (:func:`multiplier_geometry`) and the critical value (:func:`boot_crit`)
are shared with the CATE curve (estimators/cate.py), as the device core is
(csrc/boot_common.hpp).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..parallel import rng
from ..result import AteResult, GateResult, boot_rank
from .common import as_np
from .irm import (arm_split_panel, comm_counts, irm_finalize, irm_fit_phases, mean_se,
                  phase_scores, propensity_args, propensity_link, check_logit_scope, run_body,
                  run_phases)

N_GROUPS_MAX = 64
N_BOOT_MAX = 4096
_SLAB_BYTES = 64 << 20      # cap of the bootstrap kernels' partial workspace


def check_boot(n_boot, level=0.95):
    if int(n_boot) != n_boot or not 1 <= int(n_boot) <= N_BOOT_MAX:
        raise ValueError(f"n_boot must be an integer in [1, {N_BOOT_MAX}], got {n_boot}")
    boot_rank(level, int(n_boot))


def check_groups(counts):
    """``counts``: (global) rows per group. At most 64 groups, each with at least 2 rows
    (a group's SE needs a sample variance)."""
    c = np.asarray(counts)
    if len(c) < 1 or len(c) > N_GROUPS_MAX:
        raise ValueError(f"between 1 and {N_GROUPS_MAX} groups are supported, got {len(c)}")
    for g in np.flatnonzero(c < 2):
        raise ValueError(f"group {int(g)} has {int(c[g])} row(s): every group needs at least 2")


def multiplier_geometry(n_boot: int, slots: int, ld: int, bytes_per_item: int, cap: int):
    """(threads per workgroup, stream blocks, workgroups along the rows) of the multiplier
    bootstrap kernels, the host side of ``geometry`` in csrc/boot_common.hpp: 32 threads per
    Philox stream of 128 replicates, up to 8 streams per workgroup; about 1024 workgroups in
    all, fewer when the [workgroup][slot][replicate] partials of ``bytes_per_item`` bytes
    each would exceed ``cap`` bytes."""
    nst = -(-n_boot // 128)
    ch = 64 * ((min(nst, 8) + 1) // 2)
    nby = -(-nst // (ch // 32))
    nbx = min(-(-ld // ch), max(1, 1024 // nby))
    nbx = max(1, min(nbx, cap // (nby * slots * 4 * ch * bytes_per_item)))
    return ch, nby, nbx


def boot_geometry(n_boot: int, n_groups: int, ld: int):
    """:func:`multiplier_geometry` of csrc/gate.hip: a slot per group, an fp64 sum and an
    integer count per replicate."""
    return multiplier_geometry(n_boot, n_groups, ld, 12, _SLAB_BYTES)


def boot_crit(t: torch.Tensor, n_boot: int, level: float) -> torch.Tensor:
    """The critical value of a joint band from the replicates' statistics t [B, points]: the
    ceil(level B)-th smallest of max |t[b, .]|. Device ops only."""
    return torch.sort(t.abs().max(dim=1).values).values[boot_rank(level, n_boot) - 1]


def group_boot(psi: torch.Tensor, gid: torch.Tensor, rid: torch.Tensor, n_groups: int,
               n_boot: int, seed: int, nbx: int | None = None) -> torch.Tensor:
    """The grouped multiplier-bootstrap sums of per-row scores, one fp64 buffer
    ``mom [G, 3] | A [B, G] | Z [B, G]`` (flat): mom = (n_g, S psi, S psi^2), A = S xi psi,
    Z = S xi (exact integers) over the rows with ``gid == g``; rows with gid -1 are skipped.
    ``rid``: int64 global row ids, the multipliers' key. Sums over row shards add up, so one
    all-reduce of the buffer covers a sharded panel. GPU: csrc/gate.hip (``nbx`` workgroups
    along the rows; one geometry, one set of bits); CPU: the float64 twin below."""
    G, B = int(n_groups), int(n_boot)
    if not 1 <= G <= N_GROUPS_MAX:
        raise ValueError(f"between 1 and {N_GROUPS_MAX} groups are supported, got {G}")
    check_boot(B)
    ld = psi.numel()
    if gid.numel() != ld or rid.numel() != ld:
        raise ValueError("psi, gid and rid must have one entry per panel row")
    if not psi.is_cuda:
        keep = torch.nonzero((gid >= 0) & (gid < G)).reshape(-1)
        p = psi.double()[keep].numpy()
        g = gid[keep].numpy().astype(np.int64)
        r = rid[keep].numpy().astype(np.int64)
        mom = np.stack([np.bincount(g, minlength=G).astype(np.float64),
                        np.bincount(g, weights=p, minlength=G),
                        np.bincount(g, weights=p * p, minlength=G)], axis=1)
        A = np.zeros((B, G))
        Z = np.zeros((B, G), dtype=np.int64)
        for i0 in range(0, len(p), 8192):                 # row blocks: bounded temporaries
            sl = slice(i0, i0 + 8192)
            xi = rng.rademacher(seed, r[sl], B)           # int8 [rows, B]
            onehot = np.zeros((len(p[sl]), G))
            onehot[np.arange(len(p[sl])), g[sl]] = 1.0
            A += xi.T.astype(np.float64) @ (onehot * p[sl, None])
            Z += xi.T.astype(np.int64) @ onehot.astype(np.int64)
        return torch.from_numpy(np.concatenate([mom.ravel(), A.ravel(),
                                                Z.astype(np.float64).ravel()]))
    dev = psi.device
    if nbx is None:
        nbx = boot_geometry(B, G, ld)[2]
    nbytes = _native.hip().ate_group_boot_scratch(G, B, int(nbx))
    if nbytes < 0:
        raise ValueError(f"ate_group_boot_scratch rejected G={G}, B={B}, nbx={nbx}")
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(3 * G + 2 * B * G, dtype=torch.float64, device=dev)
    psi = psi.double().contiguous()
    gid = gid.to(torch.int32).contiguous()
    rid = rid.to(torch.int64).contiguous()
    _native.call("ate_group_boot", psi.data_ptr(), gid.data_ptr(), rid.data_ptr(), ld, G, B,
                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(nbx), scratch.data_ptr(), out.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    return out


def split_boot(buf: torch.Tensor, n_groups: int, n_boot: int):
    """(mom [G, 3], A [B, G], Z [B, G]) views of a :func:`group_boot` buffer."""
    G, B = n_groups, n_boot
    return (buf[:3 * G].view(G, 3), buf[3 * G:3 * G + B * G].view(B, G),
            buf[3 * G + B * G:].view(B, G))


def gate_finalize(buf: torch.Tensor, n_groups: int, n_boot: int, level: float = 0.95):
    """``theta [G] | SE [G] | n [G] | crit | overall theta, SE`` (flat, 3 G + 3) from the
    (all-reduced) :func:`group_boot` buffer, on the device with no host sync (capturable).
    theta_g and SE_g by the rule of ``irm_finalize``; t = (A - theta_g Z) / (n_g SE_g); crit
    the ceil(level B)-th smallest of max_g |t|; the overall ATE / SE from the summed group
    moments."""
    mom, A, Z = split_boot(buf, n_groups, n_boot)
    n, s1, s2 = mom[:, 0], mom[:, 1], mom[:, 2]
    theta, se = mean_se(s1, s2, n)
    crit = boot_crit((A - theta * Z) / (n * se), n_boot, level)
    overall = irm_finalize(torch.stack([s1.sum(), s2.sum(), n.sum()]))
    return torch.cat([theta, se, n, crit.reshape(1), overall])


def bin_groups(pan, col, edges: torch.Tensor) -> torch.Tensor:
    """Group codes int32 [ld] of a panel column on the device: the number of ``edges``
    (ascending) at or below the row's value, -1 on padding rows."""
    x = pan.col(col if isinstance(col, str) else f"x{col}").double()
    g = torch.bucketize(x, edges.to(x.device, torch.float64), right=True).to(torch.int32)
    return torch.where(pan.row_index >= 0, g, torch.full_like(g, -1))


def quantile_groups(pan, col, bins: int, edges: torch.Tensor | None = None):
    """Bin a panel column (name, or covariate index j for ``x{j}``) into ``bins`` quantile
    groups on the device -> (gid int32 [ld], edges [bins - 1]). The edges are the order
    statistics at rank k n / bins of this panel's real rows; pass ``edges`` to reuse them
    (row shards must share one set of edges to share their groups)."""
    if not 1 <= bins <= N_GROUPS_MAX:
        raise ValueError(f"between 1 and {N_GROUPS_MAX} groups are supported, got {bins}")
    if edges is None:
        x = pan.col(col if isinstance(col, str) else f"x{col}").double()
        xs = torch.sort(x[pan.row_index >= 0]).values
        at = torch.as_tensor([(k * xs.numel()) // bins for k in range(1, bins)],
                             dtype=torch.long, device=xs.device)
        edges = xs[at]
    return bin_groups(pan, col, edges), edges


def gate_phases(pan, gid, rid, n_groups: int, folds: int, lambda_rule="min", clip=0.01,
                n_boot=999, level=0.95, seed=1991, comm=None, seg_counts=None,
                propensity="linear"):
    """The group-effect step as phases for utils.graphs.SegmentedStep: those of
    ``irm_phases`` up to the fitted coefficients, then

    B'  per-row AIPW scores psi (csrc/irm.hip ate_irm_scores)               device
    B'' grouped multiplier-bootstrap sums mom | A | Z (csrc/gate.hip)       device
    C06 all-reduce of that one buffer                                       collective (world > 1)
    C   theta_g, SE_g, crit, overall theta / SE (fp64 torch ops)            device

    The result state holds "fin" [3 G + 3] (:func:`gate_finalize`), "boot" (the buffer),
    "coef" and "cv"."""
    G, B = int(n_groups), int(n_boot)
    check_boot(B, level)
    phases, reduce = irm_fit_phases(pan, folds, lambda_rule, comm, seg_counts,
                                    propensity=propensity)

    def phase_boot(st):
        return {**st, "boot": group_boot(st["psi"], gid, rid, G, B, seed)}

    def phase_final(st):
        return {**st, "fin": gate_finalize(st["boot"], G, B, level)}

    phases += [phase_scores(pan, clip, propensity_link(propensity)), phase_boot]
    if reduce is not None:
        phases.append(reduce("boot"))
    phases.append(phase_final)
    return phases


def group_counts(gid: torch.Tensor, n_groups: int, comm=None) -> np.ndarray:
    """(Global) rows per group, on the host (one tiny all-reduce over row shards)."""
    c = torch.bincount(gid[gid >= 0].long(), minlength=n_groups).double()
    if comm is not None and comm.world_size > 1:
        comm.all_reduce_(c)
    return c.cpu().numpy()


def irm_gate_panel(pan, gid: torch.Tensor, folds: int, lambda_rule="min", clip=0.01, n_boot=999,
                   level=0.95, seed=1991, comm=None, seg_counts=None, rid=None, n_groups=None,
                   propensity="linear"):
    """Group ATEs with a joint band on an arm-split fold panel (the layout of
    ``irm_crossfit_panel``) -> (fin [3 G + 3], boot buffer, cv).

    gid: int32 [ld] group codes in panel row order, -1 on padding (and on rows to leave
    out); e.g. :func:`quantile_groups`. rid: the rows' global ids (default: the panel's
    ``row_index``, which device-generated panels fill with global ids at every world size).
    n_groups: the number of groups when known -- then nothing here syncs with the host (the
    call is capturable) and the caller has checked the groups; otherwise it is read from
    ``gid`` and every group's (global) row count is checked."""
    if gid.numel() != pan.ld:
        raise ValueError(f"gid must have one code per panel row ({pan.ld}), got {gid.numel()}")
    if n_groups is None:
        n_groups = int(gid.max().item()) + 1
        if comm is not None and comm.world_size > 1:
            t = torch.as_tensor([float(n_groups)], device=pan.device)
            comm.all_reduce_max_(t)
            n_groups = int(t.item())
        if n_groups > N_GROUPS_MAX:
            raise ValueError(f"at most {N_GROUPS_MAX} groups are supported, got {n_groups}")
        check_groups(group_counts(gid, n_groups, comm))
    if rid is None:
        rid = pan.row_index
    st = run_phases(gate_phases(pan, gid, rid, n_groups, folds, lambda_rule, clip, n_boot, level,
                                seed, comm, seg_counts, propensity))
    return st["fin"], st["boot"], st.get("cv")


def _gate_body(pan, gid, rid, folds, lambda_rule, clip, n_groups, n_boot, level, seed, dist=None,
               counts=None, propensity="linear"):
    """The whole estimator as one device function (GraphCache captures it): fin | boot."""
    comm, seg_counts = comm_counts(dist, counts)
    fin, boot, _ = irm_gate_panel(pan, gid, folds, lambda_rule, clip, n_boot, level, seed,
                                  comm=comm, rid=rid, n_groups=n_groups, seg_counts=seg_counts,
                                  propensity=propensity)
    return torch.cat([fin, boot])


def dml_irm_gate_lasso(Y, W, X, groups, folds=5, seed=1991, lambda_rule="min", clip=0.01,
                       n_boot=999, level=0.95, method="DML-IRM group ATEs (LASSO)", device=None,
                       dtype="f64", dist=None, graph=True, keep_boot=False,
                       propensity="linear") -> GateResult:
    """Group average treatment effects of the cross-fitted interactive model
    (``irm.dml_irm_lasso``: same folds, same nuisances, same score) with pointwise and
    simultaneous ``level`` confidence bounds from ``n_boot`` Rademacher multiplier draws.
    ``groups``: an (n,) array of arbitrary labels, one disjoint group per distinct value
    (at most 64, each with at least 2 rows). Matches reference.estimators.dml_irm_gate.

    graph: as ``dml_irm_lasso``, one captured hipGraph on a GPU; the group codes are a graph
    input, so a call with other groups in the same panel layout replays it. keep_boot: the
    result's ``boot`` holds the raw replicate sums A, Z [n_boot, G]. propensity: as
    ``dml_irm_lasso`` ("logit": the binomial CV-LASSO propensity, with its limits)."""
    check_logit_scope(propensity, X, folds, dtype, dist)
    check_boot(n_boot, level)
    n_boot = int(n_boot)
    gl = np.asarray(groups)
    rows = len(as_np(Y))
    if gl.ndim != 1 or len(gl) != rows:
        raise ValueError(f"groups must be a vector with one label per row ({rows}), "
                         f"got shape {gl.shape}")
    if dist is not None and dist.world > 1:
        # every rank needs the same codes: the labels of all shards, gathered
        labels_all = dist.gather_rows(torch.as_tensor(gl)).numpy()
        labels = np.unique(labels_all)
        codes = np.searchsorted(labels, gl)
    else:
        labels, codes = np.unique(gl, return_inverse=True)
    G = len(labels)
    if G > N_GROUPS_MAX:
        raise ValueError(f"at most {N_GROUPS_MAX} groups are supported, got {G}")
    pan, counts, _, _, rid = arm_split_panel(
        Y, W, X, folds, seed, dtype, device, dist,
        extra_counts=np.bincount(codes, minlength=G), check_extra=check_groups)
    gid = torch.where(rid >= 0, pan.gather_rows(torch.as_tensor(codes.astype(np.int32))),
                      torch.full((pan.ld,), -1, dtype=torch.int32, device=pan.device))
    out, g = run_body("dml_irm_gate", _gate_body, (pan, gid, rid), folds, lambda_rule,
                      float(clip), G, n_boot, float(level), int(seed), dist,
                      tuple(counts.tolist()), *propensity_args(propensity), graph=graph,
                      dist=dist)
    v = out.detach().double().cpu().numpy()
    theta, se, n = v[:G], v[G:2 * G], v[2 * G:3 * G]
    crit, o_ate, o_se = v[3 * G:3 * G + 3]
    overall = AteResult.make("DML-IRM cross-fit (LASSO)", o_ate, o_se,
                             n=int(round(n.sum())) if np.isfinite(n).all() else -1)
    res = GateResult.make(method, labels, n, theta, se, crit, n_boot, level, overall, hipgraph=g)
    if propensity != "linear":
        res.diagnostics["propensity"] = propensity
    if keep_boot:
        _, A, Z = split_boot(torch.from_numpy(v[3 * G + 3:]), G, n_boot)
        res.boot = {"A": A.numpy().copy(), "Z": Z.numpy().copy()}
    return res
