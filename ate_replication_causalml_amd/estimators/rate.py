"""The rank-weighted average treatment effect (RATE) of a treatment-priority rule on the
cross-fitted interactive model: the TOC curve, its area (AUTOC), the Qini coefficient and
half-sample bootstrap standard errors (grf's ``rank_average_treatment_effect``; Yadlowsky,
Fleming, Shah, Brunskill & Wager 2021). It answers "if I treat in this order, does the order
find the rows with large effects at all": AUTOC / SE is the test for heterogeneity that the
rule can exploit.

With psi the AIPW score of ``estimators/irm.py`` and a priority S_i (higher = treat first)
on the n evaluation rows, sorted by priority descending; rows of equal priority form a run
that enters at once. k_r = rows up to and including run r, c_r its size,
A(k) = S_{j <= k} psi_(j), theta = A(n) / n:

    TOC(u) = A(e) / e - theta         e = the end of the run holding position ceil(u n)
    AUTOC  = (1 / n) S_r c_r (A(k_r) / k_r - theta)
    QINI   = (1 / n) S_r c_r (k_r / n) (A(k_r) / k_r - theta)

Half-sample replicate b keeps row i when its bit of ``rng.half_sample`` is set; with M_b, A_b
the included count and sum along the ranking, n_b = M_b(n), theta_b = A_b(n) / n_b and c_r^b
run r's included count:

    U_b = S_r c_r^b A_b(k_r) / M_b(k_r)   V_b = S_r c_r^b A_b(k_r)   W_b = S_r c_r^b M_b(k_r)
    AUTOC_b = U_b / n_b - theta_b         QINI_b = (V_b - W_b theta_b) / n_b^2
    TOC_b(u_j) = A_b(e_j) / M_b(e_j) - theta_b     at the full-sample run ends e_j

SE = the sd over b (ddof 1; a half sample of free size has the variance of the full-sample
estimator, so it is not rescaled); pointwise intervals are normal, the uniform band over the
TOC grid takes ``gate.boot_crit`` of (TOC_b - TOC) / SE over the points with SE > 0. Every
statistic is invariant to a shift of psi; the device body centres psi on the evaluation
rows' mean first, which keeps V - W theta away from cancellation.

The fit is that of ``irm_phases``; the score pass writes psi per row and csrc/rate.hip walks
the ranking for all replicates at once. The sorted order and the per-position flags are made
by :func:`rate_order` outside the captured body and are graph inputs, so a replay can take
other priorities.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..parallel import rng
from ..result import RateResult
from .common import as_np
from .gate import _SLAB_BYTES, boot_crit, check_boot, multiplier_geometry
from .irm import (arm_split_panel, check_logit_scope, comm_counts, irm_fit_phases, phase_scores,
                  propensity_args, propensity_link, run_body, run_phases)

GRID_MAX = 64
ROWS_MIN = 128              # evaluation rows: an empty half sample must be out of reach
FIRST_MIN = 64              # rows the first grid point enters: so must M_b(e_1) = 0
ROWS_END = 1 << 27          # n below this: W_b <= n^2 < 2^53 is exact in fp64
HEAD = 5                    # n_b, A_b(n), U_b, V_b, W_b before the grid pairs


def check_grid(q) -> np.ndarray:
    """The TOC grid: default 0.1, ..., 1.0; at most 64 strictly increasing points in (0, 1]."""
    g = np.arange(1, 11) / 10.0 if q is None else np.asarray(q, dtype=np.float64).reshape(-1)
    if not 1 <= len(g) <= GRID_MAX:
        raise ValueError(f"q must hold between 1 and {GRID_MAX} points, got {len(g)}")
    if not (np.isfinite(g).all() and g[0] > 0.0 and g[-1] <= 1.0 and np.all(np.diff(g) > 0)):
        raise ValueError("q must be strictly increasing in (0, 1]")
    return g


def grid_positions(q, n: int) -> np.ndarray:
    """The 1-based position ceil(u n) of every grid point (a product within 1e-9 of an
    integer counts as that integer, the rule of ``result.boot_rank``)."""
    k = np.ceil(np.asarray(q, dtype=np.float64) * n - 1e-9).astype(np.int64)
    return np.clip(k, 1, n)


def check_rows(priority, subset, q, rows: int):
    """The host checks of the evaluation rows, before any device work -> (priority fp64 [rows],
    mask bool [rows], n)."""
    pr = np.asarray(priority, dtype=np.float64).reshape(-1)
    if len(pr) != rows:
        raise ValueError(f"priority must be a vector with one value per row ({rows}), "
                         f"got {len(pr)}")
    if subset is None:
        mask = np.ones(rows, dtype=bool)
    else:
        mask = np.asarray(subset)
        if mask.dtype != bool or mask.shape != (rows,):
            raise ValueError(f"subset must be a boolean mask with one entry per row ({rows})")
    n = int(mask.sum())
    if n >= ROWS_END:
        raise ValueError(f"at most 2^27 - 1 evaluation rows are supported, got {n}")
    if n < ROWS_MIN:
        raise ValueError(f"RATE needs at least {ROWS_MIN} evaluation rows, got {n}")
    pe = pr[mask]
    if not np.isfinite(pe).all():
        raise ValueError("the priority must be finite on every evaluation row")
    k1 = int(grid_positions(q[:1], n)[0])
    entered = int((pe >= np.partition(pe, n - k1)[n - k1]).sum())
    if entered < FIRST_MIN:
        raise ValueError(f"the first grid point q = {q[0]} enters {entered} rows: at least "
                         f"{FIRST_MIN} are needed")
    return pr, mask, n


def rate_order(priority: torch.Tensor, rid: torch.Tensor, subset, grid):
    """The ranking of the evaluation rows as the kernel reads it, on the device of
    ``priority`` -> (order int32 [n], flags int32 [n]). priority, rid [ld] in panel row order;
    the evaluation rows are those with ``rid >= 0`` (and ``subset`` True, a bool [ld] or
    None). order[j]: the panel row at position j of the stable sort by priority descending,
    global row id ascending. flags[j]: bit 0 = position j ends a run of equal priorities;
    bits 1..7 = 1 + the first point of ``grid`` whose rows end at j (0: none), bits 8..14 =
    how many consecutive grid points end there. Syncs with the host: call it outside a
    captured body."""
    q = check_grid(grid)
    keep = rid >= 0
    if subset is not None:
        keep = keep & subset.to(keep.device, torch.bool)
    rows = torch.nonzero(keep).reshape(-1)
    n = rows.numel()
    if n < 1:
        raise ValueError("no evaluation rows")
    rows = rows[torch.sort(rid[rows], stable=True).indices]
    ps, idx = torch.sort(priority[rows].double(), descending=True, stable=True)
    order = rows[idx].to(torch.int32)
    end = torch.ones(n, dtype=torch.bool, device=ps.device)
    end[:-1] = ps[:-1] != ps[1:]
    flags = end.to(torch.int32)
    ends = torch.nonzero(end).reshape(-1)
    k = torch.as_tensor(grid_positions(q, n), device=ps.device)
    e = ends[torch.searchsorted(ends, k - 1)]                 # the run end at or after k - 1
    first = torch.ones(len(q), dtype=torch.bool, device=ps.device)
    first[1:] = e[1:] != e[:-1]
    j = torch.arange(len(q), device=ps.device)
    cnt = torch.searchsorted(e, e, right=True) - j
    flags[e[first]] |= (((j[first] + 1) << 1) | (cnt[first] << 8)).to(torch.int32)
    return order, flags


def rate_entered(flags: torch.Tensor) -> torch.Tensor:
    """Rows entered at every grid point (int64 [Q]) from the flags of :func:`rate_order`."""
    pos = torch.nonzero((flags >> 1) != 0).reshape(-1)
    return torch.repeat_interleave(pos + 1, ((flags[pos] >> 8) & 127).long())


def rate_geometry(n_boot: int, n: int):
    """``gate.multiplier_geometry`` of csrc/rate.hip: B + 1 slots (the full sample is one),
    one slot of six 8-byte partials per replicate -> (threads, stream blocks, pieces)."""
    return multiplier_geometry(int(n_boot) + 1, 1, n, 48, _SLAB_BYTES)


def rate_boot(psi: torch.Tensor, order: torch.Tensor, flags: torch.Tensor, rid: torch.Tensor,
              n_grid: int, n_boot: int, seed: int, nbx: int | None = None,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """The walk along the ranking for the full sample (row 0) and ``n_boot`` half samples
    (rows 1..), one fp64 buffer [B + 1, 5 + 2 Q]: n_b, A_b(n), U_b, V_b, W_b and the Q pairs
    (A_b(e_j), M_b(e_j)) -- (0, 0) where M_b(e_j) = 0. psi, rid [ld] in panel row order;
    order, flags [n] from :func:`rate_order`. GPU: csrc/rate.hip (``nbx`` pieces of the
    ranking; one geometry, one set of bits; ``out``: a buffer to fill, every entry is written);
    CPU: the float64 twin below, in blocks of positions with the prefix sums carried across."""
    Q, B = int(n_grid), int(n_boot)
    if not 1 <= Q <= GRID_MAX:
        raise ValueError(f"between 1 and {GRID_MAX} grid points are supported, got {Q}")
    check_boot(B)
    ld, n = psi.numel(), order.numel()
    if rid.numel() != ld or flags.numel() != n or not 1 <= n <= ld:
        raise ValueError("psi and rid must have one entry per panel row, order and flags one "
                         "per evaluation row")
    if not psi.is_cuda:
        o = order.long().numpy()
        p = psi.double().numpy()[o]
        r = rid.numpy().astype(np.int64)[o]
        f = flags.numpy().astype(np.int64)
        out = np.zeros((B + 1, HEAD + 2 * Q))
        A = np.zeros(B + 1)
        M = np.zeros(B + 1, dtype=np.int64)
        last = np.zeros(B + 1, dtype=np.int64)
        U, V = np.zeros(B + 1), np.zeros(B + 1)
        Wt = np.zeros(B + 1, dtype=np.int64)
        for i0 in range(0, n, 8192):                      # blocks: bounded temporaries
            sl = slice(i0, i0 + 8192)
            inc = np.ones((len(p[sl]), B + 1), dtype=np.uint8)
            inc[:, 1:] = rng.half_sample(seed, r[sl], B)
            Ab = np.cumsum(np.vstack([A[None], inc * p[sl, None]]), axis=0)[1:]
            Mb = M + np.cumsum(inc, axis=0, dtype=np.int64)
            ends = np.flatnonzero(f[sl] & 1)
            if len(ends):
                Me, Ae = Mb[ends], Ab[ends]
                c = np.diff(np.vstack([last[None], Me]), axis=0)
                on = c > 0
                U += (c * np.divide(Ae, Me, out=np.zeros_like(Ae), where=on)).sum(axis=0)
                V += (c * Ae).sum(axis=0)
                Wt += (c * Me).sum(axis=0)
                last = Me[-1]
            for jp in np.flatnonzero(f[sl] >> 1):
                j0, jn = int((f[sl][jp] >> 1) & 127) - 1, int((f[sl][jp] >> 8) & 127)
                for j in range(j0, j0 + jn):
                    out[:, HEAD + 2 * j] = np.where(Mb[jp] > 0, Ab[jp], 0.0)
                    out[:, HEAD + 2 * j + 1] = Mb[jp]
            A, M = Ab[-1], Mb[-1]
        out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4] = M, A, U, V, Wt
        return torch.from_numpy(out)
    dev = psi.device
    if nbx is None:
        nbx = rate_geometry(B, n)[2]
    nbytes = _native.hip().ate_rate_boot_scratch(Q, B, int(nbx))
    if nbytes < 0:
        raise ValueError(f"ate_rate_boot_scratch rejected Q={Q}, B={B}, nbx={nbx}")
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(B + 1, HEAD + 2 * Q, dtype=torch.float64, device=dev)
    elif (out.shape != (B + 1, HEAD + 2 * Q) or out.dtype != torch.float64
          or not out.is_contiguous() or out.device != dev):
        raise ValueError(f"out must be a contiguous fp64 [{B + 1}, {HEAD + 2 * Q}] tensor on {dev}")
    psi = psi.double().contiguous()
    order = order.to(torch.int32).contiguous()
    flags = flags.to(torch.int32).contiguous()
    rid = rid.to(torch.int64).contiguous()
    _native.call("ate_rate_boot", psi.data_ptr(), order.data_ptr(), flags.data_ptr(),
                 rid.data_ptr(), ld, n, Q, B, int(seed) & 0xFFFFFFFFFFFFFFFF, int(nbx),
                 scratch.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def rate_stats(buf: torch.Tensor):
    """(theta [B + 1], AUTOC [B + 1], QINI [B + 1], TOC [B + 1, Q]) of every row of a
    :func:`rate_boot` buffer. The products are taken so that one run through every row gives
    exact zeros: U = c A / M and V = c A there, and n_b theta_b, (W_b / n_b) A_b(n) repeat
    them bit for bit."""
    nb, An, U, V, Wt = (buf[:, k] for k in range(HEAD))
    GA, GM = buf[:, HEAD::2], buf[:, HEAD + 1::2]
    theta = An / nb
    autoc = (U - nb * theta) / nb
    qini = (V - (Wt / nb) * An) / (nb * nb)
    toc = torch.where(GM > 0, GA / GM.clamp(min=1.0), torch.zeros_like(GA)) - theta[:, None]
    return theta, autoc, qini, toc


def fin_size(n_grid: int) -> int:
    return 7 + 2 * n_grid


def rate_finalize(buf: torch.Tensor, shift, n_boot: int, level: float = 0.95) -> torch.Tensor:
    """``ate | AUTOC, SE | QINI, SE | crit | n | TOC [Q] | SE [Q]`` (flat, 7 + 2 Q) from a
    :func:`rate_boot` buffer of scores centred by ``shift`` (added back to the ATE), on the
    device with no host sync (capturable). SE: the sd over the replicates, ddof 1. crit: the
    ceil(level B)-th smallest of max_j |TOC_b(u_j) - TOC(u_j)| / SE_j over the points with
    SE_j > 0 (u = 1, where TOC is identically 0, is never among them)."""
    theta, autoc, qini, toc = rate_stats(buf)
    se_a, se_q, se_t = autoc[1:].std(), qini[1:].std(), toc[1:].std(dim=0)
    live = se_t > 0
    t = torch.where(live, (toc[1:] - toc[0]) / torch.where(live, se_t, torch.ones_like(se_t)),
                    torch.zeros_like(se_t))
    crit = boot_crit(t, n_boot, level)
    head = torch.stack([theta[0] + shift, autoc[0], se_a, qini[0], se_q, crit, buf[0, 0]])
    return torch.cat([head, toc[0], se_t])


def rate_phases(pan, rid, order, flags, n_grid: int, folds: int, lambda_rule="min", clip=0.01,
                n_boot=200, level=0.95, seed=1991, comm=None, seg_counts=None,
                propensity="linear"):
    """The RATE step as phases for utils.graphs.SegmentedStep: those of ``irm_phases`` up to
    the fitted coefficients, then

    B'  per-row AIPW scores psi (csrc/irm.hip ate_irm_scores)               device
    B'' psi centred on the evaluation rows, the walk (csrc/rate.hip)        device
    C   ATE, AUTOC, QINI, TOC, SEs, crit (fp64 torch ops)                   device

    The ranking is global, so there is no all-reduce: one device holds every row. The result
    state holds "fin" (:func:`rate_finalize`), "boot" (the buffer), "shift", "coef", "cv"."""
    Q, B = int(n_grid), int(n_boot)
    check_boot(B, level)
    if comm is not None and comm.world_size > 1:
        raise ValueError("RATE ranks all rows: row shards (world > 1) are not supported")
    phases, _ = irm_fit_phases(pan, folds, lambda_rule, comm, seg_counts, propensity=propensity)

    def phase_boot(st):
        shift = st["psi"].index_select(0, order).mean()
        return {**st, "shift": shift,
                "boot": rate_boot(st["psi"] - shift, order, flags, rid, Q, B, seed)}

    def phase_final(st):
        return {**st, "fin": rate_finalize(st["boot"], st["shift"], B, level)}

    return phases + [phase_scores(pan, clip, propensity_link(propensity)), phase_boot, phase_final]


def _rate_body(pan, rid, order, flags, folds, lambda_rule, clip, n_grid, n_boot, level, seed,
               dist=None, counts=None, propensity="linear"):
    """The whole estimator as one device function (GraphCache captures it): fin | boot."""
    comm, seg_counts = comm_counts(dist, counts)
    st = run_phases(rate_phases(pan, rid, order, flags, n_grid, folds, lambda_rule, clip, n_boot,
                                level, seed, comm, seg_counts, propensity))
    return torch.cat([st["fin"], st["boot"].reshape(-1)])


def dml_irm_rate_lasso(Y, W, X, priority, q=None, subset=None, n_boot=200, level=0.95, folds=5,
                       seed=1991, lambda_rule="min", clip=0.01,
                       method="DML-IRM RATE (LASSO)", device=None, dtype="f64", dist=None,
                       graph=True, keep_boot=False, propensity="linear", clusters=None,
                       repeats=1) -> RateResult:
    """AUTOC, the Qini coefficient and the TOC curve of the priority rule ``priority`` on the
    AIPW scores of the cross-fitted interactive model (``irm.dml_irm_lasso``: same folds, same
    nuisances, same score), with half-sample bootstrap standard errors, normal pointwise
    intervals and a uniform band over the TOC grid. Matches reference.estimators.dml_irm_rate.

    priority: an (n,) vector, or a column index into X; higher = treat first, ties enter
    together. q: the TOC grid (default 0.1, ..., 1.0; at most 64 strictly increasing points
    in (0, 1]). subset: a boolean mask of the evaluation rows (default: all).

    A priority fitted on the evaluation rows' own outcomes -- the policy tree or the CATE
    curve of the same call -- gives an optimistic RATE. Fit the rule on other rows and pass
    ``subset=`` their complement: with ``ate_dml_irm_policy(train=mask)``, ``subset=~mask``.

    ValueError before any device work: row shards (``dist`` with world > 1: the ranking is
    global), ``clusters``, ``repeats`` != 1, a non-finite priority on an evaluation row, fewer
    than 128 evaluation rows, a first grid point entering fewer than 64 rows, n >= 2^27.

    graph: as ``dml_irm_lasso``, one captured hipGraph on a GPU; the order and flags of
    :func:`rate_order` are graph inputs, so a call with another priority on the same rows
    replays it. keep_boot: the result's ``boot`` holds the raw [n_boot + 1, 5 + 2 Q] buffer."""
    Yn, Xn = as_np(Y), as_np(X)
    if dist is not None and dist.world > 1:
        raise ValueError("RATE ranks all rows: row shards (dist with world > 1) are not "
                         "supported")
    if clusters is not None:
        raise ValueError("RATE does not support clusters")
    if repeats != 1:
        raise ValueError("RATE does not support repeated cross-fitting (repeats must be 1)")
    check_logit_scope(propensity, X, folds, dtype, dist)
    check_boot(n_boot, level)
    n_boot = int(n_boot)
    grid = check_grid(q)
    Q = len(grid)
    if np.ndim(priority) == 0:
        if int(priority) != priority or not 0 <= int(priority) < Xn.shape[1]:
            raise ValueError(f"priority must index the {Xn.shape[1]} columns of X, "
                             f"got {priority}")
        priority = np.ascontiguousarray(Xn[:, int(priority)])
    pr, mask, n = check_rows(as_np(priority), subset, grid, len(Yn))
    pan, counts, _, _, rid = arm_split_panel(Y, W, X, folds, seed, dtype, device, dist)
    order, flags = rate_order(pan.gather_rows(torch.as_tensor(pr)), rid,
                              pan.gather_rows(torch.as_tensor(mask)), grid)
    out, g = run_body("dml_irm_rate", _rate_body, (pan, rid, order, flags), folds, lambda_rule,
                      float(clip), Q, n_boot, float(level), int(seed), dist,
                      tuple(counts.tolist()), *propensity_args(propensity), graph=graph,
                      dist=dist)
    v = out.detach().double().cpu().numpy()
    res = RateResult.make(method, grid, rate_entered(flags).cpu().numpy(), v[:fin_size(Q)], n,
                          int((flags & 1).sum().item()), n_boot, level, hipgraph=g)
    if propensity != "linear":
        res.diagnostics["propensity"] = propensity
    if keep_boot:
        res.boot = v[fin_size(Q):].reshape(n_boot + 1, HEAD + 2 * Q).copy()
    return res
