"""Conditional average treatment effects of the cross-fitted interactive model along one
covariate, with a uniform confidence band from a multiplier bootstrap (the ``cate(basis)`` /
``confint(joint=True)`` of DoubleML's IRM: the best linear projection of the AIPW score on a
B-spline basis, Semenova & Chernozhukov 2021; Chernozhukov, Chetverikov & Kato 2013 for the
multiplier bootstrap of a maximum).

With psi the AIPW score of ``estimators/irm.py``, x one covariate and b(x) in R^d a clamped
B-spline basis of degree q <= 3 (a partition of unity, so the intercept is in its span):

    M    = S b_i b_i'          v = S b_i psi_i          beta = M^-1 v
    e_i  = psi_i - b_i' beta   Meat = S e_i^2 b_i b_i'  Omega = M^-1 Meat M^-1     (HC0)

and on a grid x_1..x_m with g_j = b(x_j):

    cate_j = g_j' beta         se_j = sqrt(g_j' Omega g_j)
    T_b    = S xi_i^b e_i b_i  t[b, j] = g_j' M^-1 T_b / se_j,   xi Rademacher
    crit   = the ceil(level B)-th smallest of max_j |t[b, .]|

so cate -/+ crit se covers the whole curve at once with probability ``level``, where
cate -/+ 1.96 se covers one point. The fit is that of ``irm_phases``; the score pass writes
psi per row and two passes over (psi, x, row id) do the rest (csrc/cate.hip): pass 1 the
moments M, v, pass 2 -- which needs beta -- the meat and all B replicate sums with the
multipliers generated in registers, keyed by the global row id (parallel/rng.rademacher) as
those of the group estimator (estimators/gate.py). With q = 0 the basis is the indicator of
the knot cells and the curve is that estimator's step function.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..ops.linalg import spd_solve
from ..parallel import rng
from ..result import AteResult, CateResult
from .common import as_np
from .gate import _SLAB_BYTES, boot_crit, check_boot, multiplier_geometry, quantile_groups
from .irm import (arm_split_panel, check_logit_scope, comm_counts, irm_finalize, irm_fit_phases,
                  phase_scores, propensity_args, propensity_link, run_body, run_phases)

DF_MAX = 32
DEGREE_MAX = 3
GRID_MAX = 512
DF_REG = 8                    # csrc/cate.hip DREG: replicate sums in registers up to here
_SLAB_LIVE_BYTES = 16 << 20   # cap of pass 2's partial workspace when it is the working set


def check_basis(df, degree):
    if int(degree) != degree or not 0 <= int(degree) <= DEGREE_MAX:
        raise ValueError(f"degree must be an integer in 0..{DEGREE_MAX}, got {degree}")
    if int(df) != df or not int(degree) + 1 <= int(df) <= DF_MAX:
        raise ValueError(f"df must be an integer in [degree + 1, {DF_MAX}] = "
                         f"[{int(degree) + 1}, {DF_MAX}], got {df}")


def check_knots(knots, degree):
    """A clamped knot vector [df + degree + 1]: the boundary knots repeated degree + 1 times
    and strictly increasing interior knots strictly inside them. Returns df."""
    t = np.asarray(knots, dtype=np.float64).reshape(-1)
    q = int(degree)
    d = len(t) - q - 1
    check_basis(d, q)
    if not np.isfinite(t).all() or np.any(t[:q + 1] != t[0]) or np.any(t[d:] != t[-1]):
        raise ValueError("the knot vector must be finite and clamped: the boundary knots "
                         f"repeated degree + 1 = {q + 1} times")
    if not np.all(np.diff(t[q:d + 1]) > 0):
        raise ValueError("the knots are not strictly increasing (too few distinct values of "
                         f"the covariate for df = {d}, degree = {q}?): {t[q:d + 1].tolist()}")
    return d


def clamped_knots(lo, interior, hi, degree, device=None):
    """min | ... | interior | max | ... as one fp64 tensor."""
    q = int(degree)
    interior = torch.as_tensor(interior, dtype=torch.float64, device=device).reshape(-1)
    lo = torch.as_tensor(lo, dtype=torch.float64, device=interior.device).reshape(1)
    hi = torch.as_tensor(hi, dtype=torch.float64, device=interior.device).reshape(1)
    return torch.cat([lo.repeat(q + 1), interior, hi.repeat(q + 1)])


def spline_knots(pan, col, df: int, degree: int) -> torch.Tensor:
    """The clamped knot vector [df + degree + 1] of a panel column (name, or covariate index
    j for ``x{j}``) on the panel's device: the quantile edges of ``gate.quantile_groups`` with
    ``bins = df - degree`` as interior knots, between the column's min and max over the real
    rows. ValueError when they are not strictly increasing."""
    check_basis(df, degree)
    _, edges = quantile_groups(pan, col, int(df) - int(degree))
    x = pan.col(col if isinstance(col, str) else f"x{col}").double()[pan.row_index >= 0]
    t = clamped_knots(x.min(), edges, x.max(), degree)
    check_knots(t.cpu().numpy(), degree)
    return t


def quantile_knots(x, df: int, degree: int) -> np.ndarray:
    """:func:`spline_knots` of a host vector (the same order statistics)."""
    check_basis(df, degree)
    xs = np.sort(np.asarray(x, dtype=np.float64))
    bins = int(df) - int(degree)
    inner = xs[[(k * len(xs)) // bins for k in range(1, bins)]]
    t = clamped_knots(xs[0], inner, xs[-1], degree).numpy()
    check_knots(t, degree)
    return t


def basis_local(x: torch.Tensor, knots: torch.Tensor, degree: int):
    """(span [n] int64, N [n, degree + 1]): the span of every x -- the number of interior
    knots at or below it, so a point on a knot goes to the right-hand span and max x to the
    last -- and its degree + 1 non-zero basis values b_span .. b_{span + degree}, by the
    span-local Cox-de Boor recurrence of csrc/cate.hip (torch fp64, any device)."""
    q = int(degree)
    t = knots.double()
    d = t.numel() - q - 1
    x = x.double()
    sp = torch.bucketize(x, t[q + 1:d].contiguous(), right=True).clamp(max=d - q - 1)
    s = sp + q
    N = [torch.ones_like(x)] + [torch.zeros_like(x) for _ in range(q)]
    for j in range(1, q + 1):
        saved = torch.zeros_like(x)
        for r in range(j):
            hi, lo = t[s + r + 1], t[s + r + 1 - j]
            temp = N[r] / (hi - lo)
            N[r] = saved + (hi - x) * temp
            saved = (x - lo) * temp
        N[j] = saved
    return sp, torch.stack(N, dim=1)


def bspline_basis(x, knots, degree: int) -> torch.Tensor:
    """The B-spline design matrix [n, df] (fp64) of the points x on a clamped knot vector:
    the torch twin of the kernels' basis, used for the grid matrix and the CPU path."""
    knots = torch.as_tensor(knots, dtype=torch.float64)
    x = torch.as_tensor(x, dtype=torch.float64, device=knots.device).reshape(-1)
    q = int(degree)
    d = knots.numel() - q - 1
    sp, N = basis_local(x, knots, q)
    out = torch.zeros(x.numel(), d, dtype=torch.float64, device=x.device)
    out.scatter_(1, sp[:, None] + torch.arange(q + 1, device=x.device)[None, :], N)
    return out


def _check_rows(psi, x, rid, knots, degree):
    q = int(degree)
    d = knots.numel() - q - 1
    check_basis(d, q)
    ld = psi.numel()
    if x.numel() != ld or rid.numel() != ld:
        raise ValueError("psi, x and rid must have one entry per panel row")
    return d, q, ld


def moments_geometry(ld: int) -> int:
    """Workgroups (of 256 rows per chunk) of pass 1."""
    return max(1, min(-(-ld // 256), 1024))


def boot_geometry(n_boot: int, df: int, ld: int):
    """``gate.multiplier_geometry`` of pass 2: a slot per basis function, an fp64 sum per
    replicate. Up to DF_REG basis functions the replicate sums stay in registers and the
    partials are written once, under gate's workspace cap; above that they are the kernel's
    working set, read and written for every chunk, so the workspace is held to
    _SLAB_LIVE_BYTES (it stays in the last-level cache) and a workgroup walks more chunks."""
    return multiplier_geometry(n_boot, df, ld, 8, _SLAB_BYTES if df <= DF_REG else _SLAB_LIVE_BYTES)


def _cpu_rows(psi, x, rid):
    keep = torch.nonzero(rid >= 0).reshape(-1)
    return psi.double()[keep], x.double()[keep], rid[keep].numpy().astype(np.int64)


def cate_moments(psi: torch.Tensor, x: torch.Tensor, rid: torch.Tensor, knots: torch.Tensor,
                 degree: int, nbx: int | None = None) -> torch.Tensor:
    """Pass 1 over the rows with ``rid >= 0``, one fp64 buffer (flat)
    ``n | S psi | S psi^2 | rows per span [df - degree] | v [df] | M [df, df]`` with
    v = S b psi and M = S b b' (full, symmetric, banded). Sums over row shards add up.
    GPU: csrc/cate.hip ``ate_cate_moments`` (``nbx`` workgroups along the rows; one geometry,
    one set of bits); CPU: the float64 twin below, in row blocks."""
    d, q, ld = _check_rows(psi, x, rid, knots, degree)
    if not psi.is_cuda:
        p, xv, _ = _cpu_rows(psi, x, rid)
        kn = knots.double().cpu()
        cnt = torch.zeros(d - q, dtype=torch.float64)
        v = torch.zeros(d, dtype=torch.float64)
        M = torch.zeros(d, d, dtype=torch.float64)
        for i0 in range(0, p.numel(), 8192):              # row blocks: bounded temporaries
            sl = slice(i0, i0 + 8192)
            sp, _ = basis_local(xv[sl], kn, q)
            Bm = bspline_basis(xv[sl], kn, q)
            cnt += torch.bincount(sp, minlength=d - q).double()
            v += Bm.T @ p[sl]
            M += Bm.T @ Bm
        head = torch.stack([cnt.sum(), p.sum(), (p * p).sum()])
        return torch.cat([head, cnt, v, M.reshape(-1)])
    dev = psi.device
    if nbx is None:
        nbx = moments_geometry(ld)
    nbytes = _native.hip().ate_cate_moments_scratch(d, q, int(nbx))
    if nbytes < 0:
        raise ValueError(f"ate_cate_moments_scratch rejected df={d}, degree={q}, nbx={nbx}")
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(3 + (d - q) + d + d * d, dtype=torch.float64, device=dev)
    psi = psi.double().contiguous()
    x = x.double().contiguous()
    rid = rid.to(torch.int64).contiguous()
    kn = knots.to(dev, torch.float64).contiguous()
    _native.call("ate_cate_moments", psi.data_ptr(), x.data_ptr(), rid.data_ptr(), ld,
                 kn.data_ptr(), d, q, int(nbx), scratch.data_ptr(), out.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    return out


def split_moments(buf: torch.Tensor, df: int, degree: int):
    """(head [3] = n, S psi, S psi^2; span counts [df - degree]; v [df]; M [df, df]) views."""
    d, ns = df, df - degree
    return buf[:3], buf[3:3 + ns], buf[3 + ns:3 + ns + d], buf[3 + ns + d:].view(d, d)


def cate_boot(psi: torch.Tensor, x: torch.Tensor, rid: torch.Tensor, knots: torch.Tensor,
              degree: int, beta: torch.Tensor, n_boot: int, seed: int,
              nbx: int | None = None) -> torch.Tensor:
    """Pass 2 over the same rows with the fitted ``beta`` [df], one fp64 buffer (flat)
    ``Meat [df, df] | T [B, df]``: e = psi - b' beta, Meat = S e^2 b b' and
    T[r] = S xi^r e b with the Rademacher multipliers of ``rng.rademacher(seed, rid, B)``.
    GPU: csrc/cate.hip ``ate_cate_boot``; CPU: the float64 twin below, in row blocks."""
    d, q, ld = _check_rows(psi, x, rid, knots, degree)
    B = int(n_boot)
    check_boot(B)
    if beta.numel() != d:
        raise ValueError(f"beta must have df = {d} entries, got {beta.numel()}")
    if not psi.is_cuda:
        p, xv, r = _cpu_rows(psi, x, rid)
        kn = knots.double().cpu()
        be = beta.double().cpu()
        Meat = torch.zeros(d, d, dtype=torch.float64)
        T = torch.zeros(B, d, dtype=torch.float64)
        for i0 in range(0, p.numel(), 8192):              # row blocks: bounded temporaries
            sl = slice(i0, i0 + 8192)
            Bm = bspline_basis(xv[sl], kn, q)
            EB = Bm * (p[sl] - Bm @ be)[:, None]
            Meat += EB.T @ EB
            xi = torch.from_numpy(rng.rademacher(seed, r[sl], B)).double()   # [rows, B]
            T += xi.T @ EB
        return torch.cat([Meat.reshape(-1), T.reshape(-1)])
    dev = psi.device
    if nbx is None:
        nbx = boot_geometry(B, d, ld)[2]
    nbytes = _native.hip().ate_cate_boot_scratch(d, q, B, int(nbx))
    if nbytes < 0:
        raise ValueError(f"ate_cate_boot_scratch rejected df={d}, degree={q}, B={B}, nbx={nbx}")
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(d * d + B * d, dtype=torch.float64, device=dev)
    psi = psi.double().contiguous()
    x = x.double().contiguous()
    rid = rid.to(torch.int64).contiguous()
    kn = knots.to(dev, torch.float64).contiguous()
    be = beta.to(dev, torch.float64).contiguous()
    _native.call("ate_cate_boot", psi.data_ptr(), x.data_ptr(), rid.data_ptr(), ld,
                 kn.data_ptr(), be.data_ptr(), d, q, B, int(seed) & 0xFFFFFFFFFFFFFFFF, int(nbx),
                 scratch.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def split_boot(buf: torch.Tensor, df: int, n_boot: int):
    """(Meat [df, df], T [B, df]) views of a :func:`cate_boot` buffer."""
    return buf[:df * df].view(df, df), buf[df * df:].view(n_boot, df)


def cate_beta(mom: torch.Tensor, df: int, degree: int) -> torch.Tensor:
    """beta = M^-1 v from the (all-reduced) pass-1 buffer, on the device (capturable)."""
    _, _, v, M = split_moments(mom, df, degree)
    return spd_solve(M[None], v[None])[0]


def fin_size(df: int, m: int) -> int:
    return 2 * m + 4 + df + df * df


def cate_finalize(mom: torch.Tensor, boot: torch.Tensor, beta: torch.Tensor, gbasis: torch.Tensor,
                  df: int, degree: int, n_boot: int, level: float = 0.95) -> torch.Tensor:
    """``cate [m] | se [m] | crit | overall theta, SE | n | beta [df] | Omega [df, df]``
    (flat) from the (all-reduced) buffers of the two passes and the grid's basis matrix
    ``gbasis`` [m, df], on the device with no host sync (capturable). M^-1 by ``spd_solve``
    with identity right-hand sides; the overall ATE / SE by the rule of ``irm_finalize``."""
    d = df
    head, _, _, M = split_moments(mom, d, degree)
    Meat, T = split_boot(boot, d, n_boot)
    eye = torch.eye(d, dtype=torch.float64, device=mom.device)
    Minv = spd_solve(M[None].expand(d, d, d), eye)          # symmetric: rows = columns
    Omega = Minv @ Meat @ Minv.T
    G = gbasis.to(mom.device, torch.float64)
    cate = G @ beta
    se = torch.sqrt(((G @ Omega) * G).sum(dim=1).clamp(min=0))
    crit = boot_crit((T @ (Minv.T @ G.T)) / se, n_boot, level)
    overall = irm_finalize(torch.stack([head[1], head[2], head[0]]))
    return torch.cat([cate, se, crit.reshape(1), overall, head[:1], beta, Omega.reshape(-1)])


def cate_phases(pan, x, rid, knots, gbasis, degree: int, folds: int, lambda_rule="min",
                clip=0.01, n_boot=999, level=0.95, seed=1991, comm=None, seg_counts=None,
                propensity="linear"):
    """The CATE step as phases for utils.graphs.SegmentedStep: those of ``irm_phases`` up to
    the fitted coefficients, then

    B'   per-row AIPW scores psi (csrc/irm.hip ate_irm_scores)              device
    B''  pass 1: n, S psi, S psi^2, span counts, v, M (csrc/cate.hip)       device
    C06  all-reduce of that buffer                                          collective (world > 1)
    C    beta = M^-1 v (csrc/linalg.hip spd_solve)                          device
    B''' pass 2: Meat, T (csrc/cate.hip)                                    device
    C06  all-reduce of that buffer                                          collective (world > 1)
    C    M^-1, Omega, cate, se, crit, overall theta / SE (fp64 torch ops)   device

    The result state holds "fin" (:func:`cate_finalize`), "mom", "boot", "beta", "coef" and
    "cv"."""
    q, B = int(degree), int(n_boot)
    d = knots.numel() - q - 1
    check_basis(d, q)
    check_boot(B, level)
    phases, reduce = irm_fit_phases(pan, folds, lambda_rule, comm, seg_counts,
                                    propensity=propensity)

    def phase_moments(st):
        return {**st, "mom": cate_moments(st["psi"], x, rid, knots, q)}

    def phase_beta(st):
        return {**st, "beta": cate_beta(st["mom"], d, q)}

    def phase_boot(st):
        return {**st, "boot": cate_boot(st["psi"], x, rid, knots, q, st["beta"], B, seed)}

    def phase_final(st):
        return {**st, "fin": cate_finalize(st["mom"], st["boot"], st["beta"], gbasis, d, q, B,
                                           level)}

    phases += [phase_scores(pan, clip, propensity_link(propensity)), phase_moments]
    if reduce is not None:
        phases.append(reduce("mom"))
    phases += [phase_beta, phase_boot]
    if reduce is not None:
        phases.append(reduce("boot"))
    phases.append(phase_final)
    return phases


def span_counts(x: torch.Tensor, rid: torch.Tensor, knots: torch.Tensor, degree: int,
                comm=None) -> np.ndarray:
    """(Global) rows per span, on the host (one tiny all-reduce over row shards)."""
    q = int(degree)
    d = knots.numel() - q - 1
    sp, _ = basis_local(x[rid >= 0], knots.to(x.device), q)
    c = torch.bincount(sp, minlength=d - q).double()
    if comm is not None and comm.world_size > 1:
        comm.all_reduce_(c)
    return c.cpu().numpy()


def check_spans(counts):
    """Every span needs at least 2 rows (a basis function without data makes M singular)."""
    for s in np.flatnonzero(np.asarray(counts) < 2):
        raise ValueError(f"span {int(s)} of the knot vector has {int(counts[s])} row(s): "
                         "every span needs at least 2")


def check_grid(grid, lo, hi):
    if isinstance(grid, torch.Tensor):
        grid = grid.detach().cpu().numpy()
    g = np.asarray(grid, dtype=np.float64).reshape(-1)
    if not 1 <= len(g) <= GRID_MAX:
        raise ValueError(f"the grid must have between 1 and {GRID_MAX} points, got {len(g)}")
    if not (np.isfinite(g).all() and g.min() >= lo and g.max() <= hi):
        raise ValueError(f"grid points must lie inside [min x, max x] = [{lo}, {hi}]")
    return g


def irm_cate_panel(pan, x: torch.Tensor, knots: torch.Tensor, degree: int, grid, folds: int,
                   lambda_rule="min", clip=0.01, n_boot=999, level=0.95, seed=1991, comm=None,
                   seg_counts=None, rid=None, check=True, propensity="linear"):
    """The CATE curve along ``x`` with a uniform band on an arm-split fold panel (the layout
    of ``irm_crossfit_panel``) -> (fin, mom, boot, cv); ``fin`` as :func:`cate_finalize`.

    x: fp64 [ld], the covariate in panel row order (e.g. ``pan.col("x0").double()``).
    knots: the clamped knot vector (:func:`spline_knots`; row shards must share one).
    grid: the points of the curve, or their basis matrix [m, df] as a device tensor.
    rid: the rows' global ids, negative on rows to skip (default: the panel's ``row_index``,
    -1 on padding). check: validate the knots, the grid and every span's (global) row count on
    the host; with ``check=False`` and ``grid`` a basis matrix nothing here syncs with the
    host (the call is capturable)."""
    q = int(degree)
    if x.numel() != pan.ld:
        raise ValueError(f"x must have one value per panel row ({pan.ld}), got {x.numel()}")
    if rid is None:
        rid = pan.row_index
    knots = knots.to(pan.device, torch.float64)
    if check:
        kn = knots.cpu().numpy()
        check_knots(kn, q)
        check_spans(span_counts(x, rid, knots, q, comm))
    if isinstance(grid, torch.Tensor) and grid.dim() == 2:
        gbasis = grid
    else:
        kn = knots.cpu().numpy()
        gbasis = bspline_basis(check_grid(grid, kn[0], kn[-1]), knots.cpu(), q).to(pan.device)
    st = run_phases(cate_phases(pan, x, rid, knots, gbasis, q, folds, lambda_rule, clip, n_boot,
                                level, seed, comm, seg_counts, propensity))
    return st["fin"], st["mom"], st["boot"], st.get("cv")


def _cate_body(pan, x, rid, knots, gbasis, folds, lambda_rule, clip, degree, n_boot, level, seed,
               dist=None, counts=None, propensity="linear"):
    """The whole estimator as one device function (GraphCache captures it): fin | mom | boot."""
    comm, seg_counts = comm_counts(dist, counts)
    fin, mom, boot, _ = irm_cate_panel(pan, x, knots, degree, gbasis, folds, lambda_rule, clip,
                                       n_boot, level, seed, comm=comm, rid=rid, check=False,
                                       seg_counts=seg_counts, propensity=propensity)
    return torch.cat([fin, mom, boot])


def default_grid(x, points: int = 100) -> np.ndarray:
    """``points`` equally spaced points between the 5 % and 95 % order statistics of x."""
    xs = np.sort(np.asarray(x, dtype=np.float64))
    n = len(xs)
    return np.linspace(xs[(5 * n) // 100], xs[min((95 * n) // 100, n - 1)], int(points))


def read_fin(v, df: int, m: int):
    """(cate [m], se [m], crit, overall ate, overall se, n, beta [df], Omega [df, df]) of a
    :func:`cate_finalize` vector on the host."""
    v = np.asarray(v, dtype=np.float64)
    o = 2 * m
    return (v[:m], v[m:o], v[o], v[o + 1], v[o + 2], v[o + 3], v[o + 4:o + 4 + df],
            v[o + 4 + df:o + 4 + df + df * df].reshape(df, df))


def dml_irm_cate_lasso(Y, W, X, by, df=5, degree=3, knots=None, grid=None, n_boot=999, level=0.95,
                       folds=5, seed=1991, lambda_rule="min", clip=0.01,
                       method="DML-IRM CATE curve (LASSO)", device=None, dtype="f64", dist=None,
                       graph=True, keep_boot=False, propensity="linear") -> CateResult:
    """The conditional average treatment effect of the cross-fitted interactive model
    (``irm.dml_irm_lasso``: same folds, same nuisances, same score) as a B-spline curve along
    one covariate, with pointwise and uniform ``level`` confidence bounds from ``n_boot``
    Rademacher multiplier draws. Matches reference.estimators.dml_irm_cate.

    by: a column index into X, or an (n,) vector. df, degree: the basis (degree + 1 <= df <=
    32, degree 0..3); knots: a clamped knot vector [df + degree + 1] instead of the default
    quantile knots (then ``df`` is read from it). grid: the points of the curve (at most 512,
    inside [min x, max x]); default 100 equally spaced points between the 5 % and 95 % order
    statistics of x.

    graph: as ``dml_irm_lasso``, one captured hipGraph on a GPU per (layout, df, degree,
    grid size, n_boot); x, the row ids, the knots and the grid's basis matrix are graph
    inputs, so another column in the same layout replays it. keep_boot: the result's
    ``boot`` holds the raw replicate sums T [n_boot, df], M and the meat."""
    Yn, Xn = as_np(Y), as_np(X)
    check_logit_scope(propensity, X, folds, dtype, dist)
    check_boot(n_boot, level)
    check_basis(df if knots is None else len(knots) - degree - 1, degree)
    n_boot, q = int(n_boot), int(degree)
    if np.ndim(by) == 0:
        if int(by) != by or not 0 <= int(by) < Xn.shape[1]:
            raise ValueError(f"by must index the {Xn.shape[1]} columns of X, got {by}")
        xn = np.ascontiguousarray(Xn[:, int(by)])
    else:
        xn = as_np(by).reshape(-1)
        if len(xn) != len(Yn):
            raise ValueError(f"by must be a vector with one value per row ({len(Yn)}), "
                             f"got shape {np.shape(by)}")
    if not np.isfinite(xn).all():
        raise ValueError("the covariate of the curve must be finite")
    sharded = dist is not None and dist.world > 1
    # every rank needs the same knots and grid: the covariate of all shards, gathered
    x_all = dist.gather_rows(torch.as_tensor(xn)).numpy() if sharded else xn
    if knots is None:
        kn = quantile_knots(x_all, df, q)
    else:
        kn = np.asarray(knots, dtype=np.float64).reshape(-1)
        check_knots(kn, q)
        if x_all.min() < kn[0] or x_all.max() > kn[-1]:
            raise ValueError(f"the boundary knots [{kn[0]}, {kn[-1]}] must contain every x "
                             f"([{x_all.min()}, {x_all.max()}])")
    d = len(kn) - q - 1
    gr = check_grid(default_grid(x_all) if grid is None else grid, kn[0], kn[-1])
    m = len(gr)
    scount = np.bincount(np.searchsorted(kn[q + 1:d], xn, side="right"), minlength=d - q)
    pan, counts, _, _, rid = arm_split_panel(Y, W, X, folds, seed, dtype, device, dist,
                                             extra_counts=scount, check_extra=check_spans)
    x = pan.gather_rows(torch.as_tensor(xn))
    knt = torch.from_numpy(kn).to(pan.device)
    gbasis = bspline_basis(gr, kn, q).to(pan.device)
    out, g = run_body("dml_irm_cate", _cate_body, (pan, x, rid, knt, gbasis), folds, lambda_rule,
                      float(clip), q, n_boot, float(level), int(seed), dist,
                      tuple(counts.tolist()), *propensity_args(propensity), graph=graph,
                      dist=dist)
    v = out.detach().double().cpu().numpy()
    nf = fin_size(d, m)
    cate, se, crit, o_ate, o_se, n, beta, omega = read_fin(v[:nf], d, m)
    overall = AteResult.make("DML-IRM cross-fit (LASSO)", o_ate, o_se,
                             n=int(round(n)) if np.isfinite(n) else -1)
    nm = 3 + (d - q) + d + d * d
    _, cnt, _, M = split_moments(torch.from_numpy(v[nf:nf + nm]), d, q)
    res = CateResult.make(method, gr, cate, se, crit, beta, omega, kn, q, n_boot, level, overall,
                          hipgraph=g, span_counts=[int(round(c)) for c in cnt.tolist()])
    if propensity != "linear":
        res.diagnostics["propensity"] = propensity
    if keep_boot:
        Meat, T = split_boot(torch.from_numpy(v[nf + nm:]), d, n_boot)
        res.boot = {"T": T.numpy().copy(), "M": M.numpy().copy(), "meat": Meat.numpy().copy()}
    return res
