"""Exact depth-2 policy trees on the AIPW scores of the cross-fitted interactive model: whom
to treat? (policy learning on doubly robust scores, Athey & Wager 2021; the exact tree search
of ``policytree``, Zhou, Athey & Wager 2023; DoubleML's ``policy_tree`` fits a greedy CART on
the same signal).

With psi the AIPW score of ``estimators/irm.py``, r = psi - cost and a 0/1 policy pi, the
value of pi over a set of rows is mean(pi r): the gain over treating nobody. The tree is the
depth <= 2 partition of up to 32 binned features (at most 64 bins each) that maximises that
value on the training rows, found exactly:

    leaf      with S the sum of r over its training rows: value max(S, 0), treat iff S > 0
    node      at remaining depth k > 0: the best of "stay a leaf" and every split (j, t) with
              at least ``min_leaf`` training rows on each side, a split being worth the sum
              of its children's best values at depth k - 1
    ties      candidates ordered leaf first, then (j, t) ascending; a later one replaces the
              incumbent only if strictly better (so no useless split survives)

Every sum that decides the tree is an integer: q = rint(r 2^e) as int64 with
e = min(30, 61 - L - x), max|r| = m 2^x (frexp) and L = the bit length of the row count, so
S|q| < 2^62. GPU, CPU path, every launch geometry and every world size pick the same tree bit
for bit. A non-finite score is quantised as 0 and turns every reported value into NaN.

The value of every candidate tree is a combination of 2-D prefix sums of feature-pair
histograms of q, so the search is one pass over the rows (csrc/policy.hip
``ate_policy_pair_hist``: a 64 x 64 tile of (S q, count) per feature pair, accumulated in LDS)
plus a tiny search over the histograms (``ate_policy_search``).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _native
from ..result import PolicyTreeResult
from ..utils.graphs import Collective
from .common import as_np
from .irm import (arm_split_panel, check_logit_scope, comm_counts, irm_fit_phases, mean_se,
                  phase_scores, propensity_args, propensity_link, run_body,
                  run_phases)

N_FEATURES_MAX = 32
N_BINS_MAX = 64
TILE = N_BINS_MAX * N_BINS_MAX
REC = 16          # tree record: root (j, t), left (j, t), right (j, t), 4 actions, value, n
N_SUMS = 18       # per evaluation set: n, S r, S r^2, S pi r, S pi r^2, S pi, 4 x (n, S r, S r^2)
N_FIN = 20        # per evaluation set: value, treat_all, advantage with SEs, share, n, 4 x (n, mean, SE)
_JT = 3           # tiles per workgroup of the histogram kernel (csrc/policy.hip)


# ---------------------------------------------------------------- arguments, bins
def check_tree_args(depth, bins, min_leaf):
    if depth not in (0, 1, 2):
        raise ValueError(f"depth must be 0, 1 or 2, got {depth}")
    if int(bins) != bins or not 2 <= int(bins) <= N_BINS_MAX:
        raise ValueError(f"bins must be an integer in [2, {N_BINS_MAX}], got {bins}")
    if int(min_leaf) != min_leaf or int(min_leaf) < 1:
        raise ValueError(f"min_leaf must be an integer >= 1, got {min_leaf}")


def check_features(features, p: int) -> list:
    """1..32 distinct column indices into the p columns of X."""
    f = np.asarray(features).reshape(-1)
    if not 1 <= len(f) <= N_FEATURES_MAX:
        raise ValueError(f"between 1 and {N_FEATURES_MAX} features are supported, got {len(f)}")
    if not np.all(f == np.floor(f)) or f.min() < 0 or f.max() >= p:
        raise ValueError(f"features must index the {p} columns of X, got {list(f)}")
    f = [int(v) for v in f]
    if len(set(f)) != len(f):
        raise ValueError(f"features must be distinct, got {f}")
    return f


def feature_edges(x, bins: int) -> np.ndarray:
    """Ascending distinct split points of one feature: every distinct value but the smallest
    when there are at most ``bins`` of them (exact splits of dummies and small integers),
    else the order statistics at rank k n / bins, k = 1..bins-1, deduplicated (the rule of
    ``gate.quantile_groups``)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if not np.isfinite(x).all():
        raise ValueError("policy features must be finite")
    u = np.unique(x)
    if len(u) <= bins:
        return u[1:]
    xs = np.sort(x)
    return np.unique(xs[[(k * len(xs)) // bins for k in range(1, bins)]])


def bin_codes(x, edges) -> np.ndarray:
    """uint8 codes: the number of edges at or below the value (so the split (j, t) sends
    x < edges[t], codes <= t, left)."""
    return np.searchsorted(np.asarray(edges, dtype=np.float64), np.asarray(x, dtype=np.float64),
                           side="right").astype(np.uint8)


def pair_index(d: int, a: int, b: int) -> int:
    """Tile of the feature pair a <= b in a :func:`pair_hist` buffer."""
    return a * d - a * (a - 1) // 2 + (b - a)


def hist_geometry(d: int, ld: int) -> int:
    """Workgroups along the rows of the histogram kernel: at least 16384 rows each, about 512
    workgroups in all (each feature j1 takes ceil((d - j1) / 3) workgroups per row block; one
    workgroup fills a CU's LDS, and every workgroup flushes its tiles with global atomics)."""
    groups = sum(-(-(d - j) // _JT) for j in range(d))
    return max(1, min(-(-ld // 16384), max(1, 512 // groups)))


# ---------------------------------------------------------------- fixed point
def score_range(psi: torch.Tensor, cost: torch.Tensor, use: torch.Tensor) -> torch.Tensor:
    """[max |psi - cost| over the finite rows with use >= 0, 1 if one of those rows is not
    finite else 0] fp64, on the device with no host sync; row shards combine by max."""
    r = psi.double() - cost.double()
    live = use >= 0
    ok = torch.isfinite(r)
    m = torch.where(live & ok, r.abs(), torch.zeros_like(r)).max()
    return torch.stack([m, (live & ~ok).any().double()])


def scale_exponent(rng2: torch.Tensor, n_rows: int) -> torch.Tensor:
    """e = min(30, 61 - L - x) as int32 [1] from :func:`score_range` (max = m 2^x by frexp,
    L = the bit length of the (global) row count): |q| <= 2^(x + e) <= 2^(61 - L) for each of
    fewer than 2^L rows, so S|q| < 2^62. Device ops only."""
    x = torch.frexp(rng2[0]).exponent.to(torch.int64)
    e = torch.clamp(61 - int(n_rows).bit_length() - x, max=30)
    return e.to(torch.int32).reshape(1)


def quantize(psi: torch.Tensor, cost, e) -> torch.Tensor:
    """q = rint((psi - cost) 2^e) int64, round-half-even, 0 where not finite (host twin of the
    kernel's quantisation)."""
    r = psi.double().cpu().numpy() - float(cost)
    ok = np.isfinite(r)
    q = np.rint(np.ldexp(np.where(ok, r, 0.0), int(e)))
    return torch.from_numpy(q.astype(np.int64))


def _dev_scalar(v, dtype, dev):
    if isinstance(v, torch.Tensor):
        return v.to(device=dev, dtype=dtype).reshape(1)
    return torch.tensor([v], dtype=dtype, device=dev)


# ---------------------------------------------------------------- pair histogram
def pair_hist(psi: torch.Tensor, cost, e, use: torch.Tensor, codes: torch.Tensor, nb,
              nbx: int | None = None, priv: bool | None = None) -> torch.Tensor:
    """The feature-pair histograms of the quantised scores over the training rows (use == 0):
    int64 [d (d + 1) / 2, 2, 64, 64], tile :func:`pair_index` (a <= b), plane 0 the sum of q
    and plane 1 the row count, cell [code_a, code_b]. Integer sums over row shards add up, so
    one all-reduce covers a sharded panel.

    psi fp64 [ld]; cost, e: numbers or one-element device tensors (graph inputs); use [ld]
    (-1 skip, 0 train, 1 held out); codes uint8 [d, ld]; nb: bins per feature [d]. A row whose
    code of a feature is >= nb is left out of that feature's tiles: a guard against indexing
    past a tile, in every build, not a way to leave rows out (that is ``use``); the search
    expects histograms of codes < nb. GPU: csrc/policy.hip, ``nbx`` workgroups along the rows (same
    bits for every nbx); ``priv`` (default: on unless ATE_POLICY_PLAIN_SMALL=1) gives tiles of
    at most 64 cells one copy per lane. CPU: the integer torch twin."""
    d, ld = int(codes.shape[0]), int(codes.shape[1])
    if not 1 <= d <= N_FEATURES_MAX:
        raise ValueError(f"between 1 and {N_FEATURES_MAX} features are supported, got {d}")
    if psi.numel() != ld or use.numel() != ld:
        raise ValueError("psi, use and every row of codes must have one entry per panel row")
    if codes.dtype != torch.uint8:
        raise ValueError(f"codes must be uint8, got {codes.dtype}")
    dev = psi.device
    nbt = torch.as_tensor(nb, dtype=torch.int32).to(dev).reshape(-1)
    if nbt.numel() != d:
        raise ValueError(f"nb must have one bin count per feature ({d}), got {nbt.numel()}")
    npair = d * (d + 1) // 2
    if not psi.is_cuda:
        q = quantize(psi, float(torch.as_tensor(cost).reshape(-1)[0]),
                     int(torch.as_tensor(e).reshape(-1)[0]))
        c = codes.long()
        nbl = nbt.long().clamp(1, N_BINS_MAX)
        train = use.reshape(-1) == 0
        out = torch.zeros(npair * 2 * TILE, dtype=torch.int64)
        for a in range(d):
            for b in range(a, d):
                keep = train & (c[a] < nbl[a]) & (c[b] < nbl[b])
                at = pair_index(d, a, b) * 2 * TILE + c[a, keep] * N_BINS_MAX + c[b, keep]
                out.index_add_(0, at, q[keep])
                out.index_add_(0, at + TILE, torch.ones_like(at))
        return out.view(npair, 2, N_BINS_MAX, N_BINS_MAX)
    if nbx is None:
        nbx = hist_geometry(d, ld)
    if priv is None:
        priv = os.environ.get("ATE_POLICY_PLAIN_SMALL", "0") in ("", "0")
    entries = _native.hip().ate_policy_pair_hist_scratch(d)
    if entries != npair * 2 * TILE:
        raise ValueError(f"ate_policy_pair_hist_scratch({d}) = {entries}, expected {npair * 2 * TILE}")
    out = torch.empty(entries, dtype=torch.int64, device=dev).view(npair, 2, N_BINS_MAX, N_BINS_MAX)
    psi = psi.double().contiguous()
    use8 = use.to(torch.int8).contiguous()
    codes = codes.contiguous()
    ct = _dev_scalar(cost, torch.float64, dev)
    et = _dev_scalar(e, torch.int32, dev)
    _native.call("ate_policy_pair_hist", psi.data_ptr(), ct.data_ptr(), et.data_ptr(),
                 use8.data_ptr(), codes.data_ptr(), nbt.data_ptr(), ld, d, int(nbx), int(bool(priv)),
                 out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


# ---------------------------------------------------------------- search
def _pos(v):
    return np.maximum(v, 0)


def tree_search(hist: torch.Tensor, nb, depth: int = 2, min_leaf: int = 1) -> torch.Tensor:
    """The best tree of depth <= ``depth`` from the (all-reduced) :func:`pair_hist` buffer ->
    the tree record, int64 [16]: (j, t) of the root, of the left and of the right child (-1,
    -1 for a leaf; j indexes the features of the histogram), the leaf actions LL, LR, RL, RR
    (a leaf node repeats its action), the total value in q units, the training-row count.
    GPU: csrc/policy.hip (at most three launches, no host sync); CPU: the vectorised twin
    below -- cumulative sums, first maximum in key order."""
    check_tree_args(depth, 2, min_leaf)
    d = int(round((np.sqrt(8 * hist.shape[0] + 1) - 1) / 2))
    if d * (d + 1) // 2 != hist.shape[0] or tuple(hist.shape[1:]) != (2, N_BINS_MAX, N_BINS_MAX) \
            or hist.dtype != torch.int64:
        raise ValueError(f"hist must be int64 [d (d + 1) / 2, 2, 64, 64], got {tuple(hist.shape)}")
    if hist.is_cuda:
        dev = hist.device
        nbt = torch.as_tensor(nb, dtype=torch.int32).to(dev).reshape(-1)
        if nbt.numel() != d:
            raise ValueError(f"nb must have one bin count per feature ({d}), got {nbt.numel()}")
        entries = _native.hip().ate_policy_pair_hist_scratch(d)     # the prefix sums
        if entries != hist.numel():
            raise ValueError(f"ate_policy_pair_hist_scratch({d}) = {entries}, hist has {hist.numel()}")
        work = torch.empty(entries + d * N_BINS_MAX * 4, dtype=torch.int64, device=dev)
        rec = torch.empty(REC, dtype=torch.int64, device=dev)
        _native.call("ate_policy_search", hist.contiguous().data_ptr(), nbt.data_ptr(), d,
                     int(depth), int(min_leaf), work.data_ptr(), rec.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
        return rec
    nbl = np.clip(np.asarray(torch.as_tensor(nb).cpu()).reshape(-1).astype(np.int64), 1, N_BINS_MAX)
    if len(nbl) != d:
        raise ValueError(f"nb must have one bin count per feature ({d}), got {len(nbl)}")
    P = hist.numpy().cumsum(axis=2).cumsum(axis=3)
    ml = int(min_leaf)
    T = np.arange(N_BINS_MAX)

    def tile(a, b):          # [2, ta, tb]: rows with code_a <= ta and code_b <= tb
        return P[pair_index(d, a, b)] if a <= b else P[pair_index(d, b, a)].transpose(0, 2, 1)

    S0, N0 = (int(v) for v in P[0][:, -1, -1])
    margin = [tile(j, j)[:, :, -1] for j in range(d)]            # [2, t]: code_j <= t
    allowed = np.concatenate([T <= nbl[j] - 2 for j in range(d)])   # key j * 64 + t
    rec = np.zeros(REC, dtype=np.int64)
    rec[11] = N0

    def finish(value, nodes, acts):
        rec[:6] = nodes
        rec[6:10] = acts
        rec[10] = value
        return torch.from_numpy(rec)

    leaf = finish(max(S0, 0), -1, int(S0 > 0))
    if depth == 0:
        return leaf
    # per root split (key1): the two sides' best depth-(depth - 1) subtrees
    SL = np.concatenate([margin[j][0] for j in range(d)])
    NL = np.concatenate([margin[j][1] for j in range(d)])
    SR, NR = S0 - SL, N0 - NL
    root_ok = allowed & (NL >= ml) & (NR >= ml)
    val = np.stack([_pos(SL), _pos(SR)])                          # [side, key1]: leaves
    key = np.full((2, d * N_BINS_MAX), -1, dtype=np.int64)
    if depth == 2:
        for j1 in range(d):
            k1 = slice(j1 * N_BINS_MAX, (j1 + 1) * N_BINS_MAX)
            # candidates [t1, 1 + key2]: the leaf, then every (j2, t2) in key order
            cl = np.full((N_BINS_MAX, 1 + d * N_BINS_MAX), -1, dtype=np.int64)
            cr = cl.copy()
            cl[:, 0], cr[:, 0] = val[0, k1], val[1, k1]
            for j2 in range(d):
                k2 = slice(1 + j2 * N_BINS_MAX, 1 + (j2 + 1) * N_BINS_MAX)
                t12 = tile(j1, j2)
                SLL, NLL = t12[0], t12[1]                         # [t1, t2]
                SLR, NLR = SL[k1, None] - SLL, NL[k1, None] - NLL
                SRL, NRL = margin[j2][0][None, :] - SLL, margin[j2][1][None, :] - NLL
                SRR, NRR = SR[k1, None] - SRL, NR[k1, None] - NRL
                ok2 = allowed[None, j2 * N_BINS_MAX:(j2 + 1) * N_BINS_MAX]
                cl[:, k2] = np.where(ok2 & (NLL >= ml) & (NLR >= ml), _pos(SLL) + _pos(SLR), -1)
                cr[:, k2] = np.where(ok2 & (NRL >= ml) & (NRR >= ml), _pos(SRL) + _pos(SRR), -1)
            for side, c in enumerate((cl, cr)):
                at = c.argmax(axis=1)                             # the first maximum
                val[side, k1] = c[T, at]
                key[side, k1] = at - 1
    cand = np.concatenate([[max(S0, 0)], np.where(root_ok, val[0] + val[1], -1)])
    at = int(cand.argmax())
    if at == 0:
        return leaf
    k1 = at - 1
    j1, t1 = divmod(k1, N_BINS_MAX)
    nodes, acts = [j1, t1], []
    for side in (0, 1):
        S = int(SL[k1] if side == 0 else SR[k1])
        k2 = int(key[side, k1])
        if k2 < 0:
            nodes += [-1, -1]
            acts += [int(S > 0)] * 2
            continue
        j2, t2 = divmod(k2, N_BINS_MAX)
        SLL = int(tile(j1, j2)[0, t1, t2])
        lo = SLL if side == 0 else int(margin[j2][0][t2]) - SLL
        nodes += [j2, t2]
        acts += [int(lo > 0), int(S - lo > 0)]
    return finish(int(cand[at]), nodes, acts)


def apply_tree(rec: torch.Tensor, codes: torch.Tensor):
    """(policy [ld] int64 0/1, leaf [ld] int64 in 0..3 = 2 right + child right) of the tree
    record on a code matrix uint8 [d, ld], with torch ops on the record's device and no host
    sync (capturable)."""
    rec = rec.to(codes.device)
    rj, rt = rec[0], rec[1]
    c = codes.index_select(0, rj.clamp(min=0).reshape(1)).reshape(-1).long()
    right = (rj >= 0) & (c > rt)
    cj = torch.where(right, rec[4], rec[2])
    ct = torch.where(right, rec[5], rec[3])
    c = codes.gather(0, cj.clamp(min=0).reshape(1, -1)).reshape(-1).long()
    leaf = 2 * right.long() + ((cj >= 0) & (c > ct)).long()
    return rec[6:10][leaf], leaf


def mask_record(rec: torch.Tensor, bad: torch.Tensor) -> torch.Tensor:
    """The record itself when ``bad`` (the non-finite flag of :func:`score_range`) is 0, else
    the bare root leaf that treats nobody with value 0 (the training-row count is kept): a
    NaN fit never yields a tree that looks learned. Device ops only."""
    leaf = torch.cat([torch.full_like(rec[:6], -1), torch.zeros_like(rec[6:11]), rec[11:]])
    return torch.where(bad.to(rec.device) > 0, leaf, rec)


# ---------------------------------------------------------------- values
def eval_sums(psi: torch.Tensor, cost: torch.Tensor, use: torch.Tensor, codes: torch.Tensor,
              rec: torch.Tensor) -> torch.Tensor:
    """The evaluation sums of the learned policy, fp64 [2, 18]: for the training rows (use 0)
    and the held-out rows (use 1): n, S r, S r^2, S pi r, S pi r^2, S pi, and per leaf slot
    (n, S r, S r^2). Masked torch sums on the device, no atomics: deterministic."""
    r = psi.double() - cost.double()
    pi, leaf = apply_tree(rec, codes)
    zero = torch.zeros_like(r)
    out = []
    for u in (0, 1):
        on = use == u
        ru = torch.where(on, r, zero)
        r2 = ru * ru
        tr = on & (pi > 0)
        row = [on.sum().double(), ru.sum(), r2.sum(), torch.where(tr, ru, zero).sum(),
               torch.where(tr, r2, zero).sum(), tr.sum().double()]
        for l in range(4):
            inl = on & (leaf == l)
            row += [inl.sum().double(), torch.where(inl, ru, zero).sum(),
                    torch.where(inl, r2, zero).sum()]
        out.append(torch.stack(row))
    return torch.stack(out)


def policy_finalize(sums: torch.Tensor, bad: torch.Tensor) -> torch.Tensor:
    """fp64 [2, 20] from the (all-reduced) :func:`eval_sums`: per evaluation set value, SE,
    treat_all, SE, advantage, SE, share treated, n, and per leaf slot (n, mean r, SE). Every
    entry is NaN when ``bad`` (a non-finite score among the rows in use) is set. Device ops
    only."""
    rows = []
    for u in (0, 1):
        n, s1, s2, p1, p2, npi = (sums[u, k] for k in range(6))
        v, v_se = mean_se(p1, p2, n)
        t, t_se = mean_se(s1, s2, n)
        a, a_se = mean_se(p1 - s1, s2 - p2, n)        # (pi - 1) r: squares (1 - pi) r^2
        row = [v, v_se, t, t_se, a, a_se, npi / n, n]
        for l in range(4):
            nl, l1, l2 = (sums[u, 6 + 3 * l + k] for k in range(3))
            row += [nl, *mean_se(l1, l2, nl)]
        rows.append(torch.stack(row))
    fin = torch.stack(rows)
    return torch.where(bad > 0, torch.full_like(fin, float("nan")), fin)


# ---------------------------------------------------------------- estimator
def policy_phases(pan, codes, use, nb, cost, folds: int, depth=2, min_leaf=1, lambda_rule="min",
                  clip=0.01, comm=None, seg_counts=None, n_rows=None, propensity="linear"):
    """The policy-tree step as phases for utils.graphs.SegmentedStep: those of ``irm_phases``
    up to the fitted coefficients, then

    B'   per-row AIPW scores psi (csrc/irm.hip ate_irm_scores)              device
    S    max |psi - cost| and the non-finite flag                            device
    C06  all-reduce (max) of those two numbers                               collective (world > 1)
    H    scale exponent, feature-pair histograms (csrc/policy.hip)           device
    C06  all-reduce of the histograms                                        collective (world > 1)
    T    exact tree search on the histograms (csrc/policy.hip); the record
         becomes the bare root leaf if a score in use is not finite          device
    E    evaluation sums of the learned policy (masked fp64 torch sums)      device
    C06  all-reduce of the evaluation sums                                   collective (world > 1)
    C    values, SEs and the leaf table                                      device

    The result state holds "fin" [2, 20] (:func:`policy_finalize`), "rec" (the tree record),
    "e", "hist", "psi", "coef" and "cv"."""
    check_tree_args(depth, 2, min_leaf)
    phases, reduce = irm_fit_phases(pan, folds, lambda_rule, comm, seg_counts,
                                    propensity=propensity)
    n_rows = int(n_rows) if n_rows is not None else pan.ld
    cost_t = _dev_scalar(cost, torch.float64, pan.device)

    def phase_range(st):
        return {**st, "range": score_range(st["psi"], cost_t, use)}

    def phase_hist(st):
        e = scale_exponent(st["range"], n_rows)
        return {**st, "e": e, "hist": pair_hist(st["psi"], cost_t, e, use, codes, nb)}

    def phase_search(st):
        rec = tree_search(st["hist"], nb, depth, min_leaf)
        return {**st, "rec": mask_record(rec, st["range"][1])}

    def phase_eval(st):
        return {**st, "sums": eval_sums(st["psi"], cost_t, use, codes, st["rec"])}

    def phase_final(st):
        return {**st, "fin": policy_finalize(st["sums"], st["range"][1])}

    def reduce_max(name):
        def f(st):
            comm.all_reduce_max_(st[name])
            return st
        return Collective(f, capturable=bool(getattr(comm, "capturable", False)))

    phases += [phase_scores(pan, clip, propensity_link(propensity)), phase_range]
    if reduce is not None:
        phases.append(reduce_max("range"))
    phases.append(phase_hist)
    if reduce is not None:
        phases.append(reduce("hist"))
    phases += [phase_search, phase_eval]
    if reduce is not None:
        phases.append(reduce("sums"))
    phases.append(phase_final)
    return phases


def irm_policy_panel(pan, codes: torch.Tensor, use: torch.Tensor, nb, cost=0.0, folds: int = 5,
                     depth=2, min_leaf=1, lambda_rule="min", clip=0.01, comm=None,
                     seg_counts=None, n_rows=None, propensity="linear"):
    """The policy tree on an arm-split fold panel (the layout of ``irm_crossfit_panel``) ->
    (fin [2, 20], rec int64 [16], e int32 [1], cv). When a score of a row in use is not finite
    every entry of fin is NaN and rec is the bare root leaf that treats nobody
    (:func:`mask_record`).

    codes: uint8 [d, ld] bin codes in panel row order (:func:`bin_codes`; row shards must
    share the edges). use: [ld], -1 on padding rows and rows to leave out, 0 on training rows,
    1 on held-out rows. nb: bins per feature [d] (host list or device tensor). cost: a number
    or a one-element device tensor. n_rows: the (global) row count behind the scale exponent
    (default: the panel's padded rows). Nothing here syncs with the host."""
    if codes.dim() != 2 or codes.shape[1] != pan.ld or use.numel() != pan.ld:
        raise ValueError(f"codes must be [d, {pan.ld}] and use [{pan.ld}], got "
                         f"{tuple(codes.shape)} and {tuple(use.shape)}")
    st = run_phases(policy_phases(pan, codes, use, nb, cost, folds, depth, min_leaf, lambda_rule,
                                  clip, comm, seg_counts, n_rows, propensity))
    return st["fin"], st["rec"], st["e"], st.get("cv")


def _policy_body(pan, codes, use, nb, cost, folds, lambda_rule, clip, depth, min_leaf, n_rows,
                 dist=None, counts=None, propensity="linear"):
    """The whole estimator as one device function (GraphCache captures it):
    (fin [2, 20] fp64, rec | e int64 [17])."""
    comm, seg_counts = comm_counts(dist, counts)
    fin, rec, e, _ = irm_policy_panel(pan, codes, use, nb, cost, folds, depth, min_leaf,
                                      lambda_rule, clip, comm=comm, n_rows=n_rows,
                                      seg_counts=seg_counts, propensity=propensity)
    return fin, torch.cat([rec, e.to(torch.int64)])


def dml_irm_policy_lasso(Y, W, X, features, depth=2, bins=32, min_leaf=1, cost=0.0, train=None,
                         folds=5, seed=1991, lambda_rule="min", clip=0.01,
                         method="DML-IRM policy tree (LASSO)", device=None, dtype="f64", dist=None,
                         graph=True, propensity="linear") -> PolicyTreeResult:
    """Whom to treat: the exact depth <= 2 policy tree on the AIPW scores of the cross-fitted
    interactive model (``irm.dml_irm_lasso``: same folds, same nuisances, same score), over
    the columns ``features`` of X (1..32 distinct indices) binned into at most ``bins`` (2..64)
    bins each. ``cost``: the per-row cost of treating, subtracted from every score.
    ``min_leaf``: training rows every side of a split must keep. Matches
    reference.estimators.dml_irm_policy_tree.

    train: an (n,) boolean mask; the tree is learned on its rows and also evaluated on the
    others (``held_out``). The in-sample values (``in_sample``) are always reported but are
    optimistic -- the tree was chosen to maximise them on those very rows -- so without a
    held-out set ``diagnostics["honest"]`` is False. (The nuisances are cross-fitted over all
    rows either way.) A non-finite score (e.g. a truncated CV path) yields NaN values and a
    bare root leaf that treats nobody, never a tree that looks learned.

    graph: as ``dml_irm_lasso``, one captured hipGraph on a GPU; the codes, the use codes, the
    bin counts and the cost are graph inputs, so a call with other features (as many) and
    another cost in the same panel layout replays it."""
    Xn = as_np(X)
    check_logit_scope(propensity, X, folds, dtype, dist)
    check_tree_args(depth, bins, min_leaf)
    feats = check_features(features, Xn.shape[1])
    if not np.isfinite(float(cost)):
        raise ValueError(f"cost must be finite, got {cost}")
    n = len(Xn)
    if train is None:
        usen = np.zeros(n, dtype=np.int8)
    else:
        tr = np.asarray(train)
        if tr.shape != (n,) or tr.dtype != np.bool_:
            raise ValueError(f"train must be a boolean mask with one entry per row ({n})")
        usen = np.where(tr, 0, 1).astype(np.int8)
    sharded = dist is not None and dist.world > 1
    # every rank needs the same edges: the feature columns of all shards, gathered
    Xf = np.ascontiguousarray(Xn[:, feats])
    Xf_all = dist.gather_rows(torch.as_tensor(Xf)).numpy() if sharded else Xf
    edges = [feature_edges(Xf_all[:, k], int(bins)) for k in range(len(feats))]
    nb = [len(ed) + 1 for ed in edges]
    def check_train(ntrain):
        if ntrain[0] < 1:
            raise ValueError("the train mask leaves no training rows")

    pan, counts, _, n_total, _ = arm_split_panel(
        Y, W, X, folds, seed, dtype, device, dist,
        extra_counts=[(usen == 0).sum()], check_extra=check_train)
    real = pan.row_index >= 0
    cn = np.stack([bin_codes(Xf[:, k], edges[k]) for k in range(len(feats))], axis=1)
    codes = torch.stack([pan.gather_rows(torch.from_numpy(np.ascontiguousarray(cn[:, k])))
                         for k in range(len(feats))])                       # [d, ld]
    use = torch.where(real, pan.gather_rows(torch.from_numpy(usen)),
                      torch.full((pan.ld,), -1, dtype=torch.int8, device=pan.device))
    nbt = torch.tensor(nb, dtype=torch.int32, device=pan.device)
    cost_t = torch.tensor([float(cost)], dtype=torch.float64, device=pan.device)
    out, g = run_body("dml_irm_policy", _policy_body, (pan, codes, use, nbt, cost_t), folds,
                      lambda_rule, float(clip), int(depth), int(min_leaf), int(n_total), dist,
                      tuple(counts.tolist()), *propensity_args(propensity), graph=graph,
                      dist=dist)
    fin = out[0].detach().double().cpu().numpy()
    rec = out[1].detach().cpu().numpy().astype(np.int64)
    extra = {} if propensity == "linear" else {"propensity": propensity}
    return PolicyTreeResult.make(method, rec[:REC], fin, feats, edges, float(cost), int(depth),
                                 held_out=train is not None, hipgraph=g, e=int(rec[REC]),
                                 min_leaf=int(min_leaf), bins=int(bins), **extra)
