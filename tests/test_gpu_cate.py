"""GPU tests of the CATE-curve estimator (estimators/cate.py): the two passes of
csrc/cate.hip against a numpy twin at every launch shape they have (the basis of the twin
comes from the recursive Cox-de Boor definition, the kernels' from the span-local
recurrence), degree 0 against the group kernel, the estimator against the row-by-row
reference twin, and hipGraph capture and replay with the covariate, the knots and the grid
as graph inputs. Run on the MI355X box: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.estimators import cate as DC
from ate_replication_causalml_amd.estimators import gate as DG
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.reference import estimators as E

pytestmark = pytest.mark.gpu

COUNTS = (130, 7, 64, 1, 257, 70)   # the layout of tests/test_gpu_gate.py: 529 rows in 832
P_X = 300
CLIP = 0.2
RID0 = 2 ** 33                      # global row ids beyond 32 bits


def _layout():
    """Host arrays of the kernel tests (the case of tests/test_gpu_gate.py): the panel's
    scores psi [832] from ``irm_scores``, its row index and the bounds of segment 2."""
    rs = np.random.RandomState(17)
    seg = np.repeat(np.arange(6), COUNTS)
    seg = seg[rs.permutation(len(seg))]
    n = len(seg)
    W = (seg & 1).astype(float)
    X = rs.randn(n, P_X)
    Y = rs.randn(n) + W
    support = np.unique(np.r_[0, 255, 256, 299, rs.choice(P_X, 36, replace=False)])
    coef = np.zeros((3, 3, P_X + 1))
    for k in (0, 2):
        for r in range(3):
            on = support[rs.rand(len(support)) < 0.6]
            coef[k, r, 1 + on] = rs.randn(len(on)) * (0.1 if r == 2 else 0.5)
    coef[:, 0, 0], coef[:, 1, 0], coef[:, 2, 0] = 0.25, 0.75, 0.5
    pc = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    assert tuple(pc.seg_nreal) == COUNTS and pc.ld == 832
    psi = DI.irm_scores(pc, torch.from_numpy(coef), CLIP, 2).numpy()
    return psi, pc.row_index.numpy(), tuple(int(v) for v in pc.seg_bounds[2])


def _twin(psi, Bm, span, rid, nsp, beta, B, seed):
    """numpy twin of csrc/cate.hip from a dense basis matrix of the kept rows: the outputs
    of both passes and the sums of absolute terms that scale the bounds."""
    keep = rid >= 0
    p, r = psi[keep], rid[keep]
    d = Bm.shape[1]
    e = p - Bm @ beta
    EB = Bm * e[:, None]
    T = np.zeros((B, d))
    for i0 in range(0, len(p), 4096):
        sl = slice(i0, i0 + 4096)
        T += rng.rademacher(seed, r[sl], B).T.astype(np.float64) @ EB[sl]
    return dict(n=float(len(p)), s1=p.sum(), s2=(p * p).sum(),
                cnt=np.bincount(span, minlength=nsp).astype(np.float64), v=Bm.T @ p,
                M=Bm.T @ Bm, meat=EB.T @ EB, T=T, vabs=Bm.T @ np.abs(p),
                tabs=np.abs(EB).sum(axis=0))


def _check(gpu, psi, x, rid, knots, q, beta, B, seed, tw, nbx=None):
    d = len(knots) - q - 1
    args = (torch.from_numpy(psi).to(gpu), torch.from_numpy(x).to(gpu),
            torch.from_numpy(rid.astype(np.int64)).to(gpu), torch.from_numpy(knots).to(gpu), q)
    bt = torch.from_numpy(beta).to(gpu)
    m1, m2 = (DC.cate_moments(*args, nbx=nbx) for _ in range(2))
    b1, b2 = (DC.cate_boot(*args, bt, B, seed, nbx=nbx) for _ in range(2))
    torch.cuda.synchronize()
    m1, m2, b1, b2 = m1.cpu(), m2.cpu(), b1.cpu(), b2.cpu()
    assert torch.equal(m1, m2) and torch.equal(b1, b2)        # one geometry, one set of bits
    head, cnt, v, M = (t.numpy() for t in DC.split_moments(m1, d, q))
    meat, T = (t.numpy() for t in DC.split_boot(b1, d, B))
    assert head[0] == tw["n"] and np.array_equal(cnt, tw["cnt"])      # exact
    assert head[1] == pytest.approx(tw["s1"], rel=1e-11, abs=1e-11 * tw["vabs"].sum())
    assert head[2] == pytest.approx(tw["s2"], rel=1e-11)
    assert np.array_equal(M, M.T) and np.array_equal(meat, meat.T)
    off = np.abs(np.subtract.outer(np.arange(d), np.arange(d))) > q
    assert np.all(M[off] == 0) and np.all(meat[off] == 0)
    ev = np.abs(v - tw["v"]) / tw["vabs"].clip(min=1e-300)
    et = np.abs(T - tw["T"]) / tw["tabs"].clip(min=1e-300)[None, :]
    print("degree", q, "d", d, "B", B, "nbx", nbx, "max |v - v_ref| / S b|psi|", ev.max(),
          "max |T - T_ref| / S|e b|", et.max(), "max rel M", _rel(M, tw["M"]), "meat",
          _rel(meat, tw["meat"]), "geometry", DC.boot_geometry(B, d, len(psi)))
    np.testing.assert_allclose(M, tw["M"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(meat, tw["meat"], rtol=1e-11, atol=0)
    assert np.all(np.abs(v - tw["v"]) <= 1e-11 * tw["vabs"])
    assert np.all(np.abs(T - tw["T"]) <= 1e-11 * tw["tabs"][None, :])
    assert np.abs(T).max() > 0
    return m1, b1


def _rel(a, b):
    nz = b != 0
    return float((np.abs(a - b)[nz] / np.abs(b)[nz]).max()) if nz.any() else 0.0


def _small_case(q, d):
    """x, rid and knots on the 832-row layout: irregular knots, span 0 with exactly 2 rows
    (far apart), span 1 with all its rows inside segment 2 (most chunks see an empty run),
    rows exactly on interior knots (they belong to the right-hand span), one row at max x
    (the last span is closed) and 30 real rows left out."""
    psi, rix, (r0, r1) = _layout()
    real = np.flatnonzero(rix >= 0)
    rs = np.random.RandomState(5)
    nsp = d - q
    t = np.concatenate([[0.0], np.cumsum(0.3 + rs.rand(nsp))]) - 1.7      # span boundaries
    span = np.full(len(rix), -1)
    if nsp >= 3:
        span[real] = rs.randint(2, nsp, len(real))
        span[r0 + 3:r0 + 40] = 1                                  # span 1: inside segment 2 only
    else:
        span[real] = rs.randint(0, nsp, len(real))
    out = real[rs.choice(len(real), 30, replace=False)]
    span[out] = -1                                                # real rows left out
    if nsp >= 3:
        span[[real[0], real[-1]]] = 0                             # span 0: exactly 2 rows
    kept = np.flatnonzero(span >= 0)
    u = rs.rand(len(rix)) * 0.999
    u[kept[::7]] = 0.0                                            # exactly on the span's left knot
    x = np.zeros(len(rix))
    x[kept] = t[span[kept]] + u[kept] * (t[span[kept] + 1] - t[span[kept]])
    last = kept[span[kept] == nsp - 1][0]
    x[last] = t[-1]                                               # max x: the last span, closed
    x[span < 0] = 1e9                                             # never read
    rid = np.where(span >= 0, rix + RID0, -1)
    knots = np.concatenate([[t[0]] * q, t, [t[-1]] * q])
    cnt = np.bincount(span[kept], minlength=nsp)
    if nsp >= 3:
        assert cnt[0] == 2 and cnt[1] >= 30 and (span[real] < 0).sum() >= 28
        inside = np.flatnonzero(span == 1)
        assert inside.min() >= r0 and inside.max() < r1
    assert np.all(rix[kept] >= 0) and x[kept].max() == t[-1] and x[kept].min() >= t[0]
    assert nsp < 2 or np.isin(x[kept], t[1:-1]).sum() >= 5
    # the spans the kernel must find: x on a knot -> right-hand span, max x -> the last
    assert np.array_equal(np.minimum(np.searchsorted(t[1:-1], x[kept], side="right"), nsp - 1),
                          span[kept])
    return psi, x, rid, knots, span[kept]


# (degree, d, B): one span without an interior knot; the register / slab threshold (8 | 9
# basis functions), 9 streams: 256 threads and a second stream block with one stream in use;
# the indicator basis at one replicate; degrees 1 and 2; 30 spans in 64-thread workgroups
@pytest.mark.parametrize("q,d,B", [(3, 4, 200), (3, 8, 1100), (3, 9, 130), (0, 5, 1), (1, 6, 64),
                                   (2, 32, 130)])
def test_cate_kernels_small_layout(gpu, q, d, B):
    psi, x, rid, knots, span = _small_case(q, d)
    keep = rid >= 0
    Bm = E.bspline_design(x[keep], knots, q)                  # the recursive definition
    assert np.allclose(Bm.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.all((Bm != 0).sum(axis=1) <= q + 1)
    beta = np.random.RandomState(2).randn(d)
    tw = _twin(psi, Bm, span, rid, d - q, beta, B, 1991)      # computed once, shared
    for nbx in (None, 1, 3):
        _check(gpu, psi, x, rid, knots, q, beta, B, 1991, tw, nbx=nbx)


def test_cate_kernels_many_chunks(gpu):
    n, d, q, B = 70_000, 32, 3, 384                           # 547 chunks of 128 rows
    rs = np.random.RandomState(9)
    psi = rs.standard_t(5, n) * 3 + 0.1
    x = rs.randn(n)
    rid = rs.permutation(n).astype(np.int64) + RID0
    rid[rs.rand(n) < 0.01] = -1
    knots = DC.quantile_knots(x[rid >= 0], d, q)              # order statistics: rows on knots
    ch, nby, nbx = DC.boot_geometry(B, d, n)
    assert -(-n // ch) >= 3 * nbx and nbx > 1                 # several chunks per workgroup
    keep = rid >= 0
    sp, _ = DC.basis_local(torch.from_numpy(x[keep]), torch.from_numpy(knots), q)
    Bm = DC.bspline_basis(x[keep], knots, q).numpy()          # (tests/test_cate.py: the twins agree)
    beta = np.linalg.solve(Bm.T @ Bm, Bm.T @ psi[keep])
    tw = _twin(psi, Bm, sp.numpy(), rid, d - q, beta, B, 7)   # computed once, shared
    m1, _ = _check(gpu, psi, x, rid, knots, q, beta, B, 7, tw)
    # another geometry: the same sums to the bound, and the span counts to the bit
    m2, _ = _check(gpu, psi, x, rid, knots, q, beta, B, 7, tw, nbx=37)
    assert torch.equal(m1[3:3 + d - q], m2[3:3 + d - q])
    assert m1[0] == m2[0]


def test_degree0_is_the_group_kernel(gpu):
    psi, x, rid, knots, span = _small_case(0, 5)
    G, B, seed = 5, 200, 1991
    gid = np.full(len(psi), -1, dtype=np.int32)
    gid[rid >= 0] = span
    dev = lambda a: torch.from_numpy(a).to(gpu)
    gb = DG.group_boot(dev(psi), dev(gid), dev(rid.astype(np.int64)), G, B, seed)
    mom, A, Z = (t.cpu().numpy() for t in DG.split_boot(gb, G, B))
    theta = mom[:, 1] / mom[:, 0]
    mo = DC.cate_moments(dev(psi), dev(x), dev(rid.astype(np.int64)), dev(knots), 0)
    bo = DC.cate_boot(dev(psi), dev(x), dev(rid.astype(np.int64)), dev(knots), 0, dev(theta), B,
                      seed)
    torch.cuda.synchronize()
    head, cnt, v, M = (t.cpu().numpy() for t in DC.split_moments(mo, G, 0))
    meat, T = (t.cpu().numpy() for t in DC.split_boot(bo, G, B))
    assert np.array_equal(cnt, mom[:, 0]) and np.array_equal(np.diag(M), cnt)
    np.testing.assert_allclose(v, mom[:, 1], rtol=1e-11)
    tabs = np.bincount(span, weights=np.abs(psi[rid >= 0] - theta[span]), minlength=G)
    err = np.abs(T - (A - theta * Z)) / tabs[None, :]
    print("degree 0: max |T - (A - theta Z)| / S|e b|", err.max())
    assert np.all(np.abs(T - (A - theta * Z)) <= 1e-11 * tabs[None, :])
    # HC0 of an indicator basis: the diagonal meat is the groups' centred sums of squares
    css = mom[:, 2] - mom[:, 1] ** 2 / mom[:, 0]
    np.testing.assert_allclose(np.diag(meat), css, rtol=1e-9)


# ---------------------------------------------------------------- estimator
def test_estimator_vs_reference(gpu, tutorial):
    _, m, _ = tutorial
    x = m.X[:, 0]
    a = DC.dml_irm_cate_lasso(m.Y, m.W, m.X, x, df=8, degree=3, n_boot=999, device=gpu,
                              graph=False)
    torch.cuda.synchronize()
    b = E.dml_irm_cate(m.Y, m.W, m.X, x, df=8, degree=3, n_boot=999, keep_boot=True)
    # Lambda: what the projection makes of a per-row score error of size 1
    Bm = E.bspline_design(x, b.knots, 3)
    G = E.bspline_design(b.grid, b.knots, 3)
    lam = np.abs(G @ np.linalg.solve(b.boot["M"], Bm.T)).sum(axis=1).max()
    ca, cb, sa, sb = (np.asarray(v) for v in (a.cate, b.cate, a.se, b.se))
    ec = (np.abs(ca - cb) / (1e-6 + 1e-6 * np.abs(cb))).max()
    es = (np.abs(sa - sb) / (1e-6 + 1e-6 * np.abs(sb))).max()
    print("Lambda", lam, "max |cate - ref| / (1e-6 (1 + |ref|))", ec, "se", es, "crit",
          a.crit, b.crit, "overall", a.overall.ate, b.overall.ate)
    assert a.grid == b.grid and a.knots == b.knots and len(a.grid) == 100
    assert a.diagnostics["span_counts"] == b.diagnostics["span_counts"]
    assert ec <= lam and es <= lam
    assert abs(a.crit - b.crit) < 1e-4
    assert a.overall.ate == pytest.approx(b.overall.ate, abs=1e-6, rel=1e-6)


def test_graph_capture_and_replay(gpu, tutorial):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    _, m, _ = tutorial
    key = lambda r: (r.cate, r.se, r.crit, r.coef, r.cov, r.overall.ate, r.overall.se)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DC.dml_irm_cate_lasso(m.Y, m.W, m.X, 0, df=8, degree=3, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    assert key(runs[1]) == key(runs[0]) and key(runs[2]) == key(runs[0])
    # another column in the same layout: a replay equals a fresh eager run
    r4 = DC.dml_irm_cate_lasso(m.Y, m.W, m.X, 1, df=8, degree=3, device=gpu)
    torch.cuda.synchronize()
    e4 = DC.dml_irm_cate_lasso(m.Y, m.W, m.X, 1, df=8, degree=3, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert key(r4) == key(e4) and r4.cate != runs[0].cate and r4.knots != runs[0].knots
    # the same rows along another covariate: the overall ATE is the same sum in another order
    assert r4.overall.ate == pytest.approx(runs[0].overall.ate, rel=1e-12)
    assert r4.overall.se == pytest.approx(runs[0].overall.se, rel=1e-12)
    estimator_graphs.clear()
