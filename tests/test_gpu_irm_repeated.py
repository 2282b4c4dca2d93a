"""GPU tests of repeated cross-fitting for DML-IRM (estimators/irm.py): the multi-split score
kernel (csrc/irm.hip ``ate_irm_score_moments_multi``) against its float64 torch twin and,
bit for bit, against the single-split kernel on fp64, fp32 and bf16 panels (column-major and
64-row blocked), with more splits than one pass or its LDS serves; the estimator against the row-by-row
reference twin, against single-partition fits when the path problems need two launches, and
hipGraph capture and replay. Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators.lasso import micro_fold_map
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.reference import estimators as E

pytestmark = pytest.mark.gpu

K, S = 3, 3
# rows of segment 2m + a (micro-group m, arm a): padding, one-row segments, a block tail
COUNTS = (130, 7, 64, 1, 257, 70, 33, 12, 65, 8, 100, 3, 9, 40, 16, 2, 31, 129)
P_X = 300                           # two compaction trips of 256 threads
CLIP = 0.2
BLK = np.stack([s * K + micro_fold_map(K, s) for s in range(S)])       # [S, K*K]


def _case(exact: bool, p: int = P_X):
    """Host arrays of the kernel tests: 9 micro-groups arm-split into 18 segments of COUNTS
    rows and S * K = 9 coefficient blocks with different supports (~40 columns incl. 0, 255,
    256, p - 1; block 4 intercept-only). ``exact``: x on a 1/8 grid in [-4, 4] and coefficients
    on a 2^-6 grid, |c| <= 9/64, at most ~40 terms: every fp32 partial sum of the bf16 kernel
    sits on a 2^-9 grid below 2^7 and is exact."""
    rs = np.random.RandomState(23)
    seg = np.repeat(np.arange(2 * K * K), COUNTS)
    seg = seg[rs.permutation(len(seg))]
    n = len(seg)
    W = (seg & 1).astype(float)
    if exact:
        X = rs.randint(-32, 33, size=(n, p)) / 8.0
        Y = rs.randint(0, 2, n).astype(float)
    else:
        X = rs.randn(n, p)
        Y = rs.randn(n) + W
    support = np.unique(np.r_[0, 255, 256, p - 1, rs.choice(p, 36, replace=False)])
    coef = np.zeros((S * K, 3, p + 1))
    for k in range(S * K):
        if k == 4:
            continue
        for r in range(3):
            on = support[rs.rand(len(support)) < 0.6]
            if exact:
                coef[k, r, 1 + on] = rs.randint(-9, 10, len(on)) / 64.0
            else:
                coef[k, r, 1 + on] = rs.randn(len(on)) * (0.1 if r == 2 else 0.5)
        if k % 2 == 0:
            coef[k, :, 1 + np.array([0, 255, 256, p - 1])] = (np.array(
                [[3, -5, 2], [-4, 6, 1], [7, 2, -3], [-2, -7, 4]]) / 64.0)
    coef[:, 0, 0], coef[:, 1, 0], coef[:, 2, 0] = 0.25, 0.75, 0.5
    return X, W, Y, seg, coef


def _blk_many():
    """More splits than one pass serves: SMAX + 2 rows of blocks, the partitions first."""
    smax = DI.score_multi_smax()
    rs = np.random.RandomState(5)
    return np.concatenate([BLK, rs.randint(0, S * K, size=(smax + 2 - S, K * K))]), smax


def _assert_far_from_clip(X, seg, coef, blk):
    for b in blk:
        m = np.array([coef[b[s // 2], 2, 0] + coef[b[s // 2], 2, 1:] @ x for x, s in zip(X, seg)])
        assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6


def _check(got, want, n, nt):
    got, want = got.cpu().numpy(), want.numpy()
    assert got.shape == want.shape
    for t in range(len(got)):
        print("split", t, "moments gpu ", got[t].tolist())
        print("split", t, "moments twin", want[t].tolist())
        print("split", t, "rel err     ",
              (np.abs(got[t] - want[t]) / np.maximum(np.abs(want[t]), 1e-300)).tolist())
    np.testing.assert_allclose(got, want, rtol=1e-11)     # the bound of the single-split kernel
    for g, w in zip(got, want):
        assert g[2] == n == w[2] and g[7] == nt == w[7] and g[3] == w[3]
        assert 0 < g[3] < n                               # many rows clip, not all


def _bit_contract(pan, c, blk, got, nbx):
    """moments[t] of the multi-split pass: the bits of the single-split kernel with the
    coefficient blocks gathered by blk[t], at the same nbx."""
    for t in range(len(blk)):
        one = DI.irm_score_moments(pan, c.index_select(0, torch.from_numpy(blk[t]).to(c.device)),
                                   CLIP, 2, nbx=nbx)
        torch.cuda.synchronize()
        assert torch.equal(got[t], one), (t, got[t].tolist(), one.tolist())


@pytest.mark.parametrize("many", [False, True])
def test_multi_kernel_f64(gpu, many):
    X, W, Y, seg, coef = _case(exact=False)
    blk = _blk_many()[0] if many else BLK
    assert not many or len(blk) > DI.score_multi_smax()
    _assert_far_from_clip(X, seg, coef, blk)
    assert np.count_nonzero(np.any(coef[:, :, 1:] != 0, axis=(0, 1))) >= 36
    assert not coef[4, :, 1:].any() and len({tuple(np.flatnonzero(c.any(0))) for c in coef}) == 9
    pc = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    pg = build_panel(X, W, Y, folds=seg, dtype="f64", device=gpu)
    assert tuple(pg.seg_nreal) == COUNTS and pg.nseg == 2 * K * K and pg.ld > len(Y)
    c = torch.from_numpy(coef)
    want = DI.irm_score_moments_multi(pc, c, blk, CLIP, 2)
    for nbx in (None, 1):
        got = DI.irm_score_moments_multi(pg, c.to(gpu), blk, CLIP, 2, nbx=nbx)
        torch.cuda.synchronize()
        _check(got, want, len(Y), int(W.sum()))
        _bit_contract(pg, c.to(gpu), blk, got, nbx)


@pytest.mark.parametrize("many", [False, True])
def test_multi_kernel_bf16_layouts(gpu, many):
    X, W, Y, seg, coef = _case(exact=True)
    blk = _blk_many()[0] if many else BLK
    _assert_far_from_clip(X, seg, coef, blk)
    pc = build_panel(X, W, Y, folds=seg, dtype="bf16", device="cpu")
    # the stored values are the inputs: the grid is exact in bf16
    assert torch.equal(pc.data[pc.xcols].double()[:, pc.valid() != 0],
                       torch.from_numpy(X[pc.row_index[pc.valid() != 0].numpy()].T))
    cm = build_panel(X, W, Y, folds=seg, dtype="bf16", device=gpu)
    bl = dataclasses.replace(
        cm, data=cm.data.reshape(cm.P, cm.ld // 64, 64).permute(1, 0, 2).contiguous(), blocked=True)
    assert bl.strides() == (64, 64 * cm.P) and torch.equal(bl.colmajor(), cm.data)
    c = torch.from_numpy(coef)
    want = DI.irm_score_moments_multi(pc, c, blk, CLIP, 2)
    out = []
    for pan in (cm, bl):
        got = DI.irm_score_moments_multi(pan, c.to(gpu), blk, CLIP, 2)
        torch.cuda.synchronize()
        _check(got, want, len(Y), int(W.sum()))
        _bit_contract(pan, c.to(gpu), blk, got, None)
        out.append(got.cpu())
    assert torch.equal(out[0], out[1])                    # the two layouts: the same bits


def test_multi_kernel_f32(gpu):
    """The fp32 column-major instantiation (fp64 dot products of the stored fp32 values)."""
    X, W, Y, seg, coef = _case(exact=False)
    X, Y = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    blk = _blk_many()[0]
    _assert_far_from_clip(X, seg, coef, blk)
    pc = build_panel(X, W, Y, folds=seg, dtype="f32", device="cpu")
    pg = build_panel(X, W, Y, folds=seg, dtype="f32", device=gpu)
    assert pg.data.dtype == torch.float32 and tuple(pg.seg_nreal) == COUNTS
    c = torch.from_numpy(coef)
    want = DI.irm_score_moments_multi(pc, c, blk, CLIP, 2)
    got = DI.irm_score_moments_multi(pg, c.to(gpu), blk, CLIP, 2)
    torch.cuda.synchronize()
    _check(got, want, len(Y), int(W.sum()))
    _bit_contract(pg, c.to(gpu), blk, got, None)


def test_multi_kernel_wide_p_splits_for_lds(gpu):
    """fp64, p = 640, S = 4: the 12 staged coefficient vectors need 12 * 641 * 8 + 4 * 640
    bytes, past the 62 KB the pass may use, so the launcher takes 3 + 1 splits per pass."""
    p, smax = 640, DI.score_multi_smax()
    assert 3 * smax * (p + 1) * 8 + 4 * p > 64 * 1024 - 2048 >= 3 * (smax - 1) * (p + 1) * 8 + 4 * p
    X, W, Y, seg, coef = _case(exact=False, p=p)
    blk = _blk_many()[0][:smax]
    _assert_far_from_clip(X, seg, coef, blk)
    assert coef[:, :, 1 + p - 1].any() and coef[:, :, 1].any()
    pc = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    pg = build_panel(X, W, Y, folds=seg, dtype="f64", device=gpu)
    c = torch.from_numpy(coef)
    want = DI.irm_score_moments_multi(pc, c, blk, CLIP, 2)
    got = DI.irm_score_moments_multi(pg, c.to(gpu), blk, CLIP, 2)
    torch.cuda.synchronize()
    _check(got, want, len(Y), int(W.sum()))
    _bit_contract(pg, c.to(gpu), blk, got, None)


def test_multi_kernel_rejects_bad_blocks(gpu):
    X, W, Y, seg, coef = _case(exact=False)
    pg = build_panel(X, W, Y, folds=seg, dtype="f64", device=gpu)
    c = torch.from_numpy(coef).to(gpu)
    with pytest.raises(ValueError, match="blk entries"):       # checked before any launch
        DI.irm_score_moments_multi(pg, c, BLK + 1, CLIP, 2)
    with pytest.raises(ValueError, match="blk entries"):
        DI.irm_score_moments_multi(pg, c, BLK - 1, CLIP, 2)


@pytest.fixture(scope="module")
def reference3(tutorial):
    _, m, _ = tutorial
    return E.dml_irm_lasso_repeated(m.Y, m.W, m.X, 5, 3)


def test_estimator_vs_reference(gpu, tutorial, reference3):
    _, m, _ = tutorial
    a = DI.dml_irm_lasso_repeated(m.Y, m.W, m.X, 5, 3, device=gpu, graph=False)
    torch.cuda.synchronize()
    b = reference3
    print("gpu", a.ate, a.se, a.diagnostics, "reference", b.ate, b.se, b.diagnostics)
    # the bound of the single-partition twin (tests/test_gpu_irm.py)
    assert a.ate == pytest.approx(b.ate, abs=1e-6, rel=1e-6)
    assert a.se == pytest.approx(b.se, abs=1e-6, rel=1e-6)
    for sa, sb in zip(a.diagnostics["splits"], b.diagnostics["splits"]):
        assert sa == pytest.approx(sb, abs=1e-6, rel=1e-6)
    assert a.diagnostics["n_clipped"] == b.diagnostics["n_clipped"]
    assert a.diagnostics["n_treated"] == b.diagnostics["n_treated"]


def test_two_path_launches_equal_single_partition_fits(gpu, tutorial):
    """K = 5, S = 4: 4 * 75 path problems need two launches; every split is the
    single-partition fit on that partition's fold ids."""
    from ate_replication_causalml_amd.ops.enet import MAX_PATH_PROBLEMS
    _, m, _ = tutorial
    assert 3 * 75 <= MAX_PATH_PROBLEMS < 4 * 75
    r = DI.dml_irm_lasso_repeated(m.Y, m.W, m.X, 5, 4, device=gpu, graph=False)
    torch.cuda.synchronize()
    micro = rng.fold_ids(len(m.Y), 25, 1991, 0)
    a, b = np.divmod(micro, 5)
    Wn = np.asarray(m.W, dtype=np.float64)
    for s, (th, se) in enumerate(r.diagnostics["splits"]):
        fid = (a + s * b) % 5
        pan = build_panel(np.asarray(m.X), Wn, np.asarray(m.Y), folds=2 * fid + Wn.astype(np.int64),
                          dtype="f64", device=gpu)
        res, mom, _ = DI.irm_crossfit_panel(pan, 5)
        torch.cuda.synchronize()
        res = res.cpu().numpy()
        print("split", s, "repeated", th, se, "single", res.tolist())
        assert th == pytest.approx(res[0], abs=1e-6, rel=1e-6)
        assert se == pytest.approx(res[1], abs=1e-6, rel=1e-6)
        assert r.diagnostics["n_clipped"][s] == int(round(mom[3].item()))
    assert len({round(th, 12) for th, _ in r.diagnostics["splits"]}) == 4


def test_graph_capture_and_replay(gpu, tutorial):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    _, m, _ = tutorial
    rs = np.random.RandomState(4)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DI.dml_irm_lasso_repeated(m.Y, m.W, m.X, 5, 3, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    for r in runs[1:]:
        assert (r.ate, r.se, r.diagnostics["splits"], r.diagnostics["n_clipped"]) == \
            (runs[0].ate, runs[0].se, runs[0].diagnostics["splits"], runs[0].diagnostics["n_clipped"])
    # other data in the same layout (same micro-groups and arms): a replay equals an eager run
    Y2 = np.where(rs.rand(len(m.Y)) < 0.2, 1.0 - m.Y, m.Y)
    r4 = DI.dml_irm_lasso_repeated(Y2, m.W, m.X, 5, 3, device=gpu)
    torch.cuda.synchronize()
    e4 = DI.dml_irm_lasso_repeated(Y2, m.W, m.X, 5, 3, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert (r4.ate, r4.se, r4.diagnostics["splits"]) == (e4.ate, e4.se, e4.diagnostics["splits"])
    assert r4.ate != runs[0].ate
    estimator_graphs.clear()
