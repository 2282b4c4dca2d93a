"""GPU tests of DML-IRM (estimators/irm.py): the fused AIPW score kernel (csrc/irm.hip)
against its float64 torch twin on fp64 and bf16 panels (column-major and 64-row blocked),
the estimator against the row-by-row reference twin, hipGraph capture and replay, and bf16
against f64 panel storage. Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.reference import estimators as E

pytestmark = pytest.mark.gpu

COUNTS = (130, 7, 64, 1, 257, 70)   # rows of segment 2k + a: padding, a one-row segment, a
P_X = 300                           # block tail; p = 300: two compaction trips of 256 threads
CLIP = 0.2


def _case(exact: bool):
    """Host arrays of the kernel tests: 3 folds arm-split into 6 segments of COUNTS rows,
    ~40 nonzero coefficients incl. columns 0, 255, 256, 299, fold 1 intercept-only.
    ``exact``: x on a 1/8 grid in [-4, 4] and coefficients on a 2^-6 grid in [-1, 1], so
    every fp32 partial sum of the bf16 kernel sits on a 2^-9 grid below 2^7 and is exact."""
    rs = np.random.RandomState(17)
    seg = np.repeat(np.arange(6), COUNTS)
    perm = rs.permutation(len(seg))
    seg = seg[perm]
    n = len(seg)
    W = (seg & 1).astype(float)
    if exact:
        X = rs.randint(-32, 33, size=(n, P_X)) / 8.0
        Y = rs.randint(0, 2, n).astype(float)
    else:
        X = rs.randn(n, P_X)
        Y = rs.randn(n) + W
    support = np.unique(np.r_[0, 255, 256, 299, rs.choice(P_X, 36, replace=False)])
    coef = np.zeros((3, 3, P_X + 1))
    for k in (0, 2):
        for r in range(3):
            on = support[rs.rand(len(support)) < 0.6]
            if exact:
                # |sum| <= 0.5 + 14 * 4 * (9/64) < 2^7 with at most ~30 terms of |c| <= 9/64
                coef[k, r, 1 + on] = rs.randint(-9, 10, len(on)) / 64.0
            else:
                coef[k, r, 1 + on] = rs.randn(len(on)) * (0.1 if r == 2 else 0.5)
        coef[k, :, 1 + np.array([0, 255, 256, 299])] = (np.array([[3, -5, 2], [-4, 6, 1],
                                                                  [7, 2, -3], [-2, -7, 4]]) / 64.0)
    coef[:, 0, 0], coef[:, 1, 0], coef[:, 2, 0] = 0.25, 0.75, 0.5
    return X, W, Y, seg, coef


def _raw_m(X, seg, coef):
    return np.array([coef[s // 2, 2, 0] + coef[s // 2, 2, 1:] @ x for x, s in zip(X, seg)])


def _check(got, want, n, nt):
    got, want = got.cpu().numpy(), want.numpy()
    print("moments gpu ", got.tolist())
    print("moments twin", want.tolist())
    print("rel err     ", (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).tolist())
    np.testing.assert_allclose(got, want, rtol=1e-11)     # the bound of the PLR residual kernel
    assert got[2] == n == want[2] and got[7] == nt == want[7] and got[3] == want[3]
    assert 0 < got[3] < n                                 # many rows clip, not all


def test_score_kernel_f64_vs_twin(gpu):
    X, W, Y, seg, coef = _case(exact=False)
    m = _raw_m(X, seg, coef)
    assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6
    assert np.count_nonzero(np.any(coef[:, :, 1:] != 0, axis=(0, 1))) >= 36
    pc = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    pg = build_panel(X, W, Y, folds=seg, dtype="f64", device=gpu)
    assert tuple(pg.seg_nreal) == COUNTS and pg.ld > len(Y)
    c = torch.from_numpy(coef)
    want = DI.irm_score_moments(pc, c, CLIP, 2)
    for nbx in (None, 1):
        got = DI.irm_score_moments(pg, c.to(gpu), CLIP, 2, nbx=nbx)
        torch.cuda.synchronize()
        _check(got, want, len(Y), int(W.sum()))
    # a plain K-fold reading of the same panel: one coefficient block per segment
    c6 = torch.from_numpy(np.repeat(coef, 2, axis=0))
    got = DI.irm_score_moments(pg, c6.to(gpu), CLIP, 1)
    torch.cuda.synchronize()
    _check(got, DI.irm_score_moments(pc, c6, CLIP, 1), len(Y), int(W.sum()))


def test_score_kernel_bf16_layouts_vs_twin(gpu):
    X, W, Y, seg, coef = _case(exact=True)
    m = _raw_m(X, seg, coef)
    assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6
    pc = build_panel(X, W, Y, folds=seg, dtype="bf16", device="cpu")
    # the stored values are the inputs: the grid is exact in bf16
    assert torch.equal(pc.data[pc.xcols].double()[:, pc.valid() != 0],
                       torch.from_numpy(X[pc.row_index[pc.valid() != 0].numpy()].T))
    cm = build_panel(X, W, Y, folds=seg, dtype="bf16", device=gpu)
    bl = dataclasses.replace(
        cm, data=cm.data.reshape(cm.P, cm.ld // 64, 64).permute(1, 0, 2).contiguous(), blocked=True)
    assert bl.strides() == (64, 64 * cm.P) and torch.equal(bl.colmajor(), cm.data)
    c = torch.from_numpy(coef)
    want = DI.irm_score_moments(pc, c, CLIP, 2)
    out = []
    for pan in (cm, bl):
        got = DI.irm_score_moments(pan, c.to(gpu), CLIP, 2)
        torch.cuda.synchronize()
        _check(got, want, len(Y), int(W.sum()))
        out.append(got.cpu())
    assert torch.equal(out[0], out[1])                    # the two layouts: the same bits


def test_estimator_vs_reference(gpu, tutorial):
    _, m, _ = tutorial
    a = DI.dml_irm_lasso(m.Y, m.W, m.X, device=gpu)
    torch.cuda.synchronize()
    b = E.dml_irm_lasso(m.Y, m.W, m.X)
    print("gpu", a.ate, a.se, a.diagnostics, "reference", b.ate, b.se, b.diagnostics)
    # the bound of the PLR twin (tests/test_gpu.py)
    assert a.ate == pytest.approx(b.ate, abs=1e-6, rel=1e-6)
    assert a.se == pytest.approx(b.se, abs=1e-6, rel=1e-6)
    assert a.diagnostics["n_clipped"] == b.diagnostics["n_clipped"]
    assert a.diagnostics["n_treated"] == b.diagnostics["n_treated"]


def test_graph_capture_and_replay(gpu, tutorial):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    _, m, _ = tutorial
    rs = np.random.RandomState(4)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DI.dml_irm_lasso(m.Y, m.W, m.X, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    for r in runs[1:]:
        assert (r.ate, r.se, r.diagnostics["n_clipped"]) == \
            (runs[0].ate, runs[0].se, runs[0].diagnostics["n_clipped"])
    # other data in the same layout (same folds and arms): a replay equals a fresh eager run
    Y2 = np.where(rs.rand(len(m.Y)) < 0.2, 1.0 - m.Y, m.Y)
    r4 = DI.dml_irm_lasso(Y2, m.W, m.X, device=gpu)
    torch.cuda.synchronize()
    e4 = DI.dml_irm_lasso(Y2, m.W, m.X, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert (r4.ate, r4.se) == (e4.ate, e4.se) and r4.ate != runs[0].ate
    estimator_graphs.clear()


@pytest.mark.parametrize("dgp", ["rct", "tutorial"])
def test_irm_bf16_vs_f64_panel(gpu, dgp):
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    pb = synthetic_panel(200000, p=60, folds=5, seed=2, dtype="bf16", device=gpu, dgp=dgp,
                         arm_split=True)
    p64 = synthetic_panel(200000, p=60, folds=5, seed=2, dtype="f64", device=gpu, dgp=dgp,
                          arm_split=True, selection=pb.selection)
    assert pb.nseg == 10 and np.array_equal(pb.seg_nreal, p64.seg_nreal)
    rb, mb, _ = DI.irm_crossfit_panel(pb, 5)
    r64, m64, _ = DI.irm_crossfit_panel(p64, 5)
    torch.cuda.synchronize()
    rb, r64 = rb.cpu().numpy(), r64.cpu().numpy()
    print(dgp, "bf16", rb.tolist(), "f64", r64.tolist(), "dATE/SE", abs(rb[0] - r64[0]) / r64[1],
          "dSE/SE", abs(rb[1] - r64[1]) / r64[1], "mom", mb.cpu().tolist(), m64.cpu().tolist())
    # the bounds of the PLR storage test (tests/test_gpu.py test_dml_bf16_vs_f64_panel)
    assert abs(rb[0] - r64[0]) < 0.05 * r64[1]
    assert abs(rb[1] - r64[1]) < 0.02 * r64[1]
    assert mb[2].item() == 200000 == m64[2].item() and mb[7].item() == m64[7].item()
