"""GPU tests of the DML-IRM sensitivity analysis (estimators/sensitivity.py): the 14-moment
instantiation of the fused score kernel (csrc/irm.hip ate_irm_sens_moments) against its
float64 torch twin on fp64 and bf16 panels (column-major and 64-row blocked) and against the
8-moment pass it shares five sums with, the estimator against the row-by-row reference twin,
and hipGraph capture and replay. The shapes are those of tests/test_gpu_irm.py. Run on the
MI355X box: ``pytest -m gpu``."""
import dataclasses
import math
from dataclasses import asdict

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators import sensitivity as DS
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.reference import estimators as E

pytestmark = pytest.mark.gpu

COUNTS = (130, 7, 64, 1, 257, 70)   # rows of segment 2k + a: padding, a one-row segment, a
P_X = 300                           # block tail; p = 300: two compaction trips of 256 threads
CLIP = 0.2
SHARED = ([0, 1, 2, 3, 13], [0, 1, 2, 3, 7])   # S psi, S psi^2, n, n_clipped, n_treated


def _case(exact: bool):
    """The host arrays of tests/test_gpu_irm.py: 3 folds arm-split into 6 segments of COUNTS
    rows, ~40 nonzero coefficients incl. columns 0, 255, 256, 299, fold 1 intercept-only.
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
    assert got.shape == (14,)
    np.testing.assert_allclose(got, want, rtol=1e-11)     # the bound of tests/test_gpu_irm.py
    assert got[2] == n == want[2] and got[13] == nt == want[13] and got[3] == want[3]
    assert 0 < got[3] < n                                 # many rows clip, not all


def _shared_bits(pan, c, spf, nbx, got):
    base = DI.irm_score_moments(pan, c, CLIP, spf, nbx=nbx)
    torch.cuda.synchronize()
    assert torch.equal(got[SHARED[0]].cpu(), base[SHARED[1]].cpu()), (got.tolist(), base.tolist())


def test_sens_kernel_f64_vs_twin(gpu):
    X, W, Y, seg, coef = _case(exact=False)
    m = _raw_m(X, seg, coef)
    assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6
    assert np.count_nonzero(np.any(coef[:, :, 1:] != 0, axis=(0, 1))) >= 36
    pc = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    pg = build_panel(X, W, Y, folds=seg, dtype="f64", device=gpu)
    assert tuple(pg.seg_nreal) == COUNTS and pg.ld > len(Y)
    c = torch.from_numpy(coef)
    want = DS.irm_sens_moments(pc, c, CLIP, 2)
    assert want[6] > 0 and want[4] > 0                    # nu2, sigma2 of this case
    for nbx in (None, 1):
        got = DS.irm_sens_moments(pg, c.to(gpu), CLIP, 2, nbx=nbx)
        torch.cuda.synchronize()
        _check(got, want, len(Y), int(W.sum()))
        _shared_bits(pg, c.to(gpu), 2, nbx, got)
    # a plain K-fold reading of the same panel: one coefficient block per segment
    c6 = torch.from_numpy(np.repeat(coef, 2, axis=0))
    got = DS.irm_sens_moments(pg, c6.to(gpu), CLIP, 1)
    torch.cuda.synchronize()
    _check(got, DS.irm_sens_moments(pc, c6, CLIP, 1), len(Y), int(W.sum()))
    _shared_bits(pg, c6.to(gpu), 1, None, got)


def test_sens_kernel_bf16_layouts_vs_twin(gpu):
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
    want = DS.irm_sens_moments(pc, c, CLIP, 2)
    out = []
    for pan in (cm, bl):
        got = DS.irm_sens_moments(pan, c.to(gpu), CLIP, 2)
        torch.cuda.synchronize()
        _check(got, want, len(Y), int(W.sum()))
        _shared_bits(pan, c.to(gpu), 2, None, got)
        out.append(got.cpu())
    assert torch.equal(out[0], out[1])                    # the two layouts: the same bits


def test_estimator_vs_reference(gpu, tutorial):
    _, m, _ = tutorial
    a = DS.dml_irm_sensitivity(m.Y, m.W, m.X, benchmarks=[[0, 1, 2]], device=gpu)
    torch.cuda.synchronize()
    b = E.dml_irm_sensitivity(m.Y, m.W, m.X, benchmarks=[[0, 1, 2]])    # two twin fits
    sa, sb = asdict(a.scenario), asdict(b.scenario)
    # the 1e-6 abs/rel bound of tests/test_gpu_irm.py test_estimator_vs_reference
    for k in ("theta", "se", "sigma2", "nu2"):
        print(k, getattr(a, k), getattr(b, k), "diff", abs(getattr(a, k) - getattr(b, k)))
        assert getattr(a, k) == pytest.approx(getattr(b, k), abs=1e-6, rel=1e-6), k
    for k in ("theta_lower", "theta_upper", "se_lower", "se_upper", "ci_lower", "ci_upper"):
        print(k, sa[k], sb[k], "diff", abs(sa[k] - sb[k]))
        assert sa[k] == pytest.approx(sb[k], abs=1e-6, rel=1e-6), k
    # |d cf / d a| <= 1 with a = D / S and S about 1.5 here; the raw cf values divide
    # differences good to 1e-6 by sigma2 (about 0.2) or nu2 (about 10): 1e-5 absolute
    (ka,), (kb,) = a.benchmarks, b.benchmarks
    for k, x, y in (("rv", a.rv, b.rv), ("rva", a.rva, b.rva),
                    ("cf_y_raw", ka.cf_y_raw, kb.cf_y_raw), ("cf_d_raw", ka.cf_d_raw, kb.cf_d_raw),
                    ("cf_y", ka.cf_y, kb.cf_y), ("cf_d", ka.cf_d, kb.cf_d)):
        print(k, x, y, "diff", abs(x - y))
        assert abs(x - y) <= 1e-5, k
    print("delta_theta", ka.delta_theta, kb.delta_theta, "rho", ka.rho, kb.rho)
    assert ka.columns == kb.columns == (0, 1, 2)
    assert ka.delta_theta == pytest.approx(kb.delta_theta, abs=1e-6)
    if not (math.isnan(ka.rho) or math.isnan(kb.rho)):
        assert abs(ka.rho) <= 1 and abs(kb.rho) <= 1
    assert a.diagnostics["n_clipped"] == b.diagnostics["n_clipped"]
    assert a.diagnostics["n_treated"] == b.diagnostics["n_treated"]
    # the theta and SE that the estimator itself reports
    r = DI.dml_irm_lasso(m.Y, m.W, m.X, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert (a.theta, a.se) == (r.ate, r.se)


def test_graph_capture_and_replay(gpu, tutorial):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    _, m, _ = tutorial
    rs = np.random.RandomState(4)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    bench = [[0, 1, 2], [5]]
    runs = []
    for _ in range(3):
        r = DS.dml_irm_sensitivity(m.Y, m.W, m.X, benchmarks=bench, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    for r in runs[1:]:
        # (str: a NaN rho compares unequal to itself)
        assert r.moments == runs[0].moments and str(r.benchmarks) == str(runs[0].benchmarks)
        assert (r.theta, r.se, r.rv, r.rva, r.scenario) == \
            (runs[0].theta, runs[0].se, runs[0].rv, runs[0].rva, runs[0].scenario)
    # other data in the same layout (same folds and arms): a replay equals a fresh eager run
    Y2 = np.where(rs.rand(len(m.Y)) < 0.2, 1.0 - m.Y, m.Y)
    r4 = DS.dml_irm_sensitivity(Y2, m.W, m.X, benchmarks=bench, device=gpu)
    torch.cuda.synchronize()
    e4 = DS.dml_irm_sensitivity(Y2, m.W, m.X, benchmarks=bench, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert r4.moments == e4.moments and r4.moments != runs[0].moments
    assert str(r4.benchmarks) == str(e4.benchmarks)       # benchmark moments included
    assert len(r4.benchmarks) == 2 and r4.benchmarks[1].columns == (5,)
    # other benchmark sets: another graph, not this one
    r5 = DS.dml_irm_sensitivity(Y2, m.W, m.X, benchmarks=[[5]], device=gpu)
    torch.cuda.synchronize()
    assert r5.diagnostics["hipgraph"] is False and r5.moments == e4.moments
    assert str(r5.benchmarks[0]) == str(e4.benchmarks[1])
    estimator_graphs.clear()
