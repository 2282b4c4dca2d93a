"""GPU tests of the target populations of DML-IRM (estimators/targets.py): the TARGETS
instantiation of the fused score kernel (csrc/irm.hip ``ate_irm_target_moments``) against its
float64 torch twin on fp64 and bf16 panels (column-major and 64-row blocked), with one
all-zero coefficient row, the moments it shares with the ATE pass bit for bit, the estimator
against the row-by-row reference twin, hipGraph capture and replay, and bf16 against f64
panel storage. Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators import targets as DT
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.reference import estimators as E
from ate_replication_causalml_amd.result import TARGETS, TargetResult
from test_gpu_irm import CLIP, COUNTS, _case, _raw_m

pytestmark = pytest.mark.gpu

COUNT_MOMENTS = [2, 3, 11]           # n, n_clipped, n_treated
SHARED = ([0, 1, 2, 3, 11], [0, 1, 2, 3, 7])   # with irm_score_moments at the same nbx


def _check(got, want, n, nt):
    got, want = got.cpu().numpy(), want.numpy()
    print("moments gpu ", got.tolist())
    print("moments twin", want.tolist())
    print("rel err     ", (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).tolist())
    np.testing.assert_allclose(got, want, rtol=1e-11)     # the bound of test_gpu_irm._check
    assert np.array_equal(got[COUNT_MOMENTS], want[COUNT_MOMENTS])
    assert got[2] == n and got[11] == nt
    assert 0 < got[3] < n                                 # many rows clip, not all


@pytest.mark.parametrize("zero_g1", [False, True])
def test_target_kernel_f64_vs_twin(gpu, zero_g1):
    X, W, Y, seg, coef = _case(exact=False)
    if zero_g1:
        coef[:, 1] = 0.0              # what an ATT-only fit leaves: one empty support vector
    m = _raw_m(X, seg, coef)
    assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6
    pc = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    pg = build_panel(X, W, Y, folds=seg, dtype="f64", device=gpu)
    assert tuple(pg.seg_nreal) == COUNTS and pg.ld > len(Y)
    n, nt = len(Y), int(W.sum())
    for spf, c in ((2, torch.from_numpy(coef)),
                   # a plain K-fold reading of the same panel: one block per segment
                   (1, torch.from_numpy(np.repeat(coef, 2, axis=0)))):
        want = DT.irm_target_moments(pc, c, CLIP, spf)
        for nbx in (None, 1):
            got = DT.irm_target_moments(pg, c.to(gpu), CLIP, spf, nbx=nbx)
            base = DI.irm_score_moments(pg, c.to(gpu), CLIP, spf, nbx=nbx)
            torch.cuda.synchronize()
            print("spf", spf, "nbx", nbx)
            _check(got, want, n, nt)
            assert torch.equal(got[SHARED[0]], base[SHARED[1]])


def test_target_kernel_bf16_layouts_vs_twin(gpu):
    X, W, Y, seg, coef = _case(exact=True)
    m = _raw_m(X, seg, coef)
    assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6
    pc = build_panel(X, W, Y, folds=seg, dtype="bf16", device="cpu")
    cm = build_panel(X, W, Y, folds=seg, dtype="bf16", device=gpu)
    bl = dataclasses.replace(
        cm, data=cm.data.reshape(cm.P, cm.ld // 64, 64).permute(1, 0, 2).contiguous(), blocked=True)
    assert bl.strides() == (64, 64 * cm.P) and torch.equal(bl.colmajor(), cm.data)
    c = torch.from_numpy(coef)
    want = DT.irm_target_moments(pc, c, CLIP, 2)
    out = []
    for pan in (cm, bl):
        got = DT.irm_target_moments(pan, c.to(gpu), CLIP, 2)
        base = DI.irm_score_moments(pan, c.to(gpu), CLIP, 2)
        torch.cuda.synchronize()
        _check(got, want, len(Y), int(W.sum()))
        assert torch.equal(got[SHARED[0]], base[SHARED[1]])
        out.append(got.cpu())
    assert torch.equal(out[0], out[1])                    # the two layouts: the same bits


def _close(a, b):
    assert a.ate == pytest.approx(b.ate, abs=1e-6, rel=1e-6)
    assert a.se == pytest.approx(b.se, abs=1e-6, rel=1e-6)


def test_estimator_vs_reference(gpu, tutorial):
    _, m, _ = tutorial
    a = DT.dml_irm_targets(m.Y, m.W, m.X, device=gpu, graph=False)
    torch.cuda.synchronize()
    b = E.dml_irm_targets(m.Y, m.W, m.X)
    for t in TARGETS:
        print(t, "gpu", a[t].ate, a[t].se, "reference", b[t].ate, b[t].se)
        _close(a[t], b[t])
    ca, cb = a.contrast("treated", "control"), b.contrast("treated", "control")
    print("contrast gpu", ca, "reference", cb)
    assert ca.se == pytest.approx(cb.se, abs=1e-6, rel=1e-6)
    assert a.diagnostics["n_clipped"] == b.diagnostics["n_clipped"]
    assert a.diagnostics["n_treated"] == b.diagnostics["n_treated"]
    # one target: fewer path problems, the same row
    one = DT.dml_irm_targets(m.Y, m.W, m.X, targets=("treated",), device=gpu, graph=False)
    torch.cuda.synchronize()
    _close(one["treated"], b["treated"])
    print("treated row bit-equal to the three-target call:",
          (one["treated"].ate, one["treated"].se) == (a["treated"].ate, a["treated"].se))
    assert np.isnan(one["all"].ate) and np.isnan(one["control"].se)
    assert all(np.isfinite(v) for v in one.moments)


def test_graph_capture_and_replay(gpu, tutorial):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    _, m, _ = tutorial
    rs = np.random.RandomState(4)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DT.dml_irm_targets(m.Y, m.W, m.X, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    for r in runs[1:]:
        assert r.moments == runs[0].moments and r.cov == runs[0].cov
    # other data in the same layout (same folds and arms): a replay equals a fresh eager run
    Y2 = np.where(rs.rand(len(m.Y)) < 0.2, 1.0 - m.Y, m.Y)
    r4 = DT.dml_irm_targets(Y2, m.W, m.X, device=gpu)
    torch.cuda.synchronize()
    e4 = DT.dml_irm_targets(Y2, m.W, m.X, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert r4.moments == e4.moments and r4.moments != runs[0].moments
    # another set of targets is another launch sequence: its own cache entry
    n_entries = len(estimator_graphs.entries)
    sub = [DT.dml_irm_targets(m.Y, m.W, m.X, targets=("control", "all"), device=gpu)
           for _ in range(2)]
    torch.cuda.synchronize()
    assert [r.diagnostics["hipgraph"] for r in sub] == [False, True]
    assert len(estimator_graphs.entries) == n_entries + 1
    assert sub[0].targets == ("all", "control") and sub[1].moments == sub[0].moments
    assert sub[0].moments == runs[0].moments              # both need all three nuisances
    estimator_graphs.clear()


def test_targets_bf16_vs_f64_panel(gpu):
    """Storage parity at the shape of test_gpu_irm.test_irm_bf16_vs_f64_panel. The "all" row
    keeps the bounds of that test; the treated and control ratios are printed, not bounded
    (profiles/irm_targets/README.md records them)."""
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    pb = synthetic_panel(200000, p=60, folds=5, seed=2, dtype="bf16", device=gpu, dgp="tutorial",
                         arm_split=True)
    p64 = synthetic_panel(200000, p=60, folds=5, seed=2, dtype="f64", device=gpu, dgp="tutorial",
                          arm_split=True, selection=pb.selection)
    mb, _ = DT.irm_targets_panel(pb, 5)
    m64, _ = DT.irm_targets_panel(p64, 5)
    torch.cuda.synchronize()
    rb = TargetResult.from_moments("bf16", mb.cpu().numpy())
    r64 = TargetResult.from_moments("f64", m64.cpu().numpy())
    for t in TARGETS:
        print(t, "bf16", rb[t].ate, rb[t].se, "f64", r64[t].ate, r64[t].se,
              "dtheta/SE", abs(rb[t].ate - r64[t].ate) / r64[t].se,
              "dSE/SE", abs(rb[t].se - r64[t].se) / r64[t].se)
    assert abs(rb["all"].ate - r64["all"].ate) < 0.05 * r64["all"].se
    assert abs(rb["all"].se - r64["all"].se) < 0.02 * r64["all"].se
    assert mb[2].item() == 200000 == m64[2].item() and mb[11].item() == m64[11].item()
