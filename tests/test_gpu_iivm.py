"""GPU tests of the LATE of the interactive IV model (estimators/late.py): the fused
15-moment pass (csrc/iivm.hip ``ate_iivm_moments``) against its float64 torch twin on fp64 and
bf16 panels (column-major and 64-row blocked) with an all-zero r0 row and an intercept-only r1
row, the moments it shares bit for bit with the AIPW pass of csrc/irm.hip, the estimator
against the row-by-row reference twin under one-sided noncompliance, hipGraph capture and
replay, and bf16 against f64 panel storage. Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.data.dgp import make_late_data
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators import late as DL
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.reference import estimators as E
from ate_replication_causalml_amd.result import LateResult
from test_gpu_irm import CLIP, COUNTS, P_X, _case, _raw_m

pytestmark = pytest.mark.gpu

COUNT_MOMENTS = [2, 3, 7, 8, 9]      # n, n_clipped, S z, S z d, S (1-z) d
# (moments of the LATE pass, moments of irm_score_moments, coefficient rows) at the same nbx
SHARED_Y = ([0, 1, 2, 3, 7, 10, 11, 14], [0, 1, 2, 3, 7, 4, 5, 6], [0, 1, 4])
SHARED_D = ([4, 5, 12, 13], [0, 1, 4, 5], [2, 3, 4])   # on a panel whose Y column holds D


def _case5(exact: bool):
    """The edge shape of test_gpu_irm._case (segments of 130, 7, 64, 1, 257, 70 rows, p = 300,
    supports with columns 0, 255, 256, 299, fold 1 intercept-only) with its W as the
    instrument Z, a treatment taken D that follows Z on 80 % of the rows, and five coefficient
    rows (g0, g1, r0, r1, m): g0, g1, m are _case's, r0 and r1 have supports of their own;
    fold 0 has an all-zero r0 row (no always-takers) and fold 2 an r1 row that is the
    intercept 1 only (no never-takers). ``exact``: the grids of _case, so every fp32 partial
    sum of the bf16 kernel is exact. Returns (X, Z, D, Y, seg, coef [3, 5, p+1])."""
    X, Z, Y, seg, c3 = _case(exact)
    rs = np.random.RandomState(23)
    D = np.where(rs.rand(len(Z)) < 0.8, Z, 1.0 - Z)
    coef = np.zeros((3, 5, P_X + 1))
    coef[:, 0], coef[:, 1], coef[:, 4] = c3[:, 0], c3[:, 1], c3[:, 2]
    pool = np.unique(np.r_[0, 255, 256, 299, rs.choice(P_X, 30, replace=False)])
    for k, r in ((2, 2), (0, 3)):
        on = pool[rs.rand(len(pool)) < 0.5]
        # exact: at most ~34 terms of |c| <= 6/64 on |x| <= 4, below 2^7 with the intercept
        coef[k, r, 1 + on] = rs.randint(-6, 7, len(on)) / 64.0 if exact else \
            rs.randn(len(on)) * 0.1
    coef[2, 2, 1 + 255], coef[0, 3, 1 + 256] = 5 / 64.0, -3 / 64.0
    coef[:, 2, 0], coef[:, 3, 0] = 0.125, 0.875
    coef[0, 2] = 0.0                 # fold 0: r0 = 0, all-zero
    coef[2, 3] = 0.0
    coef[2, 3, 0] = 1.0              # fold 2: r1 = 1, the intercept only
    return X, Z, D, Y, seg, coef


def _panels(exact, dtype, device):
    """The LATE panel (Z in column W, D beside it) and the panel whose Y column holds D."""
    X, Z, D, Y, seg, coef = _case5(exact)
    m = _raw_m(X, seg, coef[:, [0, 1, 4]])
    assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6
    pan = build_panel(X, Z, Y, folds=seg, dtype=dtype, device=device, targets={"D": D})
    pd_ = build_panel(X, Z, D, folds=seg, dtype=dtype, device=device)
    assert tuple(pan.seg_nreal) == COUNTS and pan.ld > len(Y)
    assert np.array_equal(pan.seg_bounds, pd_.seg_bounds)
    return pan, pd_, torch.from_numpy(coef), (Z, D)


def _check(got, want, Z, D):
    got, want = got.cpu().numpy(), want.numpy()
    print("moments gpu ", got.tolist())
    print("moments twin", want.tolist())
    print("rel err     ", (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).tolist())
    np.testing.assert_allclose(got, want, rtol=1e-11)     # the bound of test_gpu_irm._check
    assert np.array_equal(got[COUNT_MOMENTS], want[COUNT_MOMENTS])
    n = len(Z)
    assert got[2] == n and got[7] == Z.sum() and got[8] == (Z * D).sum() and \
        got[9] == ((1 - Z) * D).sum()
    assert 0 < got[3] < n                                 # many rows clip, not all


def _check_shared(got, pan, pd_, c, spf, nbx):
    for (mine, theirs, rows), p in ((SHARED_Y, pan), (SHARED_D, pd_)):
        base = DI.irm_score_moments(p, c[:, rows].contiguous(), CLIP, spf, nbx=nbx)
        torch.cuda.synchronize()
        assert torch.equal(got[mine], base[theirs]), (mine, got[mine], base[theirs])


def test_late_kernel_f64_vs_twin(gpu):
    pc, _, coef, (Z, D) = _panels(False, "f64", "cpu")
    pg, pd_, _, _ = _panels(False, "f64", gpu)
    assert (coef[0, 2] == 0).all() and (coef[2, 3, 1:] == 0).all() and coef[2, 3, 0] == 1
    assert np.count_nonzero(np.any(coef.numpy()[:, :, 1:] != 0, axis=(0, 1))) >= 36
    for spf, c in ((2, coef),
                   # a plain K-fold reading of the same panel: one block per segment
                   (1, torch.from_numpy(np.repeat(coef.numpy(), 2, axis=0)))):
        want = DL.iivm_moments(pc, c, CLIP, spf)
        for nbx in (None, 1):
            got = DL.iivm_moments(pg, c.to(gpu), CLIP, spf, nbx=nbx)
            torch.cuda.synchronize()
            print("spf", spf, "nbx", nbx)
            _check(got, want, Z, D)
            _check_shared(got, pg, pd_, c.to(gpu), spf, nbx)


def test_late_kernel_bf16_layouts_vs_twin(gpu):
    pc, _, coef, (Z, D) = _panels(True, "bf16", "cpu")
    cm, cd, _, _ = _panels(True, "bf16", gpu)

    def blocked(p):
        b = dataclasses.replace(
            p, data=p.data.reshape(p.P, p.ld // 64, 64).permute(1, 0, 2).contiguous(), blocked=True)
        assert b.strides() == (64, 64 * p.P) and torch.equal(b.colmajor(), p.data)
        return b

    want = DL.iivm_moments(pc, coef, CLIP, 2)
    c = coef.to(gpu)
    out = []
    for pan, pd_ in ((cm, cd), (blocked(cm), blocked(cd))):
        got = DL.iivm_moments(pan, c, CLIP, 2)
        torch.cuda.synchronize()
        _check(got, want, Z, D)
        _check_shared(got, pan, pd_, c, 2, None)
        out.append(got.cpu())
    assert torch.equal(out[0], out[1])                    # the two layouts: the same bits


@pytest.mark.parametrize("flag", ["always_takers", "never_takers"])
def test_estimator_vs_reference_one_sided(gpu, tutorial, flag):
    _, m, _ = tutorial
    d = make_late_data(len(m.Y), 1991, **{flag: False})
    kw = {flag: False}
    a = DL.dml_iivm_lasso(d.Y, d.D, d.Z, d.X, device=gpu, graph=False, **kw)
    torch.cuda.synchronize()
    b = E.dml_iivm_lasso(d.Y, d.D, d.Z, d.X, **kw)
    print("gpu", a.late, a.se, a.diagnostics, "reference", b.late, b.se, b.diagnostics)
    # the bound of the IRM twin (tests/test_gpu_irm.py test_estimator_vs_reference)
    for x, y in ((a.late, b.late), (a.se, b.se), (a.itt.ate, b.itt.ate), (a.itt.se, b.itt.se),
                 (a.first_stage.ate, b.first_stage.ate), (a.first_stage.se, b.first_stage.se)):
        assert x == pytest.approx(y, abs=1e-6, rel=1e-6)
    for k in ("n", "n_clipped", "n_z1", "n_z0_d0", "n_z0_d1", "n_z1_d0", "n_z1_d1"):
        assert a.diagnostics[k] == b.diagnostics[k]
    assert a.diagnostics["n_z0_d1" if flag == "always_takers" else "n_z1_d0"] == 0


def test_graph_capture_and_replay(gpu, tutorial):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    _, m, _ = tutorial
    d = make_late_data(len(m.Y), 1991)
    rs = np.random.RandomState(4)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DL.dml_iivm_lasso(d.Y, d.D, d.Z, d.X, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    for r in runs[1:]:
        assert r.moments == runs[0].moments and (r.late, r.se) == (runs[0].late, runs[0].se)
    # new Y and D in the same layout (same folds and Z): a replay equals a fresh eager run
    Y2 = np.where(rs.rand(d.n) < 0.2, 1.0 - d.Y, d.Y)
    D2 = np.where(rs.rand(d.n) < 0.1, 1.0 - d.D, d.D)
    r4 = DL.dml_iivm_lasso(Y2, D2, d.Z, d.X, device=gpu)
    torch.cuda.synchronize()
    e4 = DL.dml_iivm_lasso(Y2, D2, d.Z, d.X, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert r4.moments == e4.moments and r4.moments != runs[0].moments
    # another flag setting on the same layout (D = 0 wherever Z = 0): its own cache entry
    n_entries = len(estimator_graphs.entries)
    D3 = d.D * d.Z
    sub = [DL.dml_iivm_lasso(d.Y, D3, d.Z, d.X, always_takers=False, device=gpu) for _ in range(2)]
    torch.cuda.synchronize()
    assert [r.diagnostics["hipgraph"] for r in sub] == [False, True]
    assert len(estimator_graphs.entries) == n_entries + 1
    assert sub[1].moments == sub[0].moments and sub[0].diagnostics["n_z0_d1"] == 0
    estimator_graphs.clear()


def test_late_bf16_vs_f64_panel(gpu):
    """Storage parity on a host-built 50,000 x 60 panel. The ITT keeps the bounds of
    test_gpu_irm.test_irm_bf16_vs_f64_panel; the LATE and first-stage ratios are printed, not
    bounded (profiles/iivm/README.md records them)."""
    d = make_late_data(50_000, 2, p_extra=39)
    assert d.X.shape == (50_000, 60)
    res = {}
    for dt in ("bf16", "f64"):
        pan, counts, _, n, _ = DI.arm_split_panel(d.Y, d.Z, d.X, 5, 1991, dt, gpu,
                                                  targets={"D": d.D})
        _, mom, _ = DL.late_panel(pan, 5, seg_counts=counts)
        torch.cuda.synchronize()
        res[dt] = LateResult.from_moments(dt, mom.cpu().numpy())
    rb, r64 = res["bf16"], res["f64"]
    for name, x, y, se in (("late", rb.late, r64.late, r64.se),
                           ("itt", rb.itt.ate, r64.itt.ate, r64.itt.se),
                           ("first stage", rb.first_stage.ate, r64.first_stage.ate,
                            r64.first_stage.se)):
        print(name, "bf16", x, "f64", y, "dtheta/SE", abs(x - y) / se)
    print("dSE/SE late", abs(rb.se - r64.se) / r64.se, "itt",
          abs(rb.itt.se - r64.itt.se) / r64.itt.se, "first stage",
          abs(rb.first_stage.se - r64.first_stage.se) / r64.first_stage.se)
    assert abs(rb.itt.ate - r64.itt.ate) < 0.05 * r64.itt.se
    assert abs(rb.itt.se - r64.itt.se) < 0.02 * r64.itt.se
    for k in COUNT_MOMENTS:
        if k != 3:
            assert rb.moments[k] == r64.moments[k]
    assert rb.moments[2] == 50_000
