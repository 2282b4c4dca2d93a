"""``propensity="logit"`` of DML-IRM without a GPU: the device orchestration on CPU tensors
against the reference twin, the untouched default, the limits, and what the binomial fit buys
on a design with strong selection."""
import json

import numpy as np
import pytest
import torch

import ate_replication_causalml_amd as pkg
from ate_replication_causalml_amd.config import RunConfig
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.ops.lognet import cv_lognet_groups
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.reference import estimators as R


def _design(n, p=10, seed=4):
    """Strong selection: true propensity sigmoid(-1 + 1.5 x0 + x1)."""
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, p))
    pr = 1 / (1 + np.exp(-(-1 + 1.5 * X[:, 0] + X[:, 1])))
    W = (r.uniform(size=n) < pr).astype(float)
    Y = X[:, 0] + 0.5 * X[:, 2] + (1 + X[:, 0]) * W + r.normal(size=n)
    return Y, W, X, pr


@pytest.fixture(scope="module")
def small():
    return _design(2000)


def test_cpu_backend_matches_reference_twin(small):
    Y, W, X, _ = small
    dev = DI.dml_irm_lasso(Y, W, X, device="cpu", propensity="logit")
    ref = R.dml_irm_lasso(Y, W, X, propensity="logit")
    assert dev.ate == pytest.approx(ref.ate, rel=1e-9)       # the bound of tests/test_irm.py
    assert dev.se == pytest.approx(ref.se, rel=1e-9)
    assert dev.diagnostics["n_clipped"] == ref.diagnostics["n_clipped"] > 0
    for k in ("rmse_g0", "rmse_g1", "rmse_m"):
        assert dev.diagnostics[k] == pytest.approx(ref.diagnostics[k], rel=1e-9)
    assert dev.diagnostics["propensity"] == ref.diagnostics["propensity"] == "logit"
    # through the public interface, both backends
    c = pkg.ate_dml_irm(Y, W, X, run=RunConfig(backend="cpu"), propensity="logit")
    r = pkg.ate_dml_irm(Y, W, X, run=RunConfig(backend="reference"), propensity="logit")
    assert (c.ate, c.se) == (dev.ate, dev.se) and (r.ate, r.se) == (ref.ate, ref.se)
    # and it is another estimate than the linear-probability one
    lin = DI.dml_irm_lasso(Y, W, X, device="cpu")
    assert abs(lin.ate - dev.ate) > 1e-3 and lin.diagnostics["n_clipped"] > dev.diagnostics["n_clipped"]


def test_default_is_unchanged(small):
    Y, W, X, _ = small
    a = DI.dml_irm_lasso(Y, W, X, device="cpu")
    b = DI.dml_irm_lasso(Y, W, X, device="cpu", propensity="linear")
    assert a == b
    assert list(a.diagnostics) == ["n", "n_clipped", "n_treated", "rmse_g0", "rmse_g1", "rmse_m",
                                   "hipgraph"]
    ra, rb = R.dml_irm_lasso(Y, W, X), R.dml_irm_lasso(Y, W, X, propensity="linear")
    assert ra == rb and "propensity" not in ra.diagnostics
    # the fit phases: the default names all three nuisances in the one gaussian launch
    pan, *_ = DI.arm_split_panel(Y, W, X, 5, 1991, "f64", "cpu")
    st = DI.run_phases(DI.irm_fit_phases(pan, 5)[0])
    sl = DI.run_phases(DI.irm_fit_phases(pan, 5, propensity="logit")[0])
    assert "cv_m" not in st and "cv_m" in sl
    assert torch.equal(st["coef"][:, :2], sl["coef"][:, :2])       # g0, g1: the same bits
    assert not torch.equal(st["coef"][:, 2], sl["coef"][:, 2])


def test_cv_lognet_groups_cpu_is_the_reference_per_group(small):
    from ate_replication_causalml_amd.parallel import rng
    from ate_replication_causalml_amd.reference import glmnet as gn
    Y, W, X, _ = small
    K = 3
    pan, *_ = DI.arm_split_panel(Y, W, X, K, 1991, "f64", "cpu")
    cv = cv_lognet_groups(pan, pan.xcols, pan.cols["W"], DI.logit_fold_sets(K))
    fid = rng.fold_ids(len(Y), K, 1991, stream=0)
    for k in range(K):
        rows = fid != k
        ref = gn.cv_glmnet(X[rows], W[rows], family="binomial",
                           foldid=np.where(fid > k, fid - 1, fid)[rows])
        m = len(ref.lambdas)
        assert int(cv.nlam[k]) == m and cv.sel[k].tolist() == [ref.idx_min, ref.idx_1se]
        np.testing.assert_allclose(cv.cvm[k, :m].numpy(), ref.cvm, rtol=1e-9)
        a0, b = ref.coef("lambda.min")
        np.testing.assert_allclose(cv.coef_min[k].numpy(), np.r_[a0, b], atol=1e-9)
        assert torch.isnan(cv.cvm[k, m:]).all() and torch.isnan(cv.lambdas[k, m:]).all()
    with pytest.raises(ValueError):
        cv_lognet_groups(pan, pan.xcols, pan.cols["W"], [[(0, 1), (1, 2)]])   # overlapping folds
    with pytest.raises(ValueError):
        cv_lognet_groups(pan, pan.xcols, pan.cols["W"], [[(0, 1)]])           # one fold


class _Dist:
    world = 2


def test_out_of_scope_raises(small):
    Y, W, X, _ = small
    cpu = RunConfig(backend="cpu")
    with pytest.raises(ValueError, match="repeats"):
        pkg.ate_dml_irm(Y, W, X, run=cpu, repeats=2, propensity="logit")
    with pytest.raises(ValueError, match="repeats"):
        pkg.ate_dml_irm_targets(Y, W, X, run=cpu, repeats=2, propensity="logit")
    with pytest.raises(ValueError, match="sensitivity"):
        pkg.ate_dml_irm_sensitivity(Y, W, X, run=cpu, propensity="logit")
    with pytest.raises(ValueError, match="iivm"):
        pkg.ate_dml_iivm(Y, W, W, X, run=cpu, propensity="logit")
    with pytest.raises(ValueError, match="dist"):
        DI.dml_irm_lasso(Y, W, X, device="cpu", dist=_Dist(), propensity="logit")
    with pytest.raises(ValueError, match="bf16"):
        DI.dml_irm_lasso(Y, W, X, device="cpu", dtype="bf16", propensity="logit")
    with pytest.raises(ValueError, match="p <= 96"):
        DI.dml_irm_lasso(Y, W, np.zeros((len(Y), 97)), device="cpu", propensity="logit")
    with pytest.raises(ValueError, match="K <= 16"):
        DI.dml_irm_lasso(Y, W, X, folds=17, device="cpu", propensity="logit")
    with pytest.raises(ValueError, match="propensity must be"):
        DI.dml_irm_lasso(Y, W, X, device="cpu", propensity="probit")
    with pytest.raises(ValueError, match="propensity must be"):
        R.dml_irm_lasso(Y, W, X, propensity="probit")
    # the same limits on the estimators built on the score
    from ate_replication_causalml_amd.estimators import cate, gate, policy, targets
    g = (X[:, 3] > 0).astype(int)
    for call in (lambda **kw: gate.dml_irm_gate_lasso(Y, W, X, g, **kw),
                 lambda **kw: cate.dml_irm_cate_lasso(Y, W, X, 0, **kw),
                 lambda **kw: policy.dml_irm_policy_lasso(Y, W, X, [0, 1], **kw),
                 lambda **kw: targets.dml_irm_targets(Y, W, X, **kw)):
        with pytest.raises(ValueError, match="bf16"):
            call(device="cpu", dtype="bf16", propensity="logit")
        with pytest.raises(ValueError, match="K <= 16"):
            call(device="cpu", folds=17, propensity="logit")
    # the score pass itself: no logistic link on a bf16 panel
    seg = (np.arange(len(Y)) % 3) * 2 + W.astype(np.int64)
    pb = build_panel(X, W, Y, folds=seg, dtype="bf16", device="cpu")
    with pytest.raises(ValueError, match="fp32 / fp64"):
        DI.irm_score_moments(pb, torch.zeros(3, 3, X.shape[1] + 1, dtype=torch.float64), 0.01, 2,
                             link="logistic")


def test_estimators_on_the_score_match_their_reference_twins(small):
    from ate_replication_causalml_amd.estimators import gate, targets
    Y, W, X, _ = small
    g = (X[:, 3] > 0).astype(int)
    a = gate.dml_irm_gate_lasso(Y, W, X, g, n_boot=99, device="cpu", propensity="logit")
    b = R.dml_irm_gate(Y, W, X, g, n_boot=99, propensity="logit")
    np.testing.assert_allclose(a.ate, b.ate, rtol=1e-9)
    np.testing.assert_allclose(a.se, b.se, rtol=1e-9)
    assert a.diagnostics["propensity"] == "logit"
    t = targets.dml_irm_targets(Y, W, X, device="cpu", propensity="logit")
    u = R.dml_irm_targets(Y, W, X, propensity="logit")
    for k in ("all", "treated", "control"):
        assert t.estimates[k].ate == pytest.approx(u.estimates[k].ate, rel=1e-9)
        assert t.estimates[k].se == pytest.approx(u.estimates[k].se, rel=1e-9)
    assert t.diagnostics["propensity"] == "logit"


def test_logit_propensity_is_a_probability_and_closer_to_the_truth():
    """n = 4000, seed 1, the reference backend: no held-out logit propensity leaves [0, 1]
    (hundreds of the linear-probability ones do), and its RMSE to the true propensity is
    below half the linear fit's (measured ratios <= 0.31 on seeds 1-3)."""
    Y, W, X, pr = _design(4000, seed=1)
    _, _, _, m_lin = R._irm_scores(Y, W, X, 5, 1991, "min", 0.01)
    _, _, _, m_log = R._irm_scores(Y, W, X, 5, 1991, "min", 0.01, propensity="logit")
    assert ((m_lin < 0) | (m_lin > 1)).sum() > 100
    assert ((m_log < 0) | (m_log > 1)).sum() == 0
    rmse = lambda m: float(np.sqrt(np.mean((m - pr) ** 2)))
    print("RMSE to the true propensity: linear %.4f logit %.4f" % (rmse(m_lin), rmse(m_log)))
    assert rmse(m_log) < 0.5 * rmse(m_lin)


def test_cli_names_the_propensity(capsys):
    from ate_replication_causalml_amd import cli
    assert cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64",
                     "--propensity", "logit"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["propensity"] == "logit" and np.isfinite(out["ate"]) and out["se"] > 0
    with pytest.raises(SystemExit):
        cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64",
                  "--propensity", "logit", "--sensitivity"])
    with pytest.raises(SystemExit):
        cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--propensity", "logit"])
