"""The effect on the treated and on the controls beside the ATE of DML-IRM
(estimators/targets.py, result.TargetResult) on the CPU path: the 12-moment twin and the
closed forms against the row-by-row reference, psi = a + c, the moments shared with the ATE
pass, the estimator against the reference twin, subsets of targets (fewer path problems, NaN
rows), row sharding, argument checks and the public surface."""
import json
import math

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.config import RunConfig
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators import targets as DT
from ate_replication_causalml_amd.ops.enet import cv_problem_count
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel.comm import run_simulated
from ate_replication_causalml_amd.reference import estimators as R
from ate_replication_causalml_amd.result import (TARGET_MOMENTS, TARGETS, AteResult, TargetResult,
                                                 target_estimates)
from test_gpu_irm import CLIP, COUNTS, _case

K = 5


# ---------------------------------------------------------------- twin and closed forms
@pytest.fixture(scope="module")
def case():
    """The geometry of tests/test_gpu_irm.py ``_case`` (segments of 130, 7, 64, 1, 257, 70
    rows, p = 300, clip 0.2, fold 1 intercept-only): the panel, the twin's 12 moments and the
    per-row nuisances in numpy."""
    X, W, Y, seg, coef = _case(exact=False)
    pan = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    assert tuple(pan.seg_nreal) == COUNTS and pan.ld > len(Y)
    c = torch.from_numpy(coef)
    mom = DT.irm_target_moments(pan, c, CLIP, 2)
    g0, g1, m = (np.array([coef[s // 2, r, 0] + coef[s // 2, r, 1:] @ x for x, s in zip(X, seg)])
                 for r in range(3))
    return dict(pan=pan, coef=c, mom=mom, Y=Y, W=W, g0=g0, g1=g1, m=m)


def test_twin_and_closed_forms_vs_rows(case):
    """529 rows: the closed forms subtract sums of equal magnitude and still agree with the
    per-row covariance to 1e-10 (a numpy prototype agreed to 5e-16 at this size)."""
    assert len(TARGET_MOMENTS) == 12 == case["mom"].numel() and len(case["Y"]) == 529
    got = TargetResult.from_moments("t", case["mom"].numpy())
    theta, cov = R.targets_from_rows(case["Y"], case["W"], case["g0"], case["g1"], case["m"], CLIP)
    est = np.array([got[t].ate for t in TARGETS])
    print("theta", est.tolist(), theta.tolist())
    print("cov", got.cov, cov.tolist())
    print("rel", (np.abs(np.array(got.cov) - cov) / np.abs(cov)).tolist())
    np.testing.assert_allclose(est, theta, rtol=1e-10)
    np.testing.assert_allclose(np.array(got.cov), cov, rtol=1e-10)
    np.testing.assert_allclose([got[t].se for t in TARGETS], np.sqrt(np.diag(cov)), rtol=1e-10)
    mom = case["mom"].numpy()
    assert mom[2] == 529 and mom[11] == case["W"].sum() and 0 < mom[3] < 529
    # the three effects differ here, and so do their standard errors
    assert len({round(v, 6) for v in est}) == 3
    # treated minus control from the joint covariance against the per-row influence values
    c = got.contrast("treated", "control")
    want = math.sqrt(cov[1, 1] + cov[2, 2] - 2 * cov[1, 2])
    assert c.diff == pytest.approx(theta[1] - theta[2], rel=1e-10)
    assert c.se == pytest.approx(want, rel=1e-10)
    assert (c.lower_ci, c.upper_ci) == (c.diff - 1.96 * c.se, c.diff + 1.96 * c.se)
    assert c.p_value == pytest.approx(math.erfc(abs(c.diff) / c.se / math.sqrt(2)), rel=1e-9)


def test_psi_is_a_plus_c(case):
    """|S a + S c - S psi| <= (n + 16) 2^-52 sum(|a| + |c| + |psi|): n 2^-52 sum|x| bounds
    any order of summing the 3 n terms, and each term carries about ten roundings of its own
    (two subtractions, the clip, a product, a quotient, a product and a difference per
    numerator; psi: four more)."""
    Y, W, g0, g1, m = (case[k] for k in ("Y", "W", "g0", "g1", "m"))
    e = np.clip(m, CLIP, 1 - CLIP)
    q1, q0 = W * (Y - g1) / e, (1 - W) * (Y - g0) / (1 - e)
    a = W * (Y - g0) - e * q0
    c = -(1 - W) * (Y - g1) + (1 - e) * q1
    psi = g1 - g0 + q1 - q0
    mom = case["mom"].numpy()
    lhs = abs(mom[4] + mom[7] - mom[0])
    rhs = (len(Y) + 16) * 2.0 ** -52 * (np.abs(a) + np.abs(c) + np.abs(psi)).sum()
    print("S a + S c - S psi", lhs, "bound", rhs)
    assert lhs <= rhs
    # the twin's sums are those of the per-row arrays
    np.testing.assert_allclose([mom[4], mom[7]], [a.sum(), c.sum()], rtol=1e-12)
    np.testing.assert_allclose([mom[6], mom[9]], [(a * W).sum(), (c * (1 - W)).sum()], rtol=1e-12)


@pytest.mark.parametrize("spf", [2, 1])
def test_shared_sums_are_those_of_the_ate_pass(case, spf):
    pan = case["pan"]
    c = case["coef"] if spf == 2 else torch.from_numpy(np.repeat(case["coef"].numpy(), 2, axis=0))
    mom = DT.irm_target_moments(pan, c, CLIP, spf)
    base = DI.irm_score_moments(pan, c, CLIP, spf)
    assert torch.equal(mom[[0, 1, 2, 3, 11]], base[[0, 1, 2, 3, 7]])
    fin = DI.irm_finalize(base)
    got = TargetResult.from_moments("t", mom.numpy())
    assert got["all"].ate == fin[0].item() and got["all"].se == fin[1].item()
    var = ((base[1] - base[0] * base[0] / base[2]) / (base[2] - 1) / base[2]).item()
    assert got.cov[0][0] == var


def test_zero_g1_row_leaves_the_treated_moments(case):
    """An ATT-only fit leaves the g1 row zero: S a, S a^2, S a w and the counts do not move."""
    c0 = case["coef"].clone()
    c0[:, 1] = 0.0
    mom = DT.irm_target_moments(case["pan"], c0, CLIP, 2)
    assert torch.equal(mom[[2, 3, 4, 5, 6, 11]], case["mom"][[2, 3, 4, 5, 6, 11]])
    assert torch.isfinite(mom).all() and mom[7] != case["mom"][7]


def test_target_moments_reject_wrong_coef_shape():
    pan = build_panel(np.zeros((8, 2)), np.arange(8) % 2, np.zeros(8), folds=np.arange(8) % 4)
    with pytest.raises(ValueError):
        DT.irm_target_moments(pan, torch.zeros(1, 3, 3), 0.01, 2)    # 4 segments need 2 blocks
    with pytest.raises(ValueError):
        DT.irm_target_moments(pan, torch.zeros(2, 2, 3), 0.01, 2)
    with pytest.raises(ValueError):
        target_estimates(np.zeros(8))


# ---------------------------------------------------------------- the estimator
def _close(a: AteResult, b: AteResult):
    # the project's bound for device orchestration against the row-by-row reference
    # (tests/test_gpu_irm.py test_estimator_vs_reference)
    assert a.ate == pytest.approx(b.ate, abs=1e-6, rel=1e-6)
    assert a.se == pytest.approx(b.se, abs=1e-6, rel=1e-6)


@pytest.fixture(scope="module")
def three(tutorial):
    import ate_replication_causalml_amd as pkg
    _, m, _ = tutorial
    return pkg.ate_dml_irm_targets(m.Y, m.W, m.X, run=RunConfig(backend="cpu"))


def test_estimator_vs_reference(tutorial, three):
    import ate_replication_causalml_amd as pkg
    _, m, _ = tutorial
    ref = pkg.ate_dml_irm_targets(m.Y, m.W, m.X, run=RunConfig(backend="reference"))
    assert isinstance(three, pkg.TargetResult) and isinstance(ref, pkg.TargetResult)
    assert three.targets == ref.targets == TARGETS and three.method == ref.method
    for t in TARGETS:
        print(t, three[t].ate, three[t].se, ref[t].ate, ref[t].se)
        _close(three[t], ref[t])
    a, b = three.contrast("treated", "control"), ref.contrast("treated", "control")
    print("contrast", a, b)
    assert a.se == pytest.approx(b.se, abs=1e-6, rel=1e-6)
    assert a.diff == pytest.approx(b.diff, abs=1e-6, rel=1e-6)
    for k in ("n", "n_clipped", "n_treated"):
        assert three.diagnostics[k] == ref.diagnostics[k]
    assert three.diagnostics["hipgraph"] is False and three.diagnostics["n"] == len(m.Y)
    assert 0 < three.diagnostics["n_treated"] < len(m.Y)
    # the "all" row is the ATE estimator's own theta and SE
    irm = DI.dml_irm_lasso(m.Y, m.W, m.X, device="cpu")
    assert (three["all"].ate, three["all"].se) == (irm.ate, irm.se)
    assert np.allclose(np.array(three.cov), np.array(three.cov).T) and len(three.moments) == 12


@pytest.mark.parametrize("target,other", [("treated", "control"), ("control", "treated")])
def test_subset_of_targets(tutorial, three, target, other, monkeypatch):
    _, m, _ = tutorial
    launched = []
    real = DI.cv_enet_gaussian

    def counting(G, panel, xcols, ycols, full_sets=None, **kw):
        launched.append(cv_problem_count(G.shape[0], full_sets, len(ycols), kw.get("full_y")))
        cv = real(G, panel, xcols, ycols, full_sets=full_sets, **kw)
        launched.append(len(cv.full_keys))
        return cv

    monkeypatch.setattr(DI, "cv_enet_gaussian", counting)
    one = DT.dml_irm_targets(m.Y, m.W, m.X, targets=(target,), folds=K, device="cpu")
    # per nuisance K outer folds x (1 full + K - 1 inner CV paths) = K K problems, as
    # cv_problem_count counts them: 2 K K = 50 here, 3 K K = 75 with every nuisance
    assert launched == [2 * K * K, 2 * K]
    assert one.targets == (target,)
    j = TARGETS.index(target)
    for t in ("all", other):
        r = one[t]
        assert all(math.isnan(v) for v in (r.ate, r.se, r.lower_ci, r.upper_ci))
    cov = np.array(one.cov)
    assert np.isfinite(cov[j, j]) and np.isnan(np.delete(cov.ravel(), 4 * j)).all()
    assert all(math.isfinite(v) for v in one.moments)    # zero rows: finite, never garbage
    _close(one[target], three[target])
    print(target, "bit-equal to the three-target call:",
          (one[target].ate, one[target].se) == (three[target].ate, three[target].se))
    assert math.isnan(one.contrast("treated", "control").se)
    for k in ("n", "n_clipped", "n_treated"):
        assert one.diagnostics[k] == three.diagnostics[k]
    assert "nan" in one.table()


def test_problem_counts_of_the_nuisance_subsets():
    pan = build_panel(np.zeros((40, 2)), np.arange(40) % 2, np.zeros(40),
                      folds=np.arange(40) % (2 * K))
    for targets, nu in ((("all",), (0, 1, 2)), (("treated",), (0, 2)), (("control",), (1, 2)),
                        (("treated", "control"), (0, 1, 2))):
        assert DT.target_nuisances(targets) == nu
        c3, sets, full_y, ycols = DI.fit_problems(pan, K, pan.seg_nreal, nu)
        assert cv_problem_count(3 * K, sets, len(ycols), full_y) == len(nu) * K * K
    # the default is the call of before
    assert DI.fit_problems(pan, K, pan.seg_nreal)[1:3] == \
        DI.fit_problems(pan, K, pan.seg_nreal, (0, 1, 2))[1:3]
    for bad in ((), (3,), (2, 0), (0, 0)):
        with pytest.raises(ValueError):
            DI.fit_problems(pan, K, pan.seg_nreal, bad)


# ---------------------------------------------------------------- row sharding
def test_two_ranks_equal_one():
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    one = synthetic_panel(1500, p=24, dtype="f64", arm_split=True)
    mom1, _ = DT.irm_targets_panel(one, K)
    mom1 = mom1.numpy()
    assert mom1.shape == (12,) and np.isfinite(mom1).all() and mom1[2] == 1500

    def body(comm):
        pan = synthetic_panel(1500, p=24, dtype="f64", arm_split=True, comm=comm)
        mom, _ = DT.irm_targets_panel(pan, K, comm=comm)
        return mom.numpy(), pan.n

    want = TargetResult.from_moments("t", mom1)
    out = run_simulated(2, body)
    assert sum(n for _, n in out) == 1500
    for mom, _ in out:
        print(np.abs(mom - mom1).max())
        np.testing.assert_allclose(mom, mom1, rtol=1e-12)      # the README's non-exact bound
        assert np.array_equal(mom[[2, 3, 11]], mom1[[2, 3, 11]])
        got = TargetResult.from_moments("t", mom)
        for t in TARGETS:
            assert got[t].ate == pytest.approx(want[t].ate, rel=1e-12)
            assert got[t].se == pytest.approx(want[t].se, rel=1e-12)


# ---------------------------------------------------------------- validation
def _tiny():
    rs = np.random.RandomState(0)
    X, Y = rs.randn(120, 4), rs.randn(120)
    return Y, (rs.rand(120) < 0.5).astype(float), X


@pytest.mark.parametrize("kw", [dict(targets=("all", "att")), dict(targets=()),
                                dict(targets=("treated", "treated")), dict(targets="everyone"),
                                dict(repeats=2), dict(w=2.0)])
@pytest.mark.parametrize("backend", ["cpu", "reference"])
def test_bad_arguments_raise(kw, backend):
    import ate_replication_causalml_amd as pkg
    Y, W, X = _tiny()
    kw = dict(kw)
    if "w" in kw:
        W = W.copy()
        W[3] = kw.pop("w")                               # a non-binary treatment
    with pytest.raises(ValueError):
        pkg.ate_dml_irm_targets(Y, W, X, run=RunConfig(backend=backend), **kw)


def test_result_surface(three):
    txt = three.table()
    assert all(t in txt for t in TARGETS) and "trt - ctl" in txt
    out = json.loads(three.to_json())
    assert out["targets"] == list(TARGETS) and len(out["moments"]) == 12
    assert [r["target"] for r in out["estimates"]] == list(TARGETS)
    assert out["cov"][1][2] == three.cov[1][2] == three.cov[2][1]
    r = three["treated"]
    assert (r.lower_ci, r.upper_ci) == (r.ate - 1.96 * r.se, r.ate + 1.96 * r.se)
    back = three.contrast("control", "treated")
    fwd = three.contrast("treated", "control")
    assert (back.diff, back.se, back.p_value) == (-fwd.diff, fwd.se, fwd.p_value)
    with pytest.raises(ValueError):
        three.contrast("treated", "treated")
    with pytest.raises(ValueError):
        three.contrast("treated", "att")


def test_cli_targets(capsys):
    from ate_replication_causalml_amd import cli
    base = ["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64"]
    assert cli.main(base + ["--targets", "all,treated,control"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["targets"] == list(TARGETS)
    for r in out["estimates"]:
        assert all(np.isfinite(r[k]) for k in ("ATE", "se", "lower_ci", "upper_ci")), r
    assert np.isfinite(np.array(out["cov"])).all() and 0 < out["n_treated"] < 3000
    assert np.isfinite(out["contrast"]["se"]) and 0 <= out["contrast"]["p_value"] <= 1
    assert cli.main(base + ["--targets", "treated"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1].replace("NaN", "null"))
    assert out["targets"] == ["treated"] and "contrast" not in out
    assert [r["ATE"] is None for r in out["estimates"]] == [True, False, True]
    for extra in (["--repeats", "2"], ["--gate-col", "0"], ["--cate-col", "0"],
                  ["--policy-cols", "0,1"], ["--sensitivity"]):
        with pytest.raises(SystemExit):
            cli.main(base + ["--targets", "treated"] + extra)
    with pytest.raises(SystemExit):
        cli.main(base + ["--targets", "att"])
