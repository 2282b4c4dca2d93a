"""Sensitivity of DML-IRM to unobserved confounding (estimators/sensitivity.py,
result.SensitivityResult) on the CPU path: the device orchestration against the row-by-row
float64 reference twin, the closed forms from moments against the per-row route and their
defining properties, the 14-moment twin against a plain loop, covariate benchmarks, row
sharding, input validation and the public surface."""
import json
import math
from dataclasses import asdict

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators import sensitivity as DS
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel.comm import run_simulated
from ate_replication_causalml_amd.reference import estimators as R
from ate_replication_causalml_amd.result import (SensitivityResult, sens_benchmark, sens_bounds,
                                                 sens_plugins)
from ate_replication_causalml_amd.utils.guards import NumericalError

REL = 1e-9     # the bound of tests/test_irm.py test_matches_reference_twin


@pytest.fixture(scope="module")
def df_mod():
    from ate_replication_causalml_amd.data.dgp import make_tutorial_data
    from ate_replication_causalml_amd.data.selection import apply_selection_bias
    mod, _ = apply_selection_bias(make_tutorial_data(50_000, seed=1991))
    assert mod.X.shape == (9416, 21)
    return mod


@pytest.fixture(scope="module")
def small():
    """The tutorial DGP at 3,000 generated rows, 570 kept."""
    from ate_replication_causalml_amd.data.dgp import make_tutorial_data
    from ate_replication_causalml_amd.data.selection import apply_selection_bias
    mod, _ = apply_selection_bias(make_tutorial_data(3000, seed=1991))
    assert mod.X.shape == (570, 21)
    return mod


def _fields(r: SensitivityResult):
    d = {k: getattr(r, k) for k in ("theta", "se", "sigma2", "nu2", "rv", "rva", "null")}
    d.update(asdict(r.scenario))
    return d


def _close(a: SensitivityResult, b: SensitivityResult, rel=REL):
    fa, fb = _fields(a), _fields(b)
    for k in fa:
        print(k, fa[k], fb[k])
        assert fa[k] == pytest.approx(fb[k], rel=rel), k


# ---------------------------------------------------------------- twin on the tutorial data
def test_matches_reference_twin(df_mod):
    m = df_mod
    dev = DS.dml_irm_sensitivity(m.Y, m.W, m.X, device="cpu", dtype="f64")
    ref = R.dml_irm_sensitivity(m.Y, m.W, m.X)
    _close(dev, ref)
    np.testing.assert_allclose(dev.moments, ref.moments, rtol=REL)
    assert dev.diagnostics["n_clipped"] == ref.diagnostics["n_clipped"] == 0
    assert dev.diagnostics["n_treated"] == ref.diagnostics["n_treated"]
    assert dev.diagnostics["hipgraph"] is False and dev.benchmarks == []
    # the estimator's own theta and SE, exactly
    irm = DI.dml_irm_lasso(m.Y, m.W, m.X, device="cpu")
    assert (dev.theta, dev.se) == (irm.ate, irm.se)
    # the prototype's figures
    s = dev.scenario
    assert dev.sigma2 == pytest.approx(0.20912, abs=5e-6)
    assert dev.nu2 == pytest.approx(10.4312, abs=5e-5)
    assert (s.theta_lower, s.theta_upper) == pytest.approx((0.04362, 0.13359), abs=5e-6)
    assert (s.ci_lower, s.ci_upper) == pytest.approx((0.01967, 0.15727), abs=5e-6)
    assert (dev.rv, dev.rva) == pytest.approx((0.058220, 0.042777), abs=5e-7)
    assert "RV 5.8220%" in dev.table()


# ---------------------------------------------------------------- closed forms from moments
def _rows(seed=3, n=200, flip=False):
    """Hand-made per-row (psi, b, c, y): c takes negative values, nu2 stays positive."""
    rs = np.random.RandomState(seed)
    e = rs.uniform(0.05, 0.95, n)
    w = (rs.rand(n) < e).astype(float)
    b = rs.chisquare(1, n) * 0.3
    rr = w / e - (1 - w) / (1 - e)
    c = 2 * (1 / e + 1 / (1 - e)) - rr ** 2
    psi = 0.9 + 0.4 * rr * np.sqrt(b) + 0.2 * rs.randn(n)
    y = rs.randn(n)
    assert c.min() < 0 < c.mean()
    return (-psi if flip else psi), b, c, y


def _moments(psi, b, c, y):
    one = np.ones_like(psi)
    return [float(v.sum()) for v in (psi, psi * psi, one, 0 * one, b, b * b, c, c * c, psi * b,
                                     psi * c, b * c, y, y * y, one)]


def test_zero_strength_is_the_plain_estimate():
    psi, b, c, y = _rows()
    r = SensitivityResult.from_moments("t", _moments(psi, b, c, y))
    n = len(psi)
    assert r.theta == pytest.approx(psi.mean(), rel=1e-14)
    assert r.se == pytest.approx(psi.std(ddof=1) / math.sqrt(n), rel=1e-13)
    for s in (r.bounds(0.0, 0.0), r.bounds(0.0, 0.5), r.bounds(0.5, 0.0), r.bounds(0.3, 0.3, rho=0.0)):
        assert s.theta_lower == s.theta_upper == r.theta
        assert s.se_lower == s.se_upper == r.se


def test_bounds_widen_monotonically():
    psi, b, c, y = _rows()
    r = SensitivityResult.from_moments("t", _moments(psi, b, c, y))
    grid = [0.0, 0.01, 0.05, 0.2, 0.5, 0.9]
    for fixed in (0.1, 0.4):
        for sweep in (lambda v: r.bounds(v, fixed), lambda v: r.bounds(fixed, v),
                      lambda v: r.bounds(fixed, fixed, rho=v),
                      lambda v: r.bounds(fixed, fixed, rho=-v)):
            s = [sweep(v) for v in grid]
            lo, hi = [x.theta_lower for x in s], [x.theta_upper for x in s]
            assert all(a > b for a, b in zip(lo, lo[1:])) and all(a < b for a, b in zip(hi, hi[1:]))
    # rho enters by its absolute value only
    assert r.bounds(0.1, 0.2, rho=-0.5).theta_lower == r.bounds(0.1, 0.2, rho=0.5).theta_lower


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("rho,level,null", [(1.0, 0.95, 0.0), (0.6, 0.9, 0.25)])
def test_robustness_values_reach_the_null(flip, rho, level, null):
    psi, b, c, y = _rows(flip=flip)
    null = -null if flip else null
    r = SensitivityResult.from_moments("t", _moments(psi, b, c, y), rho=rho, level=level, null=null)
    assert (r.theta < null) == flip and 0 < r.rva < r.rv < 1
    at_rv, at_rva = r.bounds(r.rv, r.rv, rho, level), r.bounds(r.rva, r.rva, rho, level)
    if flip:       # the mirrored case: the upper bound comes down to the null
        assert at_rv.theta_upper == pytest.approx(null, abs=1e-12)
        assert at_rva.ci_upper == pytest.approx(null, abs=1e-9)
    else:
        assert at_rv.theta_lower == pytest.approx(null, abs=1e-12)
        assert at_rva.ci_lower == pytest.approx(null, abs=1e-9)
    # the mirror image has the same robustness
    pm, bm, cm, ym = _rows(flip=not flip)
    m = SensitivityResult.from_moments("t", _moments(pm, bm, cm, ym), rho=rho, level=level, null=-null)
    assert (m.rv, m.rva) == pytest.approx((r.rv, r.rva), rel=1e-12)


def test_rva_is_zero_when_the_ci_covers_the_null():
    psi, b, c, y = _rows()
    psi = psi - psi.mean() + 0.5 * psi.std(ddof=1) / math.sqrt(len(psi))   # theta = SE / 2
    r = SensitivityResult.from_moments("t", _moments(psi, b, c, y))
    z = 1.6448536269514722
    assert 0 < r.theta < z * r.se                  # not significant one-sided
    assert r.rva == 0.0 and r.rv > 0
    assert r.bounds(r.rv, r.rv).theta_lower == pytest.approx(0.0, abs=1e-12)


@pytest.mark.parametrize("flip", [False, True])
def test_moment_route_equals_row_route(flip):
    psi, b, c, y = _rows(flip=flip)
    for cf_y, cf_d, rho, level, null in ((0.03, 0.03, 1.0, 0.95, 0.0), (0.2, 0.1, -0.7, 0.99, 0.3)):
        r = SensitivityResult.from_moments("t", _moments(psi, b, c, y), cf_y, cf_d, rho, level, null)
        theta, se, sigma2, nu2, scen, rv, rva = R.sensitivity_from_rows(psi, b, c, cf_y, cf_d, rho,
                                                                        level, null)
        got = _fields(r)
        want = dict(theta=theta, se=se, sigma2=sigma2, nu2=nu2, rv=rv, rva=rva, null=null,
                    **asdict(scen))
        for k in got:
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), k


def test_benchmark_from_moments():
    psi, b, c, y = _rows()
    long = _moments(psi, b, c, y)
    # a short model: worse outcome fit, less variable representer, another theta
    short = _moments(psi + 0.05, b * 1.2, c * 0.9, y)
    k = sens_benchmark((1, 4), long, short)
    n, th, s2, nu = sens_plugins(long)[:4]
    var_y = y.var()
    assert k.columns == (1, 4) and k.delta_theta == pytest.approx(0.05, rel=1e-12)
    assert k.cf_y_raw == pytest.approx(0.2, rel=1e-12)            # (1.2 s2 - s2) / s2
    assert k.cf_d_raw == pytest.approx(0.1 / 0.9, rel=1e-12)
    assert (k.cf_y, k.cf_d) == (k.cf_y_raw, k.cf_d_raw)
    assert k.rho == pytest.approx(min(0.05 / math.sqrt(0.2 * s2 * 0.1 * nu), 1.0), rel=1e-12)
    assert 0 < k.rho <= 1 and var_y > 0
    back = sens_benchmark((1, 4), short, long)                    # both gains negative
    assert back.cf_y == back.cf_d == 0.0 and back.cf_y_raw < 0 and back.cf_d_raw < 0
    assert math.isnan(back.rho) and back.delta_theta == pytest.approx(-0.05, rel=1e-12)


# ---------------------------------------------------------------- the 14-moment twin
def _loop_moments(X, W, Y, seg, coef, clip, spf):
    mom = np.zeros(14)
    for i in range(len(Y)):
        k = coef[seg[i] // spf]
        g0, g1, m = (k[r, 0] + k[r, 1:] @ X[i] for r in range(3))
        e = min(max(m, clip), 1 - clip)
        psi = g1 - g0 + W[i] * (Y[i] - g1) / e - (1 - W[i]) * (Y[i] - g0) / (1 - e)
        b = (Y[i] - (g1 if W[i] == 1 else g0)) ** 2
        rr = W[i] / e - (1 - W[i]) / (1 - e)
        c = 2 * (1 / e + 1 / (1 - e)) - rr * rr
        mom += [psi, psi * psi, 1.0, float(m < clip or m > 1 - clip), b, b * b, c, c * c, psi * b,
                psi * c, b * c, Y[i], Y[i] * Y[i], W[i]]
    return mom


@pytest.mark.parametrize("spf", [1, 2])
def test_sens_moments_twin_vs_loop(spf):
    rs = np.random.RandomState(11)
    n, p, K = 200, 7, 3
    X = rs.randn(n, p)
    W = (rs.rand(n) < 0.45).astype(float)
    Y = rs.randn(n) + W
    fold = rs.randint(0, K, n)
    seg = 2 * fold + W.astype(int) if spf == 2 else fold
    pan = build_panel(X, W, Y, folds=seg, dtype="f64")
    assert pan.ld > n                                    # padding rows in every segment
    coef = rs.randn(K, 3, p + 1) * (rs.rand(K, 3, p + 1) < 0.5)
    coef[:, 2, 1:] *= 0.15
    coef[:, 2, 0] = 0.5                                  # propensities around 0.5, some clipped
    coef[1, :, 1:] = 0.0                                 # an all-intercept block
    got = DS.irm_sens_moments(pan, torch.from_numpy(coef), 0.2, spf).numpy()
    want = _loop_moments(X, W, Y, seg, coef, 0.2, spf)
    assert 0 < want[3] < n
    np.testing.assert_allclose(got, want, rtol=1e-12)
    assert got[2] == n and got[13] == W.sum() and got[3] == want[3]
    # the moments shared with the score pass of the estimator
    base = DI.irm_score_moments(pan, torch.from_numpy(coef), 0.2, spf).numpy()
    assert np.array_equal(got[[0, 1, 2, 3, 13]], base[[0, 1, 2, 3, 7]])
    # S b is the sum of the two arms' squared residuals
    assert got[4] == pytest.approx(base[4] + base[5], rel=1e-14)


def test_sens_moments_rejects_wrong_coef_shape():
    pan = build_panel(np.zeros((8, 2)), np.arange(8) % 2, np.zeros(8), folds=np.arange(8) % 4)
    with pytest.raises(ValueError):
        DS.irm_sens_moments(pan, torch.zeros(1, 3, 3), 0.01, 2)      # 4 segments need 2 blocks
    with pytest.raises(ValueError):
        DS.irm_sens_moments(pan, torch.zeros(2, 2, 3), 0.01, 2)


# ---------------------------------------------------------------- benchmarks
def test_benchmark_set_matches_twin(small):
    m = small
    dev = DS.dml_irm_sensitivity(m.Y, m.W, m.X, benchmarks=[[0]], device="cpu")
    ref = R.dml_irm_sensitivity(m.Y, m.W, m.X, benchmarks=[[0]])
    _close(dev, ref)
    (a,), (b,) = dev.benchmarks, ref.benchmarks
    print(asdict(a), asdict(b))
    assert a.columns == b.columns == (0,)
    for k in ("cf_y", "cf_d", "delta_theta", "cf_y_raw", "cf_d_raw", "theta_short",
              "sigma2_short", "nu2_short"):
        assert getattr(a, k) == pytest.approx(getattr(b, k), rel=REL, abs=1e-12), k
    assert (math.isnan(a.rho) and math.isnan(b.rho)) or a.rho == pytest.approx(b.rho, rel=REL)
    # the prototype's negative gain: dropping column 0 improves the held-out outcome fit
    assert a.cf_y_raw == pytest.approx(-1.4e-3, abs=1e-4) and a.cf_y == 0.0
    assert a.cf_d == a.cf_d_raw > 0 and math.isnan(a.rho)


# ---------------------------------------------------------------- row sharding
def test_two_ranks_equal_one():
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    bench = ((1, 3),)
    one = synthetic_panel(1500, p=24, dtype="f64", arm_split=True)
    mom1, _ = DS.irm_sens_panel(one, 5, benchmarks=bench)
    assert mom1.shape == (2, 14) and torch.isfinite(mom1).all() and mom1[0, 2] == 1500

    def body(comm):
        pan = synthetic_panel(1500, p=24, dtype="f64", arm_split=True, comm=comm)
        mom, _ = DS.irm_sens_panel(pan, 5, benchmarks=bench, comm=comm)
        return mom.numpy(), pan.n

    def fin(mom):
        return SensitivityResult.from_moments("t", mom[0], short=[(c, mom[1 + j])
                                                                  for j, c in enumerate(bench)])

    want = fin(mom1.numpy())
    out = run_simulated(2, body)
    assert sum(n for _, n in out) == 1500
    for mom, _ in out:
        print(np.abs(mom - mom1.numpy()).max())
        np.testing.assert_allclose(mom, mom1.numpy(), rtol=1e-12)
        assert np.array_equal(mom[:, [2, 3, 13]], mom1.numpy()[:, [2, 3, 13]])
        got = fin(mom)
        _close(got, want, rel=1e-12)
        for a, b in zip(got.benchmarks, want.benchmarks):
            for k in ("delta_theta", "theta_short", "sigma2_short", "nu2_short"):
                assert getattr(a, k) == pytest.approx(getattr(b, k), rel=1e-12, abs=1e-12), k


# ---------------------------------------------------------------- validation
def _tiny():
    rs = np.random.RandomState(0)
    X, Y = rs.randn(120, 4), rs.randn(120)
    return Y, (rs.rand(120) < 0.5).astype(float), X


@pytest.mark.parametrize("kw", [dict(cf_d=1.0), dict(cf_y=1.0), dict(cf_y=-0.1), dict(rho=1.5),
                                dict(rho=-1.01), dict(level=0.5), dict(level=1.0),
                                dict(benchmarks=[[0, 1, 2, 3]]), dict(benchmarks=[[1, 2, 1]]),
                                dict(benchmarks=[[4]]), dict(benchmarks=[[-1]]),
                                dict(benchmarks=[[0]] * 9)])
def test_bad_arguments_raise(kw):
    Y, W, X = _tiny()
    with pytest.raises(ValueError):
        DS.dml_irm_sensitivity(Y, W, X, device="cpu", **kw)
    with pytest.raises(ValueError):
        R.dml_irm_sensitivity(Y, W, X, **kw)


def test_nonpositive_plugins_raise():
    psi, b, c, y = _rows()
    with pytest.raises(NumericalError, match="nu2"):
        SensitivityResult.from_moments("t", _moments(psi, b, c - 2 * c.mean(), y))
    with pytest.raises(NumericalError, match="sigma2"):
        sens_bounds(_moments(psi, 0 * b, c, y), 0.03, 0.03)
    with pytest.raises(NumericalError):
        R.sensitivity_from_rows(psi, b, -np.abs(c))
    r = SensitivityResult.from_moments("t", _moments(psi, b, c, y))
    with pytest.raises(ValueError):
        r.bounds(0.1, 1.0)
    with pytest.raises(ValueError):
        r.bounds(0.1, 0.1, rho=2.0)


# ---------------------------------------------------------------- public surface
def test_api_backends(small):
    import ate_replication_causalml_amd as pkg
    from ate_replication_causalml_amd.config import RunConfig
    m = small
    c = pkg.ate_dml_irm_sensitivity(m.Y, m.W, m.X, cf_y=0.05, rho=0.8, null=0.02,
                                    run=RunConfig(backend="cpu"))
    r = pkg.ate_dml_irm_sensitivity(m.Y, m.W, m.X, cf_y=0.05, rho=0.8, null=0.02,
                                    run=RunConfig(backend="reference"))
    assert isinstance(c, pkg.SensitivityResult) and isinstance(r, pkg.SensitivityResult)
    assert c.method == r.method == "DML-IRM sensitivity (LASSO)"
    assert (c.scenario.cf_y, c.scenario.cf_d, c.scenario.rho, c.null) == (0.05, 0.03, 0.8, 0.02)
    _close(c, r)
    irm = pkg.ate_dml_irm(m.Y, m.W, m.X, run=RunConfig(backend="cpu"))
    assert (c.theta, c.se) == (irm.ate, irm.se)
    out = json.loads(c.to_json())
    assert out["rv"] == c.rv and len(out["moments"]) == 14


def test_cli_sensitivity_prints_finite_json(capsys):
    from ate_replication_causalml_amd import cli
    assert cli.main(["dml", "--model", "irm", "--sensitivity", "--n", "3000", "--p", "24",
                     "--dtype", "f64", "--cf-y", "0.05", "--rho", "0.9", "--benchmark-cols",
                     "0,1", "--benchmark-cols", "5"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for k in ("ate", "se", "sigma2", "nu2", "theta_lower", "theta_upper", "ci_lower", "ci_upper",
              "rv", "rva"):
        assert np.isfinite(out[k]), k
    assert out["ci_lower"] < out["theta_lower"] < out["ate"] < out["theta_upper"] < out["ci_upper"]
    assert (out["cf_y"], out["cf_d"], out["rho"]) == (0.05, 0.03, 0.9)
    assert [b["columns"] for b in out["benchmarks"]] == [[0, 1], [5]]
    assert all(0 <= b["cf_y"] <= 1 and 0 <= b["cf_d"] <= 1 for b in out["benchmarks"])
