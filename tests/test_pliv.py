"""CPU tests of DML-PLIV: the reference against a closed form from its own residuals, the
cpu backend against the reference, the moment layout, the Anderson-Rubin set, every refusal,
the data generator and the command line."""
import json
import math

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import RunConfig, ate_dml_pliv
from ate_replication_causalml_amd.data.dgp import make_pliv_data
from ate_replication_causalml_amd.estimators import pliv as DP
from ate_replication_causalml_amd.reference import estimators as E
from ate_replication_causalml_amd.result import (ArGridSet, ArSet, PlivLayout, PlivResult,
                                                 chi2_quantile, pliv_finish, pliv_layout)

N = 1500


@pytest.fixture(scope="module")
def data():
    return {q: make_pliv_data(N, 1991, q) for q in (1, 3)}


@pytest.fixture(scope="module")
def reference(data):
    return {q: E.dml_pliv_lasso(d.Y, d.D, d.Z, d.X) for q, d in data.items()}


def _closed_form(yr, dr, zr):
    """theta, SE, pi, F by the direct sums over v = z~ pi (not through the moment vector)."""
    n, q = zr.shape
    pi = np.linalg.solve(zr.T @ zr, zr.T @ dr)
    v = zr @ pi
    theta = (v @ yr) / (v @ dr)
    u = yr - theta * dr
    se = math.sqrt(((v * u) ** 2).sum()) / (v @ dr)
    F = ((v @ dr) / q) / ((dr @ dr - v @ dr) / (n - q))
    return theta, se, pi, F


@pytest.mark.parametrize("q", [1, 3])
def test_reference_is_the_closed_form_of_its_residuals(data, reference, q):
    d, r = data[q], reference[q]
    yr, dr, zr = E._pliv_residuals(d.Y, d.D, d.Z, d.X, 5, 1991, "min")
    theta, se, pi, F = _closed_form(yr, dr, zr)
    assert r.theta == pytest.approx(theta, rel=1e-12)
    assert r.se == pytest.approx(se, rel=1e-12)
    assert r.pi == pytest.approx(pi.tolist(), rel=1e-12)
    assert r.first_stage_F == pytest.approx(F, rel=1e-12)
    assert (r.lower_ci, r.upper_ci) == (r.theta - 1.96 * r.se, r.theta + 1.96 * r.se)
    dg = r.diagnostics
    assert dg["n"] == N and dg["n_instruments"] == q and dg["hipgraph"] is False
    assert dg["rmse_l"] == pytest.approx(math.sqrt(yr @ yr / N), rel=1e-12)
    assert dg["rmse_r"] == pytest.approx(math.sqrt(dr @ dr / N), rel=1e-12)
    assert not r.weak_instruments and not r.rank_deficient


def test_one_instrument_equal_to_the_treatment_is_plr(data):
    d = data[1]
    a = E.dml_pliv_lasso(d.Y, d.D, d.D, d.X)
    b = E.dml_plr_lasso(d.Y, d.D, d.X)
    assert a.pi == [1.0] or a.pi[0] == pytest.approx(1.0, rel=1e-14)
    assert a.theta == pytest.approx(b.ate, rel=1e-12) and a.se == pytest.approx(b.se, rel=1e-12)


@pytest.mark.parametrize("q", [1, 3])
def test_cpu_backend_vs_reference(data, reference, q):
    d, r = data[q], reference[q]
    c = ate_dml_pliv(d.Y, d.D, d.Z, d.X, run=RunConfig(backend="cpu"))
    via = ate_dml_pliv(d.Y, d.D, d.Z, d.X, run=RunConfig(backend="reference"))
    assert (via.theta, via.se, via.pi) == (r.theta, r.se, r.pi)
    for x, y in [(c.theta, r.theta), (c.se, r.se), (c.first_stage_F, r.first_stage_F)] + \
            list(zip(c.pi, r.pi)):
        assert x == pytest.approx(y, rel=1e-9, abs=1e-9)
    np.testing.assert_allclose(c.moments, r.moments, rtol=1e-9, atol=1e-9)
    assert c.moments[0] == N and len(c.moments) == pliv_layout(q).size


def test_clusters_cpu_vs_reference_and_singletons(data):
    d = data[3]
    cl = np.random.default_rng(5).permutation(np.arange(N) // 4)
    r = ate_dml_pliv(d.Y, d.D, d.Z, d.X, clusters=cl, run=RunConfig(backend="reference"))
    c = ate_dml_pliv(d.Y, d.D, d.Z, d.X, clusters=cl, run=RunConfig(backend="cpu"))
    for x, y in ((c.theta, r.theta), (c.se, r.se),
                 (c.diagnostics["se_unclustered"], r.diagnostics["se_unclustered"])):
        assert x == pytest.approx(y, rel=1e-9, abs=1e-9)
    for k in ("n_clusters", "max_cluster", "design_effect"):
        assert c.diagnostics[k] == r.diagnostics[k]
    assert c.diagnostics["max_cluster"] == 4 and c.se != c.diagnostics["se_unclustered"]
    # the cluster SE by hand from the reference's residuals on the cluster folds
    fid = E.cluster_fold_ids(cl, 5, 1991)
    yr, dr, zr = E._pliv_residuals(d.Y, d.D, d.Z, d.X, 5, 1991, "min", fid)
    theta, _, pi, _ = _closed_form(yr, dr, zr)
    v = zr @ pi
    t = np.bincount(cl, weights=v * (yr - theta * dr))
    assert r.se == pytest.approx(math.sqrt((t * t).sum()) / (v @ dr), rel=1e-12)
    # singleton clusters: the row-level folds and, with no J / (J - 1) factor, the same SE
    s = ate_dml_pliv(d.Y, d.D, d.Z, d.X, clusters=np.arange(N), run=RunConfig(backend="cpu"))
    u = ate_dml_pliv(d.Y, d.D, d.Z, d.X, run=RunConfig(backend="cpu"))
    assert s.theta == u.theta and s.diagnostics["se_unclustered"] == u.se
    assert s.se == pytest.approx(u.se, rel=1e-12)


@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_moment_layout_round_trips(q):
    lay = PlivLayout(q)
    assert lay.size == 4 + 2 * q + 2 * q * (q + 1) == (10, 20, 34, 52)[q - 1]
    assert len(lay.names()) == lay.size == len(set(lay.names()))
    rs = np.random.RandomState(q)
    zr, yr, dr = rs.randn(40, q), rs.randn(40), rs.randn(40)
    mom = E.pliv_moments_from_residuals(yr, dr, zr)
    u = lay.unpack(mom)
    assert lay.pack(**u) == mom
    assert u["n"] == 40 and u["szy"] == pytest.approx((zr.T @ yr).tolist())
    for i in range(q):
        for j in range(q):
            assert mom[lay.zz + lay.tri(i, j)] == pytest.approx(zr[:, i] @ zr[:, j])
            assert mom[lay.qyd + lay.tri(i, j)] == pytest.approx((zr[:, i] * zr[:, j] * yr) @ dr)
            assert u["qdd"][i][j] == u["qdd"][j][i]
    assert (lay.zy, lay.zd, lay.zz, lay.qyy) == (4, 4 + q, 4 + 2 * q, 4 + 2 * q + lay.T)
    theta, se, pi, _ = _closed_form(yr, dr, zr)
    fin = pliv_finish(mom)
    assert fin[:2] == pytest.approx([theta, se], rel=1e-10) and fin[3] == 0.0
    assert fin[4:] == pytest.approx(pi.tolist(), rel=1e-10)
    assert DP.pliv_finalize(torch.tensor(mom, dtype=torch.float64)).tolist() == fin
    with pytest.raises(ValueError):
        lay.unpack(mom[:-1])
    with pytest.raises(ValueError):
        PlivLayout(5)


def test_twin_moments_and_terms_on_a_host_panel(data):
    """The torch twin on a panel equals the moments of explicit residuals, with padding rows
    left out; the terms sum to pi' S z~y~ and pi' S z~d~."""
    d = data[3]
    rs = np.random.RandomState(2)
    fid = rs.randint(0, 3, N)
    pan = DP._build(d.Y, d.D, d.Z, d.X, fid, "f64", "cpu")
    p = d.X.shape[1]
    coef = torch.from_numpy(rs.randn(3, 5, p + 1) * 0.1)
    mom, ab = DP.pliv_moments_twin(pan, coef, 3)
    c = coef.numpy()[fid]
    targets = np.column_stack([d.Y, d.D, d.Z])
    res = targets - (c[:, :, 0] + np.einsum("nrp,np->nr", c[:, :, 1:], d.X))
    want = E.pliv_moments_from_residuals(res[:, 0], res[:, 1], res[:, 2:])
    np.testing.assert_allclose(mom.numpy(), want, rtol=1e-11)
    assert (ab >= mom.abs()).all() and ab[0] == mom[0] == N and pan.ld > N
    assert torch.equal(DP.pliv_moments(pan, coef, 3), mom)
    mom2, fin = DP.pliv_moments(pan, coef, 3, finish=True)
    a, b = DP.pliv_terms(pan, coef, 3, fin[4:])
    lay = pliv_layout(3)
    assert a.numel() == pan.ld and not a[pan.valid() == 0].any()
    assert a.sum().item() == pytest.approx((fin[4:] * mom[lay.zy:lay.zy + 3]).sum().item(), rel=1e-10)
    assert b.sum().item() == pytest.approx(fin[2].item(), rel=1e-10)
    with pytest.raises(ValueError, match="coef must be"):
        DP.pliv_moments(pan, coef[:, :4], 3)


def test_anderson_rubin_one_instrument(reference):
    r = reference[1]
    crit = chi2_quantile(0.95, 1)
    assert crit == pytest.approx(3.841458820694124, rel=1e-6)
    assert chi2_quantile(0.95, 3) == pytest.approx(7.814727903251179, rel=1e-9)
    ar = r.anderson_rubin(0.95)
    assert isinstance(ar, ArSet) and ar.kind == "interval"
    assert r.theta in ar and ar.lower < r.theta < ar.upper
    assert r.ar_stat(r.theta) < crit and r.ar_stat(r.theta) == pytest.approx(0.0, abs=1e-12)
    # the end points sit on the critical value
    assert r.ar_stat(ar.lower) == pytest.approx(crit, rel=1e-8)
    assert r.ar_stat(ar.upper) == pytest.approx(crit, rel=1e-8)
    assert r.anderson_rubin(0.5).upper < ar.upper
    with pytest.raises(ValueError):
        r.anderson_rubin(1.0)


def test_anderson_rubin_tends_to_the_wald_interval():
    gaps = []
    for n in (1000, 16000):
        d = make_pliv_data(n, 7, 1)
        r = E.dml_pliv_lasso(d.Y, d.D, d.Z, d.X, folds=3)
        ar = r.anderson_rubin()
        gaps.append(max(abs(ar.lower - r.lower_ci), abs(ar.upper - r.upper_ci)) / r.se)
    print("AR vs Wald end points, in SE:", gaps)
    assert gaps[1] < gaps[0] and gaps[1] < 0.05


def _moments_q1(sy, sd, qyy, qyd, qdd):
    return pliv_layout(1).pack(100, 50.0, 10.0, 60.0, [sy], [sd], [[40.0]], [[qyy]], [[qyd]],
                               [[qdd]])


def test_anderson_rubin_unbounded_cases():
    crit = chi2_quantile(0.95, 1)
    # a weak first stage: A = sd^2 - c Qdd < 0
    weak = PlivResult.from_moments("weak", _moments_q1(3.0, 1.0, 30.0, 5.0, 20.0))
    ar = weak.anderson_rubin()
    A = 1.0 - crit * 20.0
    B = -2 * 3.0 + 2 * crit * 5.0
    C = 9.0 - crit * 30.0
    assert A < 0 and B * B - 4 * A * C < 0 and ar.kind == "all" and 1e9 in ar and -1e9 in ar
    rays = PlivResult.from_moments("rays", _moments_q1(30.0, 1.0, 30.0, 5.0, 20.0))
    ar = rays.anderson_rubin()
    assert ar.kind == "two_rays" and ar.lower < ar.upper
    assert rays.theta in ar and 0.5 * (ar.lower + ar.upper) not in ar and 1e9 in ar and -1e9 in ar
    for t in (ar.lower, ar.upper):
        assert rays.ar_stat(t) == pytest.approx(crit, rel=1e-9)
    # A = 0 exactly (S z~d~ = 0 and Q_dd = 0: the treatment residual vanishes wherever the
    # instrument's does not): B theta + C <= 0 is a single ray, or the whole line at B = 0
    ray = PlivResult.from_moments("ray", _moments_q1(3.0, 0.0, 30.0, 5.0, 0.0)).anderson_rubin()
    # B > 0: theta <= -C / B, the ray (-inf, lower]; B < 0: [upper, inf)
    assert ray.kind == "two_rays" and math.isinf(ray.upper) and not math.isinf(ray.lower)
    assert ray.lower == pytest.approx(-(9.0 - crit * 30.0) / (2 * crit * 5.0), rel=1e-14)
    assert -1e9 in ray and 1e9 not in ray
    ray = PlivResult.from_moments("ray", _moments_q1(3.0, 0.0, 30.0, -5.0, 0.0)).anderson_rubin()
    assert ray.kind == "two_rays" and math.isinf(ray.lower) and 1e9 in ray and -1e9 not in ray
    whole = PlivResult.from_moments("all", _moments_q1(3.0, 0.0, 30.0, 0.0, 0.0))
    assert whole.anderson_rubin().kind == "all"


def test_anderson_rubin_grid(reference):
    r = reference[3]
    crit = chi2_quantile(0.95, 3)
    assert r.ar_stat(r.theta) < crit
    ar = r.anderson_rubin()
    assert isinstance(ar, ArGridSet) and ar.kind == "interval" and not ar.open_ended
    assert r.theta in ar and ar.lower < r.theta < ar.upper and len(ar.grid) == 401
    assert r.theta + 9 * r.se not in ar
    tight = r.anderson_rubin(grid=np.linspace(r.theta - r.se, r.theta + r.se, 11))
    assert tight.open_ended and all(tight.inside)
    none = r.anderson_rubin(grid=[r.theta + 50 * r.se])
    assert none.kind == "empty" and r.theta not in none
    out = json.loads(r.to_json())
    assert out["anderson_rubin"]["kind"] == "interval" and "grid" not in out["anderson_rubin"]
    assert out["pi"] == r.pi and out["diagnostics"]["n"] == N
    assert "first-stage F" in r.table() and "Anderson-Rubin" in r.table()


def test_refusals_before_any_work(data, monkeypatch):
    d = data[1]
    n = d.n
    # nothing below may reach a panel or a fit
    monkeypatch.setattr(DP, "build_panel", lambda *a, **k: pytest.fail("built a panel"))
    monkeypatch.setattr(E, "_pliv_residuals", lambda *a, **k: pytest.fail("fitted"))
    rs = np.random.RandomState(0)
    for run in (RunConfig(backend="cpu"), RunConfig(backend="reference")):
        call = lambda Z=d.Z, X=d.X, **kw: ate_dml_pliv(d.Y, d.D, Z, X, run=run, **kw)
        with pytest.raises(ValueError, match="at most 4 instruments"):
            call(rs.randn(n, 5))
        with pytest.raises(ValueError, match="constant"):
            call(np.column_stack([d.Z[:, 0], np.full(n, 2.0)]))
        with pytest.raises(ValueError, match="finite"):
            call(np.where(np.arange(n) == 3, np.nan, d.Z[:, 0]))
        with pytest.raises(ValueError, match=r"\(n,\) or \(n, q\)"):
            call(d.Z[:-1])
        with pytest.raises(ValueError, match="row-sharded"):
            call(dist=object())
        with pytest.raises(ValueError, match="repeats"):
            call(repeats=3)
        with pytest.raises(ValueError, match="logit"):
            call(nuisance="logit")
        for form in ("gate", "cate", "policy", "sensitivity"):
            with pytest.raises(ValueError, match=form):
                call(form=form)
        with pytest.raises(ValueError, match="LDS"):
            call(X=np.zeros((n, 4000)))
    # the LDS bound itself: (2 + q)(p + 1) esz + 4 p <= 64 KB - 8 KB
    for p_ok, q, dt in ((2047, 1, "f64"), (2047, 4, "bf16"), (1101, 4, "f64")):
        DP.check_lds(p_ok, q, dt)                       # 28 p + 24, 28 p + 24, 52 p + 48 bytes
        with pytest.raises(ValueError, match="LDS"):
            DP.check_lds(p_ok + 1, q, dt)
    with pytest.raises(ValueError, match="clusters"):
        ate_dml_pliv(d.Y, d.D, d.Z, d.X, clusters=np.zeros(n), run=RunConfig(backend="cpu"))


def test_collinear_instruments_raise_after_the_call(data):
    d = data[1]
    dup = np.column_stack([d.Z[:, 0], d.Z[:, 0]])
    for backend in ("cpu", "reference"):
        with pytest.raises(ValueError, match="collinear"):
            ate_dml_pliv(d.Y, d.D, dup, d.X, run=RunConfig(backend=backend))
    fin = pliv_finish(E.pliv_moments_from_residuals(d.Y, d.D, dup))
    assert fin[3] == 1.0 and all(math.isnan(v) for v in fin[:3] + fin[4:])
    zero = pliv_finish(E.pliv_moments_from_residuals(d.Y, d.D, np.zeros((N, 1))))
    assert zero[3] == 1.0
    r = PlivResult.from_moments("x", E.pliv_moments_from_residuals(d.Y, d.D, dup))
    assert r.rank_deficient and math.isnan(r.theta) and "Anderson" not in r.table()
    json.loads(r.to_json())


def test_dgp_pliv_recovers_the_effect_where_plr_does_not():
    """The constants of make_pliv_data: at n = 20,000, fixed seeds, the reference alone, PLIV
    is within 3 SE of the truth and PLR more than 5 of its SEs away (an unobserved U)."""
    d = make_pliv_data(20_000, 1991, 2)
    assert d.Z.shape == (20_000, 2) and d.theta_true == 0.5
    r = E.dml_pliv_lasso(d.Y, d.D, d.Z, d.X)
    plr = E.dml_plr_lasso(d.Y, d.D, d.X)
    print("pliv", r.theta, r.se, "plr", plr.ate, plr.se, "F", r.first_stage_F)
    assert abs(r.theta - d.theta_true) < 3 * r.se
    assert abs(plr.ate - d.theta_true) > 5 * plr.se
    assert r.first_stage_F > 100


def test_dgp_draws():
    a, b = make_pliv_data(500, 3, 4), make_pliv_data(500, 3, 4)
    assert np.array_equal(a.Y, b.Y) and np.array_equal(a.Z, b.Z) and a.Z.shape == (500, 4)
    assert not np.array_equal(a.Y, make_pliv_data(500, 4, 4).Y)
    one = make_pliv_data(500, 3, 1)
    assert np.array_equal(one.Z[:, 0], a.Z[:, 0])           # an instrument is its own stream
    big = make_pliv_data(4000, 3, 2)
    yob = big.X[:, big.names.index("yob")]
    assert np.corrcoef(big.Z[:, 0], yob)[0, 1] > 0.2        # the instruments depend on X
    assert np.corrcoef(big.Z[:, 0], big.D)[0, 1] > 0.2
    assert abs(np.corrcoef(make_pliv_data(4000, 3, 1, strength=0.0).Z[:, 0]
                           - 0.4 * yob, big.D - 0.5 * yob)[0, 1]) < 0.4
    with pytest.raises(ValueError):
        make_pliv_data(100, 1, 5)


def test_cli_pliv(capsys):
    from ate_replication_causalml_amd import cli
    base = ["pliv", "--n", "1500", "--instruments", "2", "--backend", "cpu"]
    assert cli.main(base) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert all(np.isfinite(out[k]) for k in ("theta", "se", "lower_ci", "upper_ci", "theta_true"))
    assert out["diagnostics"]["n"] == 1500 and len(out["pi"]) == 2
    assert np.isfinite(out["plr"]["estimate"]) and out["plr"]["estimate"] > out["theta"] + 0.3
    assert cli.main(base + ["--cluster-size", "3", "--folds", "3"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["diagnostics"]["n_clusters"] == 500 and out["diagnostics"]["max_cluster"] == 3
    with pytest.raises(SystemExit):
        cli.main(["pliv", "--n", "300", "--instruments", "5", "--backend", "cpu"])
