"""CATE curves of DML-IRM along one covariate with a uniform multiplier-bootstrap band
(estimators/cate.py) on the CPU path: the B-spline basis (recursive reference, span-local
torch twin, scipy), degree 0 against the group estimator, the device orchestration (torch
twins) against the row-by-row float64 reference twin, the overall ATE against ate_dml_irm,
calibration of the critical value, row sharding, input validation and the public surface."""
import json

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
from ate_replication_causalml_amd.estimators import cate as DC
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.parallel.comm import run_simulated
from ate_replication_causalml_amd.reference import estimators as R

DF, DEGREE = 8, 3


@pytest.fixture(scope="module")
def fits(tutorial):
    """(device orchestration on the CPU, reference twin) on df_mod along X[:, 0], once."""
    _, m, _ = tutorial
    x = m.X[:, 0]
    return (DC.dml_irm_cate_lasso(m.Y, m.W, m.X, x, df=DF, degree=DEGREE, device="cpu",
                                  keep_boot=True),
            R.dml_irm_cate(m.Y, m.W, m.X, x, df=DF, degree=DEGREE, keep_boot=True))


# ---------------------------------------------------------------- basis
def _points(knots, q, rs):
    d = len(knots) - q - 1
    inner = knots[q + 1:d]
    return np.concatenate([rs.uniform(knots[0], knots[-1], 200), inner, [knots[0], knots[-1]]])


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_basis_twins_agree(q):
    rs = np.random.RandomState(q)
    d = q + 5                                              # 4 interior knots, 5 spans
    t = np.concatenate([[-2.0] * (q + 1), np.sort(rs.uniform(-1.5, 2.5, 4)), [3.0] * (q + 1)])
    x = _points(t, q, rs)
    ref = R.bspline_design(x, t, q)
    twin = DC.bspline_basis(x, t, q).numpy()
    assert ref.shape == twin.shape == (len(x), d)
    np.testing.assert_allclose(twin, ref, rtol=0, atol=1e-13)
    np.testing.assert_allclose(ref.sum(axis=1), 1.0, rtol=0, atol=1e-13)      # partition of unity
    np.testing.assert_allclose(twin.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    assert ref.min() >= 0 and twin.min() >= 0
    # generic points: exactly degree + 1 non-zero values, in the span's slots
    sp, N = DC.basis_local(torch.from_numpy(x[:200]), torch.from_numpy(t), q)
    for B in (ref, twin):
        assert np.all((B[:200] != 0).sum(axis=1) == q + 1)
        first = (B[:200] != 0).argmax(axis=1)
        assert np.array_equal(first, sp.numpy())
    assert N.shape == (200, q + 1)
    # x on interior knot k goes to the right-hand span (k + 1); x = max to the last span
    sp_k, _ = DC.basis_local(torch.from_numpy(x[200:204]), torch.from_numpy(t), q)
    assert sp_k.tolist() == [1, 2, 3, 4]
    for B in (ref, twin):
        for k in range(4):
            nz = np.flatnonzero(B[200 + k])
            assert nz.min() >= k + 1 and nz.max() <= k + 1 + q
        assert B[-1, d - 1] == 1.0 and np.count_nonzero(B[-1]) == 1           # max
        assert B[-2, 0] == 1.0 and np.count_nonzero(B[-2]) == 1               # min
    sp_e, _ = DC.basis_local(torch.from_numpy(x[-2:]), torch.from_numpy(t), q)
    assert sp_e.tolist() == [0, 4]


@pytest.mark.parametrize("q", [1, 2, 3])
def test_basis_matches_scipy(q):
    interpolate = pytest.importorskip("scipy.interpolate")
    if not hasattr(interpolate.BSpline, "design_matrix"):
        pytest.skip("scipy without BSpline.design_matrix")
    rs = np.random.RandomState(10 + q)
    t = np.concatenate([[-2.0] * (q + 1), np.sort(rs.uniform(-1.5, 2.5, 4)), [3.0] * (q + 1)])
    x = _points(t, q, rs)
    sc = interpolate.BSpline.design_matrix(x, t, q).toarray()
    np.testing.assert_allclose(R.bspline_design(x, t, q), sc, rtol=0, atol=1e-13)
    np.testing.assert_allclose(DC.bspline_basis(x, t, q).numpy(), sc, rtol=0, atol=1e-13)


# ---------------------------------------------------------------- degree 0
def test_degree0_is_the_group_estimator():
    rs = np.random.RandomState(3)
    n, G, B, seed = 1500, 4, 300, 1991
    x = rs.randn(n)
    psi = rs.standard_t(5, n) * 3 + 0.1 + x
    knots = DC.quantile_knots(x, G, 0)                     # min | quantile cuts | max
    assert len(knots) == G + 1
    codes = np.digitize(x, knots[1:-1])
    grid = 0.5 * (knots[:-1] + knots[1:])                  # one point per cell
    ng, theta, se, crit, A, Z = R.gate_from_scores(psi, codes, G, B, 0.95, seed)
    r = R.cate_from_scores(psi, x, knots, 0, grid, B, 0.95, seed)
    assert np.array_equal(r["span_counts"], ng)
    np.testing.assert_allclose(r["beta"], theta, rtol=1e-12)
    np.testing.assert_allclose(r["cate"], theta, rtol=1e-12)
    np.testing.assert_allclose(r["se"], se * np.sqrt((ng - 1) / ng), rtol=1e-12)   # HC0
    np.testing.assert_allclose(r["T"], A - theta * Z, rtol=0, atol=1e-12 * np.abs(A).max())
    # the same statistic up to the HC0 factor of every group: the same critical value when
    # the groups have the same size, and the device twins give the same numbers
    tp, tx, ti = torch.from_numpy(psi), torch.from_numpy(x), torch.arange(n)
    tk = torch.from_numpy(knots)
    mom = DC.cate_moments(tp, tx, ti, tk, 0)
    beta = DC.cate_beta(mom, G, 0)
    boot = DC.cate_boot(tp, tx, ti, tk, 0, beta, B, seed)
    np.testing.assert_allclose(beta.numpy(), theta, rtol=1e-12)
    _, T = DC.split_boot(boot, G, B)
    np.testing.assert_allclose(T.numpy(), A - theta * Z, rtol=0, atol=1e-12 * np.abs(A).max())
    fin = DC.cate_finalize(mom, boot, beta, DC.bspline_basis(grid, knots, 0), G, 0, B, 0.95)
    cate, s, c, o_ate, o_se, nn, b, om = DC.read_fin(fin.numpy(), G, G)
    np.testing.assert_allclose(s, r["se"], rtol=1e-12)
    assert c == pytest.approx(r["crit"], rel=1e-12) and nn == n
    assert o_ate == pytest.approx(psi.mean(), rel=1e-12)
    assert o_se == pytest.approx(psi.std(ddof=1) / np.sqrt(n), rel=1e-12)


# ---------------------------------------------------------------- twin
def test_matches_reference_twin(fits):
    dev, ref = fits
    assert dev.grid == ref.grid and dev.knots == ref.knots and len(dev.grid) == 100
    assert dev.degree == DEGREE and dev.df == DF and len(dev.knots) == DF + DEGREE + 1
    assert dev.diagnostics["span_counts"] == ref.diagnostics["span_counts"]
    assert sum(dev.diagnostics["span_counts"]) == dev.overall.diagnostics["n"] > 1000
    print("cond(M)", np.linalg.cond(ref.boot["M"]))
    np.testing.assert_allclose(dev.cate, ref.cate, rtol=1e-9)
    np.testing.assert_allclose(dev.se, ref.se, rtol=1e-9)
    np.testing.assert_allclose(dev.coef, ref.coef, rtol=1e-9)
    assert dev.crit == pytest.approx(ref.crit, rel=1e-9)
    scale = np.abs(ref.boot["T"]).max()
    assert dev.boot["T"].shape == (999, DF) and scale > 0
    np.testing.assert_allclose(dev.boot["T"], ref.boot["T"], rtol=0, atol=1e-12 * scale)
    assert dev.n_boot == 999 and dev.level == 0.95
    # a uniform band is wider than the pointwise one
    assert 1.96 < dev.crit < 4
    for j in range(len(dev.grid)):
        assert dev.lower_joint[j] < dev.lower_ci[j] < dev.cate[j] < dev.upper_ci[j] < dev.upper_joint[j]
        assert dev.upper_joint[j] == pytest.approx(dev.cate[j] + dev.crit * dev.se[j], rel=1e-14)
    # the normal equations: the residual is orthogonal to the basis
    M, T = dev.boot["M"], dev.boot["T"]
    assert np.allclose(M, M.T, rtol=0, atol=0) and np.all(np.linalg.eigvalsh(M) > 0)
    assert np.allclose(M.sum(), dev.overall.diagnostics["n"], rtol=1e-12)     # partition of unity


def test_overall_equals_ate_dml_irm(tutorial, fits):
    _, m, _ = tutorial
    dev, ref = fits
    one = DI.dml_irm_lasso(m.Y, m.W, m.X, device="cpu")
    assert dev.overall.ate == pytest.approx(one.ate, rel=1e-12)
    assert dev.overall.se == pytest.approx(one.se, rel=1e-12)
    assert ref.overall.ate == pytest.approx(one.ate, rel=1e-9)        # the bound of the IRM twin
    assert dev.overall.diagnostics["n"] == len(m.Y)


# ---------------------------------------------------------------- calibration
def _crit(psi, x, knots, q, grid, B, seed):
    n = len(psi)
    d = len(knots) - q - 1
    tp, tx, ti, tk = torch.from_numpy(psi), torch.from_numpy(x), torch.arange(n), torch.from_numpy(knots)
    mom = DC.cate_moments(tp, tx, ti, tk, q)
    beta = DC.cate_beta(mom, d, q)
    boot = DC.cate_boot(tp, tx, ti, tk, q, beta, B, seed)
    fin = DC.cate_finalize(mom, boot, beta, DC.bspline_basis(grid, knots, q), d, q, B, 0.95)
    crit = DC.read_fin(fin.numpy(), d, len(grid))[2]
    ref = R.cate_from_scores(psi, x, knots, q, grid, B, 0.95, seed)
    assert crit == pytest.approx(ref["crit"], rel=1e-9)
    return crit


@pytest.mark.parametrize("seed", [1991, 7, 12345])
def test_crit_is_calibrated(seed):
    """Heavy-tailed scores independent of x: at one point the statistic is one normal, whose
    95% point is 1.96; the maximum over a 50-point grid is larger."""
    rs = np.random.RandomState(3)
    n, B = 1500, 2048
    x = rs.randn(n)
    psi = rs.standard_t(5, n) * 3 + 0.1
    knots = DC.quantile_knots(x, 5, 3)
    c1 = _crit(psi, x, knots, 3, np.array([0.2]), B, seed)
    c50 = _crit(psi, x, knots, 3, DC.default_grid(x, 50), B, seed)
    print("seed", seed, "crit at 1 point", c1, "50 points", c50)
    assert abs(c1 - 1.96) < 0.15
    assert c50 > c1


# ---------------------------------------------------------------- row sharding
def test_row_sharded_matches_single_rank():
    q, B = 3, 200
    knots = DC.clamped_knots(-6.0, [-0.5, 0.0, 0.6], 6.0, q)
    d = knots.numel() - q - 1
    grid = np.linspace(-1.5, 1.5, 7)

    def run(comm):
        pan = synthetic_panel(1500, p=24, folds=3, dtype="f64", arm_split=True, comm=comm)
        x = pan.col("x0").double()
        fin, mom, boot, _ = DC.irm_cate_panel(pan, x, knots, q, grid, 3, n_boot=B, comm=comm)
        return fin.numpy(), mom.numpy(), pan.n

    fin1, mom1, n1 = run(None)
    cate1, se1, crit1, _, _, nn1, beta1, _ = DC.read_fin(fin1, d, len(grid))
    cnt1 = mom1[3:3 + d - q]
    assert n1 == 1500 and nn1 == 1500 and cnt1.sum() == 1500 and cnt1.min() > 50
    assert np.isfinite(fin1).all()
    for world in (2, 3):
        out = run_simulated(world, run)
        assert sum(n for _, _, n in out) == 1500
        for fin, mom, _ in out:
            cate, se, crit, _, _, nn, beta, _ = DC.read_fin(fin, d, len(grid))
            assert np.array_equal(mom[3:3 + d - q], cnt1) and nn == 1500       # span counts: exact
            print("world", world, "max rel", np.abs(fin / fin1 - 1).max())
            np.testing.assert_allclose(beta, beta1, rtol=1e-12)
            np.testing.assert_allclose(se, se1, rtol=1e-12)
            assert crit == pytest.approx(crit1, rel=1e-12)


def test_estimator_sharded_shares_knots_and_grid():
    """``dist``: every rank gathers the covariate, so all agree on the knots, the grid and
    the (global) span counts, and the curve is that of the single-rank call."""
    from ate_replication_causalml_amd.parallel.dist import DistContext
    rs = np.random.RandomState(11)
    n = 900
    X = rs.randn(n, 4)
    W = (rs.rand(n) < 0.5).astype(float)
    Y = X[:, 1] + (0.5 + 0.3 * X[:, 0]) * W + rs.randn(n)
    kw = dict(df=6, degree=2, n_boot=100, folds=3, device="cpu")
    one = DC.dml_irm_cate_lasso(Y, W, X, 0, **kw)

    def body(comm):
        dist = DistContext.for_rank(comm, n)
        return DC.dml_irm_cate_lasso(dist.local(Y), dist.local(W), dist.local(X), 0, dist=dist,
                                     **kw)

    for r in run_simulated(2, body):
        assert r.knots == one.knots and r.grid == one.grid
        assert r.diagnostics["span_counts"] == one.diagnostics["span_counts"]
        assert r.overall.diagnostics["n"] == n
        np.testing.assert_allclose(r.cate, one.cate, rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(r.se, one.se, rtol=1e-7)
        assert r.crit == pytest.approx(one.crit, rel=1e-7)


# ---------------------------------------------------------------- validation
def test_value_errors():
    rs = np.random.RandomState(0)
    n = 400
    X, Y = rs.randn(n, 3), rs.randn(n)
    X[:, 2] = rs.randint(0, 3, n)                           # too few distinct values for knots
    W = (rs.rand(n) < 0.5).astype(float)
    lo, hi = X[:, 0].min(), X[:, 0].max()
    for fn, kw in ((DC.dml_irm_cate_lasso, dict(device="cpu")), (R.dml_irm_cate, {})):
        for df, degree in ((3, 3), (33, 3), (4.5, 3)):
            with pytest.raises(ValueError, match="df must be"):
                fn(Y, W, X, 0, df=df, degree=degree, **kw)
        for degree in (-1, 4, 1.5):
            with pytest.raises(ValueError, match="degree must be"):
                fn(Y, W, X, 0, df=8, degree=degree, **kw)
        with pytest.raises(ValueError, match="degree must be"):
            fn(Y, W, X, 0, degree=1.5, knots=[lo, lo, 0.0, 0.5, hi, hi], **kw)
        with pytest.raises(ValueError, match="inside"):
            fn(Y, W, X, 0, grid=[0.0, hi + 1e-9], **kw)
        with pytest.raises(ValueError, match="inside"):
            fn(Y, W, X, 0, grid=[lo - 1e-9], **kw)
        with pytest.raises(ValueError, match="512 points"):
            fn(Y, W, X, 0, grid=np.linspace(-1, 1, 513), **kw)
        with pytest.raises(ValueError, match="strictly increasing"):
            fn(Y, W, X, 2, df=8, **kw)                      # quantile knots of a 3-valued column
        with pytest.raises(ValueError, match="strictly increasing"):
            fn(Y, W, X, 0, degree=1, knots=[lo, lo, 0.5, 0.5, hi, hi], **kw)
        with pytest.raises(ValueError, match="clamped"):
            fn(Y, W, X, 0, degree=1, knots=[lo, lo - 1, 0.0, 0.5, hi, hi], **kw)
        with pytest.raises(ValueError, match="at least 2"):
            # a span between two adjacent order statistics holds one row
            xs = np.sort(X[:, 0])
            fn(Y, W, X, 0, degree=1, knots=[lo, lo, xs[10], xs[11], hi, hi], **kw)
        for bad in (0, 4097, 10.5):
            with pytest.raises(ValueError, match="n_boot"):
                fn(Y, W, X, 0, n_boot=bad, **kw)
        with pytest.raises(ValueError, match="level"):
            fn(Y, W, X, 0, level=1.0, **kw)
        with pytest.raises(ValueError, match="binary"):
            fn(Y, W + 0.5, X, 0, **kw)
        with pytest.raises(ValueError, match="by must"):
            fn(Y, W, X, 3, **kw)
        with pytest.raises(ValueError, match="by must"):
            fn(Y, W, X, X[:-1, 0], **kw)
    z = torch.zeros(8, dtype=torch.float64)
    kn = DC.clamped_knots(0.0, [], 1.0, 1)
    with pytest.raises(ValueError):
        DC.cate_moments(z, z[:7], torch.arange(8), kn, 1)
    with pytest.raises(ValueError):
        DC.cate_boot(z, z, torch.arange(8), kn, 1, torch.zeros(3, dtype=torch.float64), 10, 1)
    with pytest.raises(ValueError):
        DC.cate_boot(z, z, torch.arange(8), kn, 1, torch.zeros(2, dtype=torch.float64), 5000, 1)
    pan = synthetic_panel(600, p=24, folds=3, dtype="f64", arm_split=True)
    with pytest.raises(ValueError, match="df must be"):
        DC.spline_knots(pan, 0, 2, 3)


# ---------------------------------------------------------------- public surface
def test_spline_knots_are_the_quantile_edges():
    from ate_replication_causalml_amd.estimators.gate import quantile_groups
    pan = synthetic_panel(900, p=24, folds=3, dtype="f64", arm_split=True)
    t = DC.spline_knots(pan, 1, 7, 3)
    _, edges = quantile_groups(pan, 1, 4)
    x = pan.col("x1").double()[pan.row_index >= 0]
    assert t.shape == (11,) and torch.equal(t[4:7], edges)
    assert torch.all(t[:4] == x.min()) and torch.all(t[7:] == x.max())
    assert np.array_equal(t.numpy(), DC.quantile_knots(x.numpy(), 7, 3))


def test_api_backends_and_result(tutorial, fits):
    import ate_replication_causalml_amd as pkg
    from ate_replication_causalml_amd.config import RunConfig
    _, m, _ = tutorial
    dev, ref = fits
    grid = [-1.0, 0.0, 0.5]
    r = pkg.ate_dml_irm_cate(m.Y, m.W, m.X, 0, df=DF, degree=DEGREE, grid=grid,
                             run=RunConfig(backend="reference"))
    assert isinstance(r, pkg.CateResult) and r.grid == grid and r.coef == ref.coef
    c = pkg.ate_dml_irm_cate(m.Y, m.W, m.X, 0, df=DF, degree=DEGREE, grid=grid,
                             run=RunConfig(backend="cpu"))
    assert c.diagnostics["hipgraph"] is False and c.coef == dev.coef and c.knots == dev.knots
    np.testing.assert_allclose(c.cate, r.cate, rtol=1e-9)
    # predict: the curve and its SE at any point, from coef and cov alone
    pc, ps = dev.predict(dev.grid)
    np.testing.assert_allclose(pc, dev.cate, rtol=1e-12)
    np.testing.assert_allclose(ps, dev.se, rtol=1e-10)
    pc, ps = dev.predict(grid)
    np.testing.assert_allclose(pc, c.cate, rtol=1e-12)
    np.testing.assert_allclose(ps, c.se, rtol=1e-10)
    with pytest.raises(ValueError):
        dev.predict([dev.knots[-1] + 1.0])
    rows = c.rows()
    assert len(rows) == 3 and set(rows[0]) == {"x", "CATE", "se", "lower_ci", "upper_ci",
                                               "lower_joint", "upper_joint"}
    d = json.loads(c.to_json())
    assert d["crit"] == c.crit and len(d["curve"]) == 3 and d["overall"]["ate"] == c.overall.ate
    assert d["coef"] == c.coef and d["knots"] == c.knots and d["degree"] == DEGREE
    assert np.asarray(d["cov"]).shape == (DF, DF)
    assert len(c.table().splitlines()) == 6


def test_cli_cate_prints_finite_json(capsys):
    from ate_replication_causalml_amd import cli
    assert cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64",
                     "--cate-col", "0", "--cate-df", "6", "--cate-degree", "2", "--cate-grid", "9",
                     "--boot", "300"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["n_boot"] == 300 and len(out["curve"]) == 9 and len(out["knots"]) == 9
    assert out["n"] == 3000 and out["degree"] == 2 and len(out["coef"]) == 6
    for g in out["curve"]:
        assert all(np.isfinite(v) for v in g.values()) and g["se"] > 0
        assert g["lower_joint"] < g["lower_ci"] < g["upper_ci"] < g["upper_joint"]
    assert np.isfinite([out["crit"], out["ate"], out["se"]]).all() and out["crit"] > 1.96
