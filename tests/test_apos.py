"""CPU tests of DML-APOS (estimators/apos.py): the mean potential outcomes of a multi-valued
treatment against the row-by-row reference twin, the two-level case against DML-IRM, the
covariance, the simultaneous band, the grouping of the path problems into launches, and what
the estimator refuses. The GPU side is tests/test_gpu_apos.py."""
import json
import math

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import ate_dml_apos
from ate_replication_causalml_amd.config import RunConfig
from ate_replication_causalml_amd.data.dgp import make_multiarm_data
from ate_replication_causalml_amd.estimators import apos as DA
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.reference import estimators as E
from ate_replication_causalml_amd.result import (ApoResult, apo_layout, band_crit, contrast_cov,
                                                 normal_quantile)

# the bound test_gpu_irm uses between an estimator and its row-by-row twin
TOL = dict(abs=1e-6, rel=1e-6)
VALUES = (0.0, 2.0, 5.0)          # original treatment values: not the level codes


@pytest.fixture(scope="module")
def three(tutorial):
    """The fixture's rows with a three-valued D (the arms of make_multiarm_data, recoded to
    VALUES), K = 3: (Y, D, X, the estimator's result, the reference twin's with its scores)."""
    _, m, _ = tutorial
    arm = make_multiarm_data(len(m.Y), 1991, levels=3).D.astype(np.int64)
    D = np.asarray(VALUES)[arm]
    a = DA.dml_apos_lasso(m.Y, D, m.X, folds=3, device="cpu")
    b = E.dml_apos_lasso(m.Y, D, m.X, folds=3, keep_scores=True)
    return m.Y, D, m.X, a, b


def test_layout_sizes():
    assert apo_layout(2).size == 14 and apo_layout(8).size == 77
    for L in range(2, 9):
        lay = apo_layout(L)
        idx = [lay.tri(c, d) for c in range(L) for d in range(c, L)]
        assert idx == list(range(lay.cross, lay.level)) and len(lay.names()) == lay.size
        assert lay.tri(1, 0) == lay.tri(0, 1)
    for L in (1, 9):
        with pytest.raises(ValueError):
            apo_layout(L)


def test_estimator_vs_reference_twin(three):
    _, _, _, a, b = three
    assert a.levels == list(VALUES) == b.levels and a.reference == 0.0
    for x, y in zip(a.apo, b.apo):
        print("apo", x.ate, y.ate, "se", x.se, y.se)
        assert x.ate == pytest.approx(y.ate, **TOL) and x.se == pytest.approx(y.se, **TOL)
    for ref in VALUES:
        for x, y in zip(a.contrasts(ref), b.contrasts(ref)):
            assert (x.level, x.reference) == (y.level, y.reference)
            assert x.effect == pytest.approx(y.effect, **TOL) and x.se == pytest.approx(y.se, **TOL)
    for c in range(3):
        for d in range(3):
            assert a.cov[c][d] == pytest.approx(b.cov[c][d], **TOL)
    for k in ("n", "n_c", "n_clipped_c"):
        assert a.diagnostics[k] == b.diagnostics[k], k
    for k in ("rmse_g_c", "ipw_c"):
        assert a.diagnostics[k] == pytest.approx(b.diagnostics[k], **TOL)
    assert a.crit == pytest.approx(b.crit, abs=1e-5)      # the same draws on R within 1e-6


def test_covariance_is_that_of_the_reference_scores(three):
    Y, _, _, a, b = three
    psi = b.scores
    n = len(Y)
    assert psi.shape == (n, 3)
    phi = (psi - psi.mean(0)).T                            # [L, n]
    want = phi @ phi.T / (n - 1) / n
    got = np.asarray(a.cov)
    print("cov", got.tolist(), want.tolist())
    for c in range(3):
        for d in range(3):
            assert got[c, d] == pytest.approx(want[c, d], **TOL)
    assert np.array_equal(got, got.T)                      # symmetric to the bit
    assert np.linalg.eigvalsh(got).min() >= -1e-12 * np.trace(got)   # positive semidefinite
    assert a.diagnostics["n"] == n == sum(a.diagnostics["n_c"])
    assert a.moments[0] == n


def test_two_levels_are_the_interactive_model(tutorial):
    """L = 2 on the fixture's own binary W: m_0 is fitted as the mirror of m_1, so the
    contrast and its SE are DML-IRM's ATE and SE."""
    _, m, _ = tutorial
    a = DA.dml_apos_lasso(m.Y, m.W, m.X, device="cpu")
    b = DI.dml_irm_lasso(m.Y, m.W, m.X, device="cpu")
    c, = a.contrasts()
    print("apos", c.effect, c.se, "irm", b.ate, b.se)
    assert c.effect == pytest.approx(b.ate, **TOL) and c.se == pytest.approx(b.se, **TOL)
    assert a.diagnostics["n_c"][1] == b.diagnostics["n_treated"]
    # one contrast: the band is the pointwise interval, the normal quantile exactly, no draws
    assert a.crit == normal_quantile(0.975)
    assert (c.lower_joint, c.upper_joint) == (c.effect - a.crit * c.se, c.effect + a.crit * c.se)
    assert a.wald().df == 1
    assert a.wald().stat == pytest.approx((c.effect / c.se) ** 2, rel=1e-9)


def test_band(three):
    Y, D, X, a, _ = three
    z = normal_quantile(0.975)
    assert a.crit >= z and a.n_boot == 999 and a.level == 0.95
    for ref in VALUES:
        cs = a.contrasts(ref)
        assert len(cs) == 2
        for c in cs:
            assert c.lower_joint <= c.lower_ci < c.upper_ci <= c.upper_joint
    # the contrast of c against r is minus the contrast of r against c, with the same SE
    c20 = [c for c in a.contrasts(0.0) if c.level == 5.0][0]
    c02 = [c for c in a.contrasts(5.0) if c.level == 0.0][0]
    assert c20.effect == -c02.effect and c20.se == pytest.approx(c02.se, rel=1e-12)
    # a pure function of (moments, seed, level): the same seed gives the same band
    again = ApoResult.from_moments(a.method, a.moments, a.levels, seed=1991)
    other = ApoResult.from_moments(a.method, a.moments, a.levels, seed=7)
    assert again.crit == a.crit and again.cov == a.cov
    assert other.crit != a.crit and other.crit >= z and other.cov == a.cov
    ccov = contrast_cov(a.cov, 0)
    assert band_crit(ccov, 1991) == a.crit
    assert band_crit(ccov, 1991, level=0.99) > a.crit
    # perfectly correlated contrasts are one contrast: the band is close to the quantile
    one = band_crit([[1.0, 1.0], [1.0, 1.0]], 3)
    two = band_crit([[1.0, 0.0], [0.0, 1.0]], 3)
    assert abs(one - z) < 0.15 and two > one
    # the wald statistic does not depend on the reference
    w0 = a.wald()
    w5 = ApoResult.from_moments(a.method, a.moments, a.levels, reference=5.0).wald()
    assert w0.df == 2 == w5.df and w0.stat == pytest.approx(w5.stat, rel=1e-9)
    assert 0.0 <= w0.p_value <= 1.0
    assert math.exp(-w0.stat / 2) == pytest.approx(w0.p_value, rel=1e-9)   # chi2_2's tail
    out = json.loads(a.json())
    assert out["levels"] == list(VALUES) and len(out["contrasts"]) == 2 and len(out["apo"]) == 3
    assert "all means equal" in a.table() and f"crit {a.crit:.4f}" in a.table()


def test_api_and_reference_backend(three):
    Y, D, X, a, b = three
    r = ate_dml_apos(Y, D, X, reference=5.0, folds=3, run=RunConfig(backend="cpu"))
    assert r.reference == 5.0 and [x.ate for x in r.apo] == [x.ate for x in a.apo]
    assert [c.level for c in r.contrasts()] == [0.0, 2.0]
    assert r[2.0].ate == a.apo[1].ate


def _small_panel(L, K, n=1500, seed=5):
    d = make_multiarm_data(n, seed, levels=L)
    pan, values, _, _, counts, _ = DA.level_split_panel(d.Y, d.D, d.X, K, 1991, "f64", "cpu")
    assert len(values) == L and pan.nseg == L * K
    return pan, counts


def test_launch_grouping_keeps_the_bits():
    """The picked coefficients do not depend on how the path problems are spread over
    launches: every launch has the lambda ratio of the whole fit."""
    L, K = 3, 3
    pan, counts = _small_panel(L, K)
    calls = []
    real = DA.cv_enet_gaussian

    def spy(*a, **kw):
        calls.append(len(kw["full_sets"]))
        assert kw["lambda_min_ratio"] == 1e-4
        return real(*a, **kw)

    mp = pytest.MonkeyPatch()
    mp.setattr(DA, "cv_enet_gaussian", spy)
    try:
        _, mom1, coef1 = DA.apos_panel(pan, K, L, seg_counts=counts)
        assert calls == [2 * L * K]
        del calls[:]
        # a cap of 27 problems holds 9 full sets of K = 3 problems: 18 sets take two launches
        _, mom2, coef2 = DA.apos_panel(pan, K, L, seg_counts=counts, max_problems=27)
        assert calls == [9, 9]
        del calls[:]
        _, mom3, coef3 = DA.apos_panel(pan, K, L, seg_counts=counts, max_problems=3)
        assert calls == [1] * 18
    finally:
        mp.undo()
    assert coef1.shape == (K, 2 * L, len(pan.xcols) + 1)
    assert torch.equal(coef1, coef2) and torch.equal(coef1, coef3)
    assert torch.equal(mom1, mom2) and torch.equal(mom1, mom3)
    with pytest.raises(ValueError, match="more than the 2 one path launch holds"):
        DA.apos_fit_phases(pan, K, L, seg_counts=counts, max_problems=2)


def test_launch_counts():
    # a nuisance with its folds is K path problems; 2 L K nuisances
    assert DA.path_launches(2 * 5 * 5, 5) == [(0, 50)]                   # L = 5, K = 5: 250
    assert DA.path_launches(2 * 6 * 5, 5) == [(0, 30), (30, 60)]         # L = 6, K = 5: 300
    assert DA.path_launches(2 * 8 * 5, 5) == [(0, 40), (40, 80)]         # L = 8, K = 5: 400
    assert len(DA.path_launches(2 * 8 * 10, 10)) == 7                    # 1600 in 7 launches
    for a, b in DA.path_launches(2 * 8 * 10, 10):
        assert 0 < (b - a) * 10 <= 256
    with pytest.raises(ValueError, match="257 path problems"):
        DA.path_launches(2 * 2 * 257, 257)


def test_launch_count_of_the_estimator():
    """L = 6 at K = 5 takes two launches, L = 5 one: counted on the fit phase itself, with the
    path solver replaced by a recorder (its results are not needed)."""
    class Stop(Exception):
        pass

    for L, want in ((5, [50]), (6, [30, 30])):
        pan, counts = _small_panel(L, 5, n=3000)
        calls = []

        def spy(*a, **kw):
            calls.append(len(kw["full_sets"]))
            if sum(calls) == 2 * L * 5:
                raise Stop
            from types import SimpleNamespace
            z = torch.zeros(len(kw["full_sets"]), len(pan.xcols) + 1, dtype=torch.float64)
            return SimpleNamespace(coef_min=z, coef_1se=z)

        mp = pytest.MonkeyPatch()
        mp.setattr(DA, "cv_enet_gaussian", spy)
        try:
            phases, _ = DA.apos_fit_phases(pan, 5, L, seg_counts=counts)
            with pytest.raises(Stop):
                phases[-1]({"G": torch.zeros(L * 5, pan.P, pan.P, dtype=torch.float64)})
        finally:
            mp.undo()
        assert calls == want


@pytest.fixture
def no_device_work(monkeypatch):
    """Any panel build, Gram or path launch after this is a failure of the test."""
    def boom(*a, **kw):
        raise AssertionError("device work before the argument check")
    for name in ("build_panel", "cv_enet_gaussian", "gram_phases", "run_body"):
        monkeypatch.setattr(DA, name, boom)


def test_refusals(tutorial, no_device_work):
    _, m, _ = tutorial
    Y, X, n = m.Y, m.X, len(m.Y)
    rs = np.random.RandomState(0)
    D3 = rs.randint(0, 3, n).astype(float)
    kw = dict(device="cpu")
    with pytest.raises(ValueError, match="D has 1 distinct value"):
        DA.dml_apos_lasso(Y, np.ones(n), X, **kw)
    with pytest.raises(ValueError, match="D has 9 distinct values"):
        DA.dml_apos_lasso(Y, np.arange(n) % 9, X, **kw)
    for bad in (np.nan, np.inf):
        Db = D3.copy()
        Db[5] = bad
        with pytest.raises(ValueError, match="finite treatment"):
            DA.dml_apos_lasso(Y, Db, X, **kw)
    with pytest.raises(ValueError, match="reference 7 is not a treatment level"):
        DA.dml_apos_lasso(Y, D3, X, reference=7, **kw)
    # level 4.5 only in fold 2 of the K = 3 fold stream: folds 0 and 1 have empty cells
    from ate_replication_causalml_amd.parallel import rng
    fid = rng.fold_ids(n, 3, 1991, 0)
    De = D3.copy()
    De[np.flatnonzero(fid == 2)[:4]] = 4.5
    with pytest.raises(ValueError, match=r"empty \(fold, level\) cell: fold 0, level D=4.5 has no"):
        DA.dml_apos_lasso(Y, De, X, folds=3, **kw)
    with pytest.raises(ValueError, match="repeats must be 1"):
        DA.dml_apos_lasso(Y, D3, X, repeats=2, **kw)
    with pytest.raises(ValueError, match='propensity must be "linear"'):
        DA.dml_apos_lasso(Y, D3, X, propensity="logit", **kw)
    for extra in (dict(repeats=3), dict(propensity="logit")):
        for backend in ("cpu", "reference"):
            with pytest.raises(ValueError):
                ate_dml_apos(Y, D3, X, run=RunConfig(backend=backend), **extra)
    with pytest.raises(ValueError, match="more than the 256 one path launch holds"):
        DA.dml_apos_lasso(Y, D3, X, folds=257, **kw)
    # the reference twin refuses the same inputs
    with pytest.raises(ValueError, match="D has 1 distinct value"):
        E.dml_apos_lasso(Y, np.ones(n), X)
    with pytest.raises(ValueError, match=r"empty \(fold, level\) cell: fold 0, level D=4.5 has no"):
        E.dml_apos_lasso(Y, De, X, folds=3)


def test_twin_pass_refusals():
    pan, _ = _small_panel(3, 2, n=600)
    p = len(pan.xcols)
    good = torch.zeros(2, 6, p + 1, dtype=torch.float64)
    assert DA.apo_moments(pan, good, 3).shape == (22,)
    for L in (1, 9):
        with pytest.raises(ValueError, match="2 to 8 treatment levels"):
            DA.apo_moments(pan, good, L)
    with pytest.raises(ValueError, match="no multiple of 4 levels"):
        DA.apo_moments(pan, torch.zeros(2, 8, p + 1, dtype=torch.float64), 4)
    with pytest.raises(ValueError, match="coef must be"):
        DA.apo_moments(pan, good[:, :5], 3)


def test_multiarm_data():
    d = make_multiarm_data(20_000, 3)
    assert d.X.shape == (20_000, 21) and d.arms[0] == "control" and d.arms[4] == "neighbors"
    assert sorted(np.unique(d.D)) == [0, 1, 2, 3, 4] and set(np.unique(d.Y)) == {0.0, 1.0}
    assert np.allclose(d.propensity.sum(1), 1.0) and d.propensity.min() > 0.01
    # the effects are ordered like the experiment's, and assignment depends on X: the naive
    # contrast of the strongest arm is biased upwards by more than its sampling error
    assert np.all(np.diff(d.apo_true) > 0)
    naive = d.Y[d.D == 4].mean() - d.Y[d.D == 0].mean()
    assert naive - (d.apo_true[4] - d.apo_true[0]) > 0.01
    # a pure function of (seed, row): a prefix of a longer draw, another seed differs
    e = make_multiarm_data(500, 3)
    assert np.array_equal(e.D, d.D[:500]) and np.array_equal(e.Y, d.Y[:500])
    assert not np.array_equal(make_multiarm_data(500, 4).D, e.D)
    assert make_multiarm_data(500, 3, levels=8, p_extra=4).X.shape == (500, 25)
    for bad in (1, 9):
        with pytest.raises(ValueError):
            make_multiarm_data(100, 3, levels=bad)


def test_cli(capsys):
    from ate_replication_causalml_amd import cli
    assert cli.main(["apos", "--n", "3000", "--levels", "3", "--folds", "3", "--backend",
                     "cpu"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["levels"] == [0.0, 1.0, 2.0] and len(out["apo_true"]) == 3
    assert out["arms"] == ["control", "civic_duty", "hawthorne"] and len(out["contrasts"]) == 2
    with pytest.raises(SystemExit, match="levels must be in 2..8"):
        cli.main(["apos", "--n", "100", "--levels", "9", "--backend", "cpu"])
