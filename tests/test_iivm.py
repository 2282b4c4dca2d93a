"""The LATE of the interactive IV model (estimators/late.py, result.LateResult) on the CPU
path: the 15-moment twin against a row-by-row numpy evaluation, the sums it shares with the
AIPW pass, the closed forms, the estimator against the reference twin and against DML-IRM
(the ITT; full compliance), one-sided noncompliance (fewer path problems, fixed rows, flag
errors), the Wald ratio as an independent oracle, the Anderson-Rubin set, row sharding,
argument checks and the public surface."""
import json
import math

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.config import RunConfig
from ate_replication_causalml_amd.data.dgp import make_late_data
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators import late as DL
from ate_replication_causalml_amd.ops.enet import cv_problem_count
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel.comm import run_simulated
from ate_replication_causalml_amd.parallel.dist import DistContext
from ate_replication_causalml_amd.reference import estimators as R
from ate_replication_causalml_amd.result import LATE_MOMENTS, LateResult, normal_quantile
from test_gpu_iivm import SHARED_D, SHARED_Y, _case5
from test_gpu_irm import CLIP, COUNTS

K = 5


# ---------------------------------------------------------------- twin and closed forms
def _rows(X, Z, D, Y, seg, coef, spf):
    """The 15 moments row by row in numpy (no panel, no torch)."""
    mom = np.zeros(15)
    for x, z, d, y, s in zip(X, Z, D, Y, seg):
        k = s // 2 if spf == 2 else s
        g0, g1, r0, r1, m = (coef[k, r, 0] + coef[k, r, 1:] @ x for r in range(5))
        e = min(max(m, CLIP), 1 - CLIP)
        b = g1 - g0 + z * (y - g1) / e - (1 - z) * (y - g0) / (1 - e)
        a = r1 - r0 + z * (d - r1) / e - (1 - z) * (d - r0) / (1 - e)
        mom += [b, b * b, 1, m < CLIP or m > 1 - CLIP, a, a * a, a * b, z, z * d, (1 - z) * d,
                z * (y - g1) ** 2, (1 - z) * (y - g0) ** 2, z * (d - r1) ** 2,
                (1 - z) * (d - r0) ** 2, (z - m) ** 2]
    return mom


@pytest.mark.parametrize("spf", [2, 1])
def test_twin_vs_rows_and_shared_sums(spf):
    X, Z, D, Y, seg, coef = _case5(exact=False)
    if spf == 1:
        coef = np.repeat(coef, 2, axis=0)
    pan = build_panel(X, Z, Y, folds=seg, dtype="f64", device="cpu", targets={"D": D})
    assert tuple(pan.seg_nreal) == COUNTS and len(LATE_MOMENTS) == 15 == DL.N_LATE
    c = torch.from_numpy(coef)
    mom = DL.iivm_moments(pan, c, CLIP, spf)
    want = _rows(X, Z, D, Y, seg, coef, spf)
    print("twin", mom.tolist())
    print("rows", want.tolist())
    # 529 rows of O(1) terms summed in another order: n eps sum|x| / |sum| stays below 1e-11
    np.testing.assert_allclose(mom.numpy(), want, rtol=1e-11)
    assert np.array_equal(mom.numpy()[[2, 3, 7, 8, 9]], want[[2, 3, 7, 8, 9]])
    assert 0 < mom[3] < len(Y) and abs(mom[4]) > 0.1 * len(Y)      # S a does not cancel
    # the sums shared with the AIPW pass: the same expressions on the same operands
    pd_ = build_panel(X, Z, D, folds=seg, dtype="f64", device="cpu")
    for (mine, theirs, rows), p in ((SHARED_Y, pan), (SHARED_D, pd_)):
        base = DI.irm_score_moments(p, c[:, rows].contiguous(), CLIP, spf)
        assert torch.equal(mom[mine], base[theirs])


def test_moments_reject_bad_arguments():
    X, Z = np.zeros((8, 2)), (np.arange(8) % 2).astype(float)
    pan = build_panel(X, Z, np.zeros(8), folds=np.arange(8) % 4, targets={"D": Z})
    with pytest.raises(ValueError):
        DL.iivm_moments(pan, torch.zeros(1, 5, 3), 0.01, 2)     # 4 segments need 2 blocks
    with pytest.raises(ValueError):
        DL.iivm_moments(pan, torch.zeros(2, 3, 3), 0.01, 2)     # three rows: the IRM shape
    with pytest.raises(ValueError):                             # no D column
        DL.iivm_moments(build_panel(X, Z, np.zeros(8), folds=np.arange(8) % 4),
                        torch.zeros(2, 5, 3), 0.01, 2)
    with pytest.raises(ValueError):
        build_panel(X, Z, np.zeros(8), targets={"Y": Z})        # a name already taken
    with pytest.raises(ValueError):
        LateResult.from_moments("t", np.zeros(8))
    # without the argument the layout is today's
    a, b = build_panel(X, Z, Z, dtype="bf16"), build_panel(X, Z, Z, dtype="bf16", targets=None)
    assert a.cols == b.cols and torch.equal(a.data, b.data)
    c = build_panel(X, Z, Z, dtype="bf16", targets={"D": Z}, extra_cols=("z",))
    assert [k for k in c.cols if k not in a.cols] == ["D", "D_hi", "D_lo", "z"]
    assert all(c.cols[k] == a.cols[k] for k in a.cols)


def test_finalize_and_result_from_formulas():
    rs = np.random.RandomState(3)
    n = 400
    b, a = rs.randn(n) + 0.3, 0.5 + 0.4 * rs.randn(n)
    mom = np.zeros(15)
    mom[[0, 1, 2, 4, 5, 6]] = [b.sum(), (b * b).sum(), n, a.sum(), (a * a).sum(), (a * b).sum()]
    mom[[3, 7, 8, 9]] = [7, 180, 120, 40]
    mom[10:] = [45.0, 55.0, 20.0, 11.0, 100.0]
    theta = b.sum() / a.sum()
    phi = (b - theta * a) / a.mean()
    se = math.sqrt((phi ** 2).sum() / (n - 1) / n)
    fin = DL.late_finalize(torch.from_numpy(mom)).numpy()
    r = LateResult.from_moments("t", mom, hipgraph=False)
    assert fin[0] == pytest.approx(theta, rel=1e-13) and fin[1] == pytest.approx(se, rel=1e-12)
    assert r.late == pytest.approx(theta, rel=1e-13) and r.se == pytest.approx(se, rel=1e-12)
    assert (r.lower_ci, r.upper_ci) == (r.late - 1.96 * r.se, r.late + 1.96 * r.se)
    assert r.itt.ate == pytest.approx(b.mean(), rel=1e-13)
    assert r.itt.se == pytest.approx(b.std(ddof=1) / math.sqrt(n), rel=1e-12)
    assert r.first_stage.ate == pytest.approx(a.mean(), rel=1e-13)
    assert r.first_stage.se == pytest.approx(a.std(ddof=1) / math.sqrt(n), rel=1e-12)
    assert r.first_stage_t == pytest.approx(a.mean() / (a.std(ddof=1) / math.sqrt(n)), rel=1e-12)
    cov = np.cov(np.stack([b, a]), ddof=1) / n
    np.testing.assert_allclose(np.array(r.cov), cov, rtol=1e-11)
    # the delta method on (ITT, first stage) gives the same variance
    g = np.array([1.0, -theta]) / a.mean()
    assert r.se ** 2 == pytest.approx(g @ cov @ g, rel=1e-10)
    d = r.diagnostics
    assert (d["n"], d["n_clipped"], d["n_z1"]) == (400, 7, 180)
    assert (d["n_z0_d0"], d["n_z0_d1"], d["n_z1_d0"], d["n_z1_d1"]) == (180, 40, 60, 120)
    assert d["rmse_g1"] == math.sqrt(45 / 180) and d["rmse_g0"] == math.sqrt(55 / 220)
    assert d["rmse_r1"] == math.sqrt(20 / 180) and d["rmse_r0"] == math.sqrt(11 / 220)
    assert d["rmse_m"] == 0.5 and d["hipgraph"] is False


# ---------------------------------------------------------------- the estimator
@pytest.fixture(scope="module")
def late(tutorial):
    """``make_late_data`` at the tutorial fixture's size."""
    _, m, _ = tutorial
    return make_late_data(len(m.Y), 1991)


@pytest.fixture(scope="module")
def fit(late):
    import ate_replication_causalml_amd as pkg
    d = late
    return pkg.ate_dml_iivm(d.Y, d.D, d.Z, d.X, run=RunConfig(backend="cpu"))


def test_estimator_vs_reference(late, fit):
    import ate_replication_causalml_amd as pkg
    d = late
    ref = pkg.ate_dml_iivm(d.Y, d.D, d.Z, d.X, run=RunConfig(backend="reference"))
    assert isinstance(fit, pkg.LateResult) and isinstance(ref, pkg.LateResult)
    print("cpu", fit.late, fit.se, "reference", ref.late, ref.se)
    # the project's bound for device orchestration against the row-by-row reference
    for x, y in ((fit.late, ref.late), (fit.se, ref.se), (fit.itt.ate, ref.itt.ate),
                 (fit.itt.se, ref.itt.se), (fit.first_stage.ate, ref.first_stage.ate),
                 (fit.first_stage.se, ref.first_stage.se), (fit.cov[0][1], ref.cov[0][1])):
        assert x == pytest.approx(y, abs=1e-6, rel=1e-6)
    for k in ("n", "n_clipped", "n_z1", "n_z0_d0", "n_z0_d1", "n_z1_d0", "n_z1_d1"):
        assert fit.diagnostics[k] == ref.diagnostics[k]
    for k in ("rmse_g0", "rmse_g1", "rmse_r0", "rmse_r1", "rmse_m"):
        assert fit.diagnostics[k] == pytest.approx(ref.diagnostics[k], abs=1e-6, rel=1e-6)
    dg = fit.diagnostics
    assert dg["n"] == d.n == dg["n_z0_d0"] + dg["n_z0_d1"] + dg["n_z1_d0"] + dg["n_z1_d1"]
    assert dg["n_z0_d1"] == int(((d.Z == 0) & (d.D == 1)).sum()) > 0 and dg["n_z1_d0"] > 0
    assert dg["hipgraph"] is False and fit.method == ref.method
    # the types' effects differ, so the LATE of the design is not its ATE
    assert set(np.unique(d.types)) == {0, 1, 2} and 0.2 < d.late_true < 0.3


def test_itt_is_the_irm_effect_of_the_instrument(late, fit):
    d = late
    irm = DI.dml_irm_lasso(d.Y, d.Z, d.X, device="cpu")
    print("ITT", fit.itt.ate, fit.itt.se, "IRM(Y, Z, X)", irm.ate, irm.se, "bit-equal:",
          (fit.itt.ate, fit.itt.se) == (irm.ate, irm.se))
    assert fit.itt.ate == pytest.approx(irm.ate, rel=1e-9)
    assert fit.itt.se == pytest.approx(irm.se, rel=1e-9)
    assert fit.diagnostics["n_clipped"] == irm.diagnostics["n_clipped"]
    assert fit.diagnostics["n_z1"] == irm.diagnostics["n_treated"]


def test_full_compliance_is_the_irm(late):
    """D = Z with both nuisances fixed: a = 1 on every row, so S a = n exactly and the LATE
    is the ATE of DML-IRM(Y, Z, X)."""
    d = late
    r = DL.dml_iivm_lasso(d.Y, d.Z, d.Z, d.X, always_takers=False, never_takers=False,
                          device="cpu")
    irm = DI.dml_irm_lasso(d.Y, d.Z, d.X, device="cpu")
    assert r.moments[4] == d.n == r.moments[5] and r.first_stage.ate == 1.0
    assert r.late == pytest.approx(irm.ate, rel=1e-12)
    assert r.se == pytest.approx(irm.se, rel=1e-12)
    assert r.diagnostics["n_z0_d1"] == 0 == r.diagnostics["n_z1_d0"]


@pytest.mark.parametrize("at,nt", [(True, True), (False, True), (True, False), (False, False)])
def test_problem_counts_and_fixed_rows(at, nt, monkeypatch):
    d = make_late_data(500, 3, always_takers=at, never_takers=nt)
    launched = []
    real = DI.cv_enet_gaussian

    def counting(G, panel, xcols, ycols, full_sets=None, **kw):
        launched.append(cv_problem_count(G.shape[0], full_sets, len(ycols), kw.get("full_y")))
        cv = real(G, panel, xcols, ycols, full_sets=full_sets, **kw)
        launched.append(len(cv.full_keys))
        return cv

    monkeypatch.setattr(DI, "cv_enet_gaussian", counting)
    pan, counts, _, n, _ = DI.arm_split_panel(d.Y, d.Z, d.X, K, 1991, "f64", "cpu",
                                              targets={"D": d.D})
    st = DI.run_phases(DL.late_phases(pan, K, seg_counts=counts, always_takers=at,
                                      never_takers=nt))
    # per nuisance K outer folds x (1 full + K - 1 inner CV paths) = K K problems
    nfit = 3 + at + nt
    assert launched == [nfit * K * K, nfit * K] and DL.fitted_nuisances(at, nt) == tuple(
        r for r in range(5) if (r != 2 or at) and (r != 3 or nt))
    coef = st["coef"]
    assert coef.shape == (K, 5, d.X.shape[1] + 1)
    if not at:
        assert (coef[:, 2] == 0).all()
    if not nt:
        assert (coef[:, 3, 1:] == 0).all() and (coef[:, 3, 0] == 1).all()
    for r in DL.fitted_nuisances(at, nt):
        assert (coef[:, r, 0] != 0).all()
    assert torch.isfinite(st["res"]).all() and torch.isfinite(st["mom"]).all()
    r = LateResult.from_moments("t", st["mom"].numpy())
    assert r.late == pytest.approx(st["res"][0].item(), rel=1e-13)     # late_finalize on device
    assert r.se == pytest.approx(st["res"][1].item(), rel=1e-12)
    assert r.diagnostics["n_z0_d1"] == (0 if not at else int(((d.Z == 0) & (d.D == 1)).sum()))
    assert r.diagnostics["n_z1_d0"] == (0 if not nt else int(((d.Z == 1) & (d.D == 0)).sum()))


@pytest.mark.parametrize("backend", ["cpu", "reference"])
def test_flag_errors(late, backend):
    import ate_replication_causalml_amd as pkg
    d = late
    run = RunConfig(backend=backend)
    # the flag set on data that violates it
    with pytest.raises(ValueError, match="always_takers=True"):
        pkg.ate_dml_iivm(d.Y, d.D, d.Z, d.X, always_takers=False, run=run)
    with pytest.raises(ValueError, match="never_takers=True"):
        pkg.ate_dml_iivm(d.Y, d.D, d.Z, d.X, never_takers=False, run=run)
    # the flag unset on data with an empty (fold, z, d) cell
    with pytest.raises(ValueError, match=r"Z=0, D=1.*always_takers=False"):
        pkg.ate_dml_iivm(d.Y, d.D * d.Z, d.Z, d.X, run=run)
    with pytest.raises(ValueError, match=r"Z=1, D=0.*never_takers=False"):
        pkg.ate_dml_iivm(d.Y, np.maximum(d.D, d.Z), d.Z, d.X, run=run)


def _noise_design(n=2000, seed=5):
    """Covariates that are pure noise, a fair-coin instrument, 20 % always-takers and 25 %
    never-takers: nothing for the nuisances to learn beyond the arm means."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, 6)
    Z = (rs.rand(n) < 0.5).astype(float)
    u = rs.rand(n)
    t = np.where(u < 0.2, 1, np.where(u > 0.75, 2, 0))
    D = np.where(t == 1, 1.0, np.where(t == 2, 0.0, Z))
    Y = 0.5 + 1.0 * D * (t == 0) + 0.3 * D * (t == 1) + rs.randn(n)
    return Y, D, Z, X


def test_wald_ratio_is_an_independent_oracle():
    """With noise covariates DML-LATE must land on the Wald ratio of the arm means. The gap
    of the reference backend on this design, measured on the CPU: |0.983968 - 0.987899| =
    3.93e-3 (0.045 SE, SE = 0.0865); the bound is twice that gap and must stay under half
    a standard error."""
    Y, D, Z, X = _noise_design()
    wald = (Y[Z == 1].mean() - Y[Z == 0].mean()) / (D[Z == 1].mean() - D[Z == 0].mean())
    r = DL.dml_iivm_lasso(Y, D, Z, X, device="cpu")
    gap = abs(r.late - wald)
    bound = 2 * 3.93e-3                                   # measured gap: 3.93e-3
    print("late", r.late, "se", r.se, "wald", wald, "gap", gap, "bound", bound)
    assert bound < 0.5 * r.se
    assert gap <= bound


def test_true_late_within_three_se():
    """n = 4000, seed 1991 (checked on the CPU: 0.2080 against 0.2502, -1.55 SE)."""
    d = make_late_data(4000, 1991)
    r = DL.dml_iivm_lasso(d.Y, d.D, d.Z, d.X, device="cpu")
    print("late", r.late, "se", r.se, "true", d.late_true, (r.late - d.late_true) / r.se)
    assert abs(r.late - d.late_true) < 3 * r.se
    assert r.first_stage_t > 10 and r.late in r.anderson_rubin()


# ---------------------------------------------------------------- Anderson-Rubin
def _moments(n, mean_a, var_a, mean_b, var_b, cov_ab):
    """A moment vector with these sample means and (n - 1)-rule (co)variances of (a, b)."""
    mom = np.zeros(15)
    mom[2] = n
    mom[4], mom[0] = n * mean_a, n * mean_b
    mom[5] = (n - 1) * var_a + n * mean_a ** 2
    mom[1] = (n - 1) * var_b + n * mean_b ** 2
    mom[6] = (n - 1) * cov_ab + n * mean_a * mean_b
    return mom


def _ar_stat(mom, theta):
    sb, sbb, n, _, sa, saa, sab = mom[:7]
    s1 = sb - theta * sa
    s2 = sbb - 2 * theta * sab + theta * theta * saa
    return n * (s1 / n) ** 2 / ((s2 - s1 * s1 / n) / (n - 1))


@pytest.mark.parametrize("mean_a,kind", [(0.5, "interval"), (0.018, "two_rays"), (0.0005, "all")])
def test_anderson_rubin_kinds_and_endpoints(mean_a, kind):
    # first-stage t_a = mean_a sqrt(n) / sd(a) = 50, 1.8, 0.05 at n = 10^4, sd 1, and t_b =
    # 0.6 t_a; b, a uncorrelated with equal variance. An interval needs t_a^2 > chi2 = 3.84;
    # below it the set is two rays while t_a^2 + t_b^2 = 1.36 t_a^2 > chi2 (4.41 here: some
    # theta is still rejected), and the whole line once that sum is under chi2 too
    mom = _moments(10_000, mean_a, 1.0, 0.6 * mean_a, 1.0, 0.0)
    r = LateResult.from_moments("t", mom)
    ar = r.anderson_rubin(0.95)
    chi2 = normal_quantile(0.975) ** 2
    assert ar.kind == kind and ar.level == 0.95
    assert r.late == pytest.approx(0.6, rel=1e-12) and r.late in ar        # theta-hat inside
    assert _ar_stat(mom, r.late) == pytest.approx(0.0, abs=1e-20)
    if kind == "all":
        assert (ar.lower, ar.upper) == (-math.inf, math.inf) and 1e9 in ar and -1e9 in ar
        return
    for end in (ar.lower, ar.upper):
        assert math.isfinite(end)
        assert _ar_stat(mom, end) == pytest.approx(chi2, rel=1e-10)   # the defining equality
    mid = 0.5 * (ar.lower + ar.upper)
    if kind == "interval":
        assert ar.lower < r.late < ar.upper and mid in ar
        assert ar.lower - 1e-3 not in ar and ar.upper + 1e-3 not in ar
    else:
        assert (r.late <= ar.lower or r.late >= ar.upper) and mid not in ar
        assert ar.lower - 1.0 in ar and ar.upper + 1.0 in ar
    with pytest.raises(ValueError):
        r.anderson_rubin(1.0)


def test_anderson_rubin_matches_wald_under_a_strong_first_stage():
    mom = _moments(100_000, 0.6, 0.2, 0.15, 0.25, 0.02)     # first-stage t = 424
    r = LateResult.from_moments("t", mom)
    ar = r.anderson_rubin()
    wald = r.upper_ci - r.lower_ci
    print("AR", ar.lower, ar.upper, "Wald", r.lower_ci, r.upper_ci)
    assert ar.kind == "interval" and abs((ar.upper - ar.lower) / wald - 1) < 0.05
    assert ar.lower < r.late < ar.upper


def test_anderson_rubin_of_the_fit(fit):
    ar = fit.anderson_rubin()
    assert ar.kind == "interval" and fit.late in ar
    chi2 = normal_quantile(0.975) ** 2
    for end in (ar.lower, ar.upper):
        assert _ar_stat(np.array(fit.moments), end) == pytest.approx(chi2, rel=1e-10)
    wide = fit.anderson_rubin(0.99)
    assert wide.lower < ar.lower and wide.upper > ar.upper


# ---------------------------------------------------------------- row sharding
def test_two_ranks_equal_one():
    d = make_late_data(600, 1991)
    kw = dict(folds=3, device="cpu")
    one = DL.dml_iivm_lasso(d.Y, d.D, d.Z, d.X, **kw)
    mom1 = np.array(one.moments)

    def body(comm):
        dist = DistContext.for_rank(comm, d.n)
        return DL.dml_iivm_lasso(dist.local(d.Y), dist.local(d.D), dist.local(d.Z),
                                 dist.local(d.X), dist=dist, **kw)

    for r in run_simulated(2, body):
        mom = np.array(r.moments)
        print(np.abs(mom - mom1).max())
        np.testing.assert_allclose(mom, mom1, rtol=1e-12)      # the README's non-exact bound
        assert np.array_equal(mom[[2, 3, 7, 8, 9]], mom1[[2, 3, 7, 8, 9]])
        assert r.late == pytest.approx(one.late, rel=1e-12)
        assert r.se == pytest.approx(one.se, rel=1e-12)
        for k in ("n", "n_clipped", "n_z1", "n_z0_d0", "n_z0_d1", "n_z1_d0", "n_z1_d1"):
            assert r.diagnostics[k] == one.diagnostics[k]


def test_sharded_flag_error_counts_the_global_cells(late):
    """The (fold, z, d) cells go through the one all-reduce of the cell counts: every rank
    raises on a violation that only one shard holds."""
    d = late
    D = d.D * d.Z                          # no always-takers ...
    D[np.flatnonzero(d.Z == 0)[0]] = 1.0   # ... but for one row, in rank 0's shard

    def body(comm):
        dist = DistContext.for_rank(comm, d.n)
        with pytest.raises(ValueError, match="always_takers=True"):
            DL.dml_iivm_lasso(dist.local(d.Y), dist.local(D), dist.local(d.Z), dist.local(d.X),
                              always_takers=False, dist=dist, device="cpu")
        return True

    assert run_simulated(2, body) == [True, True]


# ---------------------------------------------------------------- validation and surface
def _tiny():
    rs = np.random.RandomState(0)
    X, Y = rs.randn(160, 4), rs.randn(160)
    Z = (rs.rand(160) < 0.5).astype(float)
    D = np.where(rs.rand(160) < 0.7, Z, 1.0 - Z)
    return Y, D, Z, X


@pytest.mark.parametrize("bad", ["d", "z", "cell"])
@pytest.mark.parametrize("backend", ["cpu", "reference"])
def test_bad_arguments_raise(bad, backend):
    import ate_replication_causalml_amd as pkg
    Y, D, Z, X = _tiny()
    if bad == "d":
        D[3] = 0.5                                        # a treatment that is not binary
    elif bad == "z":
        Z[5] = 2.0                                        # an instrument that is not binary
    else:
        Z[:] = 1.0                                        # an empty (fold, Z = 0) cell
    with pytest.raises(ValueError):
        pkg.ate_dml_iivm(Y, D, Z, X, run=RunConfig(backend=backend))


def test_result_surface(fit):
    txt = fit.table()
    assert all(s in txt for s in ("LATE", "ITT", "first stage", "Anderson-Rubin"))
    out = json.loads(fit.json())
    assert out == json.loads(fit.to_json())
    assert out["late"] == fit.late and out["se"] == fit.se and len(out["moments"]) == 15
    assert out["itt"]["estimate"] == fit.itt.ate and out["first_stage"]["se"] == fit.first_stage.se
    assert out["first_stage_t"] == fit.first_stage.ate / fit.first_stage.se
    assert out["cov"][0][1] == out["cov"][1][0] == fit.cov[0][1]
    assert out["anderson_rubin"]["kind"] == "interval"
    assert out["diagnostics"]["n_z1_d1"] == fit.diagnostics["n_z1_d1"]
    assert fit.late == pytest.approx(fit.itt.ate / fit.first_stage.ate, rel=1e-13)


def test_make_late_data_one_sided():
    a = make_late_data(3000, 7, always_takers=False)
    assert not np.any((a.Z == 0) & (a.D == 1)) and 1 not in a.types and 2 in a.types
    b = make_late_data(3000, 7, never_takers=False)
    assert not np.any((b.Z == 1) & (b.D == 0)) and 2 not in b.types and 1 in b.types
    c = make_late_data(3000, 7)
    assert np.array_equal(c.X, a.X) and np.array_equal(c.Z, a.Z)     # the same draws
    assert np.array_equal(c.D[c.types == 0], c.Z[c.types == 0])
    assert c.late_true == pytest.approx(0.2 + 0.1 * c.X[c.types == 0, c.names.index("sex")].mean())
    # Z depends on X: its propensity moves with yob
    yob = c.X[:, c.names.index("yob")]
    assert c.Z[yob > 0.5].mean() > c.Z[yob < -0.5].mean() + 0.1


def test_cli_late(capsys):
    from ate_replication_causalml_amd import cli
    base = ["late", "--n", "1500", "--backend", "cpu"]
    assert cli.main(base) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert all(np.isfinite(out[k]) for k in ("late", "se", "lower_ci", "upper_ci", "late_true"))
    assert out["diagnostics"]["n"] == 1500 and out["diagnostics"]["n_z0_d1"] > 0
    assert out["anderson_rubin"]["kind"] == "interval" and out["first_stage_t"] > 5
    assert cli.main(base + ["--no-always-takers", "--folds", "3", "--clip", "0.05"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["diagnostics"]["n_z0_d1"] == 0 and np.isfinite(out["late"])
    with pytest.raises(SystemExit):
        cli.main(base + ["--backend", "tpu"])
