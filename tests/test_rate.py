"""RATE of a treatment-priority rule (estimators/rate.py) without a GPU: the float64 torch twin
of the ranking walk against the sample-by-sample reference, the half-sample bits, the closed
form for a binary priority against the group effects, every refusal, and that the test finds
heterogeneity where there is some and none where the priority is noise."""
import json

import numpy as np
import pytest
import torch

import ate_replication_causalml_amd as pkg
from ate_replication_causalml_amd.config import RunConfig
from ate_replication_causalml_amd.estimators import rate as DR
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.reference import estimators as R

CPU = RunConfig(backend="cpu")


# ---------------------------------------------------------------- the half-sample bits
def test_half_sample_bits_and_rate():
    ids = np.r_[np.arange(700), 2 ** 33 + np.arange(300)].astype(np.uint64)
    B, seed = 300, 77
    inc = rng.half_sample(seed, ids, B)
    assert inc.shape == (1000, B) and inc.dtype == np.uint8 and set(np.unique(inc)) == {0, 1}
    assert rng.P_HALF == 11
    for s in range(3):                                    # bit by bit against the raw words
        w = rng.random_u32(seed, rng.P_HALF, s, ids)
        for b in range(s * 128, min((s + 1) * 128, B)):
            word, bit = (b % 128) // 32, b % 32
            assert np.array_equal(inc[:, b], (w[:, word] >> np.uint32(bit)) & np.uint32(1)), b
    # other draws than the multipliers' (P_MULT) on the same rows
    assert not np.array_equal(inc, (rng.rademacher(seed, ids, B) + 1) // 2)
    # N = 300 000 fair bits: the rate is within 5 binomial sd = 5 sqrt(1 / (4 N)) of 1/2, and
    # so is every replicate's over its 1000 rows at 5 sqrt(1 / 4000) (300 of them: a
    # 6e-7 two-sided tail each)
    N = inc.size
    assert abs(inc.mean() - 0.5) <= 5 * np.sqrt(0.25 / N)
    assert np.all(np.abs(inc.mean(axis=0) - 0.5) <= 5 * np.sqrt(0.25 / 1000))


# ---------------------------------------------------------------- the twin against the reference
def _twin(psi, pr, rid, subset, q, B, seed):
    order, flags = DR.rate_order(torch.from_numpy(pr), torch.from_numpy(rid),
                                 None if subset is None else torch.from_numpy(subset), q)
    buf = DR.rate_boot(torch.from_numpy(psi), order, flags, torch.from_numpy(rid),
                       len(DR.check_grid(q)), B, seed)
    return buf, order, flags


PRIORITIES = {
    "distinct": lambda rs, n: rs.randn(n),
    "equal": lambda rs, n: np.full(n, 0.75),
    "binary": lambda rs, n: (rs.rand(n) < 0.3).astype(np.float64),
    "ties": lambda rs, n: rs.randint(0, 9, n).astype(np.float64),
}


@pytest.mark.parametrize("kind", list(PRIORITIES))
@pytest.mark.parametrize("masked", [False, True])
def test_twin_vs_reference(kind, masked):
    n, B, seed = 9000 if kind == "ties" else 700, 150, 11   # 9000: two row blocks of the twin
    rs = np.random.RandomState(3)
    psi = rs.standard_t(6, n) * 2 + 0.3
    pr = PRIORITIES[kind](rs, n)
    rid = rs.permutation(n).astype(np.int64) + 2 ** 33
    q = [0.05, 0.2, 0.5, 0.77, 1.0] if kind != "equal" else None
    subset = None
    if masked:                                            # padding rows and rows left out
        subset = rs.rand(n) < 0.8
        rid = np.where(rs.rand(n) < 0.1, -1, rid)
        psi = np.where((rid >= 0) & subset, psi, np.nan)
        pr = np.where((rid >= 0) & subset, pr, np.nan)
    buf, order, flags = _twin(psi, pr, rid, subset, q, B, seed)
    rows = np.flatnonzero((rid >= 0) & (subset if masked else True))
    assert order.numel() == len(rows) and sorted(order.tolist()) == rows.tolist()
    ref = R.rate_from_scores(psi[rows], pr[rows], rng.half_sample(seed, rid[rows], B), q)
    theta, autoc, qini, toc = (t.numpy() for t in DR.rate_stats(buf))
    assert DR.rate_entered(flags).tolist() == ref["entered"].tolist()
    assert int((flags & 1).sum()) == ref["n_runs"]
    scale = np.abs(psi[rows]).max()                       # both sides sum <= n terms below it
    tol = 64 * len(rows) * 2.0 ** -53 * scale
    assert np.abs(autoc[0] - ref["autoc"]) <= tol and np.abs(qini[0] - ref["qini"]) <= tol
    assert np.abs(toc[0] - ref["toc"]).max() <= tol
    assert np.abs(autoc[1:] - ref["autoc_b"]).max() <= tol
    assert np.abs(qini[1:] - ref["qini_b"]).max() <= tol
    assert np.abs(toc[1:] - ref["toc_b"]).max() <= tol
    # TOC(1) is exactly 0 in the full sample and in every replicate, on both sides
    assert np.all(toc[:, -1] == 0.0) and np.all(ref["toc_b"][:, -1] == 0.0)
    fin = DR.rate_finalize(buf, 0.0, B).numpy()
    Q = toc.shape[1]
    assert fin[0] == pytest.approx(ref["ate"], rel=1e-12) and fin[6] == len(rows)
    assert fin[[2, 4]] == pytest.approx([ref["autoc_se"], ref["qini_se"]], rel=1e-9, abs=tol)
    assert fin[7 + Q:] == pytest.approx(ref["toc_se"], rel=1e-9, abs=tol)
    assert fin[5] == pytest.approx(ref["crit"], rel=1e-6)
    if kind == "equal":                                   # one run: nothing to rank
        assert np.all(autoc == 0.0) and np.all(qini == 0.0) and np.all(toc == 0.0)
        assert np.all(fin[1:6] == 0.0) and np.all(fin[7:] == 0.0)
        assert np.all(ref["autoc_b"] == 0.0) and np.all(ref["qini_b"] == 0.0)
        assert ref["autoc_se"] == 0.0 and ref["crit"] == 0.0


def test_shift_invariance_and_centring():
    rs = np.random.RandomState(5)
    n, B = 600, 64
    psi, pr = rs.randn(n), np.round(rs.randn(n), 1)
    rid = np.arange(n, dtype=np.int64)
    a, _, _ = _twin(psi, pr, rid, None, None, B, 3)
    b, _, _ = _twin(psi + 1000.0, pr, rid, None, None, B, 3)
    fa, fb = DR.rate_finalize(a, 0.0, B).numpy(), DR.rate_finalize(b, -1000.0, B).numpy()
    assert fa[0] == pytest.approx(fb[0], abs=1e-11)
    assert fa[1:] == pytest.approx(fb[1:], abs=1e-9)


# ---------------------------------------------------------------- designs
def _design(n, p=10, seed=4, tau=lambda X: 1 + X[:, 0]):
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, p))
    pr = 1 / (1 + np.exp(-(0.5 * X[:, 0] + 0.4 * X[:, 1])))
    W = (r.uniform(size=n) < pr).astype(float)
    Y = X[:, 1] + 0.5 * X[:, 2] + tau(X) * W + r.normal(size=n)
    return Y, W, X


@pytest.fixture(scope="module")
def small():
    return _design(1500)


def test_binary_priority_is_the_group_contrast(small):
    Y, W, X = small
    hi = (X[:, 0] > 0.3).astype(np.float64)
    r = pkg.ate_dml_irm_rate(Y, W, X, hi, n_boot=64, run=CPU)
    g = pkg.ate_dml_irm_gate(Y, W, X, hi, n_boot=64, run=CPU)
    assert g.labels == [0.0, 1.0] and r.n_runs == 2 and r.n == len(Y)
    n1, n = g.n[1], len(Y)
    want = (n1 / n) * (1 - n1 / n) * (g.ate[1] - g.ate[0])
    assert r.autoc.estimate == pytest.approx(want, rel=1e-12)
    assert r.qini.estimate == pytest.approx((n1 / n) * want, rel=1e-12)
    assert r.ate == pytest.approx(g.overall.ate, rel=1e-12)
    assert r.toc["entered"] == [n1 if u * n <= n1 else n for u in r.toc["u"]]
    assert r.toc["estimate"][0] == pytest.approx(g.ate[1] - g.overall.ate, rel=1e-11)


def test_cpu_backend_matches_reference_and_reports(small):
    Y, W, X = small
    sub = np.arange(len(Y)) % 4 != 1
    kw = dict(q=[0.1, 0.5, 1.0], subset=sub, n_boot=100, folds=3)
    a = pkg.ate_dml_irm_rate(Y, W, X, 0, run=CPU, **kw)
    b = pkg.ate_dml_irm_rate(Y, W, X, X[:, 0], run=RunConfig(backend="reference"), **kw)
    assert isinstance(a, pkg.RateResult) and (a.n, a.n_runs, a.n_boot) == (b.n, b.n_runs, 100)
    assert a.n == int(sub.sum()) and a.toc["entered"] == b.toc["entered"]
    tol = dict(rel=1e-8, abs=1e-10)
    assert a.ate == pytest.approx(b.ate, **tol)
    for x, y in ((a.autoc, b.autoc), (a.qini, b.qini)):
        assert (x.estimate, x.se) == pytest.approx((y.estimate, y.se), **tol)
        assert x.lower_ci < x.estimate < x.upper_ci and 0.0 <= x.p_value <= 1.0
    assert a.toc["estimate"] == pytest.approx(b.toc["estimate"], **tol)
    assert a.toc["se"] == pytest.approx(b.toc["se"], **tol)
    assert a.crit == pytest.approx(b.crit, rel=1e-6)
    t = a.toc
    assert t["u"] == [0.1, 0.5, 1.0] and t["estimate"][-1] == 0.0 == t["se"][-1]
    for j in range(2):
        assert t["lower_ci"][j] < t["estimate"][j] < t["upper_ci"][j]
        assert t["lower_joint"][j] < t["estimate"][j] < t["upper_joint"][j]
    d = json.loads(a.json())
    assert d["autoc"]["estimate"] == a.autoc.estimate and len(d["toc"]) == 3 and d["n"] == a.n
    assert len(a.table().splitlines()) == 4 + 1 + 3 and a.boot is None
    k = DR.dml_irm_rate_lasso(Y, W, X, 0, device="cpu", keep_boot=True, **kw)
    assert k.boot.shape == (101, 5 + 6) and k.autoc == a.autoc


def test_finds_heterogeneity_and_ignores_noise():
    """tau(x) = x0. Seed 4 of this design: the reference itself gives AUTOC / SE > 3 for the
    priority x0 and |AUTOC| / SE < 3 for an independent noise priority."""
    Y, W, X = _design(1500, seed=4, tau=lambda X: X[:, 0])
    noise = np.random.default_rng(99).normal(size=len(Y))
    psi, _, _, _ = R._irm_scores(Y, W, X, 5, CPU.seed, "min", 0.01)
    inc = rng.half_sample(CPU.seed, np.arange(len(Y)), 200)
    for pr, found in ((X[:, 0], True), (noise, False)):
        ref = R.rate_from_scores(psi, pr, inc)
        r = pkg.ate_dml_irm_rate(Y, W, X, pr, run=CPU)
        print("reference", ref["autoc"] / ref["autoc_se"], "cpu", r.autoc.estimate / r.autoc.se)
        for z in (ref["autoc"] / ref["autoc_se"], r.autoc.estimate / r.autoc.se):
            assert (z > 3) if found else (abs(z) < 3)
        assert (r.autoc.p_value < 0.0027) == found


# ---------------------------------------------------------------- refusals
class _Dist:
    world, capturable, row_offset, n_total = 2, False, 0, 0


def test_refusals(small):
    Y, W, X = small
    n = len(Y)
    ok = X[:, 0].copy()
    with pytest.raises(ValueError, match="shards"):
        DR.dml_irm_rate_lasso(Y, W, X, ok, device="cpu", dist=_Dist())
    with pytest.raises(ValueError, match="clusters"):
        pkg.ate_dml_irm_rate(Y, W, X, ok, run=CPU, clusters=np.arange(n) // 3)
    with pytest.raises(ValueError, match="repeat"):
        pkg.ate_dml_irm_rate(Y, W, X, ok, run=CPU, repeats=2)
    with pytest.raises(ValueError, match="clusters"):
        DR.dml_irm_rate_lasso(Y, W, X, ok, device="cpu", clusters=np.arange(n) // 3)
    with pytest.raises(ValueError, match="repeat"):
        DR.dml_irm_rate_lasso(Y, W, X, ok, device="cpu", repeats=3)
    bad = ok.copy()
    bad[7] = np.inf
    with pytest.raises(ValueError, match="finite"):
        pkg.ate_dml_irm_rate(Y, W, X, bad, run=CPU)
    with pytest.raises(ValueError, match="finite"):
        pkg.ate_dml_irm_rate(Y, W, X, np.where(np.arange(n) == 9, np.nan, ok), run=CPU)
    few = np.arange(n) < 127
    with pytest.raises(ValueError, match="at least 128"):
        pkg.ate_dml_irm_rate(Y, W, X, ok, subset=few, run=CPU)
    with pytest.raises(ValueError, match="enters 15 rows"):
        pkg.ate_dml_irm_rate(Y, W, X, ok, q=[0.01, 1.0], run=CPU)
    for q in ([], np.arange(1, 66) / 65.0, [0.5, 0.5], [0.6, 0.4], [0.0, 1.0], [0.5, 1.01],
              [np.nan]):
        with pytest.raises(ValueError, match="q must"):
            pkg.ate_dml_irm_rate(Y, W, X, ok, q=q, run=CPU)
    for nb in (0, 4097, 2.5):
        with pytest.raises(ValueError, match="n_boot"):
            pkg.ate_dml_irm_rate(Y, W, X, ok, n_boot=nb, run=CPU)
    with pytest.raises(ValueError, match="one value per row"):
        pkg.ate_dml_irm_rate(Y, W, X, ok[:-1], run=CPU)
    with pytest.raises(ValueError, match="index the"):
        pkg.ate_dml_irm_rate(Y, W, X, X.shape[1], run=CPU)
    with pytest.raises(ValueError, match="boolean mask"):
        pkg.ate_dml_irm_rate(Y, W, X, ok, subset=np.ones(n), run=CPU)
    with pytest.raises(ValueError, match="propensity"):
        pkg.ate_dml_irm_rate(Y, W, X, ok, propensity="probit", run=CPU)
    # a non-finite priority off the evaluation rows is nobody's business
    r = pkg.ate_dml_irm_rate(Y, W, X, bad, subset=np.arange(n) != 7, n_boot=16, folds=3, run=CPU)
    assert r.n == n - 1
    # 64 rows entered by ties is enough: the first grid point takes its whole run
    tied = np.where(np.arange(n) < 64, 5.0, -np.arange(n, dtype=np.float64))
    assert DR.check_rows(tied, None, np.array([0.001, 1.0]), n)[2] == n
    with pytest.raises(ValueError, match="enters 63 rows"):
        DR.check_rows(np.where(np.arange(n) < 63, 5.0, -np.arange(n, dtype=np.float64)), None,
                      np.array([0.001, 1.0]), n)


def test_refuses_2_pow_27_rows_before_touching_them():
    """W_b <= n^2 must stay below 2^53. The row check runs on the host before anything is
    built, so zero-stride views stand in for the 2^27 rows."""
    big = 1 << 27
    pr = np.broadcast_to(np.float64(1.0), (big,))
    with pytest.raises(ValueError, match=r"2\^27"):
        DR.check_rows(pr, np.broadcast_to(np.True_, (big,)), np.array([1.0]), big)
    sub = np.zeros(big, dtype=bool)
    sub[:1000] = True                                     # the limit is on the evaluation rows
    assert DR.check_rows(pr, sub, np.array([1.0]), big)[2] == 1000


# ---------------------------------------------------------------- CLI
def test_cli_rate_prints_finite_json(capsys):
    from ate_replication_causalml_amd import cli
    assert cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64",
                     "--rate-col", "0", "--rate-grid", "4", "--boot", "100"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["n_boot"] == 100 and out["n"] == 3000 and out["n_runs"] == 3000
    assert [t["u"] for t in out["toc"]] == [0.25, 0.5, 0.75, 1.0]
    assert [t["entered"] for t in out["toc"]] == [750, 1500, 2250, 3000]
    assert np.isfinite([out["autoc"]["estimate"], out["autoc"]["se"], out["qini"]["estimate"],
                        out["qini"]["se"], out["crit"], out["ate"]]).all()
    assert out["autoc"]["se"] > 0 and out["toc"][-1]["estimate"] == 0.0
    for other in (["--gate-col", "1"], ["--cate-col", "1"], ["--policy-cols", "1,2"],
                  ["--sensitivity"], ["--targets", "all"], ["--repeats", "2"]):
        with pytest.raises(SystemExit, match="--rate-col is an analysis of its own"):
            cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64",
                      "--rate-col", "0", *other])
    with pytest.raises(SystemExit, match="--rate-grid"):
        cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64",
                  "--rate-col", "0", "--rate-grid", "65"])
