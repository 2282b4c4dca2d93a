"""Cluster-robust DML on the CPU path (estimators/cluster.py): the layout (whole clusters per
fold, the CSR over panel rows, the refusals), singleton clusters against the unclustered
estimators, row-permutation invariance, the device orchestration against the reference twin,
and the variance formula alone against its exact expectation."""
import json

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import api
from ate_replication_causalml_amd.config import RunConfig
from ate_replication_causalml_amd.estimators import cluster as DC
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.reference import estimators as R

N, P, K = 600, 8, 3
CPU = RunConfig(backend="cpu")
REF = RunConfig(backend="reference")
# two summation orders of n terms: the bound of the issue for SE (and theta) agreement
ORDER_BOUND = 16 * N * 2.0 ** -53
ESTIMATORS = (api.ate_dml, api.ate_dml_irm)


@pytest.fixture(scope="module")
def data():
    rs = np.random.default_rng(0)
    X = rs.normal(size=(N, P))
    W = (rs.uniform(size=N) < 1 / (1 + np.exp(-0.5 * X[:, 0]))).astype(float)
    Y = X[:, 0] + 0.5 * W + rs.normal(size=N)
    return Y, W, X


def _mixed_clusters(n, rs):
    """Clusters of sizes 1..7 (cycled) and one holding a third of the rows, rows shuffled."""
    big = n // 3
    sizes, s = [], 0
    while s < n - big:
        sizes.append(min(1 + len(sizes) % 7, n - big - s))
        s += sizes[-1]
    sizes.append(big)
    return rs.permutation(np.repeat(np.arange(len(sizes)), sizes)), sizes


# ---------------------------------------------------------------- layout
def test_layout_puts_whole_clusters_in_balanced_folds():
    rs = np.random.default_rng(1)
    cl, sizes = _mixed_clusters(N, rs)
    lay = DC.cluster_layout(cl, N, K, 1991)
    assert lay.J == len(sizes) and lay.codes.shape == (N,) and lay.fid.shape == (N,)
    for j in range(lay.J):
        assert len(set(lay.fid[lay.codes == j])) == 1          # exactly one fold per cluster
    per_fold = np.bincount([lay.fid[lay.codes == j][0] for j in range(lay.J)], minlength=K)
    assert per_fold.max() - per_fold.min() <= 1                 # balanced over clusters
    assert np.array_equal(lay.fid, rng.fold_ids(lay.J, K, 1991, 0)[lay.codes])
    assert np.array_equal(np.sort(lay.perm), np.arange(N))
    assert np.all(np.diff(lay.codes[lay.perm]) >= 0)            # sorted by cluster, stably
    for j in (0, lay.J - 1):
        assert np.all(np.diff(lay.perm[lay.codes[lay.perm] == j]) > 0)


def test_singleton_labels_give_the_row_level_folds():
    lay = DC.cluster_layout(np.arange(N), N, K, 7)
    assert np.array_equal(lay.fid, rng.fold_ids(N, K, 7, 0))
    assert np.array_equal(lay.perm, np.arange(N)) and lay.J == N


def test_string_and_integer_labels_give_the_same_layout():
    rs = np.random.default_rng(2)
    ints = rs.integers(0, 90, size=N)
    strs = np.array([f"hh{v:04d}" for v in ints])               # the same order as the integers
    a, b = DC.cluster_layout(ints, N, K, 3), DC.cluster_layout(strs, N, K, 3)
    assert a.J == b.J
    for f in ("codes", "fid", "perm"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_csr_names_panel_rows_in_runs_and_never_padding():
    rs = np.random.default_rng(3)
    cl, sizes = _mixed_clusters(N, rs)
    lay = DC.cluster_layout(cl, N, K, 1991)
    W = (rs.uniform(size=N) < 0.5).astype(float)
    q = lay.perm
    seg = 2 * lay.fid[q] + W[q].astype(np.int64)                # the arm-split layout
    pan = build_panel(rs.normal(size=(N, 2)), W[q], rs.normal(size=N), folds=seg, device="cpu",
                      nseg=2 * K)
    starts, order = DC.cluster_csr(pan.row_index, lay.codes[q], lay.J)
    assert starts.dtype == np.int32 and order.dtype == np.int32
    assert starts[0] == 0 and starts[-1] == N == len(order) and len(starts) == lay.J + 1
    assert np.array_equal(np.diff(starts), np.bincount(lay.codes, minlength=lay.J))
    ri = pan.row_index.numpy()
    assert pan.ld > N and np.all(ri[order] >= 0)                # there is padding; none named
    assert np.array_equal(np.sort(order), np.flatnonzero(ri >= 0))
    for j in range(lay.J):
        rows = order[starts[j]:starts[j + 1]]
        assert np.all(lay.codes[q][ri[rows]] == j)
        assert np.all(np.diff(rows) > 0)
        assert 1 + np.count_nonzero(np.diff(rows) != 1) <= 2    # at most segs_per_fold runs


def test_refusals(data, monkeypatch):
    Y, W, X = data
    ok = np.arange(N) // 2
    with pytest.raises(ValueError, match="labels"):
        DC.cluster_layout(ok[:-1], N, K, 1)
    with pytest.raises(ValueError, match="labels"):
        DC.cluster_layout(ok.reshape(2, -1), N, K, 1)
    nan = ok.astype(float)
    nan[5] = np.nan
    with pytest.raises(ValueError, match="NaN or None"):
        DC.cluster_layout(nan, N, K, 1)
    none = np.array([f"c{v}" for v in ok], dtype=object)
    none[7] = None
    with pytest.raises(ValueError, match="NaN or None"):
        DC.cluster_layout(none, N, K, 1)
    with pytest.raises(ValueError, match="at least"):
        DC.cluster_layout(np.zeros(N, dtype=int), N, 1, 1)      # J = 1 < 2
    with pytest.raises(ValueError, match="at least"):
        DC.cluster_layout(np.arange(N) % 4, N, 5, 1)            # J = 4 < K = 5
    with pytest.raises(ValueError, match="dist"):
        DC.cluster_layout(ok, N, K, 1, dist=object())
    with pytest.raises(ValueError, match="repeats"):
        DC.cluster_layout(ok, N, K, 1, repeats=2)
    monkeypatch.setattr(DC, "INT_MAX", N)                       # n at the limit
    with pytest.raises(ValueError, match="2\\^31"):
        DC.cluster_layout(ok, N, K, 1)
    monkeypatch.undo()
    for f in ESTIMATORS:
        with pytest.raises(ValueError, match="repeats"):
            f(Y, W, X, folds=K, run=CPU, clusters=ok, repeats=2)
        with pytest.raises(ValueError, match="labels"):
            f(Y, W, X, folds=K, run=REF, clusters=ok[:-1])
    # the (fold, arm) cell check of IRM still applies: two clusters, one per arm
    with pytest.raises(ValueError, match="empty \\(fold, arm\\) cell"):
        api.ate_dml_irm(Y, W, X, folds=2, run=CPU, clusters=W.astype(int))


# ---------------------------------------------------------------- singletons, permutation
@pytest.fixture(scope="module")
def unclustered(data):
    Y, W, X = data
    return {f.__name__: f(Y, W, X, folds=K, run=CPU) for f in ESTIMATORS}


@pytest.mark.parametrize("f", ESTIMATORS, ids=lambda f: f.__name__)
def test_singleton_clusters_reproduce_the_unclustered_estimator(data, unclustered, f):
    Y, W, X = data
    a = unclustered[f.__name__]
    b = f(Y, W, X, folds=K, run=CPU, clusters=np.arange(N))
    print(f.__name__, a.ate, b.ate, a.se, b.se, abs(b.se / a.se - 1), ORDER_BOUND)
    assert b.ate == a.ate                                       # the same launch, the same bits
    assert abs(b.se - a.se) <= ORDER_BOUND * a.se
    assert b.diagnostics["se_unclustered"] == a.se
    assert b.diagnostics["n_clusters"] == N and b.diagnostics["max_cluster"] == 1
    assert b.diagnostics["design_effect"] == 1.0


@pytest.mark.parametrize("f", ESTIMATORS, ids=lambda f: f.__name__)
def test_row_permutation_leaves_folds_and_result(data, f):
    Y, W, X = data
    rs = np.random.default_rng(4)
    cl = rs.integers(0, 150, size=N)
    q = rs.permutation(N)
    la, lb = DC.cluster_layout(cl, N, K, CPU.seed), DC.cluster_layout(cl[q], N, K, CPU.seed)
    assert np.array_equal(la.fid[q], lb.fid)                    # every row keeps its fold
    a = f(Y, W, X, folds=K, run=CPU, clusters=cl)
    b = f(Y[q], W[q], X[q], folds=K, run=CPU, clusters=cl[q])
    print(f.__name__, a.ate, b.ate, a.se, b.se)
    assert abs(b.ate - a.ate) <= ORDER_BOUND * abs(a.ate)
    assert abs(b.se - a.se) <= ORDER_BOUND * a.se
    assert a.se != a.diagnostics["se_unclustered"]


# ---------------------------------------------------------------- twin parity
def test_plr_matches_reference_twin(data):
    Y, W, X = data
    cl, sizes = _mixed_clusters(N, np.random.default_rng(5))
    a = api.ate_dml(Y, W, X, folds=K, run=CPU, clusters=cl)
    b = api.ate_dml(Y, W, X, folds=K, run=REF, clusters=cl)
    print("plr", a.ate, b.ate, a.se, b.se, a.diagnostics)
    # the bound of the unclustered CPU test of the PLR estimator (tests/test_device_cpu.py)
    assert a.ate == pytest.approx(b.ate, abs=1e-7, rel=1e-7)
    assert a.se == pytest.approx(b.se, abs=1e-7, rel=1e-7)
    assert a.diagnostics["se_unclustered"] == pytest.approx(b.diagnostics["se_unclustered"],
                                                            abs=1e-7, rel=1e-7)
    assert a.diagnostics["n_clusters"] == b.diagnostics["n_clusters"] == len(sizes)
    assert a.diagnostics["max_cluster"] == b.diagnostics["max_cluster"] == N // 3
    assert a.diagnostics["design_effect"] == pytest.approx(b.diagnostics["design_effect"])
    # the reference's clustered theta is its fold_ids= run on the cluster folds
    c = R.dml_plr_lasso(Y, W, X, folds=K, seed=REF.seed,
                        fold_ids=R.cluster_fold_ids(cl, K, REF.seed))
    assert c.ate == b.ate and c.se == b.diagnostics["se_unclustered"]


@pytest.mark.parametrize("propensity", ["linear", "logit"])
def test_irm_matches_reference_twin(data, propensity):
    Y, W, X = data
    cl, sizes = _mixed_clusters(N, np.random.default_rng(6))
    a = api.ate_dml_irm(Y, W, X, folds=K, run=CPU, clusters=cl, propensity=propensity)
    b = api.ate_dml_irm(Y, W, X, folds=K, run=REF, clusters=cl, propensity=propensity)
    print("irm", propensity, a.ate, b.ate, a.se, b.se, a.diagnostics)
    rel = 1e-9      # the bound of the unclustered CPU tests (tests/test_irm.py, test_irm_logit.py)
    assert a.ate == pytest.approx(b.ate, rel=rel)
    assert a.se == pytest.approx(b.se, rel=rel)
    assert a.diagnostics["se_unclustered"] == pytest.approx(b.diagnostics["se_unclustered"],
                                                            rel=rel)
    assert a.diagnostics["n_clusters"] == len(sizes) and a.diagnostics["max_cluster"] == N // 3
    assert a.diagnostics.get("propensity") == b.diagnostics.get("propensity")


# ---------------------------------------------------------------- the kernel's CPU twin
def test_cluster_moments_twin_against_add_at():
    rs = np.random.default_rng(7)
    sizes = np.r_[rs.integers(1, 9, size=80), 300, 1]
    n, J = int(sizes.sum()), len(sizes)
    ld = n + 40
    order = rs.permutation(ld)[:n].astype(np.int32)             # a random gather with gaps
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    a, b = rs.normal(size=ld), rs.uniform(size=ld)
    codes = np.repeat(np.arange(J), sizes)
    for bb, theta in ((None, 0.0), (None, 0.3), (b, 0.0), (b, -1.7)):
        got = DC.cluster_moments(torch.from_numpy(a), None if bb is None else torch.from_numpy(bb),
                                 torch.from_numpy(starts), torch.from_numpy(order), J,
                                 torch.tensor([theta], dtype=torch.float64)).numpy()
        A, B = np.zeros(J), np.zeros(J)
        np.add.at(A, codes, a[order])
        np.add.at(B, codes, 1.0 if bb is None else bb[order])
        t = A - theta * B
        np.testing.assert_allclose(got[:2], [(t * t).sum(), t.sum()], rtol=1e-12, atol=1e-12)
        assert got[2] == (sizes.astype(float) ** 2).sum() and got[3] == 300
        # ... and the reference's SE is the same formula
        se = R.cluster_se(a[order], None if bb is None else bb[order], theta, codes, bb is None)
        fin = DC.cluster_finalize(torch.from_numpy(got), torch.tensor(B.sum()), J, bb is None)
        assert float(fin) == pytest.approx(se, rel=1e-12)


# ---------------------------------------------------------------- the variance formula alone
def test_cluster_se_is_unbiased_where_the_iid_formula_falls_short():
    """psi = u_c + e_i with known variances, J = 100 unequal clusters: the mean of cluster_se^2
    over 400 draws is the exact Var(mean psi) = s_u^2 sum n_j^2 / n^2 + s_e^2 / n within 10 %
    (its Monte Carlo error is about 1 %); the i.i.d. formula misses it by more than that."""
    rs = np.random.default_rng(8)
    J, s_u, s_e = 100, 1.0, 2.0
    sizes = 1 + np.arange(J) % 12
    n = int(sizes.sum())
    codes = np.repeat(np.arange(J), sizes)
    exact = s_u ** 2 * (sizes.astype(float) ** 2).sum() / n ** 2 + s_e ** 2 / n
    v_cl, v_iid = [], []
    for _ in range(400):
        psi = s_u * rs.normal(size=J)[codes] + s_e * rs.normal(size=n)
        v_cl.append(R.cluster_se(psi, None, psi.mean(), codes, True) ** 2)
        v_iid.append(psi.var(ddof=1) / n)
    v_cl, v_iid = float(np.mean(v_cl)), float(np.mean(v_iid))
    print("exact", exact, "clustered", v_cl, "iid", v_iid)
    assert abs(v_cl / exact - 1) < 0.10
    assert v_iid / exact < 0.90


# ---------------------------------------------------------------- around it
def test_clustered_data_and_cli(capsys):
    from ate_replication_causalml_amd import cli
    from ate_replication_causalml_amd.data.dgp import make_clustered_data
    d = make_clustered_data(1200, cluster_size=4, icc=0.5, seed=3, assign="cluster")
    assert d.X.shape == (1200, 21) and np.array_equal(d.clusters, np.arange(1200) // 4)
    for j in range(0, 300, 37):
        assert len(set(d.W[d.clusters == j])) == 1              # one draw per cluster
    r = make_clustered_data(1200, cluster_size=4, icc=0.5, seed=3, assign="row")
    assert any(len(set(r.W[r.clusters == j])) == 2 for j in range(300))
    with pytest.raises(ValueError):
        make_clustered_data(100, assign="household")
    for model in ("irm", "plr"):
        assert cli.main(["cluster", "--n", "1200", "--cluster-size", "4", "--icc", "0.5",
                         "--model", model, "--folds", "3", "--backend", "cpu"]) == 0
        out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert out["diagnostics"]["n_clusters"] == 300
        assert out["se"] > 1.2 * out["se_unclustered"] > 0      # sqrt(1 + 3 * 0.5) = 1.58
        assert abs(out["ate"] - out["tau_true"]) < 4 * out["se"]
