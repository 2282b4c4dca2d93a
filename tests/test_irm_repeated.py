"""Repeated cross-fitting for DML-IRM (Chernozhukov et al. 2018 §3.4): S K-fold partitions
from K*K micro-groups, one micro-arm Gram pass and one fused score pass shared by all
partitions (estimators/irm.irm_repeated_phases), median aggregation -- against the float64
row-by-row twin (reference/estimators.dml_irm_lasso_repeated), across a simulated row
sharding, through the public API and the command line."""
import json

import numpy as np
import pytest
import torch

import ate_replication_causalml_amd as ate
from ate_replication_causalml_amd.config import RunConfig
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators.lasso import micro_fold_map
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.parallel.comm import LocalComm, run_simulated
from ate_replication_causalml_amd.reference import estimators as R


def _data(n=2500, p=10, seed=3):
    """The data of tests/test_repeated_crossfit.py: ~50 rows per micro-arm cell at K = 5."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, p)
    W = (rs.rand(n) < 1 / (1 + np.exp(-X[:, 0]))).astype(float)
    Y = X[:, 1] + 0.5 * W + rs.randn(n)
    return Y, W, X


@pytest.mark.parametrize("repeats,aggregate", [(3, "median"), (4, "median"), (2, "mean")])
def test_repeated_irm_matches_reference(repeats, aggregate):
    """The device pipeline on host tensors (one micro-arm Gram stack, per-partition fold-arm
    Grams, CV-LASSO paths, the multi-split score twin, aggregate) equals the reference, which
    refits each partition row by row."""
    Y, W, X = _data()
    micro = rng.fold_ids(len(Y), 25, 1991, 0)
    assert np.bincount(2 * micro + W.astype(int), minlength=50).min() > 0   # every cell populated
    a = R.dml_irm_lasso_repeated(Y, W, X, 5, repeats, aggregate=aggregate)
    b = DI.dml_irm_lasso_repeated(Y, W, X, 5, repeats, aggregate=aggregate, device="cpu")
    sa, sb = np.array(a.diagnostics["splits"]), np.array(b.diagnostics["splits"])
    print("reference", sa.tolist(), a.ate, a.se, "device pipeline", sb.tolist(), b.ate, b.se)
    np.testing.assert_allclose(sb, sa, rtol=1e-9)
    assert b.ate == pytest.approx(a.ate, rel=1e-9) and b.se == pytest.approx(a.se, rel=1e-9)
    assert len(set(np.round(sa[:, 0], 12))) == repeats     # distinct partitions, distinct fits
    d = b.diagnostics
    assert (d["n"], d["repeats"], d["aggregate"], d["hipgraph"]) == (len(Y), repeats, aggregate,
                                                                     False)
    assert d["n_clipped"] == a.diagnostics["n_clipped"] and len(d["n_clipped"]) == repeats
    assert d["n_treated"] == int(W.sum()) == a.diagnostics["n_treated"]


def test_one_partition_is_an_irm_fit():
    """S = 1 is one cross-fitted AIPW over the folds a = micro // K."""
    Y, W, X = _data(1500, 8, 5)
    micro = rng.fold_ids(len(Y), 25, 1991, 0)
    one = R.dml_irm_lasso(Y, W, X, 5, fold_ids=micro // 5)
    r = DI.dml_irm_lasso_repeated(Y, W, X, 5, 1, device="cpu")
    assert r.ate == pytest.approx(one.ate, rel=1e-9) and r.se == pytest.approx(one.se, rel=1e-9)


def test_repeated_irm_row_sharded():
    """Row shards (thread simulator, world 3): the micro-arm Gram stack and the [S, 8]
    moments are all-reduced; the same splits and aggregate as world 1."""
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel

    def run(world, rank, comm):
        pan = synthetic_panel(3000, p=24, folds=25, seed=3, dtype="f64", device="cpu",
                              rank=rank, world=world, arm_split=True)
        assert pan.nseg == 50
        res, splits, mom = DI.irm_repeated_panel(pan, 5, 3, comm=comm)
        return res.numpy(), splits.numpy(), mom.numpy()
    ref, rsp, rmom = run(1, 0, LocalComm())
    assert rmom[:, 2].tolist() == [3000.0] * 3
    for res, sp, mom in run_simulated(3, lambda c: run(3, c.rank, c)):
        np.testing.assert_allclose(res, ref, rtol=1e-9)
        np.testing.assert_allclose(sp, rsp, rtol=1e-9)
        assert np.array_equal(mom[:, [2, 3, 7]], rmom[:, [2, 3, 7]])


def test_multi_twin_equals_single_pass_per_split():
    """The float64 twin of the multi-split pass: row t is, bit for bit, the single pass with
    the coefficient blocks gathered by blk[t]."""
    rs = np.random.RandomState(11)
    K, S, p = 3, 3, 12
    counts = rs.randint(1, 40, 2 * K * K)
    seg = rs.permutation(np.repeat(np.arange(2 * K * K), counts))
    n = len(seg)
    X, W = rs.randn(n, p), (seg & 1).astype(float)
    Y = rs.randn(n) + W
    pan = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    coef = torch.from_numpy(rs.randn(S * K, 3, p + 1) * (rs.rand(S * K, 3, p + 1) < 0.5))
    coef[:, 2] *= 0.1
    coef[:, 2, 0] = 0.5
    blk = np.stack([s * K + micro_fold_map(K, s) for s in range(S)])
    got = DI.irm_score_moments_multi(pan, coef, blk, 0.2, 2)
    assert got.shape == (S, 8)
    for s in range(S):
        want = DI.irm_score_moments(pan, coef.index_select(0, torch.from_numpy(blk[s])), 0.2, 2)
        assert torch.equal(got[s], want)
    assert 0 < got[0, 3] < n and not torch.equal(got[0], got[1])
    with pytest.raises(ValueError, match="blk entries"):
        DI.irm_score_moments_multi(pan, coef, blk + 1, 0.2, 2)
    with pytest.raises(ValueError, match="blk must be"):
        DI.irm_score_moments_multi(pan, coef, blk[:, :-1], 0.2, 2)


def test_empty_cells():
    """An empty (fold, arm) cell of a used partition is an error that names it; an empty
    micro-arm cell inside full fold cells is legal."""
    K = 3
    Y, W, X = _data(400, 4, 9)
    micro = rng.fold_ids(len(Y), K * K, 1991, 0)
    # micro-groups 0, 1, 2 are fold 0 of partition 0: no treated row there
    W0 = np.where(micro < K, 0.0, W)
    with pytest.raises(ValueError, match=r"partition 0: fold 0, arm W=1"):
        DI.dml_irm_lasso_repeated(Y, W0, X, K, 2, device="cpu")
    with pytest.raises(ValueError, match=r"partition 0: fold 0, arm W=1"):
        R.dml_irm_lasso_repeated(Y, W0, X, K, 2)
    # micro-groups 0, 5, 7 are fold 0 of partition 1 (a + b = 0 mod 3)
    assert np.flatnonzero(micro_fold_map(K, 1) == 0).tolist() == [0, 5, 7]
    W1 = np.where(np.isin(micro, (0, 5, 7)), 1.0, W)
    with pytest.raises(ValueError, match=r"partition 1: fold 0, arm W=0"):
        DI.dml_irm_lasso_repeated(Y, W1, X, K, 2, device="cpu")
    r1 = DI.dml_irm_lasso_repeated(Y, W1, X, K, 1, device="cpu")      # partition 1 is not used
    assert np.isfinite(r1.ate)
    # one micro-group without control rows: every fold cell of every partition still has rows
    W2 = np.where(micro == 4, 1.0, W)
    assert np.bincount(2 * micro + W2.astype(int), minlength=2 * K * K)[8] == 0
    a = R.dml_irm_lasso_repeated(Y, W2, X, K, 3)
    b = DI.dml_irm_lasso_repeated(Y, W2, X, K, 3, device="cpu")
    np.testing.assert_allclose(np.array(b.diagnostics["splits"]),
                               np.array(a.diagnostics["splits"]), rtol=1e-9)
    # the LAST micro-arm cell (segment 2 K*K - 1) empty: the panel keeps all 2 K*K segments
    W3 = np.where(micro == K * K - 1, 0.0, W)
    assert np.bincount(2 * micro + W3.astype(int), minlength=2 * K * K)[-1] == 0
    a = R.dml_irm_lasso_repeated(Y, W3, X, K, 3)
    b = DI.dml_irm_lasso_repeated(Y, W3, X, K, 3, device="cpu")
    np.testing.assert_allclose(np.array(b.diagnostics["splits"]),
                               np.array(a.diagnostics["splits"]), rtol=1e-9)
    assert b.ate == pytest.approx(a.ate, rel=1e-9) and b.se == pytest.approx(a.se, rel=1e-9)
    with pytest.raises(ValueError, match="repeats must be in 1..3"):
        DI.dml_irm_lasso_repeated(Y, W, X, K, 4, device="cpu")


def test_one_partition_too_large_for_a_path_launch():
    """3 K^2 problems per partition: K = 10 does not fit one path launch; refused up front."""
    from ate_replication_causalml_amd.ops.enet import MAX_PATH_PROBLEMS, cv_problem_count
    K = 10
    rs = np.random.RandomState(2)
    seg = np.repeat(np.arange(2 * K * K), 2)
    X = rs.randn(len(seg), 3)
    pan = build_panel(X, (seg & 1).astype(float), rs.randn(len(seg)), folds=seg, dtype="f64",
                      device="cpu")
    _, sets, full_y, ycols = DI.fit_problems(pan, K, np.ones(2 * K))
    assert cv_problem_count(3 * K, sets, len(ycols), full_y) == 3 * K * K > MAX_PATH_PROBLEMS
    with pytest.raises(ValueError, match="300 path problems"):
        DI.irm_repeated_phases(pan, K, 2)
    assert DI._path_launches([1e-4] * 4, 3) == [(0, 2), (2, 4)]
    assert DI._path_launches([1e-4] * 3, 3) == [(0, 3)]
    assert DI._path_launches([1e-4, 1e-2, 1e-2], 3) == [(0, 1), (1, 3)]


def test_api_repeats():
    Y, W, X = _data(1500, 8, 7)
    a = ate.ate_dml_irm(Y, W, X, repeats=3, run=RunConfig(backend="reference"))
    b = ate.ate_dml_irm(Y, W, X, repeats=3, run=RunConfig(backend="cpu"))
    assert b.ate == pytest.approx(a.ate, rel=1e-9) and b.se == pytest.approx(a.se, rel=1e-9)
    assert b.diagnostics["repeats"] == 3 and len(b.diagnostics["splits"]) == 3
    one = ate.ate_dml_irm(Y, W, X, run=RunConfig(backend="cpu"))
    assert "repeats" not in one.diagnostics                 # repeats = 1: the single fit


def test_cli_irm_repeats(capsys):
    from ate_replication_causalml_amd.cli import main
    rc = main(["dml", "--model", "irm", "--repeats", "3", "--n", "12000", "--p", "24",
               "--dtype", "f64"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rc == 0 and out["repeats"] == 3 and len(out["splits"]) == 3
    assert out["lower_ci"] < out["ate"] < out["upper_ci"] and out["se"] > 0
    with pytest.raises(SystemExit, match="ATE only"):
        main(["dml", "--model", "irm", "--repeats", "2", "--sensitivity", "--n", "12000",
              "--p", "24", "--dtype", "f64"])
