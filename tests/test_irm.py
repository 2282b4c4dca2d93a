"""DML-IRM (cross-fitted AIPW with CV-LASSO nuisances, estimators/irm.py) on the CPU path:
the device orchestration against the row-by-row float64 reference twin, the per-set target
option of the CV path launcher, the score-moment twin against a plain loop, the arm-split
panel generator, row sharding, input validation and the public surface."""
import json

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.ops.enet import cv_enet_gaussian
from ate_replication_causalml_amd.ops.gram import gram
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel.comm import run_simulated
from ate_replication_causalml_amd.reference import estimators as R


@pytest.fixture(scope="module")
def df_mod():
    from ate_replication_causalml_amd.data.dgp import make_tutorial_data
    from ate_replication_causalml_amd.data.selection import apply_selection_bias
    mod, _ = apply_selection_bias(make_tutorial_data(50_000, seed=1991))
    assert mod.X.shape == (9416, 21)
    return mod


@pytest.fixture(scope="module")
def fits(df_mod):
    """(device orchestration on the CPU, reference twin) per clip, computed once."""
    m = df_mod
    return {clip: (DI.dml_irm_lasso(m.Y, m.W, m.X, clip=clip, device="cpu"),
                   R.dml_irm_lasso(m.Y, m.W, m.X, clip=clip)) for clip in (0.01, 0.05)}


def test_matches_reference_twin(fits):
    dev, ref = fits[0.01]
    assert dev.ate == pytest.approx(ref.ate, rel=1e-9)
    assert dev.se == pytest.approx(ref.se, rel=1e-9)
    assert dev.diagnostics["n_clipped"] == 0 and ref.diagnostics["n_clipped"] == 0
    assert dev.diagnostics["n"] == 9416
    assert dev.diagnostics["n_treated"] == ref.diagnostics["n_treated"]
    for k in ("rmse_g0", "rmse_g1", "rmse_m"):
        assert dev.diagnostics[k] == pytest.approx(ref.diagnostics[k], rel=1e-9)
    # the prototype's numbers; between the naive and the oracle rows of the replication
    assert dev.ate == pytest.approx(0.08860, abs=5e-6) and dev.se == pytest.approx(0.01446, abs=5e-6)


def test_clipping_counts_and_still_matches(fits):
    # the LASSO propensity's minimum on this data is 0.033: rows clip at 0.05
    dev, ref = fits[0.05]
    assert ref.diagnostics["n_clipped"] > 0
    assert dev.diagnostics["n_clipped"] == ref.diagnostics["n_clipped"]
    assert dev.ate == pytest.approx(ref.ate, rel=1e-9)
    assert dev.se == pytest.approx(ref.se, rel=1e-9)
    assert dev.ate != fits[0.01][0].ate


# ---------------------------------------------------------------- full_y of the CV launcher
def _three_seg_panel():
    rs = np.random.RandomState(5)
    n, p = 420, 12
    X = rs.randn(n, p)
    W = (rs.rand(n) < 1 / (1 + np.exp(-X[:, 0]))).astype(float)
    Y = X[:, :3] @ [1.0, -0.5, 0.25] + 0.5 * W + rs.randn(n)
    pan = build_panel(X, W, Y, folds=rs.randint(0, 3, n), dtype="f64")
    return pan, gram(pan)


_FIELDS = ("lambdas", "nlam", "cvm", "cvsd", "sel", "coef_path", "coef_min", "coef_1se", "npass")


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    for f in _FIELDS:
        x, y = getattr(a, f)[rows_a].numpy(), getattr(b, f)[rows_b].numpy()
        np.testing.assert_allclose(x, y, rtol=0, atol=0, equal_nan=True, err_msg=f)


def test_full_y_default_is_unchanged():
    pan, G = _three_seg_panel()
    ycols = [pan.cols["Y"], pan.cols["W"]]
    base = cv_enet_gaussian(G, pan, pan.xcols, ycols)
    _same(base, cv_enet_gaussian(G, pan, pan.xcols, ycols, full_y=None))
    assert base.full_keys == [(0, 0), (0, 1)]
    # the default is every target for every full set: the same two problems, named one by one
    split = cv_enet_gaussian(G, pan, pan.xcols, ycols, full_sets=[[0, 1, 2], [0, 1, 2]],
                             full_y=[0, 1])
    assert split.full_keys == [(0, 0), (1, 1)]
    _same(base, split)


def test_full_y_equals_per_target_calls():
    pan, G = _three_seg_panel()
    ycols = [pan.cols["Y"], pan.cols["W"]]
    both = cv_enet_gaussian(G, pan, pan.xcols, ycols, full_sets=[[0, 1], [1, 2], [0, 2]],
                            full_y=[0, 1, 0])
    assert both.coef_min.shape[0] == 3
    for i, (fs, y) in enumerate((([0, 1], 0), ([1, 2], 1), ([0, 2], 0))):
        one = cv_enet_gaussian(G, pan, pan.xcols, [ycols[y]], full_sets=[fs])
        _same(both, one, slice(i, i + 1), slice(0, 1))
    with pytest.raises(ValueError):
        cv_enet_gaussian(G, pan, pan.xcols, ycols, full_sets=[[0, 1], [1, 2]], full_y=[0])
    with pytest.raises(ValueError):
        cv_enet_gaussian(G, pan, pan.xcols, ycols, full_sets=[[0, 1]], full_y=[2])


def test_one_arm_training_sets_do_not_poison():
    """The W statistics of a one-arm training set (zero variance) are computed for every
    (training set, y) pair but named by no problem: every output stays finite."""
    rs = np.random.RandomState(2)
    n, p = 300, 6
    X = rs.randn(n, p)
    W = (rs.rand(n) < 0.4).astype(float)
    Y = X[:, 0] + W + rs.randn(n)
    res, mom, cv = DI.irm_crossfit_panel(
        build_panel(X, W, Y, folds=2 * rs.randint(0, 3, n) + W.astype(int), dtype="f64"), 3)
    assert torch.isfinite(res).all() and torch.isfinite(mom).all()
    assert torch.isfinite(cv.coef_min).all() and torch.isfinite(cv.cvm[:, 0]).all()
    assert cv.full_keys == [(f, (0, 0, 1)[f % 3]) for f in range(9)]


# ---------------------------------------------------------------- score moments twin
def _loop_moments(X, W, Y, seg, coef, clip, spf):
    mom = np.zeros(8)
    for i in range(len(Y)):
        c = coef[seg[i] // spf]
        g0, g1, m = (c[r, 0] + c[r, 1:] @ X[i] for r in range(3))
        e = min(max(m, clip), 1 - clip)
        psi = g1 - g0 + W[i] * (Y[i] - g1) / e - (1 - W[i]) * (Y[i] - g0) / (1 - e)
        mom += [psi, psi * psi, 1.0, float(m < clip or m > 1 - clip), W[i] * (Y[i] - g1) ** 2,
                (1 - W[i]) * (Y[i] - g0) ** 2, (W[i] - m) ** 2, W[i]]
    return mom


@pytest.mark.parametrize("spf", [1, 2])
def test_score_moments_twin_vs_loop(spf):
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
    got = DI.irm_score_moments(pan, torch.from_numpy(coef), 0.2, spf).numpy()
    want = _loop_moments(X, W, Y, seg, coef, 0.2, spf)
    assert 0 < want[3] < n
    np.testing.assert_allclose(got, want, rtol=1e-12)
    assert got[2] == n and got[7] == W.sum() and got[3] == want[3]
    np.testing.assert_allclose(DI.irm_finalize(torch.from_numpy(want)).numpy(),
                               [want[0] / n, np.sqrt((want[1] - want[0] ** 2 / n) / (n - 1) / n)],
                               rtol=1e-14)


def test_score_moments_rejects_wrong_coef_shape():
    pan = build_panel(np.zeros((8, 2)), np.arange(8) % 2, np.zeros(8), folds=np.arange(8) % 4)
    with pytest.raises(ValueError):
        DI.irm_score_moments(pan, torch.zeros(1, 3, 3), 0.01, 2)     # 4 segments need 2 blocks
    with pytest.raises(ValueError):
        DI.irm_score_moments(pan, torch.zeros(2, 2, 3), 0.01, 2)


# ---------------------------------------------------------------- arm-split panel generator
def _rows(pan):
    v = pan.valid() != 0
    return pan.colmajor()[:, v].double().numpy().T


@pytest.mark.parametrize("dgp", ["rct", "tutorial"])
def test_arm_split_panel_is_a_reordering(dgp):
    base = synthetic_panel(3000, p=24, dtype="f64", dgp=dgp)
    split = synthetic_panel(3000, p=24, dtype="f64", dgp=dgp, arm_split=True)
    assert split.nseg == 2 * base.nseg and split.n == base.n == 3000
    assert split.cols == base.cols and split.xcols == base.xcols
    a, b = _rows(base), _rows(split)
    order = lambda m: m[np.lexsort(m.T[::-1])]
    assert np.array_equal(order(a), order(b))            # the same rows, bit for bit
    rid = split.row_index.numpy()
    assert np.array_equal(np.sort(rid[rid >= 0]), np.arange(3000))
    W = split.col("W").numpy()
    for s, (r0, _) in enumerate(split.seg_bounds):
        seg_w = W[r0:r0 + split.seg_nreal[s]]
        assert split.seg_nreal[s] > 0 and np.all(seg_w == s % 2)
        assert np.all(np.diff(rid[r0:r0 + split.seg_nreal[s]]) > 0)   # stable: fold order kept
        # the rows come from fold s // 2 of the unsplit panel
        b0, b1 = base.seg_bounds[s // 2]
        assert np.isin(rid[r0:r0 + split.seg_nreal[s]], base.row_index.numpy()[b0:b1]).all()
    Gs, Gb = gram(split), gram(base)
    np.testing.assert_allclose((Gs[0::2] + Gs[1::2]).numpy(), Gb.numpy(), rtol=1e-12, atol=0)


def test_arm_split_blocked_bf16_matches_column_major():
    cm = synthetic_panel(3000, p=24, dtype="bf16", arm_split=True)
    bl = synthetic_panel(3000, p=24, dtype="bf16", arm_split=True, blocked=True)
    assert bl.blocked and torch.equal(bl.colmajor(), cm.data)
    assert np.array_equal(bl.seg_nreal, cm.seg_nreal)


def test_arm_split_rejects_align():
    with pytest.raises(ValueError):
        synthetic_panel(3000, p=24, dtype="f64", arm_split=True, align=64)


# ---------------------------------------------------------------- row sharding
def test_row_sharded_matches_single_rank():
    one = synthetic_panel(1500, p=24, dtype="f64", arm_split=True)
    res1, mom1, _ = DI.irm_crossfit_panel(one, 5)
    assert torch.isfinite(res1).all() and mom1[2] == 1500

    def body(comm):
        pan = synthetic_panel(1500, p=24, dtype="f64", arm_split=True, comm=comm)
        res, mom, _ = DI.irm_crossfit_panel(pan, 5, comm=comm)
        return res.numpy(), mom.numpy(), pan.n

    for world in (2, 3):
        out = run_simulated(world, body)
        assert sum(n for _, _, n in out) == 1500
        for res, mom, _ in out:
            # the bound of reordered fp64 sums (tests/test_gpu.py, sharded DML)
            np.testing.assert_allclose(res, res1.numpy(), rtol=1e-9)
            assert mom[2] == 1500 and mom[7] == mom1[7] and mom[3] == mom1[3]


# ---------------------------------------------------------------- validation
def test_non_binary_treatment_raises():
    rs = np.random.RandomState(0)
    X, Y = rs.randn(60, 3), rs.randn(60)
    W = (rs.rand(60) < 0.5).astype(float)
    W[7] = 0.5
    with pytest.raises(ValueError, match="binary"):
        DI.dml_irm_lasso(Y, W, X, device="cpu")
    with pytest.raises(ValueError, match="binary"):
        R.dml_irm_lasso(Y, W, X)


def test_empty_fold_arm_cell_raises():
    from ate_replication_causalml_amd.parallel import rng
    rs = np.random.RandomState(0)
    n = 60
    X, Y = rs.randn(n, 3), rs.randn(n)
    fid = rng.fold_ids(n, 5, 1991, 0)
    W = (rs.rand(n) < 0.5).astype(float)
    W[fid == 3] = 0.0                                    # fold 3 has no treated row
    with pytest.raises(ValueError, match=r"fold 3, arm W=1"):
        DI.dml_irm_lasso(Y, W, X, device="cpu")
    with pytest.raises(ValueError, match=r"fold 3, arm W=1"):
        R.dml_irm_lasso(Y, W, X)
    pan = build_panel(X, W, Y, folds=2 * fid + W.astype(int))
    with pytest.raises(ValueError, match=r"fold 3, arm W=1"):
        DI.irm_crossfit_panel(pan, 5)


# ---------------------------------------------------------------- public surface
def test_api_backends(df_mod, fits):
    import ate_replication_causalml_amd as pkg
    from ate_replication_causalml_amd.config import RunConfig
    m = df_mod
    dev, ref = fits[0.01]
    r = pkg.ate_dml_irm(m.Y, m.W, m.X, run=RunConfig(backend="reference"))
    assert (r.ate, r.se) == (ref.ate, ref.se) and r.method == "DML-IRM cross-fit (LASSO)"
    c = pkg.ate_dml_irm(m.Y, m.W, m.X, run=RunConfig(backend="cpu"))
    assert (c.ate, c.se) == (dev.ate, dev.se)
    assert c.diagnostics["n_clipped"] == 0 and c.diagnostics["hipgraph"] is False


def test_cli_irm_prints_finite_json(capsys):
    from ate_replication_causalml_amd import cli
    assert cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(out) == {"ate", "se", "lower_ci", "upper_ci", "n_clipped"}
    assert all(np.isfinite(out[k]) for k in out) and out["se"] > 0
    assert out["n_clipped"] == int(out["n_clipped"]) >= 0
