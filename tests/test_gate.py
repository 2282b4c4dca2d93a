"""Group ATEs of DML-IRM with a multiplier-bootstrap joint band (estimators/gate.py) on the
CPU path: the Rademacher bit mapping, the device orchestration (torch twins) against the
row-by-row float64 reference twin, the overall ATE against ate_dml_irm, calibration of the
critical value, row sharding, input validation and the public surface."""
import json

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
from ate_replication_causalml_amd.estimators import gate as DG
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.parallel.comm import run_simulated
from ate_replication_causalml_amd.reference import estimators as R
from ate_replication_causalml_amd.result import boot_rank


def _quartiles(x):
    return np.digitize(x, np.quantile(x, [0.25, 0.5, 0.75]))


@pytest.fixture(scope="module")
def fits(tutorial):
    """(device orchestration on the CPU, reference twin) on df_mod with 4 groups, once."""
    _, m, _ = tutorial
    lab = _quartiles(m.X[:, 0])
    return (DG.dml_irm_gate_lasso(m.Y, m.W, m.X, lab, device="cpu", keep_boot=True),
            R.dml_irm_gate(m.Y, m.W, m.X, lab, keep_boot=True))


# ---------------------------------------------------------------- multipliers
def test_rademacher_bit_mapping():
    B, seed = 200, 1991                      # replicates 31/32, 127/128, a partial 2nd stream
    idx = np.array([0, 1, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 33, 2 ** 33 + 7, 2 ** 40 + 3], dtype=np.uint64)
    xi = rng.rademacher(seed, idx, B)
    assert xi.shape == (len(idx), B) and xi.dtype == np.int8
    assert rng.P_MULT == 9
    for r, i in enumerate(idx):
        for b in range(B):
            q = b % 128
            w = rng.random_u32(seed, rng.P_MULT, b // 128, np.uint64(i))[q // 32]
            assert xi[r, b] == (1 if (int(w) >> (q % 32)) & 1 else -1), (i, b)
    assert set(np.unique(xi)) == {-1, 1}
    # rows >= 2^32 are keyed by the whole id, and other seeds give other draws
    assert not np.array_equal(xi[0], xi[4]) and not np.array_equal(xi[5], xi[6])
    assert not np.array_equal(xi, rng.rademacher(seed + 1, idx, B))
    assert np.array_equal(rng.rademacher(seed, idx, 1), xi[:, :1])


def test_boot_rank():
    assert boot_rank(0.95, 999) == 950 and boot_rank(0.95, 200) == 190
    assert boot_rank(0.95, 2048) == 1946 and boot_rank(0.95, 1) == 1
    with pytest.raises(ValueError):
        boot_rank(1.0, 10)


# ---------------------------------------------------------------- twin
def test_matches_reference_twin(fits):
    dev, ref = fits
    assert dev.labels == ref.labels == [0, 1, 2, 3] and dev.n == ref.n and sum(dev.n) > 1000
    np.testing.assert_allclose(dev.ate, ref.ate, rtol=1e-12)
    np.testing.assert_allclose(dev.se, ref.se, rtol=1e-12)
    assert dev.crit == pytest.approx(ref.crit, rel=1e-12)
    assert np.array_equal(dev.boot["Z"], ref.boot["Z"])              # exact integers
    assert dev.boot["Z"].shape == (999, 4) and np.abs(dev.boot["Z"]).max() > 0
    scale = np.abs(ref.boot["A"]).max()
    np.testing.assert_allclose(dev.boot["A"], ref.boot["A"], rtol=0, atol=1e-12 * scale)
    assert dev.n_boot == 999 and dev.level == 0.95
    # a joint band is wider than the pointwise one and narrower than Bonferroni's at 4 x 1e-3
    assert 1.96 < dev.crit < 3.5
    for g in range(4):
        assert dev.lower_joint[g] < dev.lower_ci[g] < dev.ate[g] < dev.upper_ci[g] < dev.upper_joint[g]
        assert dev.upper_joint[g] == pytest.approx(dev.ate[g] + dev.crit * dev.se[g], rel=1e-14)


def test_overall_equals_ate_dml_irm(tutorial, fits):
    _, m, _ = tutorial
    dev, ref = fits
    one = DI.dml_irm_lasso(m.Y, m.W, m.X, device="cpu")
    assert dev.overall.ate == pytest.approx(one.ate, rel=1e-12)
    assert dev.overall.se == pytest.approx(one.se, rel=1e-12)
    assert ref.overall.ate == pytest.approx(one.ate, rel=1e-9)        # the bound of the IRM twin
    assert dev.overall.diagnostics["n"] == len(m.Y)


def test_scores_twin_sums_to_the_moments():
    pan = synthetic_panel(1500, p=24, dtype="f64", arm_split=True)
    _, _, cv = DI.irm_crossfit_panel(pan, 5)
    coef = cv.coef_min.reshape(5, 3, -1).double()
    psi = DI.irm_scores(pan, coef, 0.01, 2)
    mom = DI.irm_score_moments(pan, coef, 0.01, 2)
    assert psi.shape == (pan.ld,) and torch.all(psi[pan.row_index < 0] == 0)
    assert psi.sum().item() == pytest.approx(mom[0].item(), rel=1e-12)
    assert (psi * psi).sum().item() == pytest.approx(mom[1].item(), rel=1e-12)


# ---------------------------------------------------------------- calibration
def _crit(psi, codes, G, B, seed):
    n = len(psi)
    buf = DG.group_boot(torch.from_numpy(psi), torch.from_numpy(codes.astype(np.int32)),
                        torch.arange(n), G, B, seed)
    fin = DG.gate_finalize(buf, G, B, 0.95).numpy()
    ref = R.gate_from_scores(psi, codes, G, B, 0.95, seed)
    assert fin[3 * G] == pytest.approx(ref[3], rel=1e-12)
    return fin[3 * G]


@pytest.mark.parametrize("seed", [1991, 7, 12345])
def test_crit_is_calibrated(seed):
    """Independent heavy-tailed scores in disjoint groups: the maximal |t| over G groups is
    that of G independent normals, whose 95% point is the Sidak value."""
    rs = np.random.RandomState(3)
    n, B = 1500, 2048
    psi = rs.standard_t(5, n) * 3 + 0.1
    c4 = _crit(psi, np.arange(n) % 4, 4, B, seed)
    c1 = _crit(psi, np.zeros(n, dtype=np.int64), 1, B, seed)
    print("seed", seed, "crit G=4", c4, "G=1", c1)
    assert abs(c4 - 2.4909) < 0.15
    assert abs(c1 - 1.96) < 0.15


# ---------------------------------------------------------------- row sharding
def test_row_sharded_matches_single_rank():
    edges = torch.tensor([-0.5, 0.0, 0.6], dtype=torch.float64)

    def run(comm):
        pan = synthetic_panel(1500, p=24, folds=3, dtype="f64", arm_split=True, comm=comm)
        gid = DG.bin_groups(pan, "x0", edges)
        fin, boot, _ = DG.irm_gate_panel(pan, gid, 3, n_boot=200, comm=comm)
        return fin.numpy(), boot.numpy(), pan.n

    fin1, boot1, n1 = run(None)
    G, B = 4, 200
    assert n1 == 1500 and len(fin1) == 3 * G + 3 and fin1[2 * G:3 * G].sum() == 1500
    assert np.isfinite(fin1).all() and fin1[2 * G:3 * G].min() > 50
    for world in (2, 3):
        out = run_simulated(world, run)
        assert sum(n for _, _, n in out) == 1500
        for fin, boot, _ in out:
            assert np.array_equal(boot[3 * G + B * G:], boot1[3 * G + B * G:])      # Z: exact
            assert np.array_equal(fin[2 * G:3 * G], fin1[2 * G:3 * G])              # n_g
            print("world", world, "max rel", np.abs(fin / fin1 - 1).max())
            np.testing.assert_allclose(fin, fin1, rtol=1e-12)


# ---------------------------------------------------------------- validation
def test_value_errors():
    rs = np.random.RandomState(0)
    n = 400
    X, Y = rs.randn(n, 3), rs.randn(n)
    W = (rs.rand(n) < 0.5).astype(float)
    ok = np.arange(n) % 4
    for fn, kw in ((DG.dml_irm_gate_lasso, dict(device="cpu")), (R.dml_irm_gate, {})):
        with pytest.raises(ValueError, match="64 groups"):
            fn(Y, W, X, np.arange(n) % 65, **kw)
        lonely = ok.copy()
        lonely[5] = 9                                    # a group of one row
        with pytest.raises(ValueError, match="at least 2"):
            fn(Y, W, X, lonely, **kw)
        with pytest.raises(ValueError, match="one label per row"):
            fn(Y, W, X, ok[:-1], **kw)
        for bad in (0, 4097, 10.5):
            with pytest.raises(ValueError, match="n_boot"):
                fn(Y, W, X, ok, n_boot=bad, **kw)
    with pytest.raises(ValueError):
        DG.group_boot(torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.int32),
                      torch.arange(8), 65, 10, 1)
    with pytest.raises(ValueError):
        DG.group_boot(torch.zeros(8, dtype=torch.float64), torch.zeros(7, dtype=torch.int32),
                      torch.arange(8), 2, 10, 1)


# ---------------------------------------------------------------- public surface
def test_api_backends_and_result(tutorial, fits):
    import ate_replication_causalml_amd as pkg
    from ate_replication_causalml_amd.config import RunConfig
    _, m, _ = tutorial
    dev, ref = fits
    lab = _quartiles(m.X[:, 0])
    r = pkg.ate_dml_irm_gate(m.Y, m.W, m.X, lab, run=RunConfig(backend="reference"))
    assert isinstance(r, pkg.GateResult) and (r.ate, r.se, r.crit) == (ref.ate, ref.se, ref.crit)
    names = np.array(["d", "a", "c", "b"])[lab]              # arbitrary labels, sorted by unique
    c = pkg.ate_dml_irm_gate(m.Y, m.W, m.X, names, run=RunConfig(backend="cpu"))
    assert c.labels == ["a", "b", "c", "d"] and c.diagnostics["hipgraph"] is False
    assert [c.ate[i] for i in (3, 0, 2, 1)] == dev.ate and c.crit == pytest.approx(dev.crit, rel=1e-12)
    rows = c.rows()
    assert len(rows) == 4 and set(rows[0]) == {"group", "n", "ATE", "se", "lower_ci", "upper_ci",
                                               "lower_joint", "upper_joint"}
    d = json.loads(c.to_json())
    assert d["crit"] == c.crit and len(d["groups"]) == 4 and d["overall"]["ate"] == c.overall.ate
    assert len(c.table().splitlines()) == 7


def test_cli_gate_prints_finite_json(capsys):
    from ate_replication_causalml_amd import cli
    assert cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64",
                     "--gate-col", "0", "--gate-bins", "3", "--boot", "300"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["n_boot"] == 300 and len(out["groups"]) == 3 and len(out["edges"]) == 2
    assert sum(g["n"] for g in out["groups"]) == 3000
    for g in out["groups"]:
        assert all(np.isfinite(v) for v in g.values()) and g["se"] > 0
        assert g["lower_joint"] < g["lower_ci"] < g["upper_ci"] < g["upper_joint"]
    assert np.isfinite([out["crit"], out["ate"], out["se"]]).all() and out["crit"] > 1.96
