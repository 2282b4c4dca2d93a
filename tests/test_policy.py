"""Exact depth-2 policy trees on the AIPW scores of DML-IRM (estimators/policy.py) on the CPU
path: the histogram / prefix-sum search against the brute-force reference twin, recovery of
XOR-shaped and planted policies, the held-out evaluation, row sharding, NaN scores, input
validation and the public surface."""
import json

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
from ate_replication_causalml_amd.estimators import policy as DP
from ate_replication_causalml_amd.parallel.comm import run_simulated
from ate_replication_causalml_amd.parallel.dist import DistContext
from ate_replication_causalml_amd.reference import estimators as R
from ate_replication_causalml_amd.result import PolicyTreeResult


def _learn(r, X, bins, depth=2, min_leaf=1, train=None, cost=0.0):
    """The device orchestration on host tensors from given scores: (rec, fin, e, edges)."""
    n, d = X.shape
    edges = [DP.feature_edges(X[:, j], bins) for j in range(d)]
    nb = [len(ed) + 1 for ed in edges]
    codes = torch.from_numpy(np.stack([DP.bin_codes(X[:, j], edges[j]) for j in range(d)]))
    use = torch.zeros(n, dtype=torch.int8) if train is None else \
        torch.from_numpy(np.where(train, 0, 1).astype(np.int8))
    psi = torch.from_numpy(np.asarray(r, dtype=np.float64))
    c = torch.tensor([float(cost)], dtype=torch.float64)
    rg = DP.score_range(psi, c, use)
    e = DP.scale_exponent(rg, n)
    rec = DP.tree_search(DP.pair_hist(psi, c, e, use, codes, nb), nb, depth, min_leaf)
    rec = DP.mask_record(rec, rg[1])
    fin = DP.policy_finalize(DP.eval_sums(psi, c, use, codes, rec), rg[1])
    return rec.tolist(), fin.numpy(), int(e), edges


def _mixed(rs, n=300):
    """One binary, one continuous and one 5-level feature."""
    return np.stack([(rs.rand(n) < 0.4).astype(float), rs.randn(n),
                     rs.randint(0, 5, n).astype(float)], axis=1)


# ---------------------------------------------------------------- search vs brute force
@pytest.mark.parametrize("variant", ["plain", "duplicate", "scaled", "zero"])
def test_prefix_sum_search_matches_brute_force(variant):
    rs = np.random.RandomState(11)
    X = _mixed(rs)
    r = 2.0 * rs.randn(300) + 1.5 * X[:, 0] - 1.2 * (X[:, 1] > 0.3) + 0.4 * (X[:, 2] - 2)
    if variant == "duplicate":
        X = np.c_[X[:, 1], X]                       # column 0 repeats column 2
    elif variant == "scaled":
        r = r * 1e6
    elif variant == "zero":
        r = np.zeros(300)
    seen = set()
    for bins in (3, 4, 8):
        edges = [DP.feature_edges(X[:, j], bins) for j in range(X.shape[1])]
        for depth in (0, 1, 2):
            for ml in (1, 25):
                rec, fin, e, _ = _learn(r, X, bins, depth, ml)
                ref, rfin, re = R.policy_tree_from_scores(r, X, edges, None, depth, ml)
                assert rec == ref, (variant, bins, depth, ml, rec, ref)     # tree and q value
                assert e == re
                np.testing.assert_allclose(fin[0], rfin[0], rtol=1e-10, atol=1e-9)
                seen.add(tuple(rec[:6]))
                if variant == "duplicate":
                    assert 2 not in (rec[0], rec[2], rec[4])                # the smaller index
                if depth == 0 or variant == "zero":
                    assert rec[:6] == [-1] * 6
    if variant == "scaled":
        assert e < 30
    elif variant == "zero":
        assert rec[6:12] == [0, 0, 0, 0, 0, 300] and e == 30
    else:
        assert e == 30 and len(seen) > 3                                    # real trees were found


def test_pruned_and_min_leaf():
    rs = np.random.RandomState(2)
    X = _mixed(rs)
    # every score positive: treat everybody, no split is strictly better than the leaf
    rec, fin, _, _ = _learn(np.abs(rs.randn(300)) + 0.1, X, 8)
    assert rec[:10] == [-1] * 6 + [1] * 4 and fin[0, 6] == 1.0
    assert fin[0, 0] == pytest.approx(fin[0, 2], rel=1e-14) and abs(fin[0, 4]) < 1e-15
    # min_leaf larger than half the rows: no split is allowed
    rec, _, _, _ = _learn(rs.randn(300), X, 8, 2, 151)
    assert rec[:6] == [-1] * 6


# ---------------------------------------------------------------- recovery
def test_xor_needs_exact_depth_two():
    rs = np.random.RandomState(5)
    n = 2000
    X = rs.randn(n, 2)
    r = np.where((X[:, 0] < 0) != (X[:, 1] < 0), 1.0, -1.0) + 0.1 * rs.randn(n)
    _, f2, _, _ = _learn(r, X, 8, 2)
    _, f1, _, _ = _learn(r, X, 8, 1)
    print("XOR value: depth 2", f2[0, 0], "depth 1", f1[0, 0])
    assert f2[0, 0] > 0.45 and f1[0, 0] < 0.1 and f2[0, 0] <= 0.5 + 0.05


def test_planted_policy_on_quantile_edges():
    rs = np.random.RandomState(9)
    n = 1500
    X = rs.randn(n, 3)
    edges = [DP.feature_edges(X[:, j], 8) for j in range(3)]
    assert all(len(ed) == 7 for ed in edges)
    a, b = edges[0][2], edges[1][5]
    plant = (X[:, 0] >= a) & (X[:, 1] < b)
    r = np.where(plant, 1.0, -1.0) + 0.1 * rs.randn(n)
    rec, fin, _, _ = _learn(r, X, 8)
    res = PolicyTreeResult.make("t", rec, fin, [4, 7, 9], edges, 0.0, 2)
    root, left, right = res.nodes
    assert (root["feature"], root["threshold"]) == (4, a)       # columns of X, edge values
    assert left["feature"] is None and (right["feature"], right["threshold"]) == (7, b)
    assert res.actions == [0, 0, 1, 0]
    assert fin[0, 6] == pytest.approx(plant.mean(), abs=1e-15)
    assert [lf["leaf"] for lf in res.in_sample["leaves"]] == ["L", "RL", "RR"]
    assert sum(lf["n"] for lf in res.in_sample["leaves"]) == n


# ---------------------------------------------------------------- held-out rows
def test_train_mask():
    rs = np.random.RandomState(3)
    n = 900
    X = _mixed(rs, n)
    r = rs.randn(n) + 1.0 * X[:, 0] - 0.8 * (X[:, 1] > 0)
    train = rs.rand(n) < 0.6
    rec, fin, e, edges = _learn(r, X, 8, train=train)
    other = r.copy()
    other[~train] = 0.25 * rs.randn(int((~train).sum()))    # |.| stays below max |r|: the same e
    rec2, fin2, e2, _ = _learn(other, X, 8, train=train)
    assert rec2 == rec and e2 == e and np.array_equal(fin2[0], fin[0], equal_nan=True)
    assert not np.array_equal(fin2[1], fin[1], equal_nan=True)
    assert rec[11] == int(train.sum()) and rec[0] >= 0
    res = PolicyTreeResult.make("t", rec, fin, [0, 1, 2], edges, 0.0, 2, held_out=True)
    pi = res.predict(X)
    held = res.held_out
    assert held["n"] == int((~train).sum()) and res.diagnostics["honest"] is True
    assert held["value"] == pytest.approx((pi * r)[~train].mean(), rel=1e-12)
    assert held["treat_all"] == pytest.approx(r[~train].mean(), rel=1e-12)
    assert held["advantage"] == pytest.approx(held["value"] - held["treat_all"], rel=1e-10)
    v = (pi * r)[~train]
    assert held["value_se"] == pytest.approx(v.std(ddof=1) / np.sqrt(len(v)), rel=1e-10)
    assert res.in_sample["share_treated"] == pytest.approx(pi[train].mean(), abs=1e-15)
    assert res.value == held["value"] and res.in_sample["value"] > held["value"] - 1.0
    no = PolicyTreeResult.make("t", rec, fin, [0, 1, 2], edges, 0.0, 2)
    assert no.held_out is None and no.diagnostics["honest"] is False


def test_cost_shifts_the_scores():
    rs = np.random.RandomState(4)
    X = _mixed(rs)
    r = rs.randn(300) + X[:, 0]
    a = _learn(r, X, 8, cost=0.3)
    b = _learn(r - 0.3, X, 8)
    assert a[0] == b[0] and np.array_equal(a[1], b[1], equal_nan=True)


# ---------------------------------------------------------------- row sharding
def test_row_sharded_matches_single_rank():
    edges = [np.array([-0.5, 0.0, 0.6]), np.array([0.1]), np.array([-1.0, -0.2, 0.3, 1.1])]

    def run(comm):
        pan = synthetic_panel(1500, p=24, folds=3, dtype="f64", arm_split=True, comm=comm)
        codes = torch.stack([torch.bucketize(pan.col(f"x{j}").double(), torch.from_numpy(ed),
                                             right=True).to(torch.uint8)
                             for j, ed in enumerate(edges)])
        use = torch.where(pan.row_index < 0, -1, (pan.row_index % 4 == 0).long()).to(torch.int8)
        fin, rec, e, _ = DP.irm_policy_panel(pan, codes, use, [4, 2, 5], 0.01, 3, comm=comm,
                                             n_rows=1500)
        return fin.numpy(), rec.tolist(), int(e), pan.n

    fin1, rec1, e1, n1 = run(None)
    assert n1 == 1500 and np.isfinite(fin1[:, :8]).all()
    assert fin1[0, 7] + fin1[1, 7] == 1500 and rec1[11] == fin1[0, 7] and fin1[1, 7] > 300
    for world in (2, 3):
        out = run_simulated(world, run)
        assert sum(n for _, _, _, n in out) == 1500
        for fin, rec, e, _ in out:
            assert rec == rec1 and e == e1                  # tree and value in q units: exact
            assert np.array_equal(fin[:, 7], fin1[:, 7])    # n
            print("world", world, "max abs", np.nanmax(np.abs(fin - fin1)))
            np.testing.assert_allclose(fin, fin1, rtol=1e-12, atol=1e-12)


def test_estimator_row_sharded_matches_single_rank():
    """dml_irm_policy_lasso under dist=: shared edges from the gathered feature columns, global
    cell and training-row counts, a train mask per shard."""
    rs = np.random.RandomState(8)
    n = 900
    X = rs.randn(n, 4)
    X[:, 2] = rs.randint(0, 3, n)
    W = (rs.rand(n) < 0.5).astype(float)
    Y = X[:, 1] + (0.5 + 0.8 * (X[:, 0] > 0.2) - 0.6 * (X[:, 2] == 1)) * W + rs.randn(n)
    train = rs.rand(n) < 0.7
    kw = dict(bins=8, cost=0.1, folds=3, min_leaf=5, device="cpu")
    one = DP.dml_irm_policy_lasso(Y, W, X, [0, 2, 3], train=train, **kw)
    assert one.nodes[0]["feature"] is not None and one.n_train == int(train.sum())

    def body(comm):
        dist = DistContext.for_rank(comm, n)
        return DP.dml_irm_policy_lasso(dist.local(Y), dist.local(W), dist.local(X), [0, 2, 3],
                                       train=dist.local(train), dist=dist, **kw)

    for r in run_simulated(2, body):
        assert r.edges == one.edges and r.n_train == one.n_train
        assert r.diagnostics["e"] == one.diagnostics["e"] and r.diagnostics["honest"] is True
        assert r.held_out["n"] == one.held_out["n"] == int((~train).sum())
        # the fit differs in the last digits between world sizes (Gram sums in another order),
        # so here the values are compared, and the tree where the scores leave no near tie
        for ev, ov in ((r.in_sample, one.in_sample), (r.held_out, one.held_out)):
            for k in ("treat_all", "treat_all_se"):
                assert ev[k] == pytest.approx(ov[k], rel=1e-7, abs=1e-10), k
        assert r.in_sample["value"] == pytest.approx(one.in_sample["value"], rel=1e-7, abs=1e-10)
        if r.nodes == one.nodes and r.actions == one.actions:
            for k in ("value", "value_se", "advantage", "share_treated"):
                assert r.held_out[k] == pytest.approx(one.held_out[k], rel=1e-7, abs=1e-10), k


# ---------------------------------------------------------------- NaN scores
@pytest.mark.parametrize("where", ["train", "held_out"])
def test_nan_scores_give_nan_values_and_no_tree(where):
    rs = np.random.RandomState(6)
    X = _mixed(rs)
    r = rs.randn(300) + 2.0 * X[:, 0]
    train = np.arange(300) % 3 != 0
    r[0 if where == "held_out" else 1] = np.nan
    rec, fin, _, edges = _learn(r, X, 8, train=train)
    assert np.isnan(fin).all()
    assert rec[:11] == [-1] * 6 + [0] * 5 and rec[11] == int(train.sum())   # masked on the device path
    res = PolicyTreeResult.make("t", rec, fin, [0, 1, 2], edges, 0.0, 2, held_out=True)
    assert all(nd["feature"] is None for nd in res.nodes) and res.actions == [0] * 4
    assert res.diagnostics["nan"] is True and np.isnan(res.value)
    assert not res.predict(X).any()
    ref, rfin, _ = R.policy_tree_from_scores(r, X, edges, train)
    assert np.isnan(rfin).all()


# ---------------------------------------------------------------- validation
def test_value_errors():
    rs = np.random.RandomState(0)
    n = 400
    X, Y = rs.randn(n, 40), rs.randn(n)
    W = (rs.rand(n) < 0.5).astype(float)
    for fn, kw in ((DP.dml_irm_policy_lasso, dict(device="cpu")), (R.dml_irm_policy_tree, {})):
        with pytest.raises(ValueError, match="32 features"):
            fn(Y, W, X, list(range(33)), **kw)
        with pytest.raises(ValueError, match="32 features"):
            fn(Y, W, X, [], **kw)
        with pytest.raises(ValueError, match="distinct"):
            fn(Y, W, X, [1, 2, 1], **kw)
        with pytest.raises(ValueError, match="columns of X"):
            fn(Y, W, X, [1, 40], **kw)
        for bad in (1, 65, 7.5):
            with pytest.raises(ValueError, match="bins"):
                fn(Y, W, X, [0, 1], bins=bad, **kw)
        for bad in (-1, 3, 1.5):
            with pytest.raises(ValueError, match="depth"):
                fn(Y, W, X, [0, 1], depth=bad, **kw)
        with pytest.raises(ValueError, match="min_leaf"):
            fn(Y, W, X, [0, 1], min_leaf=0, **kw)
        with pytest.raises(ValueError, match="binary treatment"):
            fn(Y, W + 0.5, X, [0, 1], **kw)
        with pytest.raises(ValueError, match="no training rows"):
            fn(Y, W, X, [0, 1], train=np.zeros(n, dtype=bool), **kw)
        with pytest.raises(ValueError, match="boolean mask"):
            fn(Y, W, X, [0, 1], train=np.zeros(n - 1, dtype=bool), **kw)
    psi, use = torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.int8)
    with pytest.raises(ValueError):
        DP.pair_hist(psi, 0.0, 30, use, torch.zeros((33, 8), dtype=torch.uint8), [2] * 33)
    with pytest.raises(ValueError):
        DP.pair_hist(psi, 0.0, 30, use, torch.zeros((2, 7), dtype=torch.uint8), [2, 2])
    with pytest.raises(ValueError):
        DP.pair_hist(psi, 0.0, 30, use, torch.zeros((2, 8), dtype=torch.int32), [2, 2])
    with pytest.raises(ValueError):
        DP.tree_search(torch.zeros((2, 2, 64, 64), dtype=torch.int64), [2, 2])


# ---------------------------------------------------------------- public surface
def test_api_backends_and_result(tutorial):
    import ate_replication_causalml_amd as pkg
    from ate_replication_causalml_amd.config import RunConfig
    _, m, _ = tutorial
    cols = [m.names.index(c) for c in ("yob", "hh_size", "p2004")]
    train = np.arange(len(m.Y)) % 5 != 0
    # the gpu backend through the API: tests/test_gpu_policy.py
    ref, cpu = (pkg.ate_dml_irm_policy(m.Y, m.W, m.X, cols, train=train, cost=0.02,
                                       run=RunConfig(backend=b)) for b in ("reference", "cpu"))
    assert isinstance(cpu, pkg.PolicyTreeResult) and cpu.diagnostics["hipgraph"] is False
    print(cpu.table())
    for r in (cpu,):
        assert r.nodes == ref.nodes and r.actions == ref.actions and r.edges == ref.edges
        assert r.n_train == ref.n_train == int(train.sum())
        assert r.diagnostics["honest"] is True and r.diagnostics["e"] == ref.diagnostics["e"]
        for ev, rev in ((r.in_sample, ref.in_sample), (r.held_out, ref.held_out)):
            for k in ("value", "value_se", "treat_all", "treat_all_se", "advantage", "advantage_se",
                      "share_treated"):
                assert ev[k] == pytest.approx(rev[k], rel=1e-8, abs=1e-10), k
            assert [lf["n"] for lf in ev["leaves"]] == [lf["n"] for lf in rev["leaves"]]
    assert cpu.nodes[0]["feature"] in cols and cpu.features == cols and cpu.cost == 0.02
    pi = cpu.predict(m.X)
    assert set(np.unique(pi)) <= {0, 1}
    assert pi[train].mean() == pytest.approx(cpu.in_sample["share_treated"], abs=1e-12)
    assert pi[~train].mean() == pytest.approx(cpu.held_out["share_treated"], abs=1e-12)
    d = json.loads(cpu.to_json())
    assert d["nodes"] == cpu.nodes and d["held_out"]["value"] == cpu.held_out["value"]
    assert d["diagnostics"]["honest"] is True
    assert len(cpu.table().splitlines()) > 10
    # without a held-out set only the optimistic in-sample value is there, and says so
    ins = pkg.ate_dml_irm_policy(m.Y, m.W, m.X, cols, depth=1, run=RunConfig(backend="cpu"))
    assert ins.held_out is None and ins.diagnostics["honest"] is False
    assert ins.nodes[1]["feature"] is None and ins.nodes[2]["feature"] is None
    assert ins.value == ins.in_sample["value"] >= max(ins.in_sample["treat_all"], 0.0) - 1e-12


def test_cli_policy_prints_finite_json(capsys):
    from ate_replication_causalml_amd import cli
    assert cli.main(["dml", "--model", "irm", "--n", "3000", "--p", "24", "--dtype", "f64",
                     "--policy-cols", "0,3,21", "--policy-bins", "8", "--policy-cost", "0.01"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["n"] == 3000 and out["features"] == [0, 3, 21] and out["depth"] == 2
    assert len(out["nodes"]) == 3 and len(out["actions"]) == 4 and out["honest"] is False
    vals = [out[k] for k in ("value", "value_se", "treat_all", "treat_all_se", "advantage",
                             "advantage_se", "share_treated")]
    assert np.isfinite(vals).all() and out["value"] >= max(out["treat_all"], 0.0)
    assert sum(lf["n"] for lf in out["leaves"]) == 3000
    for lf in out["leaves"]:
        assert np.isfinite([lf["mean"], lf["se"]]).all() and lf["action"] in (0, 1)
