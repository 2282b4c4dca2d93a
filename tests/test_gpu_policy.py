"""GPU tests of the policy-tree estimator (estimators/policy.py): the feature-pair histogram
kernel (csrc/policy.hip) against an integer numpy twin at every path it has, the search
kernels against the brute-force reference twin and the CPU prefix-sum path, the estimator
against the reference, hipGraph capture and replay with the codes and the cost as graph
inputs, and determinism. Run on the MI355X box: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.estimators import policy as DP
from ate_replication_causalml_amd.reference import estimators as E

pytestmark = pytest.mark.gpu

LD, REAL = 832, 529                 # the layout of tests/test_gpu_irm.py: 529 real rows in 832


def _hist_twin(q, use, codes, nb):
    """Integer numpy twin of ate_policy_pair_hist, pair by pair."""
    d = len(codes)
    out = np.zeros((d * (d + 1) // 2, 2, 64, 64), dtype=np.int64)
    k = 0
    for a in range(d):
        for b in range(a, d):
            keep = (use == 0) & (codes[a] < nb[a]) & (codes[b] < nb[b])
            np.add.at(out[k, 0], (codes[a][keep], codes[b][keep]), q[keep])
            np.add.at(out[k, 1], (codes[a][keep], codes[b][keep]), 1)
            k += 1
    return out


def _rows(rs, n, nb, scale=1.0, n_real=None):
    """(psi, use, codes): scores, use codes with -1 / 0 / 1 and codes below nb."""
    psi = rs.standard_t(5, n) * scale
    use = rs.choice([0, 0, 0, 1], n).astype(np.int8)
    if n_real is not None:
        use[rs.permutation(n)[:n - n_real]] = -1
    codes = np.stack([rs.randint(0, b, n) for b in nb]).astype(np.uint8)
    return psi, use, codes


def _gpu_hist(gpu, psi, cost, e, use, codes, nb, **kw):
    h = DP.pair_hist(torch.from_numpy(psi).to(gpu), cost, e, torch.from_numpy(use).to(gpu),
                     torch.from_numpy(codes).to(gpu), nb, **kw)
    torch.cuda.synchronize()
    return h.cpu().numpy()


def _exponent(psi, cost, use, n_rows):
    rg = DP.score_range(torch.from_numpy(psi), torch.tensor([cost], dtype=torch.float64),
                        torch.from_numpy(use))
    return int(DP.scale_exponent(rg, n_rows))


# (bins per feature, score scale): one feature; binary / 3 / 37 / 64 bins with a feature
# whose rows all share one bin; 32 features of every size class (528 tiles, both small-tile
# and plain tiles in one workgroup); scores of magnitude 2^50
CASES = [([37], 1.0), ([2, 64, 3], 1.0), ([2, 1, 37], 2.0 ** 50),
         ([2, 3, 37, 64, 8, 1, 5, 2] * 4, 1.0)]


@pytest.mark.parametrize("nb,scale", CASES, ids=["d1", "d3", "d3_big", "d32"])
def test_pair_hist_matches_integer_twin(gpu, nb, scale):
    rs = np.random.RandomState(len(nb))
    psi, use, codes = _rows(rs, LD, nb, scale, n_real=REAL)
    bad = int(np.flatnonzero(use == 0)[3])
    psi[bad] = np.inf                                # a non-finite score counts as 0
    cost = 0.125 * scale
    e = _exponent(psi, cost, use, LD)
    assert (e < 15) if scale > 1 else (e == 30)
    assert (use == -1).sum() == LD - REAL and (use == 1).sum() > 50
    q = DP.quantize(torch.from_numpy(psi), cost, e).numpy()
    assert q[bad] == 0 and np.abs(q).max() > 2 ** 30
    want = _hist_twin(q, use, codes, nb)
    assert want[:, 1].sum() == (use == 0).sum() * len(want)
    cpu = DP.pair_hist(torch.from_numpy(psi), cost, e, torch.from_numpy(use),
                       torch.from_numpy(codes), nb).numpy()
    assert np.array_equal(cpu, want)                 # the CPU path is the same integers
    for nbx in (None, 1, 3):
        for priv in (True, False):                   # per-lane copies | plain small tiles
            got = _gpu_hist(gpu, psi, cost, e, use, codes, nb, nbx=nbx, priv=priv)
            assert got.dtype == np.int64 and np.array_equal(got, want), (nbx, priv)


def test_pair_hist_skips_codes_past_nb(gpu):
    rs = np.random.RandomState(1)
    psi, use, codes = _rows(rs, LD, [4, 2])
    codes[0, ::7] = 200                              # never indexed: the row is left out
    got = _gpu_hist(gpu, psi, 0.0, 30, use, codes, [4, 2])
    q = DP.quantize(torch.from_numpy(psi), 0.0, 30).numpy()
    assert np.array_equal(got, _hist_twin(q, use, codes, [4, 2]))


def test_pair_hist_one_row_per_thread(gpu):
    n, nb = 1531, [2, 37, 64, 3]                     # ld no multiple of 4: the byte-wise kernel
    rs = np.random.RandomState(3)
    psi, use, codes = _rows(rs, n, nb)
    q = DP.quantize(torch.from_numpy(psi), 0.5, 30).numpy()
    want = _hist_twin(q, use, codes, nb)
    for nbx, priv in ((None, True), (2, False)):
        assert np.array_equal(_gpu_hist(gpu, psi, 0.5, 30, use, codes, nb, nbx=nbx, priv=priv),
                              want)


def test_pair_hist_many_chunks(gpu):
    n, nb = 70_000, [2, 64, 3, 37, 2, 8]
    rs = np.random.RandomState(9)
    psi, use, codes = _rows(rs, n, nb)
    e = _exponent(psi, 0.0, use, n)
    assert DP.hist_geometry(len(nb), n) * 2048 * 3 <= n      # several chunks per workgroup
    want = _hist_twin(DP.quantize(torch.from_numpy(psi), 0.0, e).numpy(), use, codes, nb)
    assert np.array_equal(_gpu_hist(gpu, psi, 0.0, e, use, codes, nb), want)
    assert np.array_equal(_gpu_hist(gpu, psi, 0.0, e, use, codes, nb, nbx=37), want)


# ---------------------------------------------------------------- search
def _search_gpu(gpu, r, X, edges):
    """Device histograms of the scores r over X, then (depth, min_leaf) -> record."""
    n, d = X.shape
    nb = [len(ed) + 1 for ed in edges]
    codes = np.stack([DP.bin_codes(X[:, j], edges[j]) for j in range(d)])
    use = np.zeros(n, dtype=np.int8)
    e = _exponent(r, 0.0, use, n)
    h = DP.pair_hist(torch.from_numpy(r).to(gpu), 0.0, e, torch.from_numpy(use).to(gpu),
                     torch.from_numpy(codes).to(gpu), nb)
    return h, nb, e


@pytest.mark.parametrize("variant", ["plain", "duplicate", "scaled", "zero"])
def test_search_kernel_matches_brute_force(gpu, variant):
    rs = np.random.RandomState(11)                   # the cases of tests/test_policy.py
    n = 300
    X = np.stack([(rs.rand(n) < 0.4).astype(float), rs.randn(n),
                  rs.randint(0, 5, n).astype(float)], axis=1)
    r = 2.0 * rs.randn(n) + 1.5 * X[:, 0] - 1.2 * (X[:, 1] > 0.3) + 0.4 * (X[:, 2] - 2)
    if variant == "duplicate":
        X = np.c_[X[:, 1], X]
    elif variant == "scaled":
        r = r * 1e6
    elif variant == "zero":
        r = np.zeros(n)
    for bins in (3, 4, 8):
        edges = [DP.feature_edges(X[:, j], bins) for j in range(X.shape[1])]
        h, nb, e = _search_gpu(gpu, r, X, edges)
        recs = {(depth, ml): DP.tree_search(h, nb, depth, ml) for depth in (0, 1, 2)
                for ml in (1, 25)}
        torch.cuda.synchronize()
        for (depth, ml), rec in recs.items():
            ref, _, re = E.policy_tree_from_scores(r, X, edges, None, depth, ml)
            assert rec.cpu().tolist() == ref and e == re, (variant, bins, depth, ml)


def test_search_kernel_wide(gpu):
    n, d = 6000, 16                                  # 16 features of 64 bins: 136 full tiles
    rs = np.random.RandomState(21)
    X = rs.randn(n, d)
    r = rs.randn(n) + 0.8 * ((X[:, 3] > 0.4) != (X[:, 11] < -0.2)) - 0.3
    edges = [DP.feature_edges(X[:, j], 64) for j in range(d)]
    assert all(len(ed) == 63 for ed in edges)
    h, nb, _ = _search_gpu(gpu, r, X, edges)
    for depth, ml in ((2, 1), (2, 40), (1, 1)):
        got = DP.tree_search(h, nb, depth, ml)
        torch.cuda.synchronize()
        want = DP.tree_search(h.cpu(), nb, depth, ml)
        assert got.cpu().tolist() == want.tolist(), (depth, ml)
    assert sorted((want[0].item(), want[2].item(), want[4].item())) != [-1, -1, -1]


# ---------------------------------------------------------------- estimator
def _cols(m):
    return [m.names.index(c) for c in ("yob", "hh_size", "p2004")]


def _key(r):
    return (r.nodes, r.actions, r.value_q, r.n_train, r.diagnostics["e"],
            repr(r.in_sample), repr(r.held_out))


def test_estimator_vs_reference(gpu, tutorial):
    _, m, _ = tutorial
    cols = _cols(m)
    train = np.arange(len(m.Y)) % 5 != 0
    a = DP.dml_irm_policy_lasso(m.Y, m.W, m.X, cols, train=train, cost=0.02, device=gpu,
                                graph=False)
    torch.cuda.synchronize()
    b = E.dml_irm_policy_tree(m.Y, m.W, m.X, cols, train=train, cost=0.02)
    print("gpu", a.nodes, a.actions, a.in_sample["value"], a.held_out["value"])
    print("reference", b.nodes, b.actions, b.in_sample["value"], b.held_out["value"])
    assert a.n_train == b.n_train and a.edges == b.edges and a.diagnostics["honest"] is True
    # the scores differ in their last digits, so two trees that tie to rounding may swap:
    # the GPU's tree on the reference's scores is as good as the reference's best
    psi = E._irm_scores(E._arr(m.Y), E._arr(m.W), E._arr(m.X), 5, 1991, "min", 0.01)[0]
    r = psi - 0.02
    pi = a.predict(m.X)
    assert (pi * r)[train].mean() == pytest.approx(b.in_sample["value"], abs=1e-6)
    assert pi[train].mean() == pytest.approx(a.in_sample["share_treated"], abs=1e-12)
    # the GPU's values are those of its own tree on the reference's scores
    for ev, rows in ((a.in_sample, train), (a.held_out, ~train)):
        v, t = (pi * r)[rows], r[rows]
        for k, x in (("value", v), ("treat_all", t), ("advantage", v - t)):
            assert ev[k] == pytest.approx(x.mean(), abs=1e-6, rel=1e-6), k
            assert ev[k + "_se"] == pytest.approx(x.std(ddof=1) / np.sqrt(len(x)), abs=1e-6,
                                                  rel=1e-6), k
    if a.nodes == b.nodes and a.actions == b.actions:
        for ev, rev in ((a.in_sample, b.in_sample), (a.held_out, b.held_out)):
            for k in ("value", "value_se", "treat_all", "treat_all_se", "advantage",
                      "advantage_se"):
                assert ev[k] == pytest.approx(rev[k], abs=1e-6, rel=1e-6), k


def test_api_gpu_backend(gpu, tutorial):
    import ate_replication_causalml_amd as pkg
    from ate_replication_causalml_amd.config import RunConfig
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    _, m, _ = tutorial
    train = np.arange(len(m.Y)) % 5 != 0
    estimator_graphs.clear()
    a = pkg.ate_dml_irm_policy(m.Y, m.W, m.X, _cols(m), train=train, cost=0.02,
                               run=RunConfig(backend="gpu"))
    torch.cuda.synchronize()
    b = DP.dml_irm_policy_lasso(m.Y, m.W, m.X, _cols(m), train=train, cost=0.02, device=gpu,
                                graph=False)
    torch.cuda.synchronize()
    assert isinstance(a, pkg.PolicyTreeResult) and _key(a) == _key(b)
    assert a.diagnostics["honest"] is True and np.isfinite(a.value)
    estimator_graphs.clear()


def test_graph_capture_and_replay(gpu, tutorial):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    _, m, _ = tutorial
    cols = _cols(m)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DP.dml_irm_policy_lasso(m.Y, m.W, m.X, cols, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    assert _key(runs[1]) == _key(runs[0]) and _key(runs[2]) == _key(runs[0])
    # other features and another cost in the same layout: a replay equals a fresh eager run
    cols2 = [m.names.index(c) for c in ("median_age", "sex", "g2002")]
    r4 = DP.dml_irm_policy_lasso(m.Y, m.W, m.X, cols2, cost=0.05, device=gpu)
    torch.cuda.synchronize()
    e4 = DP.dml_irm_policy_lasso(m.Y, m.W, m.X, cols2, cost=0.05, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert _key(r4) == _key(e4) and _key(r4) != _key(runs[0])
    assert r4.in_sample["treat_all"] == pytest.approx(runs[0].in_sample["treat_all"] - 0.05,
                                                      abs=1e-12)
    estimator_graphs.clear()


def test_eager_runs_are_deterministic(gpu, tutorial):
    _, m, _ = tutorial
    train = np.arange(len(m.Y)) % 3 != 0
    a, b = (DP.dml_irm_policy_lasso(m.Y, m.W, m.X, _cols(m), train=train, min_leaf=25,
                                    device=gpu, graph=False) for _ in range(2))
    torch.cuda.synchronize()
    assert _key(a) == _key(b) and np.isfinite(a.value)
