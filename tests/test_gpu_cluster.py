"""GPU tests of the cluster-robust DML (estimators/cluster.py): the segmented reduction
(csrc/cluster.hip ``ate_cluster_moments``) against numpy in extended precision at the edges of
its chunk, run to run, and its refusals; the per-row PLR terms (csrc/dml.hip
``ate_dml_resid_terms``) against the float64 torch twin and the moment pass; the estimators
against the CPU path, eager against captured against replayed, and singleton clusters against
the unclustered GPU estimators. Run on the MI355X box: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.estimators import cluster as DC
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators import lasso as DL
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel import rng
from test_gpu_irm import COUNTS

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


# ---------------------------------------------------------------- the kernel against numpy
def _rows(n, layout, rs):
    """(rows, ld): the n panel rows the clusters name. "dense": 0..n-1; "gaps": the real rows
    of segments padded to 64 rows (what a fold panel looks like); "tail": dense, with 100
    unused rows after them."""
    if layout == "gaps":
        rows, r0, left = [], 0, n
        while left > 0:
            c = min(left, int(rs.integers(1, 200)))
            rows.append(np.arange(r0, r0 + c))
            r0 += -(-c // 64) * 64
            left -= c
        return np.concatenate(rows), r0
    return np.arange(n), n + (100 if layout == "tail" else 0)


def _check(gpu, sizes, layout="dense", shuffle=False, seed=0):
    """One size profile, b null and given, theta zero and not, against np.add.at in long
    double. Bounds: every cluster sum carries at most n roundings of terms bounded by
    S_j = sum |a| + |theta| sum |b|, and sum t^2 (sum t) at most n more of terms bounded by
    S_j^2 (S_j): 4 n 2^-53 sum_j S_j^2 for sum t^2, 4 n 2^-53 sum_j S_j for sum t."""
    rs = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n, J = int(sizes.sum()), len(sizes)
    rows, ld = _rows(n, layout, rs)
    order = rs.permutation(rows) if shuffle else rows
    starts = np.concatenate([[0], np.cumsum(sizes)])
    codes = np.repeat(np.arange(J), sizes)
    a, b = rs.normal(size=ld), rs.uniform(0.1, 2.0, size=ld)
    ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    ts = torch.from_numpy(starts.astype(np.int32)).to(gpu)
    to = torch.from_numpy(order.astype(np.int32)).to(gpu)
    for hasb in (False, True):
        for theta in (0.0, -0.83):
            th = torch.tensor([theta], dtype=torch.float64, device=gpu)
            got = DC.cluster_moments(ta, tb if hasb else None, ts, to, J, th)
            again = DC.cluster_moments(ta, tb if hasb else None, ts, to, J, th)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int64), again.view(torch.int64))   # run to run
            got = got.cpu().numpy()
            A, B, SA, SB = (np.zeros(J, dtype=np.longdouble) for _ in range(4))
            bo = b[order] if hasb else np.ones(n)
            np.add.at(A, codes, a[order].astype(np.longdouble))
            np.add.at(B, codes, bo.astype(np.longdouble))
            np.add.at(SA, codes, np.abs(a[order]).astype(np.longdouble))
            np.add.at(SB, codes, np.abs(bo).astype(np.longdouble))
            t = A - np.longdouble(theta) * B
            S = SA + abs(theta) * SB
            want2, want1 = float((t * t).sum()), float(t.sum())
            tol2, tol1 = 4 * n * EPS * float((S * S).sum()), 4 * n * EPS * float(S.sum())
            print(f"J={J} n={n} {layout} shuffle={shuffle} b={hasb} theta={theta}: "
                  f"sum t^2 {got[0]!r} err {abs(got[0] - want2):.3g} tol {tol2:.3g}; "
                  f"sum t {got[1]!r} err {abs(got[1] - want1):.3g} tol {tol1:.3g}")
            assert abs(got[0] - want2) <= tol2
            assert abs(got[1] - want1) <= tol1
            assert got[2] == float((sizes.astype(np.float64) ** 2).sum())
            assert got[3] == float(sizes.max())


def _among_singletons(size):
    return [1] * 37 + [size] + [1] * 50


def _profiles():
    C = DC.cluster_chunk()
    rs = np.random.default_rng(5)
    p = {"one_cluster": [5], "mixed_1_70": rs.permutation(np.arange(1, 71)),
         "two_giants": [3 * C + 5] * 2,
         "wave_sized": [33] * 70 + [40] * 30 + [32] * 9}
    p.update({f"singletons_{n}": [1] * n for n in (63, 64, 65, 257)})
    p.update({f"edge_{k}": _among_singletons(s) for k, s in
              (("chunk_minus_1", C - 1), ("chunk", C), ("chunk_plus_1", C + 1),
               ("two_chunks_plus_1", 2 * C + 1))})
    return p


PROFILES = ("one_cluster", "mixed_1_70", "two_giants", "wave_sized", "singletons_63",
            "singletons_64", "singletons_65", "singletons_257", "edge_chunk_minus_1",
            "edge_chunk", "edge_chunk_plus_1", "edge_two_chunks_plus_1")


@pytest.mark.parametrize("shuffle", [False, True], ids=["runs", "shuffled"])
@pytest.mark.parametrize("name", PROFILES)
def test_cluster_kernel_vs_numpy(gpu, name, shuffle):
    assert DC.cluster_chunk() >= 64
    _check(gpu, _profiles()[name], shuffle=shuffle, seed=len(name))


@pytest.mark.parametrize("layout", ["gaps", "tail"])
def test_cluster_kernel_rows_with_padding_gaps_and_an_empty_tail(gpu, layout):
    C = DC.cluster_chunk()
    sizes = np.r_[np.random.default_rng(6).integers(1, 10, size=700), C + 7, [1] * 90]
    for shuffle in (False, True):
        _check(gpu, sizes, layout=layout, shuffle=shuffle, seed=7)


def test_cluster_kernel_joins_more_pieces_than_one_thread_span(gpu):
    """140 clusters of two chunks each: 280 chunks, 560 open pieces -- the joining launch's
    256 threads fold spans of several pieces, and clusters end inside spans."""
    _check(gpu, [2 * DC.cluster_chunk()] * 140, seed=8)


def test_cluster_kernel_refusals(gpu):
    lib = _native.hip()
    f64 = dict(dtype=torch.float64, device=gpu)
    a, th, out = torch.zeros(8, **f64), torch.zeros(1, **f64), torch.full((4,), 7.0, **f64)
    starts = torch.tensor([0, 8], dtype=torch.int32, device=gpu)
    order = torch.arange(8, dtype=torch.int32, device=gpu)
    work = torch.zeros(int(lib.ate_cluster_work(8)), **f64)
    s = torch.cuda.current_stream().cuda_stream

    def call(a_=a, ld=8, st=starts, o=order, n=8, J=1, t=th, w=work, r=out):
        p = [None if x is None else x.data_ptr() for x in (a_, st, o, t, w, r)]
        return lib.ate_cluster_moments(p[0], None, ld, p[1], p[2], n, J, p[3], p[4], p[5], s)

    assert call(J=0) == -1 and call(J=-3) == -1
    assert call(ld=-1) == -1 and call(n=-1) == -1 and call(n=2 ** 31) == -1
    for k in ("a_", "st", "o", "t", "w", "r"):
        assert call(**{k: None}) == -1, k
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((4,), 7.0, dtype=torch.float64))   # no launch
    assert lib.ate_cluster_work(-1) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 0.0, 64.0, 8.0]
    with pytest.raises(ValueError):
        DC.cluster_moments(a, None, starts.long(), order, 1, th)
    with pytest.raises(ValueError):
        DC.cluster_moments(a, None, starts, order, 2, th)


# ---------------------------------------------------------------- the per-row PLR terms
P_X = 40


def _terms_case(dtype):
    """A 6-segment PLR panel of COUNTS rows on host and device, and [6, 2, p+1] coefficients
    (segment 3 intercepts only). bf16: x on a 1/8 grid, coefficients on a 2^-6 grid, binary
    targets, so the kernel's fp32 dot products are exact (as tests/test_gpu_irm.py)."""
    rs = np.random.RandomState(23)
    seg = rs.permutation(np.repeat(np.arange(6), COUNTS))
    n = len(seg)
    bf = dtype == "bf16"
    X = rs.randint(-32, 33, size=(n, P_X)) / 8.0 if bf else rs.randn(n, P_X)
    W = rs.randint(0, 2, n).astype(float)
    Y = rs.randint(0, 2, n).astype(float) if bf else rs.randn(n) + W
    coef = np.zeros((6, 2, P_X + 1))
    for k in range(6):
        on = rs.rand(2, P_X) < 0.4
        coef[k, :, 1:] = on * (rs.randint(-9, 10, (2, P_X)) / 64.0 if bf else rs.randn(2, P_X) * 0.3)
    coef[3, :, 1:] = 0.0
    coef[:, 0, 0], coef[:, 1, 0] = 0.25, 0.5
    return X, W, Y, seg, coef


@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_resid_terms_vs_twin_and_moment_pass(gpu, dtype):
    X, W, Y, seg, coef = _terms_case(dtype)
    pc = build_panel(X, W, Y, folds=seg, dtype=dtype, device="cpu")
    pg = build_panel(X, W, Y, folds=seg, dtype=dtype, device=gpu)
    assert tuple(pg.seg_nreal) == COUNTS and pg.ld > len(Y)
    c = torch.from_numpy(coef)
    wa, wb = DC.dml_resid_terms(pc, c)                          # the float64 torch twin
    ga, gb = DC.dml_resid_terms(pg, c.to(gpu))
    mom = DL.dml_residual_moments(pg, c.to(gpu))
    torch.cuda.synchronize()
    ga, gb, mom = ga.cpu().numpy(), gb.cpu().numpy(), mom.cpu().numpy()
    valid = pc.valid().double().numpy() != 0
    assert valid.sum() == len(Y) and np.all(ga[~valid] == 0) and np.all(gb[~valid] == 0)
    # per row: each residual is y - (c0 + sum c_j x_j), p + 2 roundings of terms bounded by
    # Sy = |y| + sum |c_j x_j| (Sw alike); a = wr yr and b = wr^2 then err by at most
    # 2 (p + 3) 2^-53 Sy Sw and 2 (p + 3) 2^-53 Sw^2 (the stored values are exact inputs)
    Xs = pc.colmajor().double().numpy()
    ax = np.abs(Xs[pc.xcols])
    kseg = np.searchsorted(np.asarray(pc.seg_bounds)[:, 1], np.arange(pc.ld), side="right")
    ac = np.abs(coef[kseg])                                     # [ld, 2, p+1]
    Sy = np.abs(Xs[pc.cols["Y"]]) + ac[:, 0, 0] + (ac[:, 0, 1:].T * ax).sum(0)
    Sw = np.abs(Xs[pc.cols["W"]]) + ac[:, 1, 0] + (ac[:, 1, 1:].T * ax).sum(0)
    tol = 2 * (P_X + 3) * EPS
    ea, eb = np.abs(ga - wa.numpy()), np.abs(gb - wb.numpy())
    print(dtype, "max err a", ea.max(), "bound", (tol * Sy * Sw)[valid].min(),
          "max err b", eb.max(), "bound", (tol * Sw * Sw)[valid].min())
    assert np.all(ea <= tol * Sy * Sw) and np.all(eb <= tol * Sw * Sw)
    assert np.abs(ga).max() > 0.1 and np.abs(gb).max() > 0.1
    # the column sums are the moment pass's S wr yr and S wr^2
    n = len(Y)
    for got, m in ((ga, mom[0]), (gb, mom[1])):
        s = float(got.astype(np.longdouble).sum())
        bound = 4 * n * EPS * float(np.abs(got).sum())
        print(dtype, "column sum", s, "moment", m, "err", abs(s - m), "bound", bound)
        assert abs(s - m) <= bound
    assert mom[5] == n


# ---------------------------------------------------------------- the estimators
N_EST, P_EST, K = 4000, 20, 3


def _est_data(seed):
    rs = np.random.default_rng(seed)
    X = rs.normal(size=(N_EST, P_EST))
    W = (rs.uniform(size=N_EST) < 1 / (1 + np.exp(-0.5 * X[:, 0]))).astype(float)
    return X[:, 0] - 0.5 * X[:, 1] + 0.4 * W + rs.normal(size=N_EST), W, X


def _mixed_clusters(rs):
    """Sizes 1..9 (cycled) and one cluster of 800, rows shuffled."""
    sizes, s = [], 0
    while s < N_EST - 800:
        sizes.append(min(1 + len(sizes) % 9, N_EST - 800 - s))
        s += sizes[-1]
    sizes.append(800)
    return rs.permutation(np.repeat(np.arange(len(sizes)), sizes))


ESTIMATORS = {"plr": DC.dml_plr_lasso_cluster, "irm": DC.dml_irm_lasso_cluster}


def _same(a, b):
    return a.ate == b.ate and a.se == b.se and \
        a.diagnostics["se_unclustered"] == b.diagnostics["se_unclustered"]


@pytest.mark.parametrize("model", ["plr", "irm"])
def test_estimator_vs_cpu_eager_captured_replayed(gpu, model):
    f = ESTIMATORS[model]
    Y, W, X = _est_data(11)
    cl = _mixed_clusters(np.random.default_rng(12))
    cpu = f(Y, W, X, cl, folds=K, device="cpu")
    eager = f(Y, W, X, cl, folds=K, device=gpu, graph=False)
    runs = [f(Y, W, X, cl, folds=K, device=gpu) for _ in range(3)]   # eager, captured, replayed
    torch.cuda.synchronize()
    print(model, "cpu", cpu.ate, cpu.se, "gpu", eager.ate, eager.se, eager.diagnostics)
    # the bound of the GPU estimator tests (tests/test_gpu.py, tests/test_gpu_irm.py)
    assert eager.ate == pytest.approx(cpu.ate, abs=1e-6, rel=1e-6)
    assert eager.se == pytest.approx(cpu.se, abs=1e-6, rel=1e-6)
    assert eager.diagnostics["se_unclustered"] == pytest.approx(cpu.diagnostics["se_unclustered"],
                                                                abs=1e-6, rel=1e-6)
    for k in ("n_clusters", "max_cluster", "design_effect"):
        assert eager.diagnostics[k] == cpu.diagnostics[k], k
    assert eager.diagnostics["max_cluster"] == 800 and eager.se != eager.diagnostics["se_unclustered"]
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    for r in runs:
        print(model, "graph", r.diagnostics["hipgraph"], r.ate, r.se)
        assert _same(r, eager)


@pytest.mark.parametrize("model", ["plr", "irm"])
def test_replay_with_another_size_distribution(gpu, model):
    """Same n, same J, same rows per fold: even clusters of 10, then one giant cluster (and
    new outcomes) -- the captured graph replays with the new CSR and matches its own eager
    run. Relabelling only inside fold 0 keeps every row's fold, hence the panel's shape."""
    f = ESTIMATORS[model]
    Y, W, X = _est_data(13)
    even = np.arange(N_EST) // 10
    J = N_EST // 10
    fold0 = np.flatnonzero(rng.fold_ids(J, K, 1991, 0) == 0)
    giant = even.copy()
    for j in fold0[1:]:
        giant[np.flatnonzero(even == j)[1:]] = fold0[0]          # one row stays, nine move
    assert len(np.unique(giant)) == J and np.bincount(giant).max() == 10 + 9 * (len(fold0) - 1)
    first = [f(Y, W, X, even, folds=K, device=gpu) for _ in range(2)]
    assert [r.diagnostics["hipgraph"] for r in first] == [False, True] and _same(*first)
    Y2 = Y + 0.3 * np.random.default_rng(14).normal(size=N_EST)
    replayed = f(Y2, W, X, giant, folds=K, device=gpu)
    eager = f(Y2, W, X, giant, folds=K, device=gpu, graph=False)
    torch.cuda.synchronize()
    print(model, "even", first[1].se, "giant replayed", replayed.ate, replayed.se, "eager",
          eager.ate, eager.se, replayed.diagnostics)
    assert replayed.diagnostics["hipgraph"] is True
    assert replayed.diagnostics["max_cluster"] == 10 + 9 * (len(fold0) - 1)
    assert replayed.diagnostics["n_clusters"] == J
    assert _same(replayed, eager)
    assert replayed.se != first[1].se


def test_singleton_clusters_have_the_unclustered_theta_bits(gpu):
    rs = np.random.default_rng(15)
    n = 600
    X = rs.normal(size=(n, 8))
    W = (rs.uniform(size=n) < 1 / (1 + np.exp(-0.5 * X[:, 0]))).astype(float)
    Y = X[:, 0] + 0.5 * W + rs.normal(size=n)
    for plain, clustered in ((DL.dml_plr_lasso, DC.dml_plr_lasso_cluster),
                             (DI.dml_irm_lasso, DC.dml_irm_lasso_cluster)):
        a = plain(Y, W, X, folds=K, device=gpu, graph=False)
        b = clustered(Y, W, X, np.arange(n), folds=K, device=gpu, graph=False)
        torch.cuda.synchronize()
        print(plain.__name__, a.ate, b.ate, a.se, b.se, abs(b.se / a.se - 1), 16 * n * EPS)
        assert b.ate == a.ate
        assert b.diagnostics["se_unclustered"] == a.se
        assert abs(b.se - a.se) <= 16 * n * EPS * a.se            # two summation orders
        assert b.diagnostics["max_cluster"] == 1 and b.diagnostics["design_effect"] == 1.0
