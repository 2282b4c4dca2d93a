"""GPU tests of DML-PLIV (estimators/pliv.py): the fused held-out pass and its in-kernel
finish (csrc/pliv.hip) against their float64 twins on fp64, fp32 and bf16 panels (column-major
and 64-row blocked), the per-row terms, the estimator against PLR (Z = D), against the
row-by-row reference, hipGraph capture and replay, clusters, and bf16 against f64 panel
storage. Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.data.dgp import make_pliv_data
from ate_replication_causalml_amd.estimators import lasso as DL
from ate_replication_causalml_amd.estimators import pliv as DP
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.reference import estimators as E
from ate_replication_causalml_amd.result import PlivResult, pliv_layout

from test_gpu_irm import COUNTS, P_X, _case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
CORNERS = np.array([0, 255, 256, 299])


def _pliv_case(q: int, exact: bool):
    """The rows of ``test_gpu_irm._case`` as a plain six-fold panel (segments of COUNTS rows,
    p = 300: two compaction trips), a real D, q real instruments and coefficient blocks
    [6, 2 + q, 301] whose supports include columns 0, 255, 256, 299. Block 1 is intercept-only,
    block 3 has an all-zero m_0 row, block 4's instrument rows have supports disjoint from l
    and r. ``exact``: everything on the grids of ``_case(exact=True)`` (x and the targets on a
    1/8 grid in [-4, 4], coefficients on a 2^-6 grid), so the bf16 kernel's fp32 partial sums
    are exact."""
    X, _, Y, seg, _ = _case(exact)
    n = len(seg)
    rs = np.random.RandomState(23 + q)
    if exact:
        D = rs.randint(-32, 33, n) / 8.0
        Z = rs.randint(-32, 33, size=(n, q)) / 8.0
    else:
        Z = rs.randn(n, q) + 0.3 * X[:, :1]
        D = Z @ (0.7 / (1.0 + np.arange(q))) + rs.randn(n)
    support = np.unique(np.r_[CORNERS, rs.choice(P_X, 36, replace=False)])
    half = rs.rand(len(support)) < 0.5
    coef = np.zeros((6, 2 + q, P_X + 1))
    for k in (0, 2, 3, 4, 5):
        for r in range(2 + q):
            pool = support
            if k == 4:
                pool = support[half] if r < 2 else support[~half]
            on = pool[rs.rand(len(pool)) < 0.6]
            coef[k, r, 1 + on] = rs.randint(-9, 10, len(on)) / 64.0 if exact else \
                rs.randn(len(on)) * 0.3
    for k in (0, 2, 5):
        coef[k, :, 1 + CORNERS] = (np.array([3, -5, 2, 7, -4, 6])[None, :2 + q]
                                   * np.array([[1], [-1], [2], [-2]])) / 64.0
    coef[:, :, 0] = (np.arange(2 + q) + 1) / 4.0
    coef[3, 2] = 0.0
    assert not coef[1, :, 1:].any() and not coef[3, 2].any()
    sl, sz = coef[4, :2, 1:].any(0), coef[4, 2:, 1:].any(0)
    assert sl.any() and sz.any() and not (sl & sz).any()
    assert coef[[0, 2, 5]][:, :, 1 + CORNERS].all()
    return X, Y, D, Z, seg, coef


def _panel(case, dtype, device):
    X, Y, D, Z, seg, _ = case
    targets = {f"Z{j}": Z[:, j] for j in range(Z.shape[1])}
    return build_panel(X, D, Y, folds=seg, dtype=dtype, device=device, targets=targets)


def _blocked(p):
    b = dataclasses.replace(
        p, data=p.data.reshape(p.P, p.ld // 64, 64).permute(1, 0, 2).contiguous(), blocked=True)
    assert b.strides() == (64, 64 * p.P) and torch.equal(b.colmajor(), p.data)
    return b


def _check(got, want, ab, n):
    """Every moment within 1e-11 of the twin relative to the twin's sum of |term| (the bound
    of the residual and score kernel tests; the signed cross moments cancel, so they get the
    absolute-sum denominator); n exact."""
    got, want, ab = got.cpu().numpy(), want.numpy(), ab.numpy()
    err = np.abs(got - want) / ab
    print("moments gpu ", got.tolist())
    print("moments twin", want.tolist())
    print("err / sum|term|", err.tolist())
    assert np.all(err <= 1e-11)
    assert got[0] == n == want[0]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_moment_kernel_vs_twin(gpu, q, dtype):
    case = _pliv_case(q, exact=False)
    pc, pg = _panel(case, dtype, "cpu"), _panel(case, dtype, gpu)
    assert tuple(pg.seg_nreal) == COUNTS and pg.ld > len(case[1]) and pg.nseg == 6
    c = torch.from_numpy(case[5])
    want, ab = DP.pliv_moments_twin(pc, c, q)
    assert want.numel() == pliv_layout(q).size == 4 + 2 * q + 2 * q * (q + 1)
    for nbx in (None, 1):
        got = DP.pliv_moments(pg, c.to(gpu), q, nbx=nbx)
        again = DP.pliv_moments(pg, c.to(gpu), q, nbx=nbx)
        torch.cuda.synchronize()
        print("q", q, dtype, "nbx", nbx)
        _check(got, want, ab, len(case[1]))
        assert torch.equal(got, again)                      # run to run: the same bits


@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_moment_kernel_bf16_layouts_vs_twin(gpu, q):
    case = _pliv_case(q, exact=True)
    pc = _panel(case, "bf16", "cpu")
    v = pc.valid() != 0
    # the stored values are the inputs: the grid is exact in bf16
    assert torch.equal(pc.data[pc.xcols].double()[:, v],
                       torch.from_numpy(case[0][pc.row_index[v].numpy()].T))
    assert torch.equal(pc.data[pc.cols["Z0_hi"]].double()[v],
                       torch.from_numpy(case[3][pc.row_index[v].numpy(), 0]))
    cm = _panel(case, "bf16", gpu)
    c = torch.from_numpy(case[5])
    want, ab = DP.pliv_moments_twin(pc, c, q)
    out = []
    for pan in (cm, _blocked(cm)):
        got = DP.pliv_moments(pan, c.to(gpu), q)
        again = DP.pliv_moments(pan, c.to(gpu), q)
        torch.cuda.synchronize()
        _check(got, want, ab, len(case[1]))
        assert torch.equal(got, again)
        out.append(got.cpu())
    assert torch.equal(out[0], out[1])                      # the two layouts: the same bits


@pytest.mark.parametrize("dtype,exact", [("f64", False), ("bf16", True)])
@pytest.mark.parametrize("q", [1, 3])
def test_terms_vs_twin_and_moment_pass(gpu, q, dtype, exact):
    case = _pliv_case(q, exact)
    pc, pg = _panel(case, dtype, "cpu"), _panel(case, dtype, gpu)
    c = torch.from_numpy(case[5])
    mom, res = DP.pliv_moments(pg, c.to(gpu), q, finish=True)
    pi = res[4:4 + q]
    assert res[3].item() == 0.0
    a, b = DP.pliv_terms(pg, c.to(gpu), q, pi)
    torch.cuda.synchronize()
    wa, wb = DP.pliv_terms(pc, c, q, pi.cpu())
    a, b = a.cpu(), b.cpu()
    for name, x, w in (("a", a, wa), ("b", b, wb)):
        err = ((x - w).abs().max() / w.abs().max()).item()
        print("q", q, dtype, name, "max err / max |term|", err)
        assert err <= 1e-12
    pad = (pc.valid() == 0)
    assert pad.any() and not a[pad].any() and not b[pad].any()   # padding rows: exactly 0
    lay = pliv_layout(q)
    m, w = mom.cpu(), pi.cpu()
    for name, x, at in (("sum a", a, lay.zy), ("sum b", b, lay.zd)):
        want = (w * m[at:at + q]).sum().item()
        err = abs(x.sum().item() - want) / x.abs().sum().item()
        print("q", q, dtype, name, x.sum().item(), "pi'S", want, "err / sum|term|", err)
        assert err <= 1e-11


@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_in_kernel_finish_vs_host_twin(gpu, q):
    case = _pliv_case(q, exact=False)
    pg = _panel(case, "f64", gpu)
    mom, res = DP.pliv_moments(pg, torch.from_numpy(case[5]).to(gpu), q, finish=True)
    torch.cuda.synchronize()
    got, want = res.cpu().numpy(), DP.pliv_finalize(mom.cpu()).numpy()
    print("q", q, "finish gpu ", got.tolist())
    print("q", q, "finish twin", want.tolist())
    assert got.shape == (4 + q,) and got[3] == 0.0 == want[3]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    r = PlivResult.from_moments("x", mom.cpu().numpy())
    assert [r.theta, r.se] + r.pi == [want[0], want[1]] + want[4:].tolist()


def test_duplicated_instrument_sets_the_flag(gpu):
    X, Y, D, Z, seg, coef = _pliv_case(1, exact=False)
    Z2 = np.column_stack([Z[:, 0], Z[:, 0]])
    c2 = np.concatenate([coef, coef[:, 2:3]], axis=1)
    pg = _panel((X, Y, D, Z2, seg, c2), "f64", gpu)
    mom, res = DP.pliv_moments(pg, torch.from_numpy(c2).to(gpu), 2, finish=True)
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    print("duplicated instrument:", got.tolist())
    assert got[3] == 1.0 and np.isnan(np.delete(got, 3)).all()
    want = DP.pliv_finalize(mom.cpu()).numpy()
    assert want[3] == 1.0 and np.isnan(np.delete(want, 3)).all()
    d = make_pliv_data(1500, 3, 1)
    with pytest.raises(ValueError, match="collinear"):
        DP.dml_pliv_lasso(d.Y, d.D, np.column_stack([d.Z[:, 0], d.Z[:, 0]]), d.X, device=gpu,
                          graph=False)
    # z~ identically 0 (an instrument its nuisance reproduces exactly): the largest diagonal
    # entry is 0 and the flag is set at q = 1 too
    c0 = coef.copy()
    c0[:, 2] = 0.0
    pz = _panel((X, Y, D, np.zeros_like(Z), seg, c0), "f64", gpu)
    _, res0 = DP.pliv_moments(pz, torch.from_numpy(c0).to(gpu), 1, finish=True)
    torch.cuda.synchronize()
    assert res0[3].item() == 1.0 and torch.isnan(res0[0]).item()


def test_one_instrument_equal_to_the_treatment_is_plr(gpu, tutorial):
    """q = 1 and Z = D: pi = 1 and the score is PLR's (profiles/pliv/README.md records whether
    the two are bit-equal)."""
    _, m, _ = tutorial
    a = DP.dml_pliv_lasso(m.Y, m.W, m.W, m.X, device=gpu, graph=False)
    b = DL.dml_plr_lasso(m.Y, m.W, m.X, device=gpu, graph=False)
    torch.cuda.synchronize()
    print("pliv(Z=D)", a.theta, a.se, a.pi, "plr", b.ate, b.se)
    print("bit-equal theta:", a.theta == b.ate, "bit-equal SE:", a.se == b.se)
    assert a.theta == pytest.approx(b.ate, rel=1e-10, abs=0)
    assert a.se == pytest.approx(b.se, rel=1e-10, abs=0)
    assert a.pi[0] == pytest.approx(1.0, rel=1e-12)


@pytest.fixture(scope="module")
def reference_fits(tutorial):
    """The reference on make_pliv_data(len(tutorial), 1991, q): computed once, shared."""
    _, m, _ = tutorial
    out = {}
    for q in (1, 3):
        d = make_pliv_data(len(m.Y), 1991, q)
        out[q] = (d, E.dml_pliv_lasso(d.Y, d.D, d.Z, d.X))
    return out


@pytest.mark.parametrize("q", [1, 3])
def test_estimator_vs_reference(gpu, reference_fits, q):
    d, b = reference_fits[q]
    a = DP.dml_pliv_lasso(d.Y, d.D, d.Z, d.X, device=gpu, graph=False)
    torch.cuda.synchronize()
    print("gpu", a.theta, a.se, a.pi, a.first_stage_F, "reference", b.theta, b.se, b.pi,
          b.first_stage_F)
    # the bound of the PLR-vs-reference check of tests/test_gpu.py: the same nuisance code
    for x, y in [(a.theta, b.theta), (a.se, b.se), (a.first_stage_F, b.first_stage_F)] + \
            list(zip(a.pi, b.pi)):
        assert x == pytest.approx(y, abs=1e-6, rel=1e-6)
    assert a.diagnostics["n"] == b.diagnostics["n"] == d.n and not a.weak_instruments


def test_graph_capture_and_replay(gpu, reference_fits):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    d, _ = reference_fits[3]
    rs = np.random.RandomState(4)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DP.dml_pliv_lasso(d.Y, d.D, d.Z, d.X, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    for r in runs[1:]:
        assert r.moments == runs[0].moments
        assert (r.theta, r.se, r.pi) == (runs[0].theta, runs[0].se, runs[0].pi)
    # new Y, D and Z in the same layout (same folds): a replay equals a fresh eager run
    Y2, D2 = d.Y + 0.3 * rs.randn(d.n), d.D + 0.2 * rs.randn(d.n)
    Z2 = d.Z + 0.1 * rs.randn(*d.Z.shape)
    r4 = DP.dml_pliv_lasso(Y2, D2, Z2, d.X, device=gpu)
    torch.cuda.synchronize()
    e4 = DP.dml_pliv_lasso(Y2, D2, Z2, d.X, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert r4.moments == e4.moments and r4.moments != runs[0].moments
    assert (r4.theta, r4.se, r4.pi) == (e4.theta, e4.se, e4.pi)
    # another q: its own cache entry
    n_entries = len(estimator_graphs.entries)
    sub = [DP.dml_pliv_lasso(d.Y, d.D, d.Z[:, :2], d.X, device=gpu) for _ in range(2)]
    torch.cuda.synchronize()
    assert [r.diagnostics["hipgraph"] for r in sub] == [False, True]
    assert len(estimator_graphs.entries) == n_entries + 1
    assert sub[1].moments == sub[0].moments and len(sub[0].pi) == 2
    estimator_graphs.clear()


def test_singleton_clusters_have_the_unclustered_theta_bits(gpu):
    d = make_pliv_data(600, 15, 2)
    n = d.n
    a = DP.dml_pliv_lasso(d.Y, d.D, d.Z, d.X, device=gpu, graph=False)
    b = DP.dml_pliv_lasso_cluster(d.Y, d.D, d.Z, d.X, np.arange(n), device=gpu, graph=False)
    torch.cuda.synchronize()
    print(a.theta, b.theta, a.se, b.se, abs(b.se / a.se - 1), 16 * n * EPS)
    assert b.theta == a.theta and b.pi == a.pi
    assert b.diagnostics["se_unclustered"] == a.se
    assert abs(b.se - a.se) <= 16 * n * EPS * a.se                # two summation orders
    assert b.diagnostics["max_cluster"] == 1 and b.diagnostics["design_effect"] == 1.0


def test_clusters_vs_reference_and_replay(gpu):
    n, K = 3000, 5
    d = make_pliv_data(n, 16, 2)
    rs = np.random.default_rng(17)
    sizes, s = [], 0
    while s < n:                                                  # clusters of 1..40 rows
        sizes.append(min(1 + len(sizes) % 40, n - s))
        s += sizes[-1]
    cl = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    ref = E.dml_pliv_lasso(d.Y, d.D, d.Z, d.X, clusters=cl)
    eager = DP.dml_pliv_lasso_cluster(d.Y, d.D, d.Z, d.X, cl, device=gpu, graph=False)
    torch.cuda.synchronize()
    print("reference", ref.theta, ref.se, ref.diagnostics, "gpu", eager.theta, eager.se,
          eager.diagnostics)
    for x, y in ((eager.theta, ref.theta), (eager.se, ref.se),
                 (eager.diagnostics["se_unclustered"], ref.diagnostics["se_unclustered"])):
        assert x == pytest.approx(y, abs=1e-6, rel=1e-6)
    for k in ("n_clusters", "max_cluster", "design_effect"):
        assert eager.diagnostics[k] == ref.diagnostics[k], k
    assert eager.diagnostics["max_cluster"] == 40
    # a replay with new labels of the same J (relabelled inside fold 0: every row keeps its
    # fold, hence the panel its shape) equals its own eager run
    even = np.arange(n) // 10
    J = n // 10
    fold0 = np.flatnonzero(rng.fold_ids(J, K, 1991, 0) == 0)
    giant = even.copy()
    for j in fold0[1:]:
        giant[np.flatnonzero(even == j)[1:]] = fold0[0]
    assert len(np.unique(giant)) == J
    first = [DP.dml_pliv_lasso_cluster(d.Y, d.D, d.Z, d.X, even, device=gpu) for _ in range(2)]
    assert [r.diagnostics["hipgraph"] for r in first] == [False, True]
    replayed = DP.dml_pliv_lasso_cluster(d.Y, d.D, d.Z, d.X, giant, device=gpu)
    torch.cuda.synchronize()
    fresh = DP.dml_pliv_lasso_cluster(d.Y, d.D, d.Z, d.X, giant, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert replayed.diagnostics["hipgraph"] is True and replayed.diagnostics["n_clusters"] == J
    assert (replayed.theta, replayed.se) == (fresh.theta, fresh.se)
    assert replayed.diagnostics["max_cluster"] == fresh.diagnostics["max_cluster"] == \
        10 + 9 * (len(fold0) - 1)
    assert replayed.se != first[1].se


def test_pliv_bf16_vs_f64_panel(gpu):
    """Storage parity on a host-built 50,000 x 60 panel: the differences are printed, not
    bounded (profiles/pliv/README.md records them); n and the rank flag must agree."""
    d = make_pliv_data(50_000, 2, 2, p_extra=39)
    assert d.X.shape == (50_000, 60)
    fid = np.asarray(rng.fold_ids(d.n, 5, 1991, 0), dtype=np.int64)
    out = {}
    for dt in ("bf16", "f64"):
        pan = DP._build(d.Y, d.D, d.Z, d.X, fid, dt, gpu)
        res, mom, _ = DP.pliv_panel(pan, 5, 2)
        torch.cuda.synchronize()
        out[dt] = (res.cpu().numpy(), mom.cpu().numpy())
    (rb, mb), (r64, m64) = out["bf16"], out["f64"]
    print("theta bf16", rb[0], "f64", r64[0], "dtheta/SE", abs(rb[0] - r64[0]) / r64[1])
    print("SE bf16", rb[1], "f64", r64[1], "dSE/SE", abs(rb[1] - r64[1]) / r64[1])
    assert mb[0] == m64[0] == 50_000
    assert rb[3] == r64[3] == 0.0


def test_lds_bound_is_the_kernels(gpu):
    from ate_replication_causalml_amd import _native
    assert int(_native.hip().ate_pliv_lds_max()) == DP.PLIV_LDS_MAX
