"""``propensity="logit"`` of DML-IRM on the GPU: the logistic link of the fused score pass
(csrc/irm.hip ``ate_irm_score_link``) against its float64 twin, and the estimators against
reference.estimators with the binomial CV-LASSO propensity.

Estimator tolerance. The binomial path converges to glmnet's 1e-7 threshold, so the 1e-6 of
the linear estimator's test is not derivable here. Measured against the reference twin on the
two designs (n = 2000 seed 4; n = 4000 seeds 1-3; profiles/irm_logit/README.md), the largest
|dATE| was 3.4e-9 and the largest |dSE| 1.6e-9; the bound is 10 x the larger, rounded up to a
power of ten: 1e-7 absolute, tighter than 1e-4 of the smallest SE there (0.046: 4.6e-6)."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.estimators import cate as DC
from ate_replication_causalml_amd.estimators import gate as DG
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.estimators import policy as DP
from ate_replication_causalml_amd.estimators import targets as DT
from ate_replication_causalml_amd.ops.panel import build_panel, dtype_code
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.reference import estimators as E
from ate_replication_causalml_amd.reference import glmnet as gn
from ate_replication_causalml_amd.result import SENS_MOMENTS, TARGET_MOMENTS

pytestmark = pytest.mark.gpu

COUNTS = (130, 7, 64, 1, 257, 70)   # the layout of test_gpu_irm.py::_case(exact=False)
P_X = 300
CLIP = 0.2
TOL = 1e-7                          # |dATE|, |dSE| against the reference twin (module docstring)
FOLDS = 5


def _case():
    """test_gpu_irm.py::_case(exact=False) with the row-2 coefficients scaled by 8, so that
    sigmoid(eta) spans both clip bounds."""
    rs = np.random.RandomState(17)
    seg = np.repeat(np.arange(6), COUNTS)
    seg = seg[rs.permutation(len(seg))]
    n = len(seg)
    W = (seg & 1).astype(float)
    X = rs.randn(n, P_X)
    Y = rs.randn(n) + W
    support = np.unique(np.r_[0, 255, 256, 299, rs.choice(P_X, 36, replace=False)])
    coef = np.zeros((3, 3, P_X + 1))
    for k in (0, 2):
        for r in range(3):
            on = support[rs.rand(len(support)) < 0.6]
            coef[k, r, 1 + on] = rs.randn(len(on)) * (0.1 if r == 2 else 0.5)
        coef[k, :, 1 + np.array([0, 255, 256, 299])] = (np.array([[3, -5, 2], [-4, 6, 1],
                                                                  [7, 2, -3], [-2, -7, 4]]) / 64.0)
    coef[:, 0, 0], coef[:, 1, 0], coef[:, 2, 0] = 0.25, 0.75, 0.5
    coef[:, 2, 1:] *= 8.0
    return X, W, Y, seg, coef


def _prob(X, seg, coef):
    eta = np.array([coef[s // 2, 2, 0] + coef[s // 2, 2, 1:] @ x for x, s in zip(X, seg)])
    return 1.0 / (1.0 + np.exp(-eta))


def _check(got, want, counts):
    got, want = got.cpu().numpy(), want.numpy()
    print("moments gpu ", got.tolist())
    print("moments twin", want.tolist())
    print("rel err     ", (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).tolist())
    np.testing.assert_allclose(got, want, rtol=1e-11)
    for i in counts:
        assert got[i] == want[i]
    assert 0 < got[3] < got[2]                            # many rows clip, not all


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_score_pass_logistic_vs_twin(gpu, dtype):
    X, W, Y, seg, coef = _case()
    pc = build_panel(X, W, Y, folds=seg, dtype=dtype, device="cpu")
    pg = build_panel(X, W, Y, folds=seg, dtype=dtype, device=gpu)
    assert tuple(pg.seg_nreal) == COUNTS and pg.ld > len(Y)
    # the probabilities of the panel's own (rounded) values: both clip bounds are crossed and
    # no row sits within 1e-6 of one
    Xp = X if dtype == "f64" else X.astype(np.float32).astype(np.float64)
    m = _prob(Xp, seg, coef)
    assert (m < CLIP).sum() > 20 and (m > 1 - CLIP).sum() > 20
    assert ((m > CLIP) & (m < 1 - CLIP)).sum() > 20
    assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6
    c = torch.from_numpy(coef)
    cg = c.to(gpu)
    passes = [(DI.irm_score_moments, (2, 3, 7)),
              (DI.irm_sens_moments, (2, 3, len(SENS_MOMENTS) - 1)),
              (DI.irm_target_moments, (2, 3, len(TARGET_MOMENTS) - 1))]
    for f, counts in passes:
        want = f(pc, c, CLIP, 2, link="logistic")
        assert want[2] == len(Y)
        for nbx in (None, 1):
            got = f(pg, cg, CLIP, 2, nbx=nbx, link="logistic")
            torch.cuda.synchronize()
            _check(got, want, counts)
    # ROWS: per row, and 0 on padding
    want = DI.irm_scores(pc, c, CLIP, 2, link="logistic").numpy()
    for nbx in (None, 1):
        got = DI.irm_scores(pg, cg, CLIP, 2, nbx=nbx, link="logistic").cpu().numpy()
        real = pg.row_index.cpu().numpy() >= 0
        assert np.array_equal(real, pc.row_index.numpy() >= 0)
        np.testing.assert_allclose(got[real], want[real], rtol=1e-11, atol=1e-13)
        assert np.all(got[~real] == 0) and real.sum() == len(Y)
    # the logistic link changes the result (the identity pass reads eta as a probability)
    assert not torch.equal(DI.irm_score_moments(pg, cg, CLIP, 2).cpu(),
                           DI.irm_score_moments(pg, cg, CLIP, 2, link="logistic").cpu())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_identity_link_entry_equals_old_entries(gpu, dtype):
    """ate_irm_score_link with link 0 gives the bits of the four existing entry points."""
    X, W, Y, seg, coef = _case()
    pg = build_panel(X, W, Y, folds=seg, dtype=dtype, device=gpu)
    cg = torch.from_numpy(coef).to(gpu)
    old = [DI.irm_score_moments(pg, cg, CLIP, 2), DI.irm_scores(pg, cg, CLIP, 2),
           DI.irm_sens_moments(pg, cg, CLIP, 2), DI.irm_target_moments(pg, cg, CLIP, 2)]
    y0, y1, w0, w1 = DI._yw_columns(pg)
    xc = torch.tensor(pg.xcols, dtype=torch.int32, device=gpu)
    segs = torch.as_tensor(np.asarray(pg.seg_bounds, dtype=np.int64), device=gpu)
    cs, bs = pg.strides()
    nbx = 256
    for mode, want in enumerate(old):
        n_out = want.numel()
        out = torch.full((n_out,), float("nan"), dtype=torch.float64, device=gpu)
        partial = out if mode == 1 else torch.empty(pg.nseg * nbx * n_out, dtype=torch.float64,
                                                    device=gpu)
        _native.call("ate_irm_score_link", mode, 0, dtype_code(pg.data), pg.data.data_ptr(), cs, bs,
                     xc.data_ptr(), P_X, segs.data_ptr(), pg.nseg, 2, cg.data_ptr(), y0, y1, w0,
                     w1, pg.cols["one"], CLIP, nbx, partial.data_ptr(),
                     None if mode == 1 else out.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want.cpu()), mode


def test_bf16_raises(gpu):
    X, W, Y, seg, coef = _case()
    pg = build_panel(X, W, Y, folds=seg, dtype="bf16", device=gpu)
    cg = torch.from_numpy(coef).to(gpu)
    for f in (DI.irm_score_moments, DI.irm_sens_moments, DI.irm_target_moments, DI.irm_scores):
        with pytest.raises(ValueError, match="fp32 / fp64"):
            f(pg, cg, CLIP, 2, link="logistic")
    # the entry point itself: -1 without a launch
    y0, y1, w0, w1 = DI._yw_columns(pg)
    z = torch.zeros(4096, dtype=torch.float64, device=gpu)
    cs, bs = pg.strides()
    with pytest.raises(_native.NativeError) as e:
        _native.call("ate_irm_score_link", 0, 1, 3, pg.data.data_ptr(), cs, bs, z.data_ptr(), P_X,
                     z.data_ptr(), pg.nseg, 2, cg.data_ptr(), y0, y1, w0, w1, pg.cols["one"], CLIP,
                     1, z.data_ptr(), z.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert e.value.status == -1
    torch.cuda.synchronize()
    assert torch.all(z == 0)


# ---------------------------------------------------------------- the estimators
def _design(n=2000, p=10, seed=4):
    """Strong selection: true propensity sigmoid(-1 + 1.5 x0 + x1)."""
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, p))
    pr = 1 / (1 + np.exp(-(-1 + 1.5 * X[:, 0] + X[:, 1])))
    W = (r.uniform(size=n) < pr).astype(float)
    Y = X[:, 0] + 0.5 * X[:, 2] + (1 + X[:, 0]) * W + r.normal(size=n)
    return Y, W, X


_CACHE = {}


def _ref_m_fits():
    """The reference's K binomial propensity fits of the design (folds of seed 1991)."""
    if "m" not in _CACHE:
        Y, W, X = _design()
        fid = rng.fold_ids(len(Y), FOLDS, 1991, stream=0)
        fits = []
        for k in range(FOLDS):
            rows = fid != k
            inner = np.where(fid > k, fid - 1, fid)
            fits.append(gn.cv_glmnet(X[rows], W[rows], family="binomial", foldid=inner[rows]))
        _CACHE["m"] = fits
    return _CACHE["m"]


def _ref(name, f, *a, **kw):
    if name not in _CACHE:
        _CACHE[name] = f(*a, **kw)
    return _CACHE[name]


def test_estimator_vs_reference(gpu):
    Y, W, X = _design()
    # the margins that keep the reference's lambda.min pick of m stable
    gaps = []
    for cv in _ref_m_fits():
        c, i = cv.cvm, cv.idx_min
        gaps.append(min(c[j] - c[i] for j in (i - 1, i + 1) if 0 <= j < len(c)) / c[i])
    print("relative margins at idx_min of m per fold:", gaps)
    assert min(gaps) >= 1.85e-5                           # 1.9e-5 to two digits: 186 x the cvm
                                                          # tolerance of the path test
    pan, counts, _, n, _ = DI.arm_split_panel(Y, W, X, FOLDS, 1991, "f64", gpu)
    st = DI.run_phases(DI.irm_fit_phases(pan, FOLDS, propensity="logit")[0])
    lin = DI.run_phases(DI.irm_fit_phases(pan, FOLDS)[0])
    torch.cuda.synchronize()
    sel = st["cv_m"].check().sel.cpu().numpy()
    for k, cv in enumerate(_ref_m_fits()):
        assert (sel[k, 0], sel[k, 1]) == (cv.idx_min, cv.idx_1se), k
        a0, b = cv.coef("lambda.min")
        np.testing.assert_allclose(st["coef"][k, 2].cpu().numpy(), np.r_[a0, b], atol=1e-7)
    # g0 and g1 carry the bits of the linear fit
    assert torch.equal(st["coef"][:, :2].cpu(), lin["coef"][:, :2].cpu())
    assert not torch.equal(st["coef"][:, 2].cpu(), lin["coef"][:, 2].cpu())
    a = DI.dml_irm_lasso(Y, W, X, folds=FOLDS, device=gpu, propensity="logit", graph=False)
    b = _ref("irm", E.dml_irm_lasso, Y, W, X, folds=FOLDS, propensity="logit")
    print("gpu", a.ate, a.se, a.diagnostics, "reference", b.ate, b.se, b.diagnostics)
    print("|dATE| %.3g |dSE| %.3g" % (abs(a.ate - b.ate), abs(a.se - b.se)))
    assert abs(a.ate - b.ate) <= TOL and abs(a.se - b.se) <= TOL and TOL <= 1e-4 * b.se
    assert a.diagnostics["propensity"] == "logit"
    assert a.diagnostics["n_clipped"] == b.diagnostics["n_clipped"]
    assert a.diagnostics["n_treated"] == b.diagnostics["n_treated"]


def test_graph_equals_eager_and_replays(gpu):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    Y, W, X = _design()
    estimator_graphs.clear()
    e = DI.dml_irm_lasso(Y, W, X, folds=FOLDS, device=gpu, propensity="logit", graph=False)
    runs = []
    for _ in range(3):
        runs.append(DI.dml_irm_lasso(Y, W, X, folds=FOLDS, device=gpu, propensity="logit"))
        torch.cuda.synchronize()
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    for r in runs:
        assert (r.ate, r.se, r.diagnostics["n_clipped"]) == (e.ate, e.se, e.diagnostics["n_clipped"])
    # the linear fit of the same layout is another cache entry, and another number
    lin = DI.dml_irm_lasso(Y, W, X, folds=FOLDS, device=gpu)
    assert lin.diagnostics["hipgraph"] is False and lin.ate != e.ate
    assert "propensity" not in lin.diagnostics
    estimator_graphs.clear()


def test_gate_logit_vs_reference(gpu):
    Y, W, X = _design()
    groups = (X[:, 3] > 0).astype(int) + 2 * (X[:, 4] > 0.5)
    a = DG.dml_irm_gate_lasso(Y, W, X, groups, folds=FOLDS, n_boot=199, device=gpu,
                              propensity="logit")
    b = _ref("gate", E.dml_irm_gate, Y, W, X, groups, folds=FOLDS, n_boot=199, propensity="logit")
    assert a.diagnostics["propensity"] == "logit" and a.n == b.n
    np.testing.assert_allclose(a.ate, b.ate, rtol=0, atol=TOL)
    np.testing.assert_allclose(a.se, b.se, rtol=0, atol=TOL)
    assert abs(a.overall.ate - b.overall.ate) <= TOL and abs(a.overall.se - b.overall.se) <= TOL


def test_cate_logit_vs_reference(gpu):
    Y, W, X = _design()
    a = DC.dml_irm_cate_lasso(Y, W, X, 0, df=5, n_boot=199, folds=FOLDS, device=gpu,
                              propensity="logit")
    b = _ref("cate", E.dml_irm_cate, Y, W, X, 0, df=5, n_boot=199, folds=FOLDS,
             propensity="logit")
    assert a.diagnostics["propensity"] == "logit"
    np.testing.assert_allclose(a.cate, b.cate, rtol=0, atol=TOL)
    np.testing.assert_allclose(a.se, b.se, rtol=0, atol=TOL)
    assert abs(a.overall.ate - b.overall.ate) <= TOL and abs(a.overall.se - b.overall.se) <= TOL


def test_policy_logit_vs_reference(gpu):
    Y, W, X = _design()
    a = DP.dml_irm_policy_lasso(Y, W, X, [0, 1, 2], bins=8, folds=FOLDS, device=gpu,
                                propensity="logit")
    b = _ref("policy", E.dml_irm_policy_tree, Y, W, X, [0, 1, 2], bins=8, folds=FOLDS,
             propensity="logit")
    assert a.diagnostics["propensity"] == "logit"
    keys = ("treat_all", "treat_all_se")                  # the mean score: whatever the tree
    if a.nodes == b.nodes and a.actions == b.actions:
        keys += ("value", "value_se", "advantage", "advantage_se")
    for k in keys:
        assert abs(a.in_sample[k] - b.in_sample[k]) <= TOL, k


def test_targets_logit_vs_reference(gpu):
    Y, W, X = _design()
    a = DT.dml_irm_targets(Y, W, X, folds=FOLDS, device=gpu, propensity="logit")
    b = _ref("targets", E.dml_irm_targets, Y, W, X, folds=FOLDS, propensity="logit")
    assert a.diagnostics["propensity"] == "logit"
    for t in ("all", "treated", "control"):
        assert abs(a.estimates[t].ate - b.estimates[t].ate) <= TOL, t
        assert abs(a.estimates[t].se - b.estimates[t].se) <= TOL, t
    assert a.diagnostics["n_clipped"] == b.diagnostics["n_clipped"]
