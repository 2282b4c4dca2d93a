"""The grouped concurrent binomial path (csrc/lognet.hip ``ate_lognet_path_groups``), the
held-out deviance over segment sets (``ate_lognet_cvloss_set``) and ``ops.lognet.cv_lognet_groups``
against reference.glmnet.cv_glmnet(family="binomial") per group, with the comparisons and
tolerances of test_gpu_lognet_shapes.py.

The layout is the one a cross-fit uses: an arm-split panel of K = 3 folds (six segments, the
target is W itself), group k = the training set without fold k, its CV folds the two other
folds, each two segments. One case per instantiation of lognet_path_kernel (p = 5: <24, 512>,
p = 25: <32, 256>, p = 70: <96, 256> with the second lane chunk)."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.estimators.irm import logit_fold_sets
from ate_replication_causalml_amd.ops.lognet import cv_lognet_groups
from ate_replication_causalml_amd.ops.panel import build_panel, dtype_code
from ate_replication_causalml_amd.reference import glmnet as gn

pytestmark = pytest.mark.gpu

N, L, K = 700, 30, 3
FOLD_SIZES = (201, 233, 266)
CASES = [(5, 5001), (25, 25000), (70, 70000)]
SEED = dict(CASES)
_DATA, _REF = {}, {}


def _data(p):
    if p not in _DATA:
        r = np.random.default_rng(SEED[p])
        X = r.normal(size=(N, p))
        eta = -0.4 + X[:, :4] @ np.array([0.8, -0.5, 0.3, 0.2])
        W = (r.uniform(size=N) < 1 / (1 + np.exp(-eta))).astype(float)
        fid = r.permutation(np.repeat(np.arange(K), FOLD_SIZES))
        _DATA[p] = (X, W, fid)
    return _DATA[p]


def _reference(p, dtype):
    """Per group k: cv.glmnet on the rows outside fold k, the other folds as CV folds."""
    if (p, dtype) not in _REF:
        X, W, fid = _data(p)
        Xr = X if dtype == "f64" else X.astype(np.float32).astype(np.float64)
        out = []
        for k in range(K):
            rows = fid != k
            inner = np.where(fid > k, fid - 1, fid)
            out.append(gn.cv_glmnet(Xr[rows], W[rows], family="binomial", foldid=inner[rows],
                                    nlambda=L))
        _REF[p, dtype] = out
    return _REF[p, dtype]


def _panel(gpu, p, dtype):
    X, W, fid = _data(p)
    pan = build_panel(X, W, W, folds=2 * fid + W.astype(np.int64), dtype=dtype, device=gpu,
                      nseg=2 * K)
    assert pan.nseg == 2 * K and 70 <= min(pan.seg_nreal) and max(pan.seg_nreal) <= 175
    return pan


def _fit(gpu, p, dtype):
    pan = _panel(gpu, p, dtype)
    return cv_lognet_groups(pan, pan.xcols, pan.cols["W"], logit_fold_sets(K), nlambda=L)


def _np(t):
    return t.detach().cpu().numpy()


def _margins(ref):
    """(relative gap of cvm[idx_min] to its neighbours, relative gap of the 1-SE threshold to
    the nearest cvm): what keeps the picks stable under the 1e-7 cvm tolerance."""
    c, i = ref.cvm, ref.idx_min
    nb = [c[j] for j in (i - 1, i + 1) if 0 <= j < len(c)]
    thr = c[i] + ref.cvsd[i]
    return min(v - c[i] for v in nb) / c[i], np.min(np.abs(c - thr)) / thr


@pytest.mark.parametrize("p,dtype", [(5, "f64"), (25, "f64"), (70, "f64"), (25, "f32")])
def test_groups_vs_reference(gpu, p, dtype):
    refs = _reference(p, dtype)
    for k, ref in enumerate(refs):
        gmin, g1se = _margins(ref)
        print("p=%d %s group %d: margin at idx_min %.3g, at the 1-SE threshold %.3g" % (
            p, dtype, k, gmin, g1se))
        if dtype == "f64":                       # the scanned margins of the three f64 cases
            assert gmin >= 1.7e-4 and g1se >= 1.6e-3
        assert gmin >= 1e-4 and g1se >= 1e-4     # 1000 x the cvm tolerance
    cv = _fit(gpu, p, dtype).check()
    torch.cuda.synchronize()
    assert (_np(cv.npass) >= 0).all() and cv.npass.shape[0] == K * K
    lam, cvm, cvsd, sel, nlam = (_np(t) for t in (cv.lambdas, cv.cvm, cv.cvsd, cv.sel, cv.nlam))
    for k, ref in enumerate(refs):
        m = int(nlam[k])
        assert m == len(ref.lambdas) and 5 <= m <= L
        print("p=%d %s group %d: nlam %d lambda rel %.3g cvm rel %.3g" % (
            p, dtype, k, m, np.max(np.abs(lam[k, :m] / ref.lambdas - 1)),
            np.max(np.abs(cvm[k, :m] / ref.cvm - 1))))
        np.testing.assert_allclose(lam[k, :m], ref.lambdas, rtol=1e-9)
        np.testing.assert_allclose(cvm[k, :m], ref.cvm, rtol=1e-7)
        assert (sel[k, 0], sel[k, 1]) == (ref.idx_min, ref.idx_1se)
        for name, got in (("lambda.min", cv.coef_min), ("lambda.1se", cv.coef_1se)):
            a0, b = ref.coef(name)
            np.testing.assert_allclose(_np(got)[k], np.r_[a0, b], atol=1e-7)
        for a in (lam[k], cvm[k], cvsd[k]):
            assert np.isfinite(a[:m]).all() and np.isnan(a[m:]).all()


def test_groups_two_runs_same_bits(gpu):
    a, b = _fit(gpu, 25, "f64"), _fit(gpu, 25, "f64")
    torch.cuda.synchronize()
    for f in ("lambdas", "nlam", "cvm", "cvsd", "sel", "coef_min", "coef_1se", "npass"):
        assert np.array_equal(_np(getattr(a, f)), _np(getattr(b, f)), equal_nan=True), f


def _raw_path(pan, p, masks, leader, flmin=1e-4):
    """ate_lognet_path in concurrent mode (leader None) or ate_lognet_path_groups on the same
    problems; every per-problem output."""
    dev = pan.device
    nq, nseg = masks.shape
    f64 = dict(dtype=torch.float64, device=dev)
    segs = np.stack([pan.seg_bounds[:, 0], pan.seg_bounds[:, 0] + pan.seg_nreal], 1)
    segs_t = torch.as_tensor(segs.astype(np.int64), device=dev)
    xc = torch.tensor(pan.xcols, dtype=torch.int32, device=dev)
    vp = torch.ones(p, **f64)
    mk = torch.from_numpy(masks).to(dev)
    out = dict(a0=torch.zeros((nq, L), **f64), beta=torch.zeros((nq, L, p), **f64),
               lam=torch.full((nq, L), float("nan"), **f64), dev=torch.zeros((nq, L), **f64),
               nlam=torch.zeros(nq, dtype=torch.int32, device=dev),
               npass=torch.zeros(nq, dtype=torch.int32, device=dev))
    ngroups = 1 if leader is None else int(np.sum(leader == np.arange(nq)))
    progress = torch.zeros((ngroups, 2), dtype=torch.int32, device=dev)
    lampub = torch.zeros((ngroups, L), **f64)
    st = torch.cuda.current_stream().cuda_stream
    head = (dtype_code(pan.data), pan.data.data_ptr(), pan.cm_ld, xc.data_ptr(), p,
            pan.cols["Y"], segs_t.data_ptr(), nseg, mk.data_ptr(), nq)
    tail = (L, *(out[f].data_ptr() for f in ("a0", "beta", "lam", "dev", "nlam", "npass")),
            progress.data_ptr(), lampub.data_ptr(), st)
    if leader is None:
        _native.call("ate_lognet_path", *head, vp.data_ptr(), 1.0, flmin, 1e-7, 100000, None, None,
                     *tail)
    else:
        lead_t = torch.from_numpy(leader).to(dev)
        fl = torch.full((ngroups,), flmin, **f64)
        _native.call("ate_lognet_path_groups", *head, leader.ctypes.data, lead_t.data_ptr(),
                     vp.data_ptr(), 1.0, fl.data_ptr(), 1e-7, 100000, *tail)
    torch.cuda.synchronize()
    return {f: _np(t) for f, t in out.items()}


@pytest.mark.parametrize("p", [5, 25, 70])
def test_one_group_equals_lognet_path(gpu, p):
    """One group with cv_lognet's masks (the full problem, then each segment left out) through
    the grouped entry point: the bits of ate_lognet_path in concurrent mode."""
    X, W, fid = _data(p)
    pan = build_panel(X, None, W, folds=fid, dtype="f64", device=gpu)
    masks = np.ones((1 + K, K), dtype=np.uint8)
    for k in range(K):
        masks[1 + k, k] = 0
    a = _raw_path(pan, p, masks, None)
    b = _raw_path(pan, p, masks, np.zeros(1 + K, dtype=np.int32))
    assert (a["npass"] > 0).all() and (a["nlam"] >= 5).all()
    for f in a:
        assert np.array_equal(a[f], b[f], equal_nan=True), f


def test_groups_refusals(gpu):
    """-1 without a launch: a leader behind a follower, a follower of a follower, 257 problems,
    L = 2; the buffer every pointer names stays untouched."""
    z = torch.zeros(1 << 16, dtype=torch.float64, device=gpu)
    zp = z.data_ptr()

    def status(leader, nlambda=L):
        leader = np.asarray(leader, dtype=np.int32)
        with pytest.raises(_native.NativeError) as e:
            _native.call("ate_lognet_path_groups", 2, zp, 64, zp, 8, 0, zp, 3, zp, len(leader),
                         leader.ctypes.data, zp, zp, 1.0, zp, 1e-7, 100, nlambda, zp, zp, zp, zp,
                         zp, zp, zp, zp, torch.cuda.current_stream().cuda_stream)
        return e.value.status

    assert status([0, 0, 2]) == -1                       # a leader behind a follower
    assert status([0, 0, 1]) == -1                       # a follower of a follower
    assert status([0] * 257) == -1                       # more than 256 problems
    assert status([0, 0, 0], nlambda=2) == -1            # L = 2
    torch.cuda.synchronize()
    assert torch.all(z == 0)
