"""The binomial CV-LASSO kernels (csrc/lognet.hip) at the shapes where they take another route,
against reference.glmnet.cv_glmnet(family="binomial") with the comparison and tolerances of
test_gpu_glm.py::test_lognet_cv_gpu_vs_reference.

lognet_path_kernel dispatches on p to three instantiations: <24, 512> for p <= 24, <32, 256>
for p <= 32 and <96, 256> beyond, whose lanes own the coordinates in chunks of 64 (p > 64 uses
the second chunk). The cases sit on both sides of every threshold, put a constant column in
each chunk (the last lane of chunk 2 among them), and use three folds of unequal size whose
training row counts (700, 499, 467, 434) are multiples of none of 64, 256 or 512."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.ops.lognet import cv_lognet
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.reference import glmnet as gn

pytestmark = pytest.mark.gpu

N, L = 700, 30
FOLD_SIZES = (201, 233, 266)
ALPHA = {32: 0.7}
CONST = {65: 40, 96: 95}
_DATA, _REF = {}, {}


def _data(p):
    if p not in _DATA:
        r = np.random.default_rng(400 + p)
        X = r.normal(size=(N, p))
        if p in CONST:
            X[:, CONST[p]] = 1.0
        k = min(p, 4)
        eta = -0.4 + X[:, :k] @ np.array([0.8, -0.5, 0.3, 0.2])[:k]
        y = (r.uniform(size=N) < 1 / (1 + np.exp(-eta))).astype(float)
        fid = r.permutation(np.repeat(np.arange(3), FOLD_SIZES))
        tr = [N] + [N - s for s in FOLD_SIZES]
        assert all(t % 64 and t % 256 and t % 512 for t in tr)
        _DATA[p] = (X, y, fid)
    return _DATA[p]


def _reference(p, dtype):
    if (p, dtype) not in _REF:
        X, y, fid = _data(p)
        Xr = X if dtype == "f64" else X.astype(np.float32).astype(np.float64)
        _REF[p, dtype] = gn.cv_glmnet(Xr, y, family="binomial", alpha=ALPHA.get(p, 1.0),
                                      foldid=fid, nlambda=L)
    return _REF[p, dtype]


def _fit(gpu, p, dtype, **kw):
    X, y, fid = _data(p)
    pan = build_panel(X, None, y, folds=fid, dtype=dtype, device=gpu)
    assert pan.seg_nreal.tolist() == list(FOLD_SIZES)
    return cv_lognet(pan, pan.xcols, pan.cols["Y"], alpha=ALPHA.get(p, 1.0), nlambda=L, **kw)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("p,dtype", [(1, "f64"), (24, "f64"), (25, "f64"), (32, "f64"), (33, "f64"),
                                     (64, "f64"), (65, "f64"), (96, "f64"), (25, "f32"),
                                     (96, "f32")])
def test_lognet_shapes_vs_reference(gpu, p, dtype):
    ref = _reference(p, dtype)
    cv = _fit(gpu, p, dtype).check()
    m = int(cv.nlam[0])
    assert 5 <= len(ref.lambdas) < L                 # the reference path stops early
    assert m == len(ref.lambdas)
    lam, cvm, cvsd, path = _np(cv.lambdas), _np(cv.cvm), _np(cv.cvsd), _np(cv.coef_path)
    print("lognet p=%d %s: nlam %d lambda rel %.3g cvm rel %.3g coef_1se abs %.3g" % (
        p, dtype, m, np.max(np.abs(lam[:m] / ref.lambdas - 1)), np.max(np.abs(cvm[:m] / ref.cvm - 1)),
        np.max(np.abs(_np(cv.coef_1se) - np.r_[ref.coef()[0], ref.coef()[1]]))))
    np.testing.assert_allclose(lam[:m], ref.lambdas, rtol=1e-9)
    np.testing.assert_allclose(cvm[:m], ref.cvm, rtol=1e-7)
    sel = _np(cv.sel)
    assert (sel[0], sel[1]) == (ref.idx_min, ref.idx_1se)
    a0, b = ref.coef()
    np.testing.assert_allclose(_np(cv.coef_1se), np.r_[a0, b], atol=1e-7)
    # beyond the path's end everything per-lambda is NaN, as in the CPU twin
    assert path.shape == (L, p + 1)
    for a in (lam, cvm, cvsd, path):
        assert np.isfinite(a[:m]).all() and np.isnan(a[m:]).all()
    if p in CONST:
        j = CONST[p]
        assert np.all(ref.fit.beta[:, j] == 0) and np.all(path[:m, 1 + j] == 0)
        assert np.count_nonzero(path[m - 1, 1:]) >= 3


@pytest.mark.parametrize("p", [25, 96])
def test_lognet_concurrent_equals_two_launch_at(gpu, p):
    """The one-launch and the two-launch forms give the same bits on the <32> and the <96>
    (two lane chunks) instantiations, which test_gpu_glm.py's equality test does not reach."""
    a = _fit(gpu, p, "f64", concurrent=True)
    b = _fit(gpu, p, "f64", concurrent=False)
    assert (_np(a.npass) >= 0).all()
    assert torch.equal(a.nlam.cpu(), b.nlam.cpu()) and torch.equal(a.npass.cpu(), b.npass.cpu())
    assert torch.equal(a.sel.cpu(), b.sel.cpu())
    for f in ("lambdas", "cvm", "cvsd", "coef_path", "coef_min", "coef_1se"):
        x, y = _np(getattr(a, f)), _np(getattr(b, f))
        assert np.array_equal(x, y, equal_nan=True), f


def test_lognet_refusals(gpu):
    """p = 97 is refused by cv_lognet; the entry point itself returns -1 without a launch for
    p = 97, p = 0 and more than 64 segments."""
    r = np.random.default_rng(5)
    X = r.normal(size=(300, 97))
    y = (r.uniform(size=300) < 0.5).astype(float)
    pan = build_panel(X, None, y, folds=np.arange(300) % 3, dtype="f64", device=gpu)
    with pytest.raises(ValueError):
        cv_lognet(pan, pan.xcols, pan.cols["Y"], nlambda=L)
    z = torch.zeros(4096, dtype=torch.float64, device=gpu)
    zp = z.data_ptr()

    def status(p, nseg):
        with pytest.raises(_native.NativeError) as e:
            _native.call("ate_lognet_path", 2, zp, 64, zp, p, 0, zp, nseg, zp, 1, zp, 1.0, 1e-4,
                         1e-7, 100, None, None, L, zp, zp, zp, zp, zp, zp, None, None,
                         torch.cuda.current_stream().cuda_stream)
        return e.value.status

    assert status(97, 3) == -1 and status(0, 3) == -1 and status(8, 65) == -1
    torch.cuda.synchronize()
    assert torch.all(z == 0)
