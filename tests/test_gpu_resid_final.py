"""``ate_dml_resid_moments_final`` (csrc/dml.hip: the residual pass finishes its own moments
and theta / SE) against ``ate_dml_resid_moments`` + ``ate_dml_finalize`` on the same device
inputs, bit for bit, moments and result.

Fold sizes that are no multiple of a block's 8 x 256 rows (bf16) or 4 x 256 (float64), grids
of fewer and more workgroups than the 256 partials one summing thread takes, a fold with an
empty LASSO support and one with a single column, continuous (hi + lo) and binary
(y1 = w1 = -1) targets."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
from ate_replication_causalml_amd.ops.panel import dtype_code

pytestmark = pytest.mark.gpu

K, P_X = 3, 30


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def panels(gpu):
    return {dt: synthetic_panel(13001, p=P_X, folds=K, seed=11, dtype=dt, device=gpu)
            for dt in ("bf16", "f64")}


@pytest.fixture(scope="module")
def coef(gpu):
    """[K, 2, p + 1]: fold 0 dense-ish, fold 1 intercepts only (empty support), fold 2 one
    column (in the W fit only)."""
    rs = np.random.RandomState(3)
    c = rs.randn(K, 2, P_X + 1) * 0.2 * (rs.rand(K, 2, P_X + 1) < 0.4)
    c[:, :, 0] = rs.randn(K, 2)
    c[1, :, 1:] = 0.0
    c[2, :, 1:] = 0.0
    c[2, 1, 7] = 0.31
    return torch.from_numpy(c).to(gpu)


def _args(pan, coef, binary):
    dev = pan.device
    xc = torch.as_tensor(pan.xcols, dtype=torch.int32, device=dev)
    segs = torch.as_tensor(np.asarray(pan.seg_bounds[:K], dtype=np.int64), device=dev)
    bf = pan.dtype == torch.bfloat16
    y0, y1 = (pan.cols["Y_hi"], pan.cols["Y_lo"]) if bf else (pan.cols["Y"], -1)
    w0, w1 = (pan.cols["W_hi"], pan.cols["W_lo"]) if bf else (pan.cols["W"], -1)
    if binary:
        y1 = w1 = -1
    cs, bs = pan.strides()
    keep = (xc, segs)
    return [dtype_code(pan.data), pan.data.data_ptr(), cs, bs, xc.data_ptr(), len(pan.xcols),
            segs.data_ptr(), K, coef.data_ptr(), y0, y1, w0, w1, pan.cols["one"]], keep


def _chain(pan, coef, nbx, binary):
    a, keep = _args(pan, coef, binary)
    f64 = dict(dtype=torch.float64, device=pan.device)
    part, mom, res = torch.empty(K * nbx * 7, **f64), torch.empty(7, **f64), torch.empty(2, **f64)
    _native.call("ate_dml_resid_moments", *a, nbx, part.data_ptr(), mom.data_ptr(), _stream())
    _native.call("ate_dml_finalize", mom.data_ptr(), 0, res.data_ptr(), _stream())
    return mom, res, keep


def _final(pan, coef, nbx, binary, args=None):
    a, keep = args or _args(pan, coef, binary)     # (a capture cannot upload the tables)
    f64 = dict(dtype=torch.float64, device=pan.device)
    part, mom, res = torch.empty(K * nbx * 7, **f64), torch.full((7,), 7.0, **f64), \
        torch.full((2,), 7.0, **f64)
    done = torch.zeros(1, dtype=torch.int32, device=pan.device)
    _native.call("ate_dml_resid_moments_final", *a, nbx, part.data_ptr(), done.data_ptr(),
                 mom.data_ptr(), res.data_ptr(), _stream())
    return mom, res, (keep, part, done)


def _same(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("nbx", [1, 3, 512])
@pytest.mark.parametrize("dt", ["bf16", "f64"])
def test_resid_final_equals_chain(gpu, panels, coef, dt, nbx, binary):
    pan = panels[dt]
    sizes = np.diff(np.asarray(pan.seg_bounds[:K]), axis=1).ravel()
    assert all(int(s) % (8 * 256) for s in sizes) and len(pan.seg_nreal) == K
    if binary and dt != "bf16":
        binary = False                    # float64 panels: one column per target as it is
    mom0, res0, _k0 = _chain(pan, coef, nbx, binary)
    mom1, res1, _k1 = _final(pan, coef, nbx, binary)
    torch.cuda.synchronize()
    assert float(mom0[5]) == sum(int(v) for v in pan.seg_nreal) and float(res0[1]) > 0
    assert _same(mom0, mom1) and _same(res0, res1)
    assert int(_k1[2]) == K * nbx


def test_resid_final_graph_replay(gpu, panels, coef):
    """Captured once with its zeroed arrival counter, replayed three times: the same bits."""
    pan = panels["bf16"]
    mom0, res0, _k0 = _chain(pan, coef, 512, False)
    args = _args(pan, coef, False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _final(pan, coef, 512, False, args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mom1, res1, _k1 = _final(pan, coef, 512, False, args)
    for _ in range(3):
        mom1.fill_(7)
        res1.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(mom0, mom1) and _same(res0, res1)
