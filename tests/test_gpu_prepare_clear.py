"""``ate_enet_prepare_fused_clear`` (csrc/enet.hip): the fused prepare that also clears the
zero-initialised block of the launches behind it (the path launch's counters and R^2 table,
the tail's arrival counter, a spare counter for the DML residual pass), so the fused chain
runs no fill launch. Its other outputs are those of ``ate_enet_prepare_fused`` bit for bit;
the block is zero over exactly its nzero words, whatever it held; ``cv_enet_gaussian`` hands
the spare counter out zeroed. (The DML call that takes it is compared with the chain of
separate launches by tests/test_cv_fused_switch.py and tests/test_gpu_resid_final.py.)"""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from test_gpu_prepare_fused import _MASKS, _bits, _design, _run, _stream

pytestmark = pytest.mark.gpu


def _run_clear(gpu, G, P, masks, xcols, ycols, c_f32, nzero, pad=3):
    nseg, (nt, p, ny) = G.shape[0], (masks.shape[0], len(xcols), len(ycols))
    ldc = (p + 63) // 64 * 64
    f64 = dict(dtype=torch.float64, device=gpu)
    Gd = torch.from_numpy(G).to(gpu)
    mk, xc, yc = (torch.from_numpy(a).to(gpu) for a in (masks, xcols, ycols))
    cdt = torch.float32 if c_f32 else torch.float64
    out = dict(C=torch.full((nt, p, ldc), 7.0, dtype=cdt, device=gpu),
               g=torch.full((nt, ny, p), 7.0, **f64), xm=torch.full((nt, p), 7.0, **f64),
               xs=torch.full((nt, p), 7.0, **f64),
               ju=torch.full((nt, p), 7, dtype=torch.uint8, device=gpu),
               ym=torch.full((nt, ny), 7.0, **f64), ys=torch.full((nt, ny), 7.0, **f64),
               nobs=torch.full((nt,), 7.0, **f64), lams=torch.full((5, 9), 7.0, **f64))
    # the block inside a larger buffer of -1: the words around it must keep their bits
    blk = torch.full((pad + nzero + pad,), -1, dtype=torch.int32, device=gpu)
    args = [Gd.data_ptr(), nseg, P, mk.data_ptr(), nt, xc.data_ptr(), p, 0, yc.data_ptr(), ny,
            out["C"].data_ptr(), c_f32] + [out[k].data_ptr() for k in
                                           ("g", "xm", "xs", "ju", "ym", "ys", "nobs")]
    args += [out["lams"].data_ptr(), out["lams"].numel(),
             blk[pad:].data_ptr() if nzero else None, nzero]
    _native.call("ate_enet_prepare_fused_clear", *args, _stream())
    torch.cuda.synchronize()
    return out, blk


# nzero: none, one word, below / at / past one workgroup's 256 threads, and more words than
# the smallest grid (p = 1: one workgroup) covers in one sweep
@pytest.mark.parametrize("p,nzero", [(1, 0), (1, 1), (1, 255), (1, 1000), (65, 256), (65, 257),
                                     (500, 6151)])
def test_prepare_clear_outputs_and_block(gpu, p, nzero):
    G, P, xcols, ycols = _design(p, 2, 5)
    masks = _MASKS[5]
    for c_f32 in (0, 1):
        ref = _run("ate_enet_prepare_fused", gpu, G, P, masks, xcols, ycols, c_f32)
        new, blk = _run_clear(gpu, G, P, masks, xcols, ycols, c_f32, nzero)
        for k in ref:
            assert torch.equal(_bits(ref[k]), _bits(new[k])), (k, c_f32)
        b = blk.cpu().numpy()
        assert (b[:3] == -1).all() and (b[3 + nzero:] == -1).all()
        assert not b[3:3 + nzero].any()


def test_cv_call_hands_out_a_cleared_spare_counter(gpu):
    """The fused chain's counters come from an uninitialised buffer that the prepare clears:
    repeated calls, each reusing the block the one before freed and left dirty, return the
    same bits, and spare_zero is 0 every time (ATE_CV_FUSED=0: there is none)."""
    from ate_replication_causalml_amd.ops import enet as E
    from ate_replication_causalml_amd.ops import gram as gram_op
    from ate_replication_causalml_amd.ops.panel import build_panel
    from ate_replication_causalml_amd.parallel import rng
    rs = np.random.RandomState(3)
    n, p = 3000, 70
    X = rs.randn(n, p)
    y = X[:, :5] @ [1.0, -1.0, 0.5, 0.3, -0.4] + rs.randn(n)
    pan = build_panel(X, None, y, folds=rng.fold_ids(n, 5, 1), dtype="f32", device=gpu)
    G = gram_op.gram(pan)
    fields = ("lambdas", "coef_path", "cvm", "cvsd", "sel", "coef_min", "coef_1se", "nlam",
              "npass", "fold_npass", "fold_nlam")
    runs = []
    for _ in range(3):
        r = E.cv_enet_gaussian(G, pan, pan.xcols, [pan.cols["Y"]]).check()
        runs.append({f: _bits(getattr(r, f)).clone() for f in fields})
        if not E.CV_FUSED:
            assert r.spare_zero is None
            continue
        assert r.spare_zero.dtype == torch.int32 and r.spare_zero.numel() == 1
        assert int(r.spare_zero.item()) == 0
        # dirty the block before it goes back to the allocator for the next call
        r.spare_zero.fill_(-1)
        r.npass.fill_(-7)
        r.nlam.fill_(-7)
        del r
    for other in runs[1:]:
        for f in fields:
            assert torch.equal(runs[0][f], other[f]), f
