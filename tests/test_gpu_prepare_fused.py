"""``ate_enet_prepare_fused`` (csrc/enet.hip: one launch) against ``ate_enet_prepare`` (two
launches, after a zero fill of C and a NaN fill of the lambda table) on the same device
inputs, bit for bit: C with its pad columns, g, xm, xs, ju, ym, ys, nobs, and the NaN table.
The old entry point is pinned against its float64 twin in tests/test_gpu_enet_kernels.py.

Shapes: p on both sides of the 16-row and 64-column tile edges and at the flagship's 500;
one and two targets; two and five segments with training sets of one segment, all but one
and all; a Gram stack that is NOT symmetric (every (j, k) must come from its own entry); an
x column and a target that are constant in the one-segment training set (ju = 0 with its
identity row / column, scale 1)."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native

pytestmark = pytest.mark.gpu

_MASKS = {2: np.array([[1, 0], [0, 1], [1, 1]], dtype=np.uint8),
          5: np.array([[0, 0, 1, 0, 0], [1, 1, 0, 1, 1], [0, 1, 1, 1, 1], [1, 1, 1, 1, 1]],
                      dtype=np.uint8)}
_LONE = {2: 0, 5: 2}     # the segment that is a training set on its own


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _design(p, ny, nseg):
    """Gram stack [nseg, P, P] of Z (ones column 0, x columns a permutation of 1..p, targets
    after them), x column p // 2 and target 0 constant in segment _LONE (0.75 and 3: their
    sums and sums of squares are exact, so the variance there is exactly 0), then every
    off-diagonal entry outside the ones row / column perturbed on ONE side only."""
    rs = np.random.RandomState(7000 + 10 * p + 3 * ny + nseg)
    P = (p + ny + 1 + 63) // 64 * 64
    rows = 24
    Z = rs.randn(nseg, rows, P) * rs.uniform(0.5, 2.0, P) + rs.uniform(-1.0, 1.0, P)
    Z[:, :, 0] = 1.0
    xcols = (1 + rs.permutation(p)).astype(np.int32)
    ycols = (p + 1 + np.arange(ny)).astype(np.int32)
    Z[_LONE[nseg], :, xcols[p // 2]] = 0.75
    Z[_LONE[nseg], :, ycols[0]] = 3.0
    G = np.einsum("sri,srj->sij", Z, Z)
    bump = np.triu(rs.uniform(0.01, 0.05, (nseg, P, P)), 1)
    bump[:, 0, :] = 0.0
    G = G + bump                                   # (j, k) != (k, j) for 0 < j < k
    assert not np.allclose(G, G.transpose(0, 2, 1))
    return G, P, xcols, ycols


def _run(entry, gpu, G, P, masks, xcols, ycols, c_f32):
    nseg, (nt, p, ny) = G.shape[0], (masks.shape[0], len(xcols), len(ycols))
    ldc = (p + 63) // 64 * 64
    f64 = dict(dtype=torch.float64, device=gpu)
    Gd = torch.from_numpy(G).to(gpu)
    mk, xc, yc = (torch.from_numpy(a).to(gpu) for a in (masks, xcols, ycols))
    cdt = torch.float32 if c_f32 else torch.float64
    fused = entry == "ate_enet_prepare_fused"
    # the fused launch owes every element: hand it buffers full of something else
    C = torch.full((nt, p, ldc), 7.0, dtype=cdt, device=gpu) if fused else \
        torch.zeros((nt, p, ldc), dtype=cdt, device=gpu)
    lams = torch.full((5, 9), 7.0 if fused else float("nan"), **f64)
    out = dict(C=C, g=torch.full((nt, ny, p), 7.0, **f64), xm=torch.full((nt, p), 7.0, **f64),
               xs=torch.full((nt, p), 7.0, **f64),
               ju=torch.full((nt, p), 7, dtype=torch.uint8, device=gpu),
               ym=torch.full((nt, ny), 7.0, **f64), ys=torch.full((nt, ny), 7.0, **f64),
               nobs=torch.full((nt,), 7.0, **f64), lams=lams)
    args = [Gd.data_ptr(), nseg, P, mk.data_ptr(), nt, xc.data_ptr(), p, 0, yc.data_ptr(), ny,
            C.data_ptr(), c_f32] + [out[k].data_ptr() for k in
                                    ("g", "xm", "xs", "ju", "ym", "ys", "nobs")]
    if fused:
        args += [lams.data_ptr(), lams.numel()]
    _native.call(entry, *args, _stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("nseg", [2, 5])
@pytest.mark.parametrize("ny", [1, 2])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 449, 500])
def test_prepare_fused_equals_two_launch_chain(gpu, p, ny, nseg):
    G, P, xcols, ycols = _design(p, ny, nseg)
    masks = _MASKS[nseg]
    for c_f32 in (0, 1):
        old = _run("ate_enet_prepare", gpu, G, P, masks, xcols, ycols, c_f32)
        new = _run("ate_enet_prepare_fused", gpu, G, P, masks, xcols, ycols, c_f32)
        # the design does what it says: the constant column / target in the lone set
        ju = old["ju"].cpu().numpy()
        assert ju[0, p // 2] == 0 and ju[-1].all() and ju.sum() == ju.size - 1
        assert float(old["ys"][0, 0]) == 1.0 and float(old["xs"][0, p // 2]) == 1.0
        assert torch.isnan(new["lams"]).all()
        for k in old:
            assert torch.equal(_bits(old[k]), _bits(new[k])), (k, c_f32)
        if p % 64:
            assert not new["C"][:, :, p:].any()          # the pad columns [p, ldc)


def test_prepare_fused_many_sets_and_segments(gpu):
    """More training sets than one LDS chunk of statistics (16) and more segments than the
    register path holds (8): the repeated cross-fit's shape."""
    p, ny, nseg = 70, 2, 10
    G, P, xcols, ycols = _design(p, ny, 5)
    G = np.concatenate([G, G[::-1] * 1.25])
    rs = np.random.RandomState(5)
    masks = (rs.rand(37, nseg) < 0.6).astype(np.uint8)
    masks[:, 0] = 1
    for c_f32 in (0, 1):
        old = _run("ate_enet_prepare", gpu, G, P, masks, xcols, ycols, c_f32)
        new = _run("ate_enet_prepare_fused", gpu, G, P, masks, xcols, ycols, c_f32)
        for k in old:
            assert torch.equal(_bits(old[k]), _bits(new[k])), (k, c_f32)
