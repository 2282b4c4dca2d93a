"""``ate_enet_cv_tail`` (csrc/enet.hip: one launch) against the chain it replaces
(``ate_enet_coef``, ``ate_enet_cvloss_gauss``, ``ate_cv_select``, ``ate_enet_pick``) on the
same device inputs, bit for bit: the full problems' coefficient rows, cvm, cvsd, the two
selected indices and the two picked rows (and the fold problems' raw losses). The chain's
kernels are pinned against their float64 twins in tests/test_gpu_enet_kernels.py.

The inputs are a path launch's outputs made by hand: sparse standardised paths whose rows at
and beyond nlam hold NaN (neither chain may read them), fold problems in shuffled order,
full problems that stopped early (nlam < L) and at once (nlam = 1)."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native

pytestmark = pytest.mark.gpu

_PROB_DT = np.dtype([("train", "<i4"), ("y", "<i4"), ("src", "<i4"), ("nlam", "<i4")])
NY = 2


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _case(gpu, L, p, K, nf, tie=False, poison=False):
    rs = np.random.RandomState(100000 + 1000 * L + 4 * p + 2 * K + nf)
    P = (p + NY + 1 + 63) // 64 * 64
    nseg, nt, nfp = K + 1, nf * (K + 1), nf * K
    nq = nf + nfp
    Z = rs.randn(nseg, 30, P)
    Z[:, :, 0] = 1.0
    G = np.einsum("sri,srj->sij", Z, Z)
    xcols = (1 + rs.permutation(p)).astype(np.int32)
    # full problem f: training set f (K + 1), target f % NY; its fold k: set f (K + 1) + 1 + k,
    # held-out segment k; the fold problems shuffled (the tables sort them by training set)
    nlam_full = [L, max(1, L - 3), 1][:nf]
    probs = [(f * (K + 1), f % NY, -1, L) for f in range(nf)]
    order = rs.permutation(nfp)
    fold_index = np.zeros((nf, K), dtype=np.int32)
    hold, ycol, nlam = [0] * nf, [0] * nf, list(nlam_full)
    for pos, i in enumerate(order):
        f, k = divmod(int(i), K)
        probs.append((f * (K + 1) + 1 + k, f % NY, f, 0))
        fold_index[f, k] = nf + pos
        hold.append(k)
        ycol.append(p + 1 + f % NY)
        nlam.append(nlam_full[f])
    apath = np.full((nq, L, p), np.nan)
    for q in range(nq):
        for m in range(nlam[q]):
            row = np.zeros(p)
            on = rs.rand(p) < min(1.0, (m // 2 if tie else m) / max(L - 1, 1) + 1.0 / p)
            row[on] = rs.randn(int(on.sum())) * 0.3
            apath[q, m] = row
    if tie:       # rows 2 i and 2 i + 1 of every problem equal: cvm ties in pairs, the minimum too
        for m in range(1, L, 2):
            keep = np.array(nlam) > m
            apath[keep, m] = apath[keep, m - 1]
    ju = (rs.rand(nt, p) < 0.9).astype(np.uint8)
    npass = np.full(nfp, 3, dtype=np.int32)
    if poison:
        npass[nfp // 2] = -1
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)   # noqa: E731
    t = dict(G=d(G), hold=d(np.array(hold, np.int32)), xc=d(xcols),
             ycol=d(np.array(ycol, np.int32)), apath=d(apath),
             probs=d(np.array(probs, dtype=_PROB_DT).view(np.uint8)),
             nlam=d(np.array(nlam, np.int32)), xm=d(rs.randn(nt, p)),
             xs=d(rs.uniform(0.5, 2.0, (nt, p))), ju=d(ju), ym=d(rs.randn(nt, NY)),
             ys=d(rs.uniform(0.5, 2.0, (nt, NY))), fidx=d(fold_index),
             nfold=d(rs.randint(20, 40, (nf, K)).astype(np.float64)), npass=d(npass))
    return dict(L=L, p=p, K=K, nf=nf, nfp=nfp, nq=nq, P=P, t=t)


def _outs(c, gpu, ncoef):
    f64 = dict(dtype=torch.float64, device=gpu)
    nf, L, p = c["nf"], c["L"], c["p"]
    return dict(coef=torch.full((ncoef, L, p + 1), 7.0, **f64),
                cvraw=torch.full((c["nq"], L), 7.0, **f64), cvm=torch.full((nf, L), 7.0, **f64),
                cvsd=torch.full((nf, L), 7.0, **f64),
                sel=torch.full((nf, 2), 7, dtype=torch.int32, device=gpu),
                cmin=torch.full((nf, p + 1), 7.0, **f64), c1se=torch.full((nf, p + 1), 7.0, **f64))


def _chain(c, gpu):
    t, o, s = c["t"], _outs(c, gpu, c["nq"]), _stream()
    L, p, nf, nfp, nq, K, P = (c[k] for k in ("L", "p", "nf", "nfp", "nq", "K", "P"))
    _native.call("ate_enet_coef", t["apath"].data_ptr(), t["probs"].data_ptr(), nq, p, NY, L,
                 t["nlam"].data_ptr(), t["xm"].data_ptr(), t["xs"].data_ptr(), t["ju"].data_ptr(),
                 t["ym"].data_ptr(), t["ys"].data_ptr(), o["coef"].data_ptr(), s)
    _native.call("ate_enet_cvloss_gauss", t["G"].data_ptr(), P, t["hold"].data_ptr(),
                 t["xc"].data_ptr(), p, 0, t["ycol"].data_ptr(), o["coef"].data_ptr(),
                 t["nlam"].data_ptr(), L, nf, nfp, o["cvraw"].data_ptr(), s)
    _native.call("ate_cv_select", o["cvraw"].data_ptr(), t["fidx"].data_ptr(),
                 t["nfold"].data_ptr(), K, nf, t["nlam"].data_ptr(), L, o["cvm"].data_ptr(),
                 o["cvsd"].data_ptr(), o["sel"].data_ptr(), t["npass"].data_ptr(), nfp, s)
    _native.call("ate_enet_pick", o["coef"].data_ptr(), o["sel"].data_ptr(), p, L, nf,
                 o["cmin"].data_ptr(), o["c1se"].data_ptr(), t["npass"].data_ptr(), nfp, s)
    o["coef"] = o["coef"][:nf]
    o["cvraw"] = o["cvraw"][nf:]
    return o


def _tail(c, gpu):
    t, o, s = c["t"], _outs(c, gpu, c["nf"]), _stream()
    L, p, nf, nfp, K, P = (c[k] for k in ("L", "p", "nf", "nfp", "K", "P"))
    done = torch.zeros(nf, dtype=torch.int32, device=gpu)
    _native.call("ate_enet_cv_tail", t["G"].data_ptr(), P, t["hold"].data_ptr(),
                 t["xc"].data_ptr(), p, 0, t["ycol"].data_ptr(), t["apath"].data_ptr(),
                 t["probs"].data_ptr(), NY, t["nlam"].data_ptr(), t["xm"].data_ptr(),
                 t["xs"].data_ptr(), t["ju"].data_ptr(), t["ym"].data_ptr(), t["ys"].data_ptr(),
                 L, nf, nfp, K, t["fidx"].data_ptr(), t["nfold"].data_ptr(), o["coef"].data_ptr(),
                 o["cvraw"].data_ptr(), o["cvm"].data_ptr(), o["cvsd"].data_ptr(),
                 o["sel"].data_ptr(), o["cmin"].data_ptr(), o["c1se"].data_ptr(),
                 t["npass"].data_ptr(), done.data_ptr(), s)
    o["cvraw"] = o["cvraw"][c["nf"]:]
    o["done"] = done
    return o


def _same(old, new, c):
    for k in old:
        assert torch.equal(_bits(old[k]), _bits(new[k])), k
    want = c["L"] + c["K"] * ((c["L"] + 7) // 8)
    assert new["done"].tolist() == [want] * c["nf"]


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("p", [1, 64, 65, 500])
@pytest.mark.parametrize("L", [5, 8, 9, 100])
def test_cv_tail_equals_chain(gpu, L, p, K, nf):
    c = _case(gpu, L, p, K, nf)
    old, new = _chain(c, gpu), _tail(c, gpu)
    torch.cuda.synchronize()
    _same(old, new, c)
    nl = c["t"]["nlam"][:nf].cpu().numpy()
    assert not torch.isnan(old["cvm"][0, :nl[0]]).any()
    for f in range(nf):                       # NaN beyond each path's end, in both
        assert torch.isnan(new["cvm"][f, nl[f]:]).all() and \
            torch.isnan(new["coef"][f, nl[f]:]).all()


@pytest.mark.parametrize("L,p,K,nf", [(9, 65, 2, 3), (100, 500, 4, 1)])
def test_cv_tail_truncated_fold_poisons(gpu, L, p, K, nf):
    """npass = -1 on one fold: cvm, cvsd and both picked rows NaN, sel 0, as in the chain."""
    c = _case(gpu, L, p, K, nf, poison=True)
    old, new = _chain(c, gpu), _tail(c, gpu)
    torch.cuda.synchronize()
    _same(old, new, c)
    for k in ("cvm", "cvsd", "cmin", "c1se"):
        assert torch.isnan(new[k]).all(), k
    assert not new["sel"].any()


@pytest.mark.parametrize("L,p,K,nf", [(8, 64, 4, 3), (100, 65, 2, 1)])
def test_cv_tail_tie_at_the_minimum(gpu, L, p, K, nf):
    """Equal rows in pairs: cvm ties at its minimum and the FIRST index must win."""
    c = _case(gpu, L, p, K, nf, tie=True)
    old, new = _chain(c, gpu), _tail(c, gpu)
    torch.cuda.synchronize()
    _same(old, new, c)
    cvm, i0 = new["cvm"][0].cpu().numpy(), int(new["sel"][0, 0])
    assert i0 % 2 == 0 and cvm[i0] == cvm[i0 + 1] == np.nanmin(cvm)


def test_cv_tail_graph_replay(gpu):
    """The call (its zeroed arrival counters included) captured once and replayed three
    times: three identical results, equal to the chain's."""
    c = _case(gpu, 9, 65, 4, 3)
    old = _chain(c, gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _tail(c, gpu)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        new = _tail(c, gpu)
    for _ in range(3):
        for k, v in new.items():
            if k != "done":
                v.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        _same(old, new, c)
