"""The CV elastic-net stack (csrc/enet.hip: K08, K09) at its edge shapes.

Part 1 calls the five kernels around the path directly (``ate_enet_prepare``,
``ate_enet_coef``, ``ate_enet_cvloss_gauss``, ``ate_cv_select``, ``ate_enet_pick``) on small
float64 inputs built in numpy and compares them with an ``np.longdouble`` evaluation of the
same expression from the same inputs. Every bound is the forward-error bound of the kernel's
own float64 expression, ``c * 2^-53 * (sum of the absolute values of the terms)`` with c the
number of roundings a term passes through (plus one for the second-order terms), divided by
the denominators the kernel divides by; nothing is fitted to what the kernel returns. The
selection kernel runs in exact arithmetic and must equal ``reference.glmnet.cv_select`` bit
for bit. Each test prints worst observed / bound.

Part 2 runs ``cv_enet_gaussian`` on the device against the same call on the CPU at the shapes
where the path kernel takes another route: one 64-wide block, a last block of one coordinate,
PMAX, every lambda hand-off route between a full problem and its folds, constant columns,
an exhausted pass budget, n < p and two targets in one launch."""
import types

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.ops.enet import cv_enet_gaussian
from ate_replication_causalml_amd.reference import glmnet as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
_PROB_DT = np.dtype([("train", "<i4"), ("y", "<i4"), ("src", "<i4"), ("nlam", "<i4")])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _d(a, gpu, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).to(gpu)


def _probs(rows, gpu):
    b = np.array(rows, dtype=_PROB_DT)
    return torch.from_numpy(b.view(np.uint8).copy()).to(gpu)


def _status(name, *args):
    with pytest.raises(_native.NativeError) as e:
        _native.call(name, *args)
    return e.value.status


def _worst(err, bound):
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    assert np.all(bound > 0)
    return float(np.max(err / bound)) if err.size else 0.0


# ------------------------------------------------------------------ ate_enet_prepare
# training sets over nseg = 3: all, the three one-out sets, and segment 2 alone
_MASKS = np.array([[1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0], [0, 0, 1]], dtype=np.uint8)
_LONE = 4          # the set in which two x columns and y column 0 are constant
_SIZES = (70, 85, 96)


def _prep_design(p, ny):
    """Z [n, P] with P = 2p + 2ny + 4 > p + ny + 1: the ones column is panel column 1, the x
    columns a permutation of the even panel columns 2..2p (no two adjacent), the y columns
    odd ones in descending order. In segment 2 the x columns p // 3 and p - 1 and y column 0
    are constant (0.75, 1.25 and 3: sums of them and of their squares are exact, so their
    variance there is exactly zero, while their products with another column round)."""
    rs = np.random.RandomState(1000 + 10 * p + ny)
    n, P = sum(_SIZES), 2 * p + 2 * ny + 4
    Z = rs.randn(n, P) * rs.uniform(0.5, 2.0, P) + rs.uniform(-1.0, 1.0, P)
    one = 1
    Z[:, one] = 1.0
    xcols = rs.permutation(2 * np.arange(p) + 2).astype(np.int32)
    ycols = np.array([2 * p + 5, 2 * p + 3][2 - ny:], dtype=np.int32)
    assert max(xcols.max(), ycols.max()) < P and np.all(np.diff(np.sort(xcols)) >= 2)
    const = sorted({p // 3, p - 1})
    r0 = _SIZES[0] + _SIZES[1]
    for v, j in enumerate(const):
        Z[r0:, xcols[j]] = 0.75 + 0.5 * v
    Z[r0:, ycols[0]] = 3.0
    b = np.cumsum((0,) + _SIZES)
    G = np.stack([Z[b[k]:b[k + 1]].T @ Z[b[k]:b[k + 1]] for k in range(3)])
    return G, one, xcols, ycols, const


def _prep_reference(G, one, xcols, ycols, const):
    """Longdouble statistics of every training set from the float64 G, with the bound of
    each: ns - 1 additions and a division per masked mean (ns roundings); a variance or a
    centred cross product S/n - m m' has ns roundings on S/n, 2 ns + 1 on the product and
    one on the difference, so 2 ns + 3 covers both terms with the second order; sqrt adds
    one, and a standardised entry two more for its denominator's product and the division."""
    Gl, Al = G.astype(LD), np.abs(G).astype(LD)
    out = []
    for s, mk in enumerate(_MASKS):
        ns = int(mk.sum())
        Gt, At = np.tensordot(mk.astype(LD), Gl, 1), np.tensordot(mk.astype(LD), Al, 1)
        n = Gt[one, one]
        cols = np.r_[xcols, ycols]
        m, M = Gt[one, cols] / n, At[one, cols] / n
        v = np.diag(Gt)[cols] / n - m * m
        e_v = (2 * ns + 3) * U * (np.diag(At)[cols] / n + M * M)
        dead = np.zeros(len(cols), bool)
        if s == _LONE:
            dead[const] = True
            dead[len(xcols)] = True
        assert np.all(v[dead] == 0) and np.all(v[~dead] > 1e-2)
        sd = np.where(dead, LD(1), np.sqrt(np.where(dead, LD(1), v)))
        r_sd = np.where(dead, LD(0), e_v / (2 * (np.where(dead, LD(1), v) - e_v)) + U)
        N = Gt[np.ix_(cols, cols)] / n - np.outer(m, m)
        e_N = (2 * ns + 3) * U * (At[np.ix_(cols, cols)] / n + np.outer(M, M))
        den = np.outer(sd, sd)
        S = N / den
        e_S = e_N / den + np.abs(S) * (r_sd[:, None] + r_sd[None, :] + 2 * U)
        out.append(dict(n=n, m=m, e_m=ns * U * M, sd=sd, e_sd=sd * r_sd, dead=dead, S=S, e_S=e_S))
    return out


@pytest.mark.parametrize("ny", [1, 2])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 130])
def test_prepare_kernels(gpu, p, ny):
    """enet_prep_stats_kernel + enet_prepare_kernel<double / float>: masked segment sums
    through xcols / ycols indirection into a larger panel, the (p + 63) / 64 * 64 row stride
    of C, and columns that are constant in one training set only."""
    G, one, xcols, ycols, const = _prep_design(p, ny)
    refs = _prep_reference(G, one, xcols, ycols, const)
    nt, ldc = len(_MASKS), (p + 63) // 64 * 64
    Gd, mk, xc, yc = _d(G, gpu), _d(_MASKS, gpu), _d(xcols, gpu), _d(ycols, gpu)
    worst = {}
    for c_f32 in (0, 1):
        f64 = dict(dtype=torch.float64, device=gpu)
        C = torch.zeros((nt, p, ldc), dtype=torch.float32 if c_f32 else torch.float64, device=gpu)
        g = torch.full((nt, ny, p), 7.0, **f64)
        xm, xs = torch.full((nt, p), 7.0, **f64), torch.full((nt, p), 7.0, **f64)
        ju = torch.full((nt, p), 9, dtype=torch.uint8, device=gpu)
        ym, ys = torch.full((nt, ny), 7.0, **f64), torch.full((nt, ny), 7.0, **f64)
        nobs = torch.full((nt,), 7.0, **f64)
        _native.call("ate_enet_prepare", Gd.data_ptr(), 3, G.shape[1], mk.data_ptr(), nt,
                     xc.data_ptr(), p, one, yc.data_ptr(), ny, C.data_ptr(), c_f32, g.data_ptr(),
                     xm.data_ptr(), xs.data_ptr(), ju.data_ptr(), ym.data_ptr(), ys.data_ptr(),
                     nobs.data_ptr(), _stream())
        C, g, xm, xs, ju, ym, ys, nobs = (t.cpu().numpy() for t in (C, g, xm, xs, ju, ym, ys, nobs))
        assert np.all(C[:, :, p:] == 0)                       # the padding stays zero
        for s, r in enumerate(refs):
            dx, dy = r["dead"][:p], r["dead"][p:]
            assert nobs[s] == float(r["n"])
            assert np.array_equal(ju[s], (~dx).astype(np.uint8))
            assert np.all(xs[s][dx] == 1.0) and np.all(ys[s][dy] == 1.0)
            assert np.all(g[s][:, dx] == 0.0)
            eye = np.eye(p)
            assert np.array_equal(C[s][dx, :p], eye[dx]) and np.array_equal(C[s][:, :p][:, dx].T, eye[dx])
            mean = np.r_[xm[s], ym[s]]
            sd = np.r_[xs[s], ys[s]]
            live = ~r["dead"]
            err = dict(mean=(np.abs(mean - r["m"]), r["e_m"]),
                       sd=(np.abs(sd - r["sd"])[live], r["e_sd"][live]))
            lx = np.flatnonzero(~dx)
            Cref, eC = r["S"][np.ix_(lx, lx)], r["e_S"][np.ix_(lx, lx)]
            Cobs = C[s][np.ix_(lx, lx)]
            if c_f32:
                # the longdouble value rounded to float32; half a float32 ulp on the bound
                Cref = Cref.astype(np.float32)
                eC = eC + np.spacing(np.abs(Cref)).astype(LD) / 2
                assert Cobs.dtype == np.float32
            err["C_f32" if c_f32 else "C"] = (np.abs(Cobs.astype(LD) - Cref.astype(LD)), eC)
            gref, eg = r["S"][np.ix_(lx, p + np.arange(ny))].T, r["e_S"][np.ix_(lx, p + np.arange(ny))].T
            err["g"] = (np.abs(g[s][:, lx] - gref), eg)
            for k, (e, b) in err.items():
                if e.size:
                    worst[k] = max(worst.get(k, 0.0), _worst(e, b))
    print("prepare p=%d ny=%d: " % (p, ny) + " ".join("%s %.3g" % kv for kv in sorted(worst.items()))
          + " [observed / bound]")
    assert all(w <= 1.0 for w in worst.values()), worst


# ------------------------------------------------------------------ ate_enet_coef
@pytest.mark.parametrize("p", [1, 129])
def test_coef_kernel(gpu, p):
    """enet_coef_kernel: beta_j = a_j ys / xs_j (two roundings; bound 3 u |beta_j|), exactly 0
    where ju = 0 whatever apath holds, the intercept ym - sum beta_j xm_j (ceil(p / 128) fmas
    per thread, 6 + 2 additions of the block sum, the two roundings of beta_j and the final
    difference: c = ceil(p / 128) + 12), and all-NaN rows from nlam on; p = 129 takes the
    second trip of the 128-thread loop."""
    rs = np.random.RandomState(50 + p)
    L, nt, ny = 5, 3, 2
    rows = [(0, 0, -1, L), (2, 1, -1, L), (1, 1, 0, 0), (2, 0, 1, 0), (1, 0, 0, 0)]
    nlam = np.array([5, 3, 0, 1, 4], dtype=np.int32)
    nq = len(rows)
    apath = rs.randn(nq, L, p) + np.sign(rs.randn(nq, L, p))      # no zero anywhere
    xm, xs = rs.randn(nt, p), rs.uniform(0.3, 3.0, (nt, p))
    ju = (rs.rand(nt, p) < 0.7).astype(np.uint8)
    ju[0, 0], ju[1, p - 1], ju[2, p // 2] = 1, 0, 0
    ym, ys = rs.randn(nt, ny), rs.uniform(0.5, 4.0, (nt, ny))
    coef = torch.full((nq, L, p + 1), 777.0, dtype=torch.float64, device=gpu)
    dev = [_d(a, gpu) for a in (apath, nlam, xm, xs, ju, ym, ys)]
    pr = _probs(rows, gpu)
    _native.call("ate_enet_coef", dev[0].data_ptr(), pr.data_ptr(), nq, p, ny, L,
                 dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(),
                 dev[5].data_ptr(), dev[6].data_ptr(), coef.data_ptr(), _stream())
    coef = coef.cpu().numpy()
    c0 = -(-p // 128) + 12
    w_b = w_0 = 0.0
    for q, (t, y, _, _) in enumerate(rows):
        assert np.isnan(coef[q, nlam[q]:]).all()
        live = ju[t] != 0
        for m in range(nlam[q]):
            b = np.where(live, apath[q, m].astype(LD) * LD(ys[t, y]) / xs[t].astype(LD), LD(0))
            a0 = LD(ym[t, y]) - np.sum(b * xm[t].astype(LD))
            assert np.all(coef[q, m, 1:][~live] == 0.0)
            if live.any():
                w_b = max(w_b, _worst(np.abs(coef[q, m, 1:] - b)[live], 3 * U * np.abs(b)[live]))
            w_0 = max(w_0, _worst(abs(coef[q, m, 0] - a0),
                                  c0 * U * (abs(LD(ym[t, y])) + np.sum(np.abs(b * xm[t])))))
    print("coef p=%d: slopes %.3g intercept %.3g [observed / bound]" % (p, w_b, w_0))
    assert w_b <= 1.0 and w_0 <= 1.0


# ------------------------------------------------------------------ ate_enet_cvloss_gauss
_CVG = {}


def _cvloss_gram(p):
    """Three small held-out Grams over P = p + 8 panel columns; the x columns are a
    permutation of a subset, the ones column and the two y columns sit between them."""
    if p not in _CVG:
        rs = np.random.RandomState(300 + p)
        P = p + 8
        Z = rs.randn(76, P)
        one, ycols = 3, (P - 1, 5)
        Z[:, one] = 1.0
        rest = np.setdiff1d(np.arange(P), [one, *ycols])
        xcols = rs.permutation(rest)[:p].astype(np.int32)
        b = (0, 20, 45, 76)
        G = np.stack([Z[b[k]:b[k + 1]].T @ Z[b[k]:b[k + 1]] for k in range(3)])
        _CVG[p] = (G, one, ycols, xcols)
    return _CVG[p]


def _cvloss_coef(rs, nq, L, p, nlam):
    """Hand-made coefficient rows. The kernel skips the rows of the held-out Gram outside
    every support of a chunk of 8 lambdas, so the support is set per chunk, cycling through:
    dense; empty (intercept only); only rows a = 3 (mod 4) (one wave of the kernel does all
    the work); only the last coordinate; only rows a = 4..7 (mod 8) (every wave alternates
    between a skipped and a kept row). Odd lambdas keep a random half of their chunk's
    support. Rows from nlam on are NaN, as enet_coef_kernel leaves them."""
    coef = rs.randn(nq, L, p + 1)
    a = np.arange(p)
    for q in range(nq):
        for m in range(L):
            kind = (q + 1 + m // 8) % 5
            keep = [np.ones(p, bool), np.zeros(p, bool), a % 4 == 3, a == p - 1, a % 8 >= 4][kind]
            if m % 2:
                keep = keep & (rs.rand(p) < 0.5)
            coef[q, m, 1:][~keep] = 0.0
        coef[q, nlam[q]:] = np.nan
    return coef


@pytest.mark.parametrize("L", [5, 9, 100])
@pytest.mark.parametrize("p", [1, 64, 65, 449, 512])
def test_cvloss_kernel(gpu, p, L):
    """enet_cvloss_gauss_kernel against the held-out SSE formula of the CPU twin in
    longdouble. L = 5: one partly filled chunk of 8 lambdas; 9: a chunk holding one lambda;
    100: 13 chunks, dispatched densest first. A term of the quadratic form passes through 8
    fmas over the lane's columns, at most ceil(p / 4) over the wave's rows, 6 + 3 additions of
    the reduction, 5 of the SSE and the division: c = ceil(p / 4) + 26 on the absolute terms."""
    G, one, ycols, xcols = _cvloss_gram(p)
    rs = np.random.RandomState(7 * p + L)
    q0 = 2
    hold = np.array([0, 0, 2, 0, 1, 1], dtype=np.int32)
    ycol = np.array([ycols[0]] * 2 + [ycols[0], ycols[1], ycols[1], ycols[0]], dtype=np.int32)
    nlam = np.array([L, L, max(1, 3 * L // 7), 0, L, max(1, L - 3)], dtype=np.int32)
    assert nlam[2] % 8 and nlam[5] % 8                       # both end inside a chunk
    nq = len(hold)
    coef = _cvloss_coef(rs, nq, L, p, nlam)
    cvraw = torch.full((nq, L), -7.0, dtype=torch.float64, device=gpu)
    dev = [_d(a, gpu) for a in (G, hold, xcols, ycol, coef, nlam)]
    _native.call("ate_enet_cvloss_gauss", dev[0].data_ptr(), G.shape[1], dev[1].data_ptr(),
                 dev[2].data_ptr(), p, one, dev[3].data_ptr(), dev[4].data_ptr(),
                 dev[5].data_ptr(), L, q0, nq - q0, cvraw.data_ptr(), _stream())
    cvraw = cvraw.cpu().numpy()
    assert np.all(cvraw[:q0] == -7.0)                         # the full problems are not scored
    c = -(-p // 4) + 26
    worst = 0.0
    for q in range(q0, nq):
        assert np.isnan(cvraw[q, nlam[q]:]).all()
        Gh = G[hold[q]].astype(LD)
        n, yy, sy = Gh[one, one], Gh[ycol[q], ycol[q]], Gh[one, ycol[q]]
        Gxy, Sx = Gh[xcols, ycol[q]], Gh[xcols, one]
        for m in range(nlam[q]):
            a0, b = LD(coef[q, m, 0]), coef[q, m, 1:].astype(LD)
            sup = np.flatnonzero(b)
            bs, Gs = b[sup], Gh[np.ix_(xcols[sup], xcols[sup])]
            terms = [yy, -2 * a0 * sy, -2 * (bs * Gxy[sup]), n * a0 * a0, 2 * a0 * (bs * Sx[sup]),
                     np.outer(bs, bs) * Gs]
            sse = sum(np.sum(t) for t in terms)
            mag = sum(np.sum(np.abs(t)) for t in terms)
            worst = max(worst, _worst(abs(cvraw[q, m] - sse / n), c * U * mag / n))
    print("cvloss p=%d L=%d: %.3g [observed / bound]" % (p, L, worst))
    assert worst <= 1.0


def test_cvloss_refuses_more_than_pmax(gpu):
    G, one, ycols, xcols = _cvloss_gram(512)
    z = torch.zeros(8, dtype=torch.float64, device=gpu)
    assert _status("ate_enet_cvloss_gauss", z.data_ptr(), G.shape[1], z.data_ptr(), z.data_ptr(),
                   513, one, z.data_ptr(), z.data_ptr(), z.data_ptr(), 5, 0, 1, z.data_ptr(),
                   _stream()) == -1


# ------------------------------------------------------------------ ate_cv_select
# Exact arithmetic: fold k of a lambda holds mu + a_k delta with sum_k w_k a_k = 0, so the
# weighted mean is mu and the weighted variance / (K - 1) is (sd delta)^2 -- integers and
# halves throughout, whatever the order of the operations.
_W = {2: np.array([1.0, 9.0]), 3: np.array([1.0, 2.0, 5.0])}
_A = {2: np.array([9.0, -1.0]), 3: np.array([-3.0, -1.0, 1.0])}
_SD = {2: 3.0, 3: 1.0}
_TIES = {7: (2, 5), 64: (3, 35), 65: (3, 64), 200: (3, 67, 130), 256: (3, 67, 130)}


def _select_problems(K, L):
    """(nlam, mu, delta, expected sel or None) per full problem of one launch."""
    rs = np.random.RandomState(10 * L + K)
    out = []
    for nl in sorted({1, 63, 64, 65, L}):
        if nl <= L:
            # random integer curves over a narrow range: ties wherever they fall
            out.append((nl, rs.randint(100, 112, L).astype(float), rs.randint(0, 5, L) / 2.0, None))
    if L in _TIES:
        ties = _TIES[L]
        mu, dl = np.full(L, 100.0), np.zeros(L)
        mu[list(ties)] = 50.0
        dl[ties[0]] = 1.0
        # minima tied in different lanes / 64-chunks: the first wins
        out.append((L, mu.copy(), dl.copy(), (ties[0], ties[0])))
        if L >= 65:
            # a strictly smaller value late in another chunk, whose mean + sd is exactly the
            # tied value: lambda.1se is the first tie, in an earlier chunk than lambda.min
            late = L - 10 if L > 65 else 64
            mu[late], dl[late] = 50.0 - _SD[K], 1.0
            if late & 63:
                dl[late & ~63] = 4.0         # lane 0 of that chunk has another sd
            out.append((L, mu, dl, (late, ties[0])))
    return out


def _launch_select(gpu, K, L, probs, fnp=None):
    rs = np.random.RandomState(L + K)
    nf = len(probs)
    nrows = nf * K + 2
    perm = rs.permutation(nrows)
    fidx = perm[:nf * K].reshape(nf, K).astype(np.int32)
    cvraw = np.full((nrows, L), -1e6)                     # nothing from nlam on may be read
    nfold = np.stack([_W[K] * (1 + f % 3) for f in range(nf)])
    for f, (nl, mu, dl, _) in enumerate(probs):
        cvraw[fidx[f], :nl] = (mu[None, :] + _A[K][:, None] * dl[None, :])[:, :nl]
    nlam = np.array([pb[0] for pb in probs], dtype=np.int32)
    cvm = torch.full((nf, L), 12345.0, dtype=torch.float64, device=gpu)
    cvsd = torch.full((nf, L), 12345.0, dtype=torch.float64, device=gpu)
    sel = torch.full((nf, 2), -9, dtype=torch.int32, device=gpu)
    dev = [_d(a, gpu) for a in (cvraw, fidx, nfold, nlam)]
    fn = None if fnp is None else _d(np.asarray(fnp, dtype=np.int32), gpu)
    _native.call("ate_cv_select", dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), K, nf,
                 dev[3].data_ptr(), L, cvm.data_ptr(), cvsd.data_ptr(), sel.data_ptr(),
                 None if fn is None else fn.data_ptr(), 0 if fn is None else len(fnp), _stream())
    return cvraw, fidx, nfold, cvm.cpu().numpy(), cvsd.cpu().numpy(), sel.cpu().numpy()


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("L", [1, 7, 64, 65, 200, 256])
def test_cv_select_exact(gpu, K, L):
    """cv_select_kernel must equal reference.glmnet.cv_select bit for bit on inputs whose
    means and variances are exact: nlam in {1, 63, 64, 65, L}, unequal fold weights, the
    tie rules across lanes and across the four 64-lambda chunks, the 1-se threshold of the
    owning lane, and NaN on [nlam, L) of outputs prefilled with a finite sentinel."""
    probs = _select_problems(K, L)
    cvraw, fidx, nfold, cvm, cvsd, sel = _launch_select(gpu, K, L, probs)
    for f, (nl, mu, dl, want) in enumerate(probs):
        raw = cvraw[fidx[f], :nl]
        cm, cs, i0, i1 = ref.cv_select(None, raw, nfold[f])
        # float64 numpy and longdouble agree bit for bit: the inputs are exact
        cml, csl, _, _ = ref.cv_select(None, raw.astype(LD), nfold[f].astype(LD))
        assert cml.dtype == LD and np.array_equal(cm.astype(LD), cml) and np.array_equal(cs.astype(LD), csl)
        assert np.array_equal(cm, mu[:nl]) and np.array_equal(cs, _SD[K] * dl[:nl])
        if want is not None:
            assert (i0, i1) == want
            if want[0] != want[1]:
                assert cm[i1] == cm[i0] + cs[i0] and i1 < i0 and (i1 >> 6) < (i0 >> 6)
        assert np.array_equal(cvm[f, :nl], cm) and np.array_equal(cvsd[f, :nl], cs), f
        assert np.isnan(cvm[f, nl:]).all() and np.isnan(cvsd[f, nl:]).all(), f
        assert tuple(sel[f]) == (i0, i1), (f, tuple(sel[f]), (i0, i1))


def test_cv_select_truncated_fold_and_limit(gpu):
    """A negative entry in fold_npass NaN-poisons every output and selects (0, 0); L = 257 is
    one more than the kernel's four lambdas per lane and is refused without a launch."""
    probs = _select_problems(3, 200)
    _, _, _, cvm, cvsd, sel = _launch_select(gpu, 3, 200, probs, fnp=[3, -1, 2])
    assert np.isnan(cvm).all() and np.isnan(cvsd).all() and np.all(sel == 0)
    _, _, _, cvm, _, sel = _launch_select(gpu, 3, 200, probs, fnp=[3, 1, 2])
    assert np.isfinite(cvm[-1]).all() and tuple(sel[-1]) == probs[-1][3]
    z = torch.zeros(8, dtype=torch.float64, device=gpu)
    assert _status("ate_cv_select", z.data_ptr(), z.data_ptr(), z.data_ptr(), 2, 1, z.data_ptr(),
                   257, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 0, _stream()) == -1


# ------------------------------------------------------------------ ate_enet_pick
def test_pick_kernel(gpu):
    """enet_pick_kernel: rows coef[f, sel[f, which]] bit for bit (p = 129: the second trip of
    the 128-thread loop writes the last two entries), NaN under a truncated fold."""
    rs = np.random.RandomState(3)
    p, L, nf, nq = 129, 7, 3, 5
    coef = rs.randn(nq, L, p + 1)
    sel = np.array([[0, 6], [3, 3], [6, 2]], dtype=np.int32)
    cd, sd = _d(coef, gpu), _d(sel, gpu)
    for fnp in (None, [2, 5], [2, -1]):
        omin = torch.full((nf, p + 1), 5.0, dtype=torch.float64, device=gpu)
        o1se = torch.full((nf, p + 1), 5.0, dtype=torch.float64, device=gpu)
        fn = None if fnp is None else _d(np.asarray(fnp, dtype=np.int32), gpu)
        _native.call("ate_enet_pick", cd.data_ptr(), sd.data_ptr(), p, L, nf, omin.data_ptr(),
                     o1se.data_ptr(), None if fn is None else fn.data_ptr(),
                     0 if fn is None else len(fnp), _stream())
        omin, o1se = omin.cpu().numpy(), o1se.cpu().numpy()
        if fnp is not None and min(fnp) < 0:
            assert np.isnan(omin).all() and np.isnan(o1se).all()
        else:
            assert np.array_equal(omin, coef[np.arange(nf), sel[:, 0]])
            assert np.array_equal(o1se, coef[np.arange(nf), sel[:, 1]])


# ------------------------------------------------------------------ path edge shapes
NESTED = [[1, 2], [0, 2], [0, 1]]


def _path_case(p, sizes, seed, signals, sd=1.0, ny=1, const=(), **kw):
    """Gram stack G[k] = Z_k' Z_k in float64 of Z = [1, X, Y] and the call's arguments."""
    rs = np.random.RandomState(seed)
    n = sum(sizes)
    X = rs.randn(n, p)
    X[:, list(const)] = 1.0
    Y = np.empty((n, ny))
    for t in range(ny):
        beta = np.zeros(p)
        free = np.setdiff1d(np.arange(p), const)
        beta[free[:signals]] = rs.choice([-1.0, 1.0], min(signals, len(free))) * \
            rs.uniform(0.2, 1.0, min(signals, len(free)))
        Y[:, t] = X @ np.roll(beta, 3 * t) + sd * rs.randn(n)
    Z = np.column_stack([np.ones(n), X, Y])
    b = np.cumsum((0,) + tuple(sizes))
    G = np.stack([Z[b[k]:b[k + 1]].T @ Z[b[k]:b[k + 1]] for k in range(len(sizes))])
    return dict(G=torch.from_numpy(G), sizes=np.array(sizes), p=p, ny=ny, kw=kw)


# name -> (case builder, properties asserted on the CPU twin)
_CASES = {
    # one 64-wide block: the "last visit prefetches block 0" rule has no other block
    "T1_p1": lambda: _path_case(1, (70, 60, 70), 21, 1),
    "T1_p63": lambda: _path_case(63, (100, 90, 110), 22, 3),
    "T1_p64": lambda: _path_case(64, (130, 140, 130), 23, 3),
    # a last block holding one coordinate, and that one dead
    "const_p65": lambda: _path_case(65, (130, 140, 130), 24, 3, const=(0, 64)),
    # full blocks (cw = 64 fills the LDS union); 40 lambdas and a noise sd of 0.1 keep the CPU
    # twin at 1-3 s, and the lasso paths still end with over 400 coordinates in the model
    "pmax_lasso": lambda: _path_case(512, (500, 480, 520), 25, 6, sd=0.1, nlambda=40),
    "pmax_enet": lambda: _path_case(512, (500, 480, 520), 26, 100, sd=0.1, alpha=0.5, nlambda=40),
    "p449": lambda: _path_case(449, (500, 480, 520), 27, 5, sd=0.1, nlambda=40),
    # lambda hand-off routes between a full problem and its folds
    "L2": lambda: _path_case(70, (100, 90, 110), 28, 4, nlambda=2),
    "L7": lambda: _path_case(70, (100, 90, 110), 28, 4, nlambda=7),
    "L200": lambda: _path_case(70, (100, 90, 110), 28, 4, nlambda=200),
    "L256": lambda: _path_case(70, (100, 90, 110), 28, 4, nlambda=256),
    # folds run ahead of a source that stops early, and must put back what they computed
    "early_stop_nested": lambda: _path_case(70, (100, 90, 110), 29, 4, sd=0.01, full_sets=NESTED),
    "pass_budget": lambda: _path_case(70, (100, 90, 110), 30, 20, maxit=40),
    "n_lt_p": lambda: _path_case(130, (20, 20, 20), 31, 5),
    "two_targets": lambda: _path_case(70, (300, 280, 320), 32, 4, ny=2, full_sets=NESTED,
                                      full_y=[0, 1, 0],
                                      penalty_factor=np.r_[0.0, np.ones(68), 0.0]),
}
_BUILT, _TWIN, _TWIN_DIAG32 = {}, {}, {}
# The fp64 kernel keeps the 64 x 64 diagonal block of the block it walks in LDS as float32
# (csrc/enet.hip: "tn's diagonal block -> LDS (fp32)"), so the gradient of a coordinate takes
# the moves of its own block's coordinates through float32 entries of C. With two unpenalised
# coordinates one of them shares a block with the coordinate that sets lambda_max, whose
# gradient, and with it the whole lambda sequence, then sits 6.9e-10 (relative) off the
# float64 twin's: more than the 1e-12 of the fp64 tolerances, which every other case meets.
# That case is compared with the twin run on C with its diagonal blocks rounded to float32,
# at the same fp64 tolerances: this separates the rounding of C from the kernel.
_DIAG32_CASES = {"two_targets"}


def _panel(case, dtype):
    return types.SimpleNamespace(seg_nreal=case["sizes"], cols={"one": 0}, dtype=dtype)


def _call(case, G, dtype):
    p, ny = case["p"], case["ny"]
    return cv_enet_gaussian(G, _panel(case, dtype), list(range(1, p + 1)),
                            list(range(p + 1, p + 1 + ny)), **case["kw"])


def _case(name):
    """The case and its CPU twin, computed once and shared by both kernels' tests."""
    if name not in _BUILT:
        _BUILT[name] = _CASES[name]()
        _TWIN[name] = _call(_BUILT[name], _BUILT[name]["G"], torch.float64)
    return _BUILT[name], _TWIN[name]


def _twin_diag32(name):
    """The CPU twin on C with each 64 x 64 diagonal block rounded to float32."""
    if name not in _TWIN_DIAG32:
        case, _ = _case(name)
        core = ref._elnet_core

        def rounded(C, *a, **k):
            C = C.copy()
            for b in range(0, len(C), 64):
                C[b:b + 64, b:b + 64] = C[b:b + 64, b:b + 64].astype(np.float32)
            return core(C, *a, **k)

        ref._elnet_core = rounded
        try:
            _TWIN_DIAG32[name] = _call(case, case["G"], torch.float64)
        finally:
            ref._elnet_core = core
    return _TWIN_DIAG32[name]


def _leaves_mode_s(rc):
    """Whether the fp32 kernel leaves its small-active-set mode on this path, read off the
    twin: more than ENET_S_ENTER = 40 coordinates ever moved, or more than ENET_S_FETCH = 8
    new ones within one lambda (csrc/enet.hip)."""
    for f in range(rc.nlam.shape[0]):
        nz = rc.coef_path[f, :int(rc.nlam[f]), 1:].numpy() != 0
        ever = np.maximum.accumulate(nz, axis=0).sum(1)
        if ever[-1] > 40 or np.diff(np.r_[0, ever]).max() > 8:
            return True
    return False


def _np(t):
    return t.detach().cpu().numpy()


def _compare(name, rg, rc, dtype, as_f32=False):
    """The project's tolerances: test_gpu.py::test_enet_cv_kernels_vs_cpu for the fp64
    kernel, test_gpu_enet_modes.py for the fp32 one (atol 5e-5 where the path leaves mode S);
    beyond nlam every per-lambda output is NaN on the device as on the CPU. ``as_f32``:
    the fp64 kernel at the fp32 kernel's tolerances (against a twin that does not round C)."""
    f32 = as_f32 or dtype == torch.float32
    rg.check()
    L = rc.lambdas.shape[1]
    atol32 = 5e-5 if f32 and _leaves_mode_s(rc) else 2e-5
    dev = {}
    for f in range(rc.nlam.shape[0]):
        ng, nc = int(rg.nlam[f]), int(rc.nlam[f])
        assert abs(ng - nc) <= (1 if f32 else 0), (f, ng, nc)
        for r, n_ in ((rg, ng), (rc, nc)):
            for fld in ("lambdas", "cvm", "cvsd"):
                a = _np(getattr(r, fld))[f]
                assert np.isnan(a[n_:]).all() and np.isfinite(a[:n_]).all(), (fld, f)
            cp = _np(r.coef_path)[f]
            assert np.isnan(cp[n_:]).all() and np.isfinite(cp[:n_]).all(), f
        nl = min(ng, nc)
        lg, lc = _np(rg.lambdas)[f, :nl], _np(rc.lambdas)[f, :nl]
        cg, cc = _np(rg.coef_path)[f, :nl], _np(rc.coef_path)[f, :nl]
        mg, mc = _np(rg.cvm)[f, :nl], _np(rc.cvm)[f, :nl]
        scale = np.abs(cc).max() + 1.0
        dev["lambda rel"] = max(dev.get("lambda rel", 0), np.max(np.abs(lg / lc - 1)))
        dev["coef abs"] = max(dev.get("coef abs", 0), np.max(np.abs(cg - cc)) / (scale if f32 else 1))
        dev["cvm rel"] = max(dev.get("cvm rel", 0), np.max(np.abs(mg / mc - 1)))
    print("%s %s: " % (name, "f32" if dtype == torch.float32 else "f64")
          + " ".join("%s %.3g" % kv for kv in sorted(dev.items()))
          + " nlam %s sel %s / %s" % (_np(rg.nlam).tolist(), _np(rg.sel).tolist(), _np(rc.sel).tolist())
          + (" (coef abs in units of max|coef| + 1, atol %.0e)" % atol32 if f32 else ""))
    for f in range(rc.nlam.shape[0]):
        nl = min(int(rg.nlam[f]), int(rc.nlam[f]))
        lg, lc = _np(rg.lambdas)[f, :nl], _np(rc.lambdas)[f, :nl]
        cg, cc = _np(rg.coef_path)[f, :nl], _np(rc.coef_path)[f, :nl]
        mg, mc = _np(rg.cvm)[f, :nl], _np(rc.cvm)[f, :nl]
        sg, sc = _np(rg.sel)[f], _np(rc.sel)[f]
        if f32:
            np.testing.assert_allclose(lg, lc, rtol=1e-6)
            np.testing.assert_allclose(cg, cc, atol=atol32 * (np.abs(cc).max() + 1.0), rtol=0)
            np.testing.assert_allclose(mg, mc, rtol=1e-4)
            # near-ties may flip: the device's choices must be as good on the twin's curve
            full = _np(rc.cvm)[f]
            np.testing.assert_allclose(full[sg], full[sc], rtol=1e-4)
        else:
            np.testing.assert_allclose(lg, lc, rtol=1e-12)
            np.testing.assert_allclose(cg, cc, atol=1e-6, rtol=0)
            np.testing.assert_allclose(mg, mc, rtol=1e-6)
            assert tuple(sg) == tuple(sc)
            np.testing.assert_allclose(_np(rg.coef_min)[f], _np(rc.coef_min)[f], atol=1e-6, rtol=0)
            np.testing.assert_allclose(_np(rg.coef_1se)[f], _np(rc.coef_1se)[f], atol=1e-6, rtol=0)
    assert L == rg.lambdas.shape[1]


def _twin_properties(name, case, rc):
    """What makes each case the case it is, asserted on the CPU twin."""
    nlam, L = rc.nlam.numpy(), rc.lambdas.shape[1]
    if name.startswith("T1") or name in ("const_p65", "early_stop_nested"):
        assert np.all((nlam >= 5) & (nlam < L))                      # the path stops early
    if name == "const_p65":
        assert np.all(rc.coef_path[0, :nlam[0], [1, 65]].numpy() == 0)
        assert np.count_nonzero(rc.coef_min[0, 1:].numpy()) >= 3
    if name in ("pmax_lasso", "p449"):
        nz = np.count_nonzero(rc.coef_path[0, nlam[0] - 1, 1:].numpy())
        assert nz > 400                       # every block is walked densely by the end
    if name == "pmax_enet":
        assert _leaves_mode_s(rc)
    if name == "L2":
        assert nlam[0] == 2
    if name == "L7":
        assert nlam[0] == 7                                          # no early-stop window hit
    if name == "L200":
        assert 128 < nlam[0] < 200       # past lam_hi's range, and stops before L
    if name == "L256":
        assert nlam[0] > 128
    if name == "early_stop_nested":
        assert len(set(nlam.tolist())) == 1 and np.all(rc.fold_nlam.numpy() == nlam[0])
    if name == "pass_budget":
        assert nlam[0] < 20 and int(rc.npass[0]) == 40               # the budget ends the path
    if name == "n_lt_p":
        assert nlam[0] == 100
    if name == "two_targets":
        assert rc.full_keys == [(0, 0), (1, 1), (2, 0)]
        assert np.all(rc.coef_path[:, 1, [1, 70]].numpy() != 0)      # unpenalised from lambda 1


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(_CASES))
def test_path_edge_shapes(gpu, name, dtype):
    case, rc = _case(name)
    _twin_properties(name, case, rc)
    rg = _call(case, case["G"].to(gpu), dtype)
    if name in _DIAG32_CASES and dtype == torch.float64:
        # the plain twin at the fp32 kernel's tolerances, the diagonal-block twin at the fp64 ones
        _compare(name + " (plain twin)", rg, rc, dtype, as_f32=True)
        rc = _twin_diag32(name)
    _compare(name, rg, rc, dtype)
    if name == "const_p65":
        assert np.all(_np(rg.coef_path)[0, :int(rg.nlam[0]), [1, 65]] == 0)
    if name == "early_stop_nested":
        # every fold ran up to FOLD_LEAD + 1 lambdas past its source's end and put them back
        src = np.repeat(_np(rg.nlam), 2)
        assert sorted(_np(rg.fold_nlam).tolist()) == sorted(src.tolist())
    if name == "pass_budget":
        assert int(rg.nlam[0]) == int(rc.nlam[0]) and int(rg.npass[0]) == int(rc.npass[0]) == 40
    if name in ("L2", "L7"):
        assert int(rg.nlam[0]) == int(rc.nlam[0])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_path_refuses_more_than_pmax(gpu, dtype):
    """p = 513: ate_enet_path returns -2 before it launches."""
    case = _path_case(513, (40, 40, 40), 33, 2, nlambda=5)
    with pytest.raises(_native.NativeError) as e:
        _call(case, case["G"].to(gpu), dtype)
    assert e.value.entry == "ate_enet_path" and e.value.status == -2


def test_path_refuses_more_than_256_lambdas(gpu):
    """nlambda = 257: the path itself has no such limit, ate_cv_select refuses (-1)."""
    case = _path_case(70, (100, 90, 110), 28, 4, nlambda=257)
    with pytest.raises(_native.NativeError) as e:
        _call(case, case["G"].to(gpu), torch.float64)
    assert e.value.entry == "ate_cv_select" and e.value.status == -1
