"""Score and bootstrap kernels (csrc/stats.hip: K03, K18, K20) at their edge shapes, each
against float64 numpy. A reduction differs from numpy in summation order only, so it is
bounded by 64 * eps * sum |terms| with the sum taken in the test; counts are exact
integers. The fixed reduction grid is 1024 x 256 rows: n = 262,144 + 77 is the smallest
size class that gives its strided loop a second trip. Each test prints observed / bound."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.ops import stats as S
from ate_replication_causalml_amd.reference import estimators as E

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
SIZES = [1, 255, 257, 262144 + 77]
BIG = 1.0e9                                   # held by valid == 0 rows: moves every sum


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _mask(rs, n, masked):
    """valid (float64 0/1) with about a fifth of the rows off; row 0 stays on."""
    if not masked:
        return None
    v = (rs.rand(n) >= 0.2).astype(np.float64)
    v[0] = 1.0
    return v


def _check_sums(name, got, terms, count_cols=()):
    """got[j] vs sum(terms[j]) within 64 eps sum |terms[j]|; count columns exactly."""
    worst = 0.0
    for j, t in enumerate(terms):
        t = np.asarray(t, dtype=np.float64)
        ref = float(np.sum(t))
        if j in count_cols:
            assert got[j] == ref, (name, j, got[j], ref)
            continue
        bound = 64 * EPS * float(np.sum(np.abs(t)))
        err = abs(got[j] - ref)
        assert err <= bound, (name, j, got[j], ref, err, bound)
        if bound > 0:
            worst = max(worst, err / bound)
    print("%s: observed / bound = %.3g" % (name, worst))


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


# Finalisers: the same formula on the same six or seven moments, under 20 roundings each
# (contraction into FMAs included); the data keep |mean| below the spread, so the variance
# subtractions cancel less than one digit. 20 * 10 * eps < 1e-13.
FINAL_RTOL = 1e-13


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_naive_moments(gpu, n, masked, dtype):
    rs = np.random.RandomState(n % 1000 + 7 * masked)
    tdt = torch.float64 if dtype == "f64" else torch.float32
    w = (rs.rand(n) < 0.4).astype(np.float64)
    if n > 1:
        w[:4] = [0, 1, 0, 1]                     # both arms have two valid rows
    y = rs.randn(n) + 0.5 * w
    v = _mask(rs, n, masked)
    if v is not None:
        v[:4] = 1.0
        y[v == 0] = BIG
    yt, wt = torch.as_tensor(y).to(tdt), torch.as_tensor(w).to(tdt)
    vt = None if v is None else torch.as_tensor(v).to(tdt)
    res, mom = S.naive(yt.to(gpu), wt.to(gpu), None if vt is None else vt.to(gpu))
    mom, res = mom.cpu().numpy(), res.cpu().numpy()
    yq = yt.double().numpy()                     # the values the kernel reads
    on = np.ones(n, bool) if v is None else v != 0
    terms = []
    for g in (0.0, 1.0):
        s = on & (w == g)
        terms += [np.ones(int(s.sum())), yq[s], yq[s] * yq[s]]
    _check_sums("naive n=%d %s masked=%d" % (n, dtype, masked), mom, terms, count_cols=(0, 3))
    if n > 1:
        want = S._naive_finalize(torch.as_tensor(mom)).numpy()
        assert _rel(res, want) < FINAL_RTOL, (res, want)


@pytest.mark.parametrize("compat", ["reference", "textbook"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_aipw_moments(gpu, n, masked, compat):
    rs = np.random.RandomState(n % 1000 + 3 * masked)
    sign = 1.0 if compat == "reference" else -1.0
    w = (rs.rand(n) < 0.4).astype(np.float64)
    y = (rs.rand(n) < 0.4).astype(np.float64)
    p = np.clip(rs.rand(n), 0.05, 0.95)
    mu0, mu1 = rs.rand(n), rs.rand(n)
    v = _mask(rs, n, masked)
    nan_rows = np.zeros(n, bool)
    if n > 1:
        w[:2] = [0, 1]
        nan_rows[2::50] = True                   # p = 0, w = 0, y = mu0: e1 = 0 / 0 + 0
        p[nan_rows], w[nan_rows] = 0.0, 0.0
        mu0[nan_rows] = y[nan_rows]
    if v is not None:
        v[:3] = 1.0
        for a in (y, mu0, mu1):
            a[v == 0] = BIG
    t = lambda a: torch.as_tensor(a, device=gpu)
    res, mom = S.aipw(t(w), t(y), t(p), t(mu0), t(mu1), None if v is None else t(v),
                      compat=compat)
    mom, res = mom.cpu().numpy(), res.cpu().numpy()
    on = np.ones(n, bool) if v is None else v != 0
    W, Y, Pp, M0, M1 = (a[on] for a in (w, y, p, mu0, mu1))
    with np.errstate(divide="ignore", invalid="ignore"):
        e1 = W * (Y - M1) / Pp + sign * (1 - W) * (Y - M0) / (1 - Pp)
        a = W * Y / Pp - M1 * (W - Pp) / Pp - ((1 - W) * Y / (1 - Pp) + M0 * (W - Pp) / (1 - Pp))
    ok, aok = ~np.isnan(e1), ~np.isnan(a)
    assert int((~ok).sum()) == int((nan_rows & on).sum()) and (n == 1 or (~ok).any())
    terms = [e1[ok], np.ones(int(ok.sum())), M1 - M0, np.ones(int(on.sum())), a[aok],
             a[aok] ** 2]
    _check_sums("aipw n=%d %s masked=%d" % (n, compat, masked), mom, terms, count_cols=(1, 3))
    if n > 1:
        want = S._aipw_finalize(torch.as_tensor(mom)).numpy()
        assert _rel(res, want) < FINAL_RTOL, (res, want)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_dml_moments_and_finalize(gpu, n, masked):
    rs = np.random.RandomState(n % 1000 + 5 * masked)
    yr, wr = rs.randn(n), rs.randn(n)
    v = _mask(rs, n, masked)
    if v is not None:
        yr[v == 0] = BIG
        wr[v == 0] = -BIG
    t = lambda a: torch.as_tensor(a, device=gpu)
    mg = S.dml_moments(t(yr), t(wr), None if v is None else t(v))
    mom = mg.cpu().numpy()
    on = np.ones(n, bool) if v is None else v != 0
    y, w = yr[on], wr[on]
    w2 = w * w
    terms = [w * y, w2, y * y * w2, y * w2 * w, w2 * w2, np.ones(y.size), y * y]
    _check_sums("dml n=%d masked=%d" % (n, masked), mom, terms, count_cols=(5,))
    if n > 1:
        for mode in ("plr", "lm"):
            got = S.dml_finalize(mg, mode).cpu().numpy()
            want = S.dml_finalize(torch.as_tensor(mom), mode).numpy()
            assert _rel(got, want) < FINAL_RTOL, (mode, got, want)


# ---------------------------------------------------------------- propensity clipping
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _clip_case(gpu, p, v=None):
    """Kernel vs its twin on every row, bit for bit; valid rows vs the reference. The two
    limits come from the valid rows; they are applied to every row (the kernel's behaviour,
    which the twin follows: no consumer reads rows with valid == 0)."""
    pg = S.clip_propensity_(torch.as_tensor(p.copy(), device=gpu),
                            None if v is None else torch.as_tensor(v, device=gpu)).cpu().numpy()
    pc = S.clip_propensity_(torch.as_tensor(p.copy()),
                            None if v is None else torch.as_tensor(v)).numpy()
    np.testing.assert_array_equal(_bits(pg), _bits(pc))
    on = np.ones(p.size, bool) if v is None else v != 0
    np.testing.assert_array_equal(_bits(pg[on]), _bits(E.clip_propensity(p[on])))
    return pg


def test_clip_no_boundary_values_keeps_the_bits(gpu):
    rs = np.random.RandomState(1)
    p = rs.rand(1000) * 0.9 + 0.05
    np.testing.assert_array_equal(_bits(_clip_case(gpu, p)), _bits(p))


@pytest.mark.parametrize("kind", ["zeros", "ones"])
def test_clip_all_boundary_one_kind_changes_nothing(gpu, kind):
    # no entry above 0 (or below 1): that limit stays infinite and is not applied
    p = np.zeros(300) if kind == "zeros" else np.ones(300)
    np.testing.assert_array_equal(_bits(_clip_case(gpu, p)), _bits(p))


def test_clip_only_zeros_and_ones_follows_the_reference(gpu):
    """Every entry in {0, 1}, both present: the least positive entry is 1 and the largest
    below one is 0, so the reference's two rules in sequence send every row to 0. (The
    kernel used to apply one rule per row and swapped the two values.)"""
    rs = np.random.RandomState(2)
    p = (rs.rand(500) < 0.5).astype(np.float64)
    assert 0 < p.sum() < 500
    got = _clip_case(gpu, p)
    np.testing.assert_array_equal(got, np.zeros(500))


def test_clip_negative_zero(gpu):
    p = np.array([0.25, -0.0, 0.5, 1.0, 0.0, 0.75])
    got = _clip_case(gpu, p)
    np.testing.assert_array_equal(got, [0.25, 0.25, 0.5, 0.75, 0.25, 0.75])
    q = np.array([-0.0, 0.0, -0.0])              # nothing positive: -0.0 keeps its sign bit
    np.testing.assert_array_equal(_bits(_clip_case(gpu, q)), _bits(q))


@pytest.mark.parametrize("n", [257, 524288 + 300])
def test_clip_limits_come_from_valid_rows(gpu, n):
    rs = np.random.RandomState(3)
    p = rs.rand(n) * 0.8 + 0.1
    p[rs.rand(n) < 0.05] = 0.0
    p[rs.rand(n) < 0.05] = 1.0
    v = (rs.rand(n) >= 0.2).astype(np.float64)
    lo, hi = n - 3, n - 2                         # in the last trip of both kernels
    p[lo], p[hi] = 1e-6, 1.0 - 1e-6               # global min / max, on rows that are off
    v[lo], v[hi] = 0.0, 0.0
    p[5], v[5] = 0.0, 1.0
    p[6], v[6] = 1.0, 1.0
    p[7], v[7] = 0.0, 0.0
    got = _clip_case(gpu, p, v)
    on = v != 0
    mn, mx = p[on & (p > 0)].min(), p[on & (p < 1)].max()
    assert mn > 1e-6 and mx < 1.0 - 1e-6
    assert got[5] == mn and got[6] == mx and got[7] == mn
    assert got[lo] == 1e-6 and got[hi] == 1.0 - 1e-6
    _clip_case(gpu, p)                            # and without a mask, same size


# ---------------------------------------------------------------- multinomial bootstrap
@pytest.mark.parametrize("n", [1, 255, 3001])
def test_bootstrap_multinomial_edges(gpu, n):
    rs = np.random.RandomState(n)
    e1, e2 = rs.randn(n), rs.randn(n)
    t = lambda a: torch.as_tensor(a, device=gpu)
    full = S.bootstrap_multinomial(t(e1), t(e2), 8, seed=1991)
    part = S.bootstrap_multinomial(t(e1), t(e2), 3, seed=1991, b0=5)
    assert torch.equal(part, full[5:8])
    want = S.bootstrap_multinomial(torch.as_tensor(e1), torch.as_tensor(e2), 8, seed=1991)
    assert np.allclose(full.cpu().numpy(), want.numpy(), rtol=1e-11)
    nan1 = np.full(n, np.nan)
    g = S.bootstrap_multinomial(t(nan1), t(e2), 4, seed=1991).cpu()
    c = S.bootstrap_multinomial(torch.as_tensor(nan1), torch.as_tensor(e2), 4, seed=1991)
    assert torch.isnan(g).all() and torch.isnan(c).all()
    if n > 1:
        e1[n // 2] = np.nan                       # one NaN row: out of numerator and count
        g = S.bootstrap_multinomial(t(e1), t(e2), 8, seed=1991).cpu().numpy()
        c = S.bootstrap_multinomial(torch.as_tensor(e1), torch.as_tensor(e2), 8, seed=1991)
        assert np.isfinite(g).all() and np.allclose(g, c.numpy(), rtol=1e-11)


# ---------------------------------------------------------------- Poisson bootstrap (K20)
def _poisson_scores(n, seed=0):
    rs = np.random.RandomState(seed)
    e1, e2 = rs.randn(n), rs.randn(n)
    e1[::13] = np.nan
    return e1, e2


def _poisson_bound(e1, e2, B, b0, n, row_offset=0):
    """[B, 4] bounds 64 eps sum |c * e| of columns 0 and 2 (columns 1, 3 are counts)."""
    ok = ~np.isnan(e1)
    out = np.zeros((B, 4))
    for b in range(B):
        c = S.poisson1_counts(n, 1991, b0 + b, row_offset).astype(np.float64)
        out[b, 0] = 64 * EPS * np.sum(c[ok] * np.abs(e1[ok]))
        out[b, 2] = 64 * EPS * np.sum(c * np.abs(e2))
    return out


def _poisson_close(name, got, want, bound):
    got, want = got.cpu().numpy() if got.is_cuda else got.numpy(), want.numpy()
    np.testing.assert_array_equal(got[:, [1, 3]], want[:, [1, 3]])
    err = np.abs(got - want)[:, [0, 2]]
    bd = bound[:, [0, 2]]
    assert np.all(err <= bd), (name, float((err - bd).max()))
    print("%s: observed / bound = %.3g" % (name, float(np.max(err / np.maximum(bd, 1e-300)))))


@pytest.mark.parametrize("nb", [1, 512])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_bootstrap_poisson_vs_twin(gpu, B, nb):
    n = 1000                                      # nb = 512: blocks 250.. have no rows
    e1, e2 = _poisson_scores(n)
    t = lambda a: torch.as_tensor(a, device=gpu)
    got = S.bootstrap_poisson_partial(t(e1), t(e2), B, 1991, nb=nb)
    want = S.bootstrap_poisson_partial(torch.as_tensor(e1), torch.as_tensor(e2), B, 1991)
    assert got.shape == (B, 4)
    assert (want[:, 1] < want[:, 3]).all() and (want[:, 3] > 0).all()
    _poisson_close("poisson B=%d nb=%d" % (B, nb), got, want, _poisson_bound(e1, e2, B, 0, n))


def test_bootstrap_poisson_padding_replicates_are_zero(gpu):
    """The partial slab is [nb][ceil(B / 64) * 64][4]: lanes past B draw nothing and write
    zeros, so a caller that sums whole tiles (or all-reduces the slab) adds nothing."""
    n, nb = 1000, 8
    e1, e2 = (torch.as_tensor(a, device=gpu) for a in _poisson_scores(n))
    for B in (1, 65, 130):
        pad = (B + 63) // 64 * 64
        part = torch.full((nb, pad, 4), -7.0, dtype=torch.float64, device=gpu)
        _native.call("ate_boot_poisson", e1.data_ptr(), e2.data_ptr(), n, 1991, 0, B, 0, nb,
                     part.data_ptr(), _stream())
        part = part.cpu()
        assert torch.equal(part[:, B:], torch.zeros(nb, pad - B, 4, dtype=torch.float64)), B
        assert (part[:, :B, 3].sum(0) > 0).all()


@pytest.mark.parametrize("nb", [1, 512])
def test_bootstrap_poisson_shard_contract(gpu, nb):
    n, m, B = 1000, 377, 65
    e1, e2 = _poisson_scores(n, seed=1)
    t = lambda a: torch.as_tensor(a, device=gpu)
    full = S.bootstrap_poisson_partial(t(e1), t(e2), B, 1991, nb=nb)
    lo = S.bootstrap_poisson_partial(t(e1[:m]), t(e2[:m]), B, 1991, row_offset=0, nb=nb)
    hi = S.bootstrap_poisson_partial(t(e1[m:]), t(e2[m:]), B, 1991, row_offset=m, nb=nb)
    want_hi = S.bootstrap_poisson_partial(torch.as_tensor(e1[m:]), torch.as_tensor(e2[m:]), B,
                                          1991, row_offset=m)
    _poisson_close("poisson shard hi nb=%d" % nb, hi, want_hi,
                   _poisson_bound(e1[m:], e2[m:], B, 0, n - m, row_offset=m))
    _poisson_close("poisson shard sum nb=%d" % nb, (lo + hi).cpu(), full.cpu(),
                   _poisson_bound(e1, e2, B, 0, n))


def test_bootstrap_poisson_replicate_offset(gpu):
    n = 1000
    e1, e2 = _poisson_scores(n, seed=2)
    t = lambda a: torch.as_tensor(a, device=gpu)
    full = S.bootstrap_poisson_partial(t(e1), t(e2), 9, 1991)
    part = S.bootstrap_poisson_partial(t(e1), t(e2), 2, 1991, b0=7)
    # the op sums the block slab with torch, whose order depends on the shape: counts are
    # exact and the sums within the bound; the kernel's own slab has the same bits (below)
    _poisson_close("poisson b0=7", part, full[7:9].cpu(), _poisson_bound(e1, e2, 2, 7, n))
    nb, g1, g2 = 8, t(e1), t(e2)
    slabs = []
    for b0, B in ((0, 9), (7, 2)):
        slab = torch.zeros((nb, 64, 4), dtype=torch.float64, device=gpu)
        _native.call("ate_boot_poisson", g1.data_ptr(), g2.data_ptr(), n, 1991, b0, B, 0, nb,
                     slab.data_ptr(), _stream())
        slabs.append(slab)
    assert torch.equal(slabs[1][:, :2], slabs[0][:, 7:9])     # another lane, the same sums
