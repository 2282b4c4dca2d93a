"""Solve, predictor and IRLS kernels (csrc/linalg.hip: K05, K06, K07) at their edge shapes.

Solves run on exact-arithmetic systems: an integer design X (entries in -2..2, aliased
columns as exact copies / integer combinations / zeros) gives a Gram A = X'X that is exact
in fp64, the true coefficients sit on a 1/8 grid, b = A beta is exact, and the embedded
G = [[A, b], [b', beta'b + 3]] has the exact solution beta and the exact RSS 3. The bound
for beta and for diag(A_kept^-1) is the Cholesky forward-error bound 8 k eps cond2(A_kept)
relative to the largest entry, for the RSS 8 k eps y'y; numpy's solve of the same system
must sit inside the same bound. Alias decisions are kept away from the tol^2 threshold: an
fp64 replay of the factorisation asserts d_j / G_jj <= tol^2 / 4 for every aliased column
and >= 1e4 tol^2 for every kept one before anything is launched. Each test prints
observed / bound."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.ops.linalg import (LM_TOL, SolveWorkspace, chol_solve,
                                                     chol_solve_active, predict, spd_solve)
from ate_replication_causalml_amd.ops.panel import build_panel, dtype_code

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
TOL2 = LM_TOL * LM_TOL


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _replay(A, tol2=TOL2):
    """The kernel's column-order factorisation in fp64, a plain loop: (d_j / G_jj, aliased)."""
    k = len(A)
    L = A.copy()
    ratio, al = np.zeros(k), np.zeros(k, bool)
    for j in range(k):
        d, orig = L[j, j], A[j, j]
        ratio[j] = d / orig if orig > 0 else 0.0
        if not (orig > 0) or not (d > tol2 * orig):
            al[j] = True
            L[j:, j] = 0.0
            continue
        ljj = np.sqrt(d)
        L[j + 1:, j] /= ljj
        L[j, j] = ljj
        c = L[j + 1:, j]
        L[j + 1:, j + 1:] -= np.outer(c, c)
    return ratio, al


class _System:
    """One exact system of k columns, built once and shared (read only) by the tests."""

    def __init__(self, k):
        rs = np.random.RandomState(100 + k)
        n = 4 * k + 80
        X = rs.randint(-2, 3, size=(n, k)).astype(np.float64)
        alias = []
        if k >= 7:
            X[:, 3] = X[:, 1]
            X[:, 5] = 0.0
            X[:, 6] = X[:, 0] - 2 * X[:, 2]
            alias = [3, 5, 6]
        if k >= 65:
            X[:, 40] = X[:, 7]
            X[:, k - 2] = X[:, 9]
            alias += [40, k - 2]
        A = X.T @ X
        assert np.abs(A).max() < 2 ** 40
        beta = rs.randint(1, 17, size=k) * rs.choice([-1.0, 1.0], size=k) / 8.0
        beta[alias] = 0.0
        b = A @ beta
        yty = float(beta @ b + 3.0)
        assert 64 * max(np.abs(b).max() * k * 2, abs(yty)) < 2 ** 52      # 1/64 grid: exact
        keep = np.setdiff1d(np.arange(k), alias)
        Ak = A[np.ix_(keep, keep)]
        self.k, self.A, self.b, self.beta, self.yty = k, A, b, beta, yty
        self.alias, self.keep = sorted(alias), keep
        self.cond = float(np.linalg.cond(Ak))
        self.invdiag = np.diag(np.linalg.inv(Ak)).copy()
        self.np_beta = np.linalg.solve(Ak, b[keep])
        ratio, al = _replay(A)
        assert np.flatnonzero(al).tolist() == self.alias
        assert np.all(ratio[self.alias] <= TOL2 / 4), ratio[self.alias]
        assert np.all(ratio[keep] >= 1e4 * TOL2), ratio[keep].min()
        self.G = np.zeros((k + 1, k + 1))
        self.G[:k, :k], self.G[:k, k], self.G[k, :k], self.G[k, k] = A, b, b, yty

    def embedded(self, gpu, indirect=False):
        """(G on the device, cols, rcol): the plain embedding, or the system scattered over
        a permuted, non-contiguous subset of a larger P x P matrix of other values."""
        k = self.k
        if not indirect:
            return torch.as_tensor(self.G, device=gpu), list(range(k)), k
        rs = np.random.RandomState(k)
        P = k + 24
        perm = rs.permutation(P)[:k + 1]
        G = rs.randint(1, 9, size=(P, P)).astype(np.float64) * 1e3
        G[np.ix_(perm, perm)] = self.G
        return torch.as_tensor(G, device=gpu), [int(c) for c in perm[:k]], int(perm[k])

    def check(self, name, beta, invdiag, aux):
        beta, invdiag, aux = (np.asarray(t.cpu()) for t in (beta, invdiag, aux))
        k, keep = self.k, self.keep
        assert np.flatnonzero(np.isnan(beta)).tolist() == self.alias
        assert np.flatnonzero(np.isnan(invdiag)).tolist() == self.alias
        bound = 8 * k * EPS * self.cond
        scale = np.abs(self.beta[keep]).max()
        e_b = np.abs(beta[keep] - self.beta[keep]).max() / scale
        e_np = np.abs(self.np_beta - self.beta[keep]).max() / scale
        e_i = np.abs(invdiag[keep] - self.invdiag).max() / self.invdiag.max()
        rss_bound = 8 * k * EPS * self.yty
        e_r = abs(aux[1] - 3.0)
        e_rnp = abs(self.yty - self.np_beta @ self.b[keep] - 3.0)
        print("%s: cond %.2f beta %.3g invdiag %.3g rss %.3g (numpy beta %.3g rss %.3g) "
              "[observed / bound]" % (name, self.cond, e_b / bound, e_i / bound,
                                      e_r / rss_bound, e_np / bound, e_rnp / rss_bound))
        assert e_np <= bound and e_rnp <= rss_bound
        assert e_b <= bound and e_i <= bound and e_r <= rss_bound
        assert aux[0] == len(keep) and aux[2] == self.yty and aux[3] == 0.0


_SYSTEMS = {}


def _system(k):
    if k not in _SYSTEMS:
        _SYSTEMS[k] = _System(k)
    return _SYSTEMS[k]


def test_alias_sets_of_the_systems():
    # pure host check of the construction (no launch): the expected alias sets
    assert _system(1).alias == [] and _system(2).alias == []
    assert _system(7).alias == [3, 5, 6]
    assert _system(65).alias == [3, 5, 6, 40, 63]
    assert _system(130).alias == [3, 5, 6, 40, 128]


# ---------------------------------------------------------------- 1. chol_solve over k
@pytest.mark.parametrize("k,indirect", [(1, False), (2, False), (7, False), (65, False),
                                        (65, True), (130, False), (130, True)])
def test_chol_solve_exact_systems(gpu, k, indirect):
    s = _system(k)
    G, cols, rcol = s.embedded(gpu, indirect)
    r = chol_solve(G, cols, rcol)
    s.check("chol_solve k=%d indirect=%d" % (k, indirect), r.beta, r.invdiag, r.aux)


def test_chol_solve_k1030_second_trip(gpu):
    """k = 1030 > 1024 threads: the smallest size at which the row loops, the one-thread-
    per-column Linv pass and the final writes take a second trip (alias set
    [3, 5, 6, 40, 1028]). Measured on the MI355X: one solve at this size takes 411 to 413 ms
    (one workgroup; printed, not asserted). The test launches it twice."""
    s = _system(1030)
    assert s.alias == [3, 5, 6, 40, 1028]
    G, cols, rcol = s.embedded(gpu)
    ws = SolveWorkspace(s.k, gpu)
    cols_t = torch.as_tensor(cols, dtype=torch.int32, device=gpu)
    r = chol_solve(G, cols_t, rcol, ws=ws)
    s.check("chol_solve k=1030", r.beta, r.invdiag, r.aux)
    first = [_bits(t) for t in (r.beta, r.invdiag, r.aux)]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    r = chol_solve(G, cols_t, rcol, ws=ws)            # the same workspace again: same bits
    t1.record()
    torch.cuda.synchronize()
    print("chol_solve k=1030: %.1f ms" % t0.elapsed_time(t1))
    for a, t in zip(first, (r.beta, r.invdiag, r.aux)):
        assert torch.equal(a, _bits(t))


# ---------------------------------------------------------------- 2. rhs= path
@pytest.mark.parametrize("k", [7, 130])
def test_chol_solve_rhs_vector(gpu, k):
    s = _system(k)
    G, cols, rcol = s.embedded(gpu)
    a = chol_solve(G, cols, rcol)
    rhs = torch.as_tensor(s.b, device=gpu)
    b = chol_solve(G, cols, -1, rhs=rhs)
    assert torch.equal(_bits(a.beta), _bits(b.beta))
    assert torch.equal(_bits(a.invdiag), _bits(b.invdiag))
    aux = b.aux.cpu().numpy()
    beta = np.nan_to_num(b.beta.cpu().numpy())
    # aux[1] = 0 - beta'b summed in column order: one sum of k terms
    bound = 8 * k * EPS * float(np.abs(beta * s.b).sum())
    err = abs(aux[1] + float(beta @ s.b))
    print("chol_solve rhs k=%d: -beta'b observed / bound = %.3g" % (k, err / bound))
    assert err <= bound
    assert aux[0] == len(s.keep) and aux[2] == 0.0 and aux[3] == 0.0


# ---------------------------------------------------------------- 3. done flag
@pytest.mark.parametrize("k", [7, 130])
def test_chol_solve_done_flag(gpu, k):
    s = _system(k)
    G, cols, rcol = s.embedded(gpu)
    plain = chol_solve(G, cols, rcol)
    ws = SolveWorkspace(k, gpu)
    for t in (ws.work, ws.beta, ws.invdiag, ws.aux):
        t.fill_(-777.0)
    done = torch.ones(1, dtype=torch.int32, device=gpu)
    chol_solve(G, cols, rcol, done=done, ws=ws)
    for t in (ws.work, ws.beta, ws.invdiag, ws.aux):
        assert bool((t == -777.0).all())
    done.zero_()
    r = chol_solve(G, cols, rcol, done=done, ws=ws)
    for x, y in ((r.beta, plain.beta), (r.invdiag, plain.invdiag), (r.aux, plain.aux)):
        assert torch.equal(_bits(x), _bits(y))
    assert int(done.item()) == 0


# ---------------------------------------------------------------- 4. threshold pair
def test_chol_solve_threshold_pair(gpu):
    """Two columns x_i + delta e whose norm after projecting out the earlier columns is
    1e-6 and 1e-8 of their own: tol = 1e-7 keeps the first and aliases the second. The
    decision has a factor 100 of room on either side (d / G_jj = 1e-12 and 1e-16 against
    tol^2 = 1e-14), far above the fp64 noise of an 8-column factorisation (~1e-15). Only the
    NaN pattern and the rank are asserted: the system is ill-conditioned by design."""
    rs = np.random.RandomState(9)
    n, k0 = 64, 6
    X0 = rs.randint(-2, 3, size=(n, k0)).astype(np.float64)
    cols_x = [X0]
    for src, ratio in ((1, 1e-6), (2, 1e-8)):
        e = rs.choice([-1.0, 1.0], size=n)            # a fresh direction for each column
        base = np.concatenate(cols_x, 1)
        res = e - base @ np.linalg.lstsq(base, e, rcond=None)[0]
        delta = ratio * np.linalg.norm(X0[:, src]) / np.linalg.norm(res)
        cols_x.append((X0[:, src] + delta * e)[:, None])
    X = np.concatenate(cols_x, 1)
    y = rs.randint(-4, 5, size=n).astype(np.float64)
    Z = np.concatenate([X, y[:, None]], 1)
    G = Z.T @ Z
    ratio, al = _replay(G[:8, :8])
    assert np.flatnonzero(al).tolist() == [7]
    assert 0.25e-12 < ratio[6] < 4e-12 and ratio[7] < TOL2 / 2 and np.all(ratio[:6] > 1e4 * TOL2)
    r = chol_solve(torch.as_tensor(G, device=gpu), list(range(8)), 8)
    beta, aux = r.beta.cpu().numpy(), r.aux.cpu().numpy()
    assert np.flatnonzero(np.isnan(beta)).tolist() == [7]
    assert np.flatnonzero(np.isnan(r.invdiag.cpu().numpy())).tolist() == [7]
    assert aux[0] == 7


# ---------------------------------------------------------------- 5. chol_solve_active
@pytest.mark.parametrize("kact", [0, 1, 64, 130, 135, -3])
def test_chol_solve_active_count(gpu, kact):
    """The device-count solve: LDS is sized by the fixed length (130) and indexed by the
    active count. Entries past the active count are unspecified and not asserted."""
    s = _system(130)
    k = s.k
    G, cols, rcol = s.embedded(gpu, indirect=True)
    cols_t = torch.as_tensor(cols, dtype=torch.int32, device=gpu)
    ka = min(max(kact, 0), k)
    r = chol_solve_active(G, cols_t, torch.tensor([kact], dtype=torch.int32, device=gpu), rcol)
    aux = r.aux.cpu().numpy()
    if ka == 0:
        np.testing.assert_array_equal(aux, [0.0, s.yty, s.yty, 0.0])
        return
    ref = chol_solve(G, cols[:ka], rcol)
    assert torch.equal(_bits(r.beta[:ka]), _bits(ref.beta))
    assert torch.equal(_bits(r.invdiag[:ka]), _bits(ref.invdiag))
    assert torch.equal(_bits(r.aux), _bits(ref.aux))
    assert aux[0] == ka - sum(a < ka for a in s.alias)
    if ka == k:
        s.check("chol_solve_active kact=%d" % kact, r.beta, r.invdiag, r.aux)


def test_solve_argument_checks(gpu):
    """k = 0, k = 4097 and A = 0 are refused by the entry points before any launch."""
    G = torch.eye(4, dtype=torch.float64, device=gpu)
    cols = torch.zeros(8, dtype=torch.int32, device=gpu)
    ws = SolveWorkspace(4, gpu)
    kdev = torch.ones(1, dtype=torch.int32, device=gpu)
    for k in (0, 4097):
        with pytest.raises(_native.NativeError) as ei:
            _native.call("ate_chol_solve", G.data_ptr(), 4, cols.data_ptr(), k, 3, 0, LM_TOL,
                         ws.work.data_ptr(), ws.beta.data_ptr(), ws.invdiag.data_ptr(),
                         ws.aux.data_ptr(), 0, _stream())
        assert ei.value.status < 0
        with pytest.raises(_native.NativeError) as ei:
            _native.call("ate_chol_solve_k", G.data_ptr(), 4, cols.data_ptr(), k,
                         kdev.data_ptr(), 3, LM_TOL, ws.work.data_ptr(), ws.beta.data_ptr(),
                         ws.invdiag.data_ptr(), ws.aux.data_ptr(), _stream())
        assert ei.value.status < 0
    for A, k in ((0, 2), (1, 0), (1, 4097)):
        with pytest.raises(_native.NativeError) as ei:
            _native.call("ate_spd_solve_batched", G.data_ptr(), G.data_ptr(), A, k,
                         ws.work.data_ptr(), ws.beta.data_ptr(), _stream())
        assert ei.value.status < 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. spd_solve
def test_spd_solve_k1(gpu):
    # perfect-square pivots and dyadic right-hand sides: every operation is exact
    K = torch.tensor([4.0, 9.0, 0.25, -1.0, 16.0, 0.0], dtype=torch.float64).view(6, 1, 1)
    x_true = torch.tensor([1.5, -0.125, 8.0, 1.0, 0.375, 1.0], dtype=torch.float64)
    r = (K.view(6) * x_true).view(6, 1)
    x = spd_solve(K.to(gpu), r.to(gpu)).cpu().view(6)
    ok = torch.tensor([True, True, True, False, True, False])
    assert torch.equal(x[ok], x_true[ok]) and torch.isnan(x[~ok]).all()
    assert torch.equal(torch.isnan(spd_solve(K, r)).view(6), ~ok)     # the CPU twin agrees


def test_spd_solve_k300_bad_systems_between_good_ones(gpu):
    """A = 5, k = 300: the 256-thread loops take a second trip. System 1 fails at the first
    pivot, system 3 at the last one (its last diagonal entry lowered by twice its Schur
    complement); both come back all NaN and their neighbours are solved within the bound."""
    A, k = 5, 300
    n = 4 * k + 80
    Ks, xs = [], []
    for a in range(A):
        rs = np.random.RandomState(300 + a)
        X = rs.randint(-2, 3, size=(n, k)).astype(np.float64)
        Ks.append(X.T @ X)
        xs.append(rs.randint(1, 17, size=k) * rs.choice([-1.0, 1.0], size=k) / 8.0)
    K, x_true = np.stack(Ks), np.stack(xs)
    r = np.einsum("aij,aj->ai", K, x_true)
    cond = [float(np.linalg.cond(K[a])) for a in range(A)]
    K[1, 0, 0] = 0.0
    schur = 1.0 / np.linalg.inv(K[3])[k - 1, k - 1]
    assert schur > 1.0
    K[3, k - 1, k - 1] -= 2.0 * schur
    x = spd_solve(torch.as_tensor(K, device=gpu), torch.as_tensor(r, device=gpu)).cpu().numpy()
    assert np.isnan(x[1]).all() and np.isnan(x[3]).all()
    xc = spd_solve(torch.as_tensor(K), torch.as_tensor(r)).numpy()
    np.testing.assert_array_equal(np.isnan(xc), np.isnan(x))
    for a in (0, 2, 4):
        bound = 8 * k * EPS * cond[a]
        scale = np.abs(x_true[a]).max()
        err = np.abs(x[a] - x_true[a]).max() / scale
        err_np = np.abs(np.linalg.solve(K[a], r[a]) - x_true[a]).max() / scale
        print("spd_solve k=300 system %d: cond %.2f observed / bound = %.3g (numpy %.3g)"
              % (a, cond[a], err / bound, err_np / bound))
        assert err_np <= bound and err <= bound


# ---------------------------------------------------------------- 7. predict
def _predict_cases(gpu, pan, name):
    cols = [pan.cols["one"], *pan.xcols]
    k = len(cols)
    Xh = pan.data.double().cpu().numpy()[cols]                 # [k, ld], padding rows too
    worst = 0.0
    for beta in ([0.5, -1.25, 2.0, 0.75], [0.5, float("nan"), 2.0, 0.75]):
        bt = torch.tensor(beta, dtype=torch.float64, device=gpu)
        for ov_idx, ov_val in ((-1, 0.0), (0, 0.0), (0, 1.0), (k - 1, 0.0), (k - 1, 1.0)):
            Xo = Xh.copy()
            if ov_idx >= 0:
                Xo[ov_idx] = ov_val
            eta = np.nan_to_num(np.asarray(beta)) @ Xo          # dyadic: exact in any order
            got = predict(pan, cols, bt, ov_idx, ov_val).cpu().numpy()
            assert got.shape == (pan.ld,)
            np.testing.assert_array_equal(got, eta)
            mu = 1.0 / (1.0 + np.exp(-eta))
            got = predict(pan, cols, bt, ov_idx, ov_val, link="logit").cpu().numpy()
            rel = float(np.max(np.abs(got - mu) / mu))
            assert rel <= 8 * EPS, (beta, ov_idx, ov_val, rel / EPS)
            worst = max(worst, rel)
    print("%s: logit observed / bound = %.3g" % (name, worst / (8 * EPS)))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_predict_second_trip(gpu, dtype):
    """predict_kernel<float/double>: 2048 x 256 threads, so rows from 524,288 on are the
    grid-stride loop's second trip; ld > n, so padding rows are predicted too."""
    n = 524288 + 300
    rs = np.random.RandomState(11)
    X = rs.randint(-8, 9, size=(n, 3)) / 4.0
    pan = build_panel(X, None, None, dtype=dtype, device=gpu, col_align=8)
    assert pan.ld > n and pan.ld > 2048 * 256
    _predict_cases(gpu, pan, "predict %s n=%d" % (dtype, n))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_predict_one_row(gpu, dtype):
    pan = build_panel(np.array([[0.75, -1.5, 2.0]]), None, None, dtype=dtype, device=gpu,
                      col_align=8)
    _predict_cases(gpu, pan, "predict %s n=1" % dtype)


def test_dtype_code_0_is_refused(gpu):
    pan = build_panel(np.ones((3, 2)), np.ones(3), None, dtype="f64", device=gpu,
                      extra_cols=("z",), col_align=8)
    cols = torch.tensor([0, 1, 2], dtype=torch.int32, device=gpu)
    beta = torch.zeros(3, dtype=torch.float64, device=gpu)
    out = torch.full((pan.ld,), -5.0, dtype=torch.float64, device=gpu)
    with pytest.raises(_native.NativeError) as ei:
        _native.call("ate_predict", 0, pan.data.data_ptr(), pan.cm_ld, pan.ld, cols.data_ptr(),
                     beta.data_ptr(), 3, -1, 0.0, 0, out.data_ptr(), _stream())
    assert ei.value.status < 0
    done = torch.zeros(1, dtype=torch.int32, device=gpu)
    devp = torch.zeros(1024, dtype=torch.float64, device=gpu)
    with pytest.raises(_native.NativeError) as ei:
        _native.call("ate_irls_update", 0, pan.data.data_ptr(), pan.cm_ld, pan.ld,
                     cols.data_ptr(), beta.data_ptr(), 3, pan.cols["W"], pan.cols["one"],
                     pan.cols["z"], 1, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                     devp.data_ptr(), 1024, done.data_ptr(), _stream())
    assert ei.value.status < 0
    assert bool((out == -5.0).all())


# ---------------------------------------------------------------- 8. ate_irls_update
NB = 1024          # the deviance grid of logistic_irls: rows from 262,144 on are a second trip


def _irls_panel(gpu, dtype, n):
    rs = np.random.RandomState(n % 997)
    X = rs.randint(-8, 9, size=(n, 3)) / 4.0
    y = rs.randint(0, 2, size=n).astype(np.float64)
    y[::5] = 0.25                                             # both deviance terms
    if n == 5:
        X = np.array([[0.0, 1.0, 0.25], [1.0, -1.0, -0.5], [0.5, 0.0, 16.0],
                      [-0.5, 0.25, -16.0], [2.0, 1.5, 0.5]])
        y = np.array([0.25, 1.0, 0.0, 1.0, 0.0])
    else:
        big = np.arange(3, n, 7)
        X[big, 2] = 16.0 * rs.choice([-1.0, 1.0], size=big.size)    # |eta| about 40
    pan = build_panel(X, y, None, dtype=dtype, device=gpu, extra_cols=("z",), col_align=8)
    off = np.flatnonzero(rs.rand(n) < 0.2) if n > 5 else np.array([4])
    pan.data[pan.cols["one"], torch.as_tensor(off, device=gpu)] = 0     # real rows, valid = 0
    return pan


def _irls_update(pan, cols_t, beta, first, eta, mu, w, devp, done):
    _native.call("ate_irls_update", dtype_code(pan.data), pan.data.data_ptr(), pan.cm_ld, pan.ld,
                 cols_t.data_ptr(), beta.data_ptr(), cols_t.numel(), pan.cols["W"],
                 pan.cols["one"], pan.cols["z"], first, eta.data_ptr(), mu.data_ptr(),
                 w.data_ptr(), devp.data_ptr(), NB, done.data_ptr(), _stream())


def _ulps(got, ref64, tdt):
    """|got - round(ref64)| in units of the spacing of the panel dtype at the reference."""
    ref = torch.as_tensor(ref64).to(tdt)
    npd = np.float32 if tdt == torch.float32 else np.float64
    r = ref.numpy().astype(npd)
    g = got.cpu().numpy().astype(npd)
    sp = np.spacing(np.maximum(np.abs(r), np.finfo(npd).tiny)).astype(np.float64)
    return np.abs(g.astype(np.float64) - r.astype(np.float64)) / sp


@pytest.mark.parametrize("first", [1, 0])
@pytest.mark.parametrize("n", [5, 262144 + 77])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_irls_update_direct(gpu, dtype, n, first):
    pan = _irls_panel(gpu, dtype, n)
    ld, tdt = pan.ld, pan.dtype
    cols = [pan.cols["one"], *pan.xcols]
    cols_t = torch.tensor(cols, dtype=torch.int32, device=gpu)
    beta = [0.5, -1.25, float("nan"), 2.5]
    bt = torch.tensor(beta, dtype=torch.float64, device=gpu)
    zc = pan.cols["z"]
    eta = torch.full((ld,), -9.0, dtype=torch.float64, device=gpu)
    mu = torch.full_like(eta, -9.0)
    w = torch.full((ld,), -9.0, dtype=tdt, device=gpu)
    devp = torch.full((NB,), -9.0, dtype=torch.float64, device=gpu)
    pan.data[zc] = -9.0
    before = pan.data.clone()
    done = torch.ones(1, dtype=torch.int32, device=gpu)
    _irls_update(pan, cols_t, bt, first, eta, mu, w, devp, done)
    for t in (eta, mu, w, devp):                              # done = 1: nothing is written
        assert bool((t == -9.0).all())
    assert torch.equal(pan.data, before)
    done.zero_()
    _irls_update(pan, cols_t, bt, first, eta, mu, w, devp, done)
    after = pan.data.clone()
    keep = [c for c in range(pan.P) if c != zc]
    assert torch.equal(after[keep], before[keep])             # only the z column is written

    Xh = before.double().cpu().numpy()
    valid, y = Xh[pan.cols["one"]], Xh[pan.cols["W"]]
    e10 = 10 * EPS
    if first:
        mu_r = (y + 0.5) * 0.5
        eta_r = np.log(mu_r / (1.0 - mu_r))
    else:
        eta_r = np.nan_to_num(np.asarray(beta)) @ Xh[cols]
        assert np.abs(eta_r).max() > 36
        mu_r = np.clip(1.0 / (1.0 + np.exp(-eta_r)), e10, 1.0 - e10)
        assert (mu_r == e10).any() and (mu_r == 1.0 - e10).any()
    me = mu_r * (1.0 - mu_r)
    w_r = valid * me
    z_r = valid * (eta_r + (y - mu_r) / me)
    on = valid != 0
    assert (~on[:pan.n]).any() and (~on[pan.n:]).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = np.where(y > 0, y * np.log(np.where(y > 0, y / mu_r, 1.0)), 0.0)
        t2 = np.where(y < 1, (1 - y) * np.log(np.where(y < 1, (1 - y) / (1 - mu_r), 1.0)), 0.0)
    terms = 2.0 * (t1 + t2)[on]
    assert (t1[on] != 0).any() and (t2[on] != 0).any() and ((t1 != 0) & (t2 != 0))[on].any()

    eta_g, mu_g = eta.cpu().numpy(), mu.cpu().numpy()
    e_eta = float(np.max(np.abs(eta_g - eta_r) / np.maximum(np.abs(eta_r), 1e-300)))
    e_mu = float(np.max(np.abs(mu_g - mu_r) / mu_r))
    u_w = _ulps(w, w_r, tdt)
    u_z = _ulps(after[zc], z_r, tdt)
    dev_bound = 64 * EPS * float(np.abs(terms).sum())
    e_dev = abs(float(devp.sum().item()) - float(terms.sum()))
    print("irls_update %s n=%d first=%d: eta %.3g mu %.3g dev %.3g [observed / bound]; "
          "w %.3g z %.3g [ulp of %s]" % (dtype, n, first, e_eta / (8 * EPS), e_mu / (8 * EPS),
                                         e_dev / dev_bound, u_w.max(), u_z.max(), dtype))
    assert e_eta <= 8 * EPS and e_mu <= 8 * EPS
    assert np.all(w.cpu().numpy()[~on] == 0) and np.all(after[zc].cpu().numpy()[~on] == 0)
    assert u_w.max() <= 1 and u_z.max() <= 1
    assert e_dev <= dev_bound


# ---------------------------------------------------------------- 9. ate_irls_check
def _check_replay(state, done, devp, first, eps, maxit):
    if done[0]:
        return
    dev = 0.0
    for v in devp:
        dev += v
    if first:
        state[:] = [dev, dev, 0.0, 0.0]
        return
    state[2] += 1.0
    state[1] = dev
    if abs(dev - state[0]) / (abs(dev) + 0.1) < eps:
        state[3] = 1.0
        done[0] = 1
    elif state[2] >= maxit:
        done[0] = 1
    state[0] = dev


def _drive_check(gpu, steps, eps, maxit):
    """Run (dev_partial, first) steps on the device and in the replay; the states after
    every step must be equal. Returns the final (state, done)."""
    state = torch.full((4,), -1.0, dtype=torch.float64, device=gpu)
    done = torch.zeros(1, dtype=torch.int32, device=gpu)
    st, dn = [-1.0] * 4, [0]
    for devp, first in steps:
        d = torch.tensor(devp, dtype=torch.float64, device=gpu)
        _native.call("ate_irls_check", d.data_ptr(), len(devp), first, eps, maxit,
                     state.data_ptr(), done.data_ptr(), _stream())
        torch.cuda.synchronize()
        _check_replay(st, dn, devp, first, eps, maxit)
        assert state.cpu().tolist() == st and int(done.item()) == dn[0], (devp, first)
    return st, dn[0]


def test_irls_check_state_machine(gpu):
    # dyadic partials: their sum is exact in any order
    steps = [([512.0, 488.0, 0.0], 1),                # first call: dev = 1000
             ([450.0, 450.0, 0.0], 0),                # |900 - 1000| / 900.1: no convergence
             ([450.0, 450.0, 2.0 ** -20], 0),         # 9.5e-7 / 900.1 < 1e-8: converged
             ([1.0, 2.0, 3.0], 0),                    # latched: changes nothing
             ([7.0, 7.0, 7.0], 1)]
    st, dn = _drive_check(gpu, steps, 1e-8, 25)
    assert st == [900.0 + 2.0 ** -20, 900.0 + 2.0 ** -20, 2.0, 1.0] and dn == 1
    steps = [([64.0], 1), ([32.0], 0), ([16.0], 0), ([16.0], 0)]
    st, dn = _drive_check(gpu, steps, 1e-8, 2)       # maxit = 2 stops unconverged
    assert st == [16.0, 16.0, 2.0, 0.0] and dn == 1
