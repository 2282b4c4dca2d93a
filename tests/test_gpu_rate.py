"""GPU tests of the RATE estimator (estimators/rate.py): the ranking walk of csrc/rate.hip
against its float64 twin at every launch shape it has -- exactly, on integer-valued scores --
its repeatability and that it writes every entry of its output, then the estimator against the
row-by-row reference twin, and hipGraph capture and replay with the order and flags as graph
inputs. Run on the MI355X box: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.estimators import rate as DR
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.reference import estimators as E

pytestmark = pytest.mark.gpu

RID0 = 2 ** 33                      # global row ids beyond 32 bits
U53 = 2.0 ** -53
SEED = 1991


def _layout(n, rs, pad=True):
    """n evaluation rows scattered in a panel with padding rows (rid -1) and rows outside the
    subset interleaved -> (eval positions [n], rid [ld], subset [ld])."""
    ld = n + (n // 3 + 5 if pad else 0)
    kind = np.zeros(ld, dtype=np.int64)
    other = rs.permutation(ld)[:ld - n]
    kind[other] = 1 + (np.arange(ld - n) % 2)             # 1: padding, 2: not in the subset
    rid = np.where(kind == 1, -1, rs.permutation(ld) + RID0)
    return np.flatnonzero(kind == 0), rid, kind != 2


def _priority(kind, n, rs):
    if kind == "distinct":
        return rs.permutation(n).astype(np.float64)
    if kind == "equal":
        return np.full(n, 2.5)
    if kind == "two":
        return (rs.rand(n) < 0.4).astype(np.float64)
    raise AssertionError(kind)


def _case(psi_eval, pr_eval, q, rs, pad=True):
    """Panel-order tensors of a kernel case: psi and priority are NaN off the evaluation
    rows, so a stray read would show."""
    n = len(psi_eval)
    rows, rid, sub = _layout(n, rs, pad)
    ld = len(rid)
    psi = np.full(ld, np.nan)
    pr = np.full(ld, np.nan)
    psi[rows], pr[rows] = psi_eval, pr_eval
    order, flags = DR.rate_order(torch.from_numpy(pr), torch.from_numpy(rid),
                                 torch.from_numpy(sub), q)
    assert order.numel() == n and int(flags[-1]) & 1
    return torch.from_numpy(psi), order, flags, torch.from_numpy(rid)


def _bounds(psi, order, flags, rid, B, seed):
    """A numpy walk of its own over the sorted rows, all replicates at once (row 0: the full
    sample): the sums that scale the rounding bounds, [B + 1] each -- S c |A / M|, S c |A|,
    S c Sabs / M, S c Sabs at the run ends (Sabs the running S |psi|), and R the run count."""
    o = order.numpy().astype(np.int64)
    p, r, f = psi.numpy()[o], rid.numpy()[o], flags.numpy()
    inc = np.ones((len(p), B + 1))
    inc[:, 1:] = rng.half_sample(seed, r, B)
    A, M, S = (np.cumsum(inc * v[:, None], axis=0) for v in (p, np.ones_like(p), np.abs(p)))
    ends = np.flatnonzero(f & 1)
    Ae, Me, Se = A[ends], M[ends], S[ends]
    c = np.diff(np.vstack([np.zeros((1, B + 1)), Me]), axis=0)
    Mz = np.where(Me > 0, Me, 1.0)
    return dict(R=len(ends), su=(c * np.abs(Ae) / Mz).sum(0), sv=(c * np.abs(Ae)).sum(0),
                sum_=(c * Se / Mz).sum(0), svm=(c * Se).sum(0), S=S, M=M, A=A, c=c, Ae=Ae, Mz=Mz)


def _exact_check(got, want, bd, tag, worst):
    """Integer-valued psi: every column but U to the bit, U within (R + 2) u S c |A / M|."""
    exact = [0, 1, 3, 4] + list(range(5, got.shape[1]))
    assert torch.equal(got[:, exact], want[:, exact]), tag
    bound = (bd["R"] + 2) * U53 * bd["su"]
    err = (got[:, 2] - want[:, 2]).abs().numpy()
    assert np.all(err <= bound), (tag, err.max())
    if bound.max() > 0:
        worst[0] = max(worst[0], float((err / np.where(bound > 0, bound, np.inf)).max()))


def _grid(Q):
    return np.arange(1, Q + 1) / Q                        # ends on the last row: u = 1


# B: one replicate; 127 | 128: the full-sample slot is the last bit of the stream | opens a
# second stream; 129; 1025: nine streams, 256 threads and a second stream block
@pytest.mark.parametrize("B", [1, 127, 128, 129, 1025])
@pytest.mark.parametrize("kind", ["distinct", "equal", "two"])
def test_walk_exact_on_integer_scores(gpu, B, kind):
    ch = DR.rate_geometry(B, 1 << 20)[0]
    assert ch == (256 if B == 1025 else 64)
    rs = np.random.RandomState(100 + B)
    worst = [0.0]
    for n in sorted({1, 63, 64, 65, ch, ch + 1, 1000}):
        psi_e = rs.randint(-8, 9, n).astype(np.float64)
        pr_e = _priority(kind, n, rs)
        for Q in (1, 64):
            psi, order, flags, rid = _case(psi_e, pr_e, _grid(Q), rs)
            want = DR.rate_boot(psi, order, flags, rid, Q, B, SEED)      # the twin, once
            bd = _bounds(psi, order, flags, rid, B, SEED)
            assert np.array_equal(want[:, 0].numpy(), bd["M"][-1])
            dev = [t.to(gpu) for t in (psi, order, flags, rid)]
            sub = -(-n // ch)
            for nbx in (1, 2, 3, 7, sub + 3):             # the last: more pieces than sub-chunks
                got = DR.rate_boot(*dev, Q, B, SEED, nbx=nbx).cpu()
                _exact_check(got, want, bd, (B, kind, n, Q, nbx), worst)
            # TOC_b(1) is exactly 0: the pair on the last row repeats (A_b(n), n_b)
            assert torch.equal(got[:, -2], torch.where(got[:, 0] > 0, got[:, 1],
                                                       torch.zeros_like(got[:, 1])))
            assert torch.equal(got[:, -1], got[:, 0])
    print("B", B, kind, "worst |U - U_twin| / bound", worst[0])


def test_walk_runs_across_pieces(gpu):
    """n = 240 in 6 pieces of 40: a run ending at 19, one over 20..99 (pieces 0, 1, 2; piece 1
    holds no run end), one ending at 119 -- exactly on the border of piece 2 -- then distinct
    priorities; and the same ranking in 3 and 240 pieces."""
    n, B, Q = 240, 200, 7
    rs = np.random.RandomState(8)
    pr_sorted = np.r_[np.full(20, 900.0), np.full(80, 800.0), np.full(20, 700.0),
                      600.0 - np.arange(120)]
    perm = rs.permutation(n)
    psi_e = rs.randint(-8, 9, n).astype(np.float64)
    psi, order, flags, rid = _case(psi_e, pr_sorted[perm], _grid(Q), rs)
    ends = np.flatnonzero(flags.numpy() & 1)
    assert ends[:4].tolist() == [19, 99, 119, 120] and len(ends) == 123
    assert not np.any((ends >= 40) & (ends < 80)) and 119 == n * 3 // 6 - 1
    want = DR.rate_boot(psi, order, flags, rid, Q, B, SEED)
    bd = _bounds(psi, order, flags, rid, B, SEED)
    dev = [t.to(gpu) for t in (psi, order, flags, rid)]
    worst = [0.0]
    for nbx in (6, 3, 240, 1):
        got = DR.rate_boot(*dev, Q, B, SEED, nbx=nbx).cpu()
        _exact_check(got, want, bd, nbx, worst)
    print("worst |U - U_twin| / bound", worst[0])


def test_walk_gaussian_scores_within_rounding(gpu):
    """Real-valued psi: the integer columns to the bit, every sum within the first-order
    bound of two differently ordered summations of the same terms (u = 2^-53; n positions,
    R runs, Sabs the running S |psi| of the replicate):
      A_b(e)  2 n u Sabs(e)
      V_b     2 u ((R + 2) S c |A| + n S c Sabs(k_r))
      U_b     2 u ((R + 2) S c |A / M| + n S c Sabs(k_r) / M(k_r))"""
    n, B, Q = 1000, 129, 10
    rs = np.random.RandomState(21)
    psi_e = rs.standard_t(5, n) * 3 + 0.4
    psi, order, flags, rid = _case(psi_e, rs.randint(0, 25, n).astype(np.float64), _grid(Q), rs)
    want = DR.rate_boot(psi, order, flags, rid, Q, B, SEED)
    bd = _bounds(psi, order, flags, rid, B, SEED)
    pos = DR.rate_entered(flags).numpy() - 1
    dev = [t.to(gpu) for t in (psi, order, flags, rid)]
    for nbx in (1, 7, 16):
        got = DR.rate_boot(*dev, Q, B, SEED, nbx=nbx).cpu()
        assert torch.equal(got[:, [0, 4]], want[:, [0, 4]])
        assert torch.equal(got[:, 6::2], want[:, 6::2])
        err = (got - want).abs().numpy()
        b_a = 2 * n * U53 * bd["S"][-1]
        b_g = 2 * n * U53 * bd["S"][pos].T
        b_v = 2 * U53 * ((bd["R"] + 2) * bd["sv"] + n * bd["svm"])
        b_u = 2 * U53 * ((bd["R"] + 2) * bd["su"] + n * bd["sum_"])
        ratios = (err[:, 1] / b_a, err[:, 5::2] / b_g, err[:, 3] / b_v, err[:, 2] / b_u)
        print("nbx", nbx, "worst err / bound: A", ratios[0].max(), "grid A", ratios[1].max(),
              "V", ratios[2].max(), "U", ratios[3].max())
        assert all(r.max() <= 1.0 for r in ratios)


def test_walk_repeats_and_fills_its_output(gpu):
    n, B, Q = 1000, 300, 64
    rs = np.random.RandomState(5)
    psi, order, flags, rid = _case(rs.randn(n), rs.randint(0, 40, n).astype(np.float64),
                                   _grid(Q), rs)
    dev = [t.to(gpu) for t in (psi, order, flags, rid)]
    outs = []
    for _ in range(2):
        out = torch.full((B + 1, 5 + 2 * Q), float("nan"), dtype=torch.float64, device=gpu)
        assert DR.rate_boot(*dev, Q, B, SEED, nbx=5, out=out) is out
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0], outs[1])                  # one geometry, one set of bits
    assert _native_refuses()


def _native_refuses():
    from ate_replication_causalml_amd import _native
    f = _native.hip().ate_rate_boot_scratch
    bad = [(0, 10, 4), (65, 10, 4), (4, 0, 4), (4, 4097, 4), (4, 10, 0), (4, 10, 65536)]
    return all(f(*a) == -1 for a in bad) and f(64, 4096, 8) > 0


# ---------------------------------------------------------------- estimator
def _design(n=2000, p=10, seed=4):
    """tau(x) = 1 + x0, confounded through x0 and x1."""
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, p))
    pr = 1 / (1 + np.exp(-(0.5 * X[:, 0] + 0.4 * X[:, 1])))
    W = (r.uniform(size=n) < pr).astype(float)
    Y = X[:, 1] + 0.5 * X[:, 2] + (1 + X[:, 0]) * W + r.normal(size=n)
    return Y, W, X


@pytest.fixture(scope="module")
def design():
    return _design()


def _key(r):
    return (r.ate, r.autoc.estimate, r.autoc.se, r.qini.estimate, r.qini.se, r.crit,
            tuple(r.toc["estimate"]), tuple(r.toc["se"]), tuple(r.toc["entered"]))


def test_estimator_vs_reference(gpu, design):
    Y, W, X = design
    sub = np.arange(len(Y)) % 5 != 0
    kw = dict(q=[0.1, 0.25, 0.5, 0.75, 1.0], subset=sub, n_boot=128, folds=3)
    a = DR.dml_irm_rate_lasso(Y, W, X, 0, device=gpu, graph=False, keep_boot=True, **kw)
    torch.cuda.synchronize()
    b = E.dml_irm_rate(Y, W, X, 0, **kw)
    print("gpu", _key(a), "reference", _key(b))
    tol = dict(abs=1e-6, rel=1e-6)                       # tests/test_gpu_gate.py, group estimates
    assert (a.n, a.n_runs, a.toc["entered"]) == (b.n, b.n_runs, b.toc["entered"])
    assert a.n == int(sub.sum()) and a.boot.shape == (129, 15)
    assert a.ate == pytest.approx(b.ate, **tol)
    for x, y in ((a.autoc, b.autoc), (a.qini, b.qini)):
        assert x.estimate == pytest.approx(y.estimate, **tol)
        assert x.se == pytest.approx(y.se, **tol)
        assert x.p_value == pytest.approx(y.p_value, abs=1e-6, rel=1e-4)
    assert a.toc["estimate"] == pytest.approx(b.toc["estimate"], **tol)
    assert a.toc["se"] == pytest.approx(b.toc["se"], **tol)
    assert a.toc["estimate"][-1] == 0.0 and a.toc["se"][-1] == 0.0
    assert abs(a.crit - b.crit) < 1e-4
    assert a.autoc.estimate / a.autoc.se > 3             # x0 orders the effects


def test_graph_capture_and_replay(gpu, design):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    Y, W, X = design
    kw = dict(n_boot=128, folds=3, device=gpu)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DR.dml_irm_rate_lasso(Y, W, X, X[:, 0], **kw)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    assert _key(runs[1]) == _key(runs[0]) and _key(runs[2]) == _key(runs[0])
    # another priority on the same rows: a replay equals a fresh eager run
    pr2 = np.round(X[:, 3], 1)                            # with ties
    r4 = DR.dml_irm_rate_lasso(Y, W, X, pr2, **kw)
    torch.cuda.synchronize()
    e4 = DR.dml_irm_rate_lasso(Y, W, X, pr2, graph=False, **kw)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert _key(r4) == _key(e4) and r4.autoc.estimate != runs[0].autoc.estimate
    assert r4.n_runs < runs[0].n_runs == len(Y)
    assert r4.ate == pytest.approx(runs[0].ate, rel=1e-12)   # the same scores, another order
    estimator_graphs.clear()


def test_logit_propensity(gpu, design):
    Y, W, X = design
    r = DR.dml_irm_rate_lasso(Y, W, X, 0, n_boot=128, folds=3, device=gpu, graph=False,
                              propensity="logit")
    torch.cuda.synchronize()
    lin = DR.dml_irm_rate_lasso(Y, W, X, 0, n_boot=128, folds=3, device=gpu, graph=False)
    assert r.diagnostics["propensity"] == "logit" and "propensity" not in lin.diagnostics
    assert np.isfinite(_key(r)[:6]).all() and r.autoc.estimate != lin.autoc.estimate
