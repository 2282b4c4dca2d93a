"""GPU tests of DML-APOS (estimators/apos.py): the fused potential-outcome pass (csrc/apo.hip
``ate_apo_moments``) against its float64 torch twin at L = 2, 3 and 8 on fp64 and bf16 panels
(column-major and 64-row blocked) with an intercept-only block and an all-zero g row, the sums
it shares bit for bit with the AIPW pass of csrc/irm.hip at L = 2, what the entry point refuses,
the estimator against the row-by-row reference twin, hipGraph capture and replay, and bf16
against f64 panel storage. Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.data.dgp import make_multiarm_data
from ate_replication_causalml_amd.estimators import apos as DA
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.ops.panel import build_panel, dtype_code
from ate_replication_causalml_amd.reference import estimators as E
from ate_replication_causalml_amd.result import ApoResult, apo_layout
from test_gpu_irm import CLIP, COUNTS, P_X, _case

pytestmark = pytest.mark.gpu

COUNTS8 = (1, 7, 64, 65, 130, 257, 3, 70)     # L = 8 over one fold
EDGE = np.array([0, 255, 256, 299])           # columns at the ends of the two compaction trips


def _levels_case(L, counts, exact, seed=29):
    """Host arrays of the kernel tests at L levels: ``len(counts) / L`` folds level-split into
    segments of ``counts`` rows (segment L k + c), p = 300, ~40 nonzero columns incl. 0, 255,
    256, 299 with a support of its own per coefficient row; the last block of two or more is
    intercept-only and row g_1 of block 0 is all zero. ``exact``: the grids of
    test_gpu_irm._case -- x on a 1/8 grid in [-4, 4], coefficients on a 2^-6 grid in [-9/64,
    9/64] -- so every fp32 partial sum of the bf16 kernel sits on a 2^-9 grid below 2^7 and is
    exact. Returns (X, D, Y, seg, coef [nfold, 2L, p+1])."""
    nfold = len(counts) // L
    assert nfold * L == len(counts)
    rs = np.random.RandomState(seed)
    seg = np.repeat(np.arange(len(counts)), counts)
    seg = seg[rs.permutation(len(seg))]
    n = len(seg)
    D = (seg % L).astype(float)
    if exact:
        X = rs.randint(-32, 33, size=(n, P_X)) / 8.0
        Y = rs.randint(0, 2, n).astype(float)
    else:
        X = rs.randn(n, P_X)
        Y = rs.randn(n) + 0.3 * D
    support = np.unique(np.r_[EDGE, rs.choice(P_X, 36, replace=False)])
    coef = np.zeros((nfold, 2 * L, P_X + 1))
    for k in range(nfold):
        for r in range(2 * L):
            on = support[rs.rand(len(support)) < 0.6]
            if exact:
                coef[k, r, 1 + on] = rs.randint(-9, 10, len(on)) / 64.0
            else:
                coef[k, r, 1 + on] = rs.randn(len(on)) * (0.1 if r >= L else 0.5)
            coef[k, r, 1 + EDGE] = rs.choice([-7, -5, -3, 2, 4, 6], 4) / 64.0
        coef[k, :L, 0] = (16 + 4 * np.arange(L)) / 64.0        # g_c: 0.25, 0.3125, ...
        coef[k, L:, 0] = 0.5                                   # m_c
    if nfold > 1:
        coef[nfold - 1, :, 1:] = 0.0                           # an intercept-only block
    coef[0, 1] = 0.0                                           # g_1 of block 0: all zero
    return X, D, Y, seg, coef


def _own_m(X, seg, coef, L):
    """Every row's raw propensity of its own level."""
    return np.array([coef[s // L, L + s % L, 0] + coef[s // L, L + s % L, 1:] @ x
                     for x, s in zip(X, seg)])


def _host_checks(X, D, seg, coef, L, counts):
    """What the inputs must have for the test to mean something (asserted on the host, as
    test_gpu_irm does): no raw m within 1e-6 of the clip, and a level that clips some of its
    rows and not all. Returns (n_c, n_clipped_c)."""
    m = _own_m(X, seg, coef, L)
    assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6
    out = (m < CLIP) | (m > 1 - CLIP)
    lev = (seg % L).astype(np.int64)
    n_c = np.bincount(lev, minlength=L)
    n_clip = np.bincount(lev, weights=out, minlength=L).astype(np.int64)
    assert np.array_equal(n_c, np.asarray(counts).reshape(-1, L).sum(0))
    assert any(0 < a < b for a, b in zip(n_clip, n_c)), (n_clip, n_c)
    assert np.count_nonzero(np.any(coef[:, :, 1:] != 0, axis=(0, 1))) >= 36
    assert (coef[0, 1] == 0).all()
    return n_c, n_clip


def _check(got, want, L, n, n_c, n_clip):
    got, want = got.cpu().numpy(), want.numpy()
    lay = apo_layout(L)
    assert got.shape == want.shape == (lay.size,)
    print("moments gpu ", got.tolist())
    print("moments twin", want.tolist())
    print("rel err     ", (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).tolist())
    np.testing.assert_allclose(got, want, rtol=1e-11)     # the bound of test_gpu_irm._check
    b = lay.level
    assert got[0] == n == want[0]
    assert np.array_equal(got[b::4], n_c) and np.array_equal(want[b::4], n_c)
    assert np.array_equal(got[b + 1::4], n_clip) and np.array_equal(want[b + 1::4], n_clip)


def _panel(X, D, Y, seg, dtype, device, W=None):
    return build_panel(X, W, Y, folds=seg, dtype=dtype, device=device, targets={"D": D})


def _blocked(p):
    b = dataclasses.replace(
        p, data=p.data.reshape(p.P, p.ld // 64, 64).permute(1, 0, 2).contiguous(), blocked=True)
    assert b.strides() == (64, 64 * p.P) and torch.equal(b.colmajor(), p.data)
    return b


@pytest.mark.parametrize("L,counts", [(3, COUNTS), (2, COUNTS), (8, COUNTS8)])
def test_apo_kernel_f64_vs_twin(gpu, L, counts):
    X, D, Y, seg, coef = _levels_case(L, counts, exact=False)
    n_c, n_clip = _host_checks(X, D, seg, coef, L, counts)
    if len(counts) > L:
        assert (coef[-1, :, 1:] == 0).all()               # the intercept-only block
    pc = _panel(X, D, Y, seg, "f64", "cpu")
    pg = _panel(X, D, Y, seg, "f64", gpu)
    assert tuple(pg.seg_nreal) == counts and pg.ld > len(Y)
    c = torch.from_numpy(coef)
    want = DA.apo_moments(pc, c, L, CLIP)
    assert DA.default_nbx(pg, L) == 1                     # every segment is one trip of rows
    for nbx in (None, 1, 3):                              # 3: two workgroups per segment idle
        got = DA.apo_moments(pg, c.to(gpu), L, CLIP, nbx=nbx)
        torch.cuda.synchronize()
        print("L", L, "nbx", nbx)
        _check(got, want, L, len(Y), n_c, n_clip)


@pytest.mark.parametrize("dtype,L", [("f64", 2), ("f64", 5), ("bf16", 2)])
def test_apo_kernel_several_workgroups_per_segment(gpu, dtype, L):
    """Segments longer than one workgroup's trip of rows (1024 at L = 2 and 512 at L = 5 on
    an fp64 panel, 2048 on a bf16 one): the default grid (one trip each), one workgroup
    striding over the segment, and a grid with idle workgroups at its end all match the twin."""
    counts = (2500, 700) + (130,) * (L - 2)
    exact = dtype == "bf16"
    X, D, Y, seg, coef = _levels_case(L, counts, exact, seed=41)
    n_c, n_clip = _host_checks(X, D, seg, coef, L, counts)
    pc = _panel(X, D, Y, seg, dtype, "cpu")
    pg = _panel(X, D, Y, seg, dtype, gpu)
    rows = 2048 if exact else (1024 if L <= 4 else 512)
    assert DA.default_nbx(pg, L) == -(-2560 // rows) >= 2 and pg.seg_bounds[0, 1] == 2560
    c = torch.from_numpy(coef)
    want = DA.apo_moments(pc, c, L, CLIP)
    for nbx in (None, 1, 2, 7):
        got = DA.apo_moments(pg, c.to(gpu), L, CLIP, nbx=nbx)
        torch.cuda.synchronize()
        print(dtype, "L", L, "nbx", nbx)
        _check(got, want, L, len(Y), n_c, n_clip)


@pytest.mark.parametrize("L,counts", [(3, COUNTS), (8, COUNTS8)])
def test_apo_kernel_bf16_layouts_vs_twin(gpu, L, counts):
    X, D, Y, seg, coef = _levels_case(L, counts, exact=True)
    n_c, n_clip = _host_checks(X, D, seg, coef, L, counts)
    pc = _panel(X, D, Y, seg, "bf16", "cpu")
    # the stored values are the inputs: the grid is exact in bf16
    assert torch.equal(pc.data[pc.xcols].double()[:, pc.valid() != 0],
                       torch.from_numpy(X[pc.row_index[pc.valid() != 0].numpy()].T))
    cm = _panel(X, D, Y, seg, "bf16", gpu)
    c = torch.from_numpy(coef)
    want = DA.apo_moments(pc, c, L, CLIP)
    out = []
    for pan in (cm, _blocked(cm)):
        got = DA.apo_moments(pan, c.to(gpu), L, CLIP)
        torch.cuda.synchronize()
        _check(got, want, L, len(Y), n_c, n_clip)
        out.append(got.cpu())
    assert torch.equal(out[0], out[1])                    # the two layouts: the same bits


@pytest.mark.parametrize("dtype,exact", [("f64", False), ("bf16", True)])
def test_two_levels_share_bits_with_the_aipw_pass(gpu, dtype, exact):
    """L = 2 on the panel of test_gpu_irm._case with rows (g_0, g_1, m_0, m_1), m_0 with a
    support of its own: S 1{D=0}(y-g_0)^2, S 1{D=1}(y-g_1)^2, n and n_1 are moments [5], [4],
    [2] and [7] of irm_score_moments with rows (g_0, g_1, m_1) at the same nbx, bit for bit
    (the argument of csrc/apo.hip's header)."""
    X, W, Y, seg, c3 = _case(exact)
    rs = np.random.RandomState(3)
    coef = np.zeros((3, 4, P_X + 1))
    coef[:, 0], coef[:, 1], coef[:, 3] = c3[:, 0], c3[:, 1], c3[:, 2]
    on = np.unique(np.r_[EDGE, rs.choice(P_X, 20, replace=False)])
    coef[:, 2, 1 + on] = rs.randint(-9, 10, (3, len(on))) / 64.0
    coef[:, 2, 0] = 0.5
    m = _own_m(X, seg, coef, 2)
    assert min(np.abs(m - CLIP).min(), np.abs(m - (1 - CLIP)).min()) > 1e-6
    pan = _panel(X, W, Y, seg, dtype, gpu, W=W)           # W for the AIPW pass, D = W for ours
    pc = _panel(X, W, Y, seg, dtype, "cpu", W=W)
    c = torch.from_numpy(coef).to(gpu)
    lay = apo_layout(2)
    mine = [lay.level + 2, lay.level + 4 + 2, 0, lay.level + 4]
    want = DA.apo_moments(pc, torch.from_numpy(coef), 2, CLIP)
    pans = (pan, _blocked(pan)) if dtype == "bf16" else (pan,)
    for p in pans:
        for nbx in (None, 1):
            got = DA.apo_moments(p, c, 2, CLIP, nbx=nbx)
            base = DI.irm_score_moments(p, c[:, [0, 1, 3]].contiguous(), CLIP, 2, nbx=nbx)
            torch.cuda.synchronize()
            print(dtype, "blocked", p.blocked, "nbx", nbx, got[mine].tolist(),
                  base[[5, 4, 2, 7]].tolist())
            assert torch.equal(got[mine], base[[5, 4, 2, 7]])
            np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-11)


def test_entry_point_refusals(gpu):
    """L = 1, L = 9, seven segments at L = 3 and L = 8 with p = 1000 (LDS) are refused with a
    NativeError that names the entry point, and nothing is launched: the output and the
    partial buffer keep their bits."""
    X, D, Y, seg, coef = _levels_case(3, COUNTS, exact=False)
    pan = _panel(X, D, Y, seg, "f64", gpu)
    p = len(pan.xcols)
    xc = torch.tensor(list(pan.xcols) + [pan.xcols[0]] * (1000 - p), dtype=torch.int32, device=gpu)
    segs = torch.tensor(np.asarray(pan.seg_bounds[[0, 1, 2, 3, 4, 5, 0, 1]]), dtype=torch.int64,
                        device=gpu)
    big = torch.zeros(8 * 16 * 1001, dtype=torch.float64, device=gpu)   # room for any coef asked
    cs, bs = pan.strides()

    def call(L, nseg, p_, clip=CLIP):
        out = torch.full((128,), -7.0, dtype=torch.float64, device=gpu)
        partial = torch.full((8 * 128,), -7.0, dtype=torch.float64, device=gpu)
        with pytest.raises(_native.NativeError) as ei:
            _native.call("ate_apo_moments", dtype_code(pan.data), pan.data.data_ptr(), cs, bs,
                         xc.data_ptr(), p_, segs.data_ptr(), nseg, L, big.data_ptr(),
                         pan.cols["Y"], -1, pan.cols["D"], -1, pan.cols["one"], float(clip), 1,
                         partial.data_ptr(), out.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert "ate_apo_moments" in str(ei.value) and ei.value.status == -1, str(ei.value)
        assert (out == -7.0).all() and (partial == -7.0).all()

    call(1, 6, p)
    call(9, 9, p)
    call(3, 7, p)
    call(8, 8, 1000)              # 9 * 1001 * 8 + 4000 bytes of dynamic LDS: over 64 KB
    call(3, 6, p, clip=0.5)
    call(3, 6, p, clip=-0.1)
    # the launcher says the same through the public function
    c = torch.from_numpy(coef).to(gpu)
    for L in (1, 9, 4):
        with pytest.raises(_native.NativeError, match="ate_apo_moments"):
            DA.apo_moments(pan, c, L, CLIP)
    # and a valid call on the same buffers goes through
    got = DA.apo_moments(pan, c, 3, CLIP, nbx=1)
    torch.cuda.synchronize()
    assert got[0].item() == len(Y)


@pytest.fixture(scope="module")
def three_levels(tutorial):
    _, m, _ = tutorial
    arm = make_multiarm_data(len(m.Y), 1991, levels=3).D
    return m.Y, arm, m.X


def test_estimator_vs_reference(gpu, three_levels):
    Y, D, X = three_levels
    a = DA.dml_apos_lasso(Y, D, X, device=gpu, graph=False)
    torch.cuda.synchronize()
    b = E.dml_apos_lasso(Y, D, X)
    print("gpu", [(r.ate, r.se) for r in a.apo], a.diagnostics)
    print("ref", [(r.ate, r.se) for r in b.apo], b.diagnostics)
    # the bound of the IRM twin (tests/test_gpu_irm.py test_estimator_vs_reference)
    for x, y in zip(a.apo, b.apo):
        assert x.ate == pytest.approx(y.ate, abs=1e-6, rel=1e-6)
        assert x.se == pytest.approx(y.se, abs=1e-6, rel=1e-6)
    for ref in a.levels:
        for x, y in zip(a.contrasts(ref), b.contrasts(ref)):
            assert x.effect == pytest.approx(y.effect, abs=1e-6, rel=1e-6)
            assert x.se == pytest.approx(y.se, abs=1e-6, rel=1e-6)
    for k in ("n", "n_c", "n_clipped_c"):
        assert a.diagnostics[k] == b.diagnostics[k], k
    assert a.diagnostics["hipgraph"] is False


def test_graph_capture_and_replay(gpu, three_levels):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    Y, D, X = three_levels
    rs = np.random.RandomState(4)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DA.dml_apos_lasso(Y, D, X, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    for r in runs[1:]:
        assert r.moments == runs[0].moments and r.cov == runs[0].cov and r.crit == runs[0].crit
    # a new Y in the same layout (same folds and levels): a replay equals a fresh eager run
    Y2 = np.where(rs.rand(len(Y)) < 0.2, 1.0 - Y, Y)
    r4 = DA.dml_apos_lasso(Y2, D, X, device=gpu)
    torch.cuda.synchronize()
    e4 = DA.dml_apos_lasso(Y2, D, X, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert r4.moments == e4.moments and r4.moments != runs[0].moments
    estimator_graphs.clear()


def test_apos_bf16_vs_f64_panel(gpu):
    """Storage parity on a host-built 50,000 x 60 panel with four arms: every contrast and its
    SE keep the bounds of test_gpu_irm.test_irm_bf16_vs_f64_panel, and the counts that test
    compares (n and the rows per arm) are equal; the clip counts are printed."""
    d = make_multiarm_data(50_000, 2, levels=4, p_extra=39)
    assert d.X.shape == (50_000, 60)
    res = {}
    for dt in ("bf16", "f64"):
        pan, values, _, _, counts, n = DA.level_split_panel(d.Y, d.D, d.X, 5, 1991, dt, gpu)
        _, mom, _ = DA.apos_panel(pan, 5, 4, seg_counts=counts)
        torch.cuda.synchronize()
        res[dt] = ApoResult.from_moments(dt, mom.cpu().numpy(), values, n=n)
    rb, r64 = res["bf16"], res["f64"]
    for x, y in zip(rb.contrasts(), r64.contrasts()):
        print("contrast", x.level, "bf16", x.effect, x.se, "f64", y.effect, y.se, "dtheta/SE",
              abs(x.effect - y.effect) / y.se, "dSE/SE", abs(x.se - y.se) / y.se)
    for x, y in zip(rb.apo, r64.apo):
        print("apo bf16", x.ate, x.se, "f64", y.ate, y.se, "dtheta/SE", abs(x.ate - y.ate) / y.se)
    print("n_clipped_c bf16", rb.diagnostics["n_clipped_c"], "f64", r64.diagnostics["n_clipped_c"])
    for x, y in zip(rb.contrasts(), r64.contrasts()):
        assert abs(x.effect - y.effect) < 0.05 * y.se
        assert abs(x.se - y.se) < 0.02 * y.se
    assert rb.moments[0] == 50_000 == r64.moments[0]
    assert rb.diagnostics["n_c"] == r64.diagnostics["n_c"] == \
        [int(v) for v in np.bincount(d.D.astype(np.int64))]
