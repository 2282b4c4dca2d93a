"""GPU tests of the group-effect estimator (estimators/gate.py): the per-row score entry
point of csrc/irm.hip against its float64 torch twin and against the moment entry point,
the grouped multiplier-bootstrap kernel (csrc/gate.hip) against a numpy twin at every launch
shape it has, the estimator against the row-by-row reference twin, and hipGraph capture and
replay with the group codes as a graph input. Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.estimators import gate as DG
from ate_replication_causalml_amd.estimators import irm as DI
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel import rng
from ate_replication_causalml_amd.reference import estimators as E

pytestmark = pytest.mark.gpu

COUNTS = (130, 7, 64, 1, 257, 70)   # the layout of tests/test_gpu_irm.py: 529 rows in 832
P_X = 300
CLIP = 0.2
RID0 = 2 ** 33                      # global row ids beyond 32 bits


def _case(exact: bool):
    """Host arrays of the kernel tests (as tests/test_gpu_irm.py builds them): 3 folds
    arm-split into 6 segments of COUNTS rows, ~40 nonzero coefficients incl. columns 0, 255,
    256, 299, fold 1 intercept-only. ``exact``: x on a 1/8 grid in [-4, 4] and coefficients on
    a 2^-6 grid, so every fp32 partial sum of the bf16 kernel is exact."""
    rs = np.random.RandomState(17)
    seg = np.repeat(np.arange(6), COUNTS)
    perm = rs.permutation(len(seg))
    seg = seg[perm]
    n = len(seg)
    W = (seg & 1).astype(float)
    if exact:
        X = rs.randint(-32, 33, size=(n, P_X)) / 8.0
        Y = rs.randint(0, 2, n).astype(float)
    else:
        X = rs.randn(n, P_X)
        Y = rs.randn(n) + W
    support = np.unique(np.r_[0, 255, 256, 299, rs.choice(P_X, 36, replace=False)])
    coef = np.zeros((3, 3, P_X + 1))
    for k in (0, 2):
        for r in range(3):
            on = support[rs.rand(len(support)) < 0.6]
            if exact:
                coef[k, r, 1 + on] = rs.randint(-9, 10, len(on)) / 64.0
            else:
                coef[k, r, 1 + on] = rs.randn(len(on)) * (0.1 if r == 2 else 0.5)
        coef[k, :, 1 + np.array([0, 255, 256, 299])] = (np.array([[3, -5, 2], [-4, 6, 1],
                                                                  [7, 2, -3], [-2, -7, 4]]) / 64.0)
    coef[:, 0, 0], coef[:, 1, 0], coef[:, 2, 0] = 0.25, 0.75, 0.5
    return X, W, Y, seg, coef


# ---------------------------------------------------------------- ate_irm_scores
def test_scores_kernel_f64_vs_twin(gpu):
    X, W, Y, seg, coef = _case(exact=False)
    pc = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    pg = build_panel(X, W, Y, folds=seg, dtype="f64", device=gpu)
    assert tuple(pg.seg_nreal) == COUNTS and pg.ld == 832
    c = torch.from_numpy(coef)
    want = DI.irm_scores(pc, c, CLIP, 2)
    pad = pc.row_index < 0
    assert int(pad.sum()) == 832 - 529 and torch.all(want[pad] == 0)
    for nbx in (None, 1):
        got = DI.irm_scores(pg, c.to(gpu), CLIP, 2, nbx=nbx)
        mom = DI.irm_score_moments(pg, c.to(gpu), CLIP, 2, nbx=nbx)
        torch.cuda.synchronize()
        got, mom = got.cpu(), mom.cpu()
        rel = ((got - want).abs() / want.abs().clamp(min=1e-300))[~pad]
        print("nbx", nbx, "max row rel err", rel.max().item(), "min |psi|", want[~pad].abs().min().item())
        assert got.shape == (832,) and got.dtype == torch.float64
        assert torch.all(got[pad] == 0)                       # padding rows: exactly 0
        np.testing.assert_allclose(got[~pad].numpy(), want[~pad].numpy(), rtol=1e-11)
        # the two entry points compute the same psi
        assert got.sum().item() == pytest.approx(mom[0].item(), rel=1e-12)
        assert (got * got).sum().item() == pytest.approx(mom[1].item(), rel=1e-12)
    # a plain K-fold reading of the same panel: one coefficient block per segment
    c6 = torch.from_numpy(np.repeat(coef, 2, axis=0))
    got = DI.irm_scores(pg, c6.to(gpu), CLIP, 1).cpu()
    np.testing.assert_allclose(got.numpy(), DI.irm_scores(pc, c6, CLIP, 1).numpy(), rtol=1e-11)


def test_scores_kernel_bf16_layouts(gpu):
    X, W, Y, seg, coef = _case(exact=True)
    pc = build_panel(X, W, Y, folds=seg, dtype="bf16", device="cpu")
    cm = build_panel(X, W, Y, folds=seg, dtype="bf16", device=gpu)
    bl = dataclasses.replace(
        cm, data=cm.data.reshape(cm.P, cm.ld // 64, 64).permute(1, 0, 2).contiguous(), blocked=True)
    assert bl.strides() == (64, 64 * cm.P)
    c = torch.from_numpy(coef)
    want = DI.irm_scores(pc, c, CLIP, 2)
    pad = pc.row_index < 0
    out = []
    for pan in (cm, bl):
        got = DI.irm_scores(pan, c.to(gpu), CLIP, 2)
        mom = DI.irm_score_moments(pan, c.to(gpu), CLIP, 2)
        torch.cuda.synchronize()
        got, mom = got.cpu(), mom.cpu()
        assert torch.all(got[pad] == 0)
        # exact grid: the fp32 dots are exact, so the rows meet the f64 bound
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-11)
        assert got.sum().item() == pytest.approx(mom[0].item(), rel=1e-12)
        assert (got * got).sum().item() == pytest.approx(mom[1].item(), rel=1e-12)
        out.append(got)
    assert torch.equal(out[0], out[1])                        # the two layouts: the same bits


# ---------------------------------------------------------------- ate_group_boot
def _boot_twin(psi, gid, rid, G, B, seed):
    """numpy twin of csrc/gate.hip: (mom [G, 3], A [B, G], Z [B, G] int64, S|psi| [G])."""
    keep = gid >= 0
    p, g, r = psi[keep], gid[keep].astype(np.int64), rid[keep]
    mom = np.stack([np.bincount(g, minlength=G).astype(float), np.bincount(g, weights=p, minlength=G),
                    np.bincount(g, weights=p * p, minlength=G)], axis=1)
    A = np.zeros((B, G))
    Z = np.zeros((B, G), dtype=np.int64)
    for i0 in range(0, len(p), 4096):
        sl = slice(i0, i0 + 4096)
        xi = rng.rademacher(seed, r[sl], B)
        oh = np.zeros((len(p[sl]), G))
        oh[np.arange(len(p[sl])), g[sl]] = 1.0
        A += xi.T.astype(np.float64) @ (oh * p[sl, None])
        Z += xi.T.astype(np.int64) @ oh.astype(np.int64)
    return mom, A, Z, np.bincount(g, weights=np.abs(p), minlength=G)


def _check_boot(gpu, psi, gid, rid, G, B, seed, nbx=None, twin=None):
    args = (torch.from_numpy(psi).to(gpu), torch.from_numpy(gid.astype(np.int32)).to(gpu),
            torch.from_numpy(rid.astype(np.int64)).to(gpu), G, B, seed)
    a = DG.group_boot(*args, nbx=nbx)
    b = DG.group_boot(*args, nbx=nbx)
    torch.cuda.synchronize()
    a, b = a.cpu(), b.cpu()
    assert torch.equal(a, b)                                  # one geometry, one set of bits
    mom, A, Z = (t.numpy() for t in DG.split_boot(a, G, B))
    mom_r, A_r, Z_r, sabs = twin if twin is not None else _boot_twin(psi, gid, rid, G, B, seed)
    assert np.array_equal(mom[:, 0], mom_r[:, 0])             # n_g exact
    assert np.array_equal(Z, Z_r.astype(np.float64))          # Z exact
    assert np.abs(Z).max() > 0 or B * G < 4
    np.testing.assert_allclose(mom, mom_r, rtol=1e-11)
    err = np.abs(A - A_r) / sabs[None, :]
    print("G", G, "B", B, "nbx", nbx, "max |A - A_ref| / S|psi|", err.max(),
          "geometry", DG.boot_geometry(B, G, len(psi)))
    assert np.all(np.abs(A - A_r) <= 1e-11 * sabs[None, :])
    return a


# (G, B): 5 groups at 2 streams in a 64-thread workgroup and at one replicate; the register /
# slab threshold (8 | 9 groups); 9 streams: 256 threads and a second stream block with one
# stream in use; 24 groups: more moment slots (72) than threads (64)
@pytest.mark.parametrize("G,B", [(5, 200), (5, 1), (8, 1100), (9, 130), (24, 64)])
def test_group_boot_small_layout(gpu, G, B):
    X, W, Y, seg, coef = _case(exact=False)
    pc = build_panel(X, W, Y, folds=seg, dtype="f64", device="cpu")
    psi = DI.irm_scores(pc, torch.from_numpy(coef), CLIP, 2).numpy()
    rix = pc.row_index.numpy()
    real = np.flatnonzero(rix >= 0)
    rs = np.random.RandomState(5)
    gid = np.full(pc.ld, -1, dtype=np.int32)
    gid[real] = rs.randint(2, G, len(real))
    r0, r1 = (int(v) for v in pc.seg_bounds[2])
    gid[gid == 1] = 2
    gid[r0 + 3:r0 + 40] = 1                                   # group 1: inside segment 2 only
    gid[real[rs.choice(len(real), 30, replace=False)]] = -1   # real rows left out
    gid[gid == 0] = 2
    gid[[real[0], real[-1]]] = 0                              # group 0: exactly 2 rows, far apart
    cnt = np.bincount(gid[gid >= 0], minlength=G)
    assert cnt[0] == 2 and cnt.min() >= 2 and len(cnt) == G and (gid[real] < 0).sum() >= 20
    assert np.all(np.flatnonzero(gid == 1) >= r0) and np.all(np.flatnonzero(gid == 1) < r1)
    rid = np.where(rix >= 0, rix + RID0, -1)
    twin = _boot_twin(psi, gid, rid, G, B, 1991)              # computed once, shared
    for nbx in (None, 1, 3):
        _check_boot(gpu, psi, gid, rid, G, B, 1991, nbx=nbx, twin=twin)


def test_group_boot_many_groups_many_chunks(gpu):
    n, G, B = 70_000, 64, 384                                 # 547 chunks of 128 rows
    rs = np.random.RandomState(9)
    psi = rs.standard_t(5, n) * 3 + 0.1
    gid = rs.randint(0, G, n).astype(np.int32)
    gid[rs.rand(n) < 0.01] = -1
    rid = rs.permutation(n).astype(np.int64) + RID0
    ch, nby, nbx = DG.boot_geometry(B, G, n)
    assert -(-n // ch) >= 3 * nbx and nbx > 1                 # several chunks per workgroup
    twin = _boot_twin(psi, gid, rid, G, B, 7)                 # computed once, shared
    a = _check_boot(gpu, psi, gid, rid, G, B, 7, twin=twin)
    # another geometry: the same sums to the bound, and Z to the bit
    b = _check_boot(gpu, psi, gid, rid, G, B, 7, nbx=37, twin=twin)
    assert torch.equal(a[3 * G + B * G:], b[3 * G + B * G:])


# ---------------------------------------------------------------- estimator
def _quartiles(x):
    return np.digitize(x, np.quantile(x, [0.25, 0.5, 0.75]))


def test_estimator_vs_reference(gpu, tutorial):
    _, m, _ = tutorial
    lab = _quartiles(m.X[:, 0])
    a = DG.dml_irm_gate_lasso(m.Y, m.W, m.X, lab, n_boot=999, device=gpu, graph=False)
    torch.cuda.synchronize()
    b = E.dml_irm_gate(m.Y, m.W, m.X, lab, n_boot=999)
    print("gpu", a.ate, a.se, a.crit, "reference", b.ate, b.se, b.crit)
    assert a.labels == b.labels and a.n == b.n
    for g in range(4):
        assert a.ate[g] == pytest.approx(b.ate[g], abs=1e-6, rel=1e-6)
        assert a.se[g] == pytest.approx(b.se[g], abs=1e-6, rel=1e-6)
    assert abs(a.crit - b.crit) < 1e-4
    assert a.overall.ate == pytest.approx(b.overall.ate, abs=1e-6, rel=1e-6)


def test_graph_capture_and_replay(gpu, tutorial):
    from ate_replication_causalml_amd.utils.graphs import estimator_graphs
    _, m, _ = tutorial
    lab = _quartiles(m.X[:, 0])
    key = lambda r: (r.ate, r.se, r.crit, r.n, r.overall.ate, r.overall.se)
    estimator_graphs.clear()          # the cache is keyed by layout: start from "never seen"
    runs = []
    for _ in range(3):
        r = DG.dml_irm_gate_lasso(m.Y, m.W, m.X, lab, device=gpu)
        torch.cuda.synchronize()
        runs.append(r)
    assert [r.diagnostics["hipgraph"] for r in runs] == [False, True, True]
    assert key(runs[1]) == key(runs[0]) and key(runs[2]) == key(runs[0])
    # other groups in the same layout: a replay equals a fresh eager run
    lab2 = np.random.RandomState(4).permutation(lab)
    r4 = DG.dml_irm_gate_lasso(m.Y, m.W, m.X, lab2, device=gpu)
    torch.cuda.synchronize()
    e4 = DG.dml_irm_gate_lasso(m.Y, m.W, m.X, lab2, device=gpu, graph=False)
    torch.cuda.synchronize()
    assert r4.diagnostics["hipgraph"] is True and e4.diagnostics["hipgraph"] is False
    assert key(r4) == key(e4) and r4.ate != runs[0].ate
    # the same rows regrouped: the overall ATE is the same sum in another order
    assert r4.overall.ate == pytest.approx(runs[0].overall.ate, rel=1e-12)
    assert r4.overall.se == pytest.approx(runs[0].overall.se, rel=1e-12)
    estimator_graphs.clear()
