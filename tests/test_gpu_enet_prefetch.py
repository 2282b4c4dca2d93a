"""Mode S of the fp32 CV path kernel with and without the helper waves' column prefetch
(csrc/enet.hip enet_prefetch_s, ATE_ENET_S_PREFETCH).

While wave 0 walks a mode-S pass, waves 1..7 load the Gram columns of the coordinates about
to enter into the LDS column cache. A column holds the same floats wherever a mover reads it,
the order of moves is untouched, and the switch to mode L is decided from the ever-moved
count alone, so every output must be bit-identical with the prefetch on and off. Each case
runs the same cv.glmnet problem both ways in one process and compares every output with
torch.equal, and checks the run against the float64 CPU twin at the tolerances of
test_gpu_enet_modes.py (its _compare).

The shapes are the smallest at which this code takes its different paths: T = 1 and 2 sets
with a partial last set (a helper whose set is >= T does nothing, lanes past p are never
fetched), the whole path in mode S, the switch to mode L part-way, fold problems consuming a
source's lambdas, a full column cache, and a fold path cut short by a timed-out wait."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.ops import gram as gram_op
from ate_replication_causalml_amd.ops.enet import cv_enet_gaussian
from ate_replication_causalml_amd.ops.panel import build_panel
from ate_replication_causalml_amd.parallel import rng
from test_gpu_enet_modes import _compare, _problem

pytestmark = pytest.mark.gpu

FIELDS = ("lambdas", "coef_path", "cvm", "cvsd", "nlam", "npass", "fold_npass", "fold_nlam",
          "sel", "coef_min", "coef_1se")


def _run(gpu, X, y, nfolds=5, **kw):
    pan = build_panel(X, None, y, folds=rng.fold_ids(len(y), nfolds, 1), dtype="f32", device=gpu)
    G = gram_op.gram(pan)
    r = cv_enet_gaussian(G, pan, pan.xcols, [pan.cols["Y"]], **kw)
    torch.cuda.synchronize()
    return r, G, pan


def _same(a, b):
    for f in FIELDS:
        ta, tb = getattr(a, f), getattr(b, f)
        # NaN rows past nlam compare equal as bits
        assert torch.equal(ta.view(torch.int64) if ta.dtype == torch.float64 else ta,
                           tb.view(torch.int64) if tb.dtype == torch.float64 else tb), f


def _on_off(gpu, monkeypatch, X, y, alpha, pf=None, full_sets=None, nfolds=5, atol=2e-5):
    """The problem with the prefetch off, then on (through the CPU-twin comparison of
    test_gpu_enet_modes.py, which runs the same call): identical outputs."""
    kw = dict(penalty_factor=pf, alpha=alpha, full_sets=full_sets)
    monkeypatch.setenv("ATE_ENET_S_PREFETCH", "0")
    off, _, _ = _run(gpu, X, y, nfolds, **kw)
    monkeypatch.setenv("ATE_ENET_S_PREFETCH", "1")
    on, rc = _compare(gpu, X, y, alpha, pf=pf, full_sets=full_sets, nfolds=nfolds, atol=atol)
    torch.cuda.synchronize()
    _same(off.check(), on)
    return on, rc


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_prefetch_whole_path_in_mode_s(gpu, monkeypatch, alpha):
    """n 4000 / p 70, 4 signals, unpenalised last column: the whole path runs in mode S and
    the second set is partial."""
    X, y = _problem(4000, 70, 4, 11)
    pf = np.ones(70)
    pf[-1] = 0.0
    _on_off(gpu, monkeypatch, X, y, alpha, pf=pf)


@pytest.mark.parametrize("alpha", [1.0, 0.7])
def test_prefetch_mode_switch(gpu, monkeypatch, alpha):
    """n 6000 / p 300, 120 correlated signals: the switch to mode L happens part-way, at the
    same lambda with and without speculative slots in the cache."""
    X, y = _problem(6000, 300, 120, 12, corr=0.5)
    _on_off(gpu, monkeypatch, X, y, alpha, atol=5e-5)


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_prefetch_nested_crossfit_sets(gpu, monkeypatch, alpha):
    """n 5000 / p 130, nested cross-fit sets: fold problems prefetch with their source's
    lambda ratio while they consume its lambdas."""
    X, y = _problem(5000, 130, 10, 13, corr=0.3)
    K = 5
    full_sets = [[s for s in range(K) if s != k] for k in range(K)]
    on, rc = _on_off(gpu, monkeypatch, X, y, alpha, full_sets=full_sets, nfolds=K)
    assert torch.equal(on.sel.cpu().long(), rc.sel.long())


@pytest.mark.parametrize("p", [63, 64, 65])
def test_prefetch_set_boundaries(gpu, monkeypatch, p):
    """p = 63, 64, 65: T = 1 and 2 sets. Helpers whose set is >= T do nothing, and the lanes
    of the last set beyond p are never eligible, so never fetched."""
    X, y = _problem(3000, p, 12, 14 + p, corr=0.2)
    _on_off(gpu, monkeypatch, X, y, 1.0)


def _pressure(n=3000, p=512, k=200, seed=21):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, p)
    beta = np.zeros(p)
    beta[rs.permutation(p)[:k]] = rs.choice([-1.0, 1.0], k) * 0.5
    return X, X @ beta + rs.randn(n)


def test_prefetch_cache_pressure(gpu, monkeypatch):
    """p = 512 (PMAX), 200 equal-strength signals, 8 lambdas down to 1e-3 lambda_max: on the
    float64 CPU twin the full problem's support is 0, 195, 200, 210, 313, 412, 468, 493 along
    the path, so 195 coordinates make their first move inside lambda 1, all of it in mode S
    (the switch is only decided at the next lambda's start): the ever-moved count passes
    S_CAP = 56 within one lambda. The helpers hit their speculative share, the cache fills,
    wave 0 falls back to reading rows of C directly, and the switch rule runs at its S_CAP
    clamp."""
    X, y = _pressure()
    kw = dict(nlambda=8, lambda_min_ratio=1e-3)
    monkeypatch.setenv("ATE_ENET_S_PREFETCH", "0")
    off, G, pan = _run(gpu, X, y, **kw)
    monkeypatch.setenv("ATE_ENET_S_PREFETCH", "1")
    on = cv_enet_gaussian(G, pan, pan.xcols, [pan.cols["Y"]], **kw)
    torch.cuda.synchronize()
    _same(off.check(), on.check())
    # the CPU twin, as test_gpu_enet_modes._compare does it (which cannot pass nlambda)
    rc = cv_enet_gaussian(G.cpu(), pan, pan.xcols, [pan.cols["Y"]], **kw)
    nl = int(rc.nlam[0])
    assert nl == 8 and abs(int(on.nlam[0]) - nl) <= 1
    nl = min(nl, int(on.nlam[0]))
    support = (rc.coef_path[0, :nl, 1:] != 0).sum(1)
    assert int(support[1]) > 56, "the input no longer fills the column cache in one lambda"
    np.testing.assert_allclose(on.lambdas[0, :nl].cpu().numpy(), rc.lambdas[0, :nl].numpy(),
                               rtol=1e-6)
    scale = np.abs(rc.coef_path[0, :nl].numpy()).max() + 1.0
    np.testing.assert_allclose(on.coef_path[0, :nl].cpu().numpy(), rc.coef_path[0, :nl].numpy(),
                               atol=2e-5 * scale)
    np.testing.assert_allclose(on.cvm[0, :nl].cpu().numpy(), rc.cvm[0, :nl].numpy(), rtol=1e-4)


def test_prefetch_fold_wait_timeout(gpu, monkeypatch):
    """A zero spin bound with the prefetch on: fold paths end early at their first wait, the
    launch still comes back with those folds flagged (npass = -1) and the selection poisoned,
    and the next, clean launch on the same stream is the prefetch-off result bit for bit
    (nothing of the cut-short launch was left in flight)."""
    from ate_replication_causalml_amd.utils.guards import NumericalError
    X, y = _problem(4000, 120, 6, 17)
    monkeypatch.setenv("ATE_ENET_S_PREFETCH", "0")
    off, G, pan = _run(gpu, X, y, nfolds=10)
    monkeypatch.setenv("ATE_ENET_S_PREFETCH", "1")
    monkeypatch.setenv("ATE_ENET_SPIN_MAX", "0")
    r = cv_enet_gaussian(G, pan, pan.xcols, [pan.cols["Y"]])
    torch.cuda.synchronize()
    assert (r.fold_npass < 0).any(), "no fold wait timed out with a zero spin bound"
    assert torch.isnan(r.cvm).all() and torch.isnan(r.coef_min).all()
    with pytest.raises(NumericalError):
        r.check()
    monkeypatch.delenv("ATE_ENET_SPIN_MAX")
    on, rc = _compare(gpu, X, y, 1.0, nfolds=10)
    torch.cuda.synchronize()
    _same(off.check(), on)
