"""Stage hand-off schedules of the paired-tile Gram (csrc/gram.hip gram_bf16_pair_kernel,
ops/gram.py GRAM_SCHED): every schedule the library holds besides "lockstep" keeps each
accumulator's k-order, so its Gram equals the lockstep schedule's BIT FOR BIT -- at every
stage count of a chunk (the rotated loop's head and tail, a warm-ahead touch clamped at the
chunk's end), in every wave role and layout and launch kind -- and, on small-integer panels
whose sums are exact in any order, equals the fp64 reference exactly (a stale or
half-overwritten LDS stage would not). Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.ops import gram as gram_op
from ate_replication_causalml_amd.ops.panel import build_panel

pytestmark = pytest.mark.gpu

NEW = [s for s in gram_op.SCHEDULES if s != "lockstep"]
STAGES = (1, 2, 3, 4, 7)            # 64-row stages per segment: one segment per fold


def _gram(monkeypatch, pan, sched, **kw):
    """The Gram of ``pan`` under schedule ``sched`` with a fresh plan (a clone: the plan owns
    the returned buffer)."""
    monkeypatch.setattr(gram_op, "GRAM_SCHED", sched)
    gram_op._plan_cache.clear()
    G = gram_op.gram(pan, **kw).clone()
    gram_op._plan_cache.clear()
    return G


def _stage_panel(gpu, p=400, seed=11):
    """Column-major bf16 panel (P = 512 for p = 400) whose segments hold exactly STAGES
    stages of 64 rows."""
    rs = np.random.RandomState(seed)
    folds = np.repeat(np.arange(len(STAGES)), [64 * k for k in STAGES])
    n = len(folds)
    return build_panel(rs.randn(n, p), rs.randint(0, 2, n), rs.rand(n), folds=folds,
                       dtype="bf16", device=gpu)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.mark.parametrize("chunks_per_seg", [1, 2])
@pytest.mark.parametrize("sched", NEW)
def test_stage_counts_same_bits_as_lockstep(gpu, monkeypatch, sched, chunks_per_seg):
    """Chunks of 1, 2, 3, 4 and 7 stages (one chunk per segment), then every segment cut in
    two (chunks of 1 ... 4 stages; the 1-stage segment stays whole): the 1-stage chunk is the
    rotated loop's tail alone, and there every warm-ahead distance exceeds the chunk, so each
    touch is clamped; at 2 stages a touch lands exactly on the chunk's last stage."""
    pan = _cached("stage", lambda: _stage_panel(gpu))
    assert pan.P == 512 and [int(b - a) // 64 for a, b in pan.seg_bounds] == list(STAGES)
    monkeypatch.setenv("ATE_GRAM_WG", str(2 * len(STAGES) * chunks_per_seg))
    gram_op._plan_cache.clear()
    pl = gram_op.plan_for(pan)
    assert pl.pair and pl.nchunks == (len(STAGES) if chunks_per_seg == 1 else 2 * len(STAGES) - 1)
    gram_op._plan_cache.clear()
    G0 = _cached(("stage", chunks_per_seg), lambda: _gram(monkeypatch, pan, "lockstep"))
    G1 = _gram(monkeypatch, pan, sched)
    assert torch.equal(G1, G0)


def _integer_panel(gpu, blocked):
    """Small-integer covariates, treatment and response: every product is an integer of
    magnitude <= 9 and a segment has < 2,000 rows, so every partial sum is an integer below
    2^15 << 2^24 -- fp32 accumulation is exact in any order. (The hi / lo copies of W and Y
    are the integers themselves and zeros.)"""
    rs = np.random.RandomState(23)
    n = 5000
    X = rs.randint(-2, 3, size=(n, 400)).astype(np.float64)
    pan = build_panel(X, rs.randint(0, 2, n), rs.randint(-3, 4, n), folds=rs.randint(0, 3, n),
                      dtype="bf16", device=gpu)
    if blocked:
        data = pan.data.reshape(pan.P, pan.ld // 64, 64).permute(1, 0, 2).contiguous()
        pan = dataclasses.replace(pan, data=data, blocked=True)
    return pan


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("sched", NEW)
def test_integer_panel_equals_reference_exactly(gpu, monkeypatch, sched, blocked):
    pan = _cached(("int", blocked), lambda: _integer_panel(gpu, blocked))
    assert pan.P == 512 and pan.blocked == blocked
    ref = _cached(("intref", blocked), lambda: gram_op.gram_reference(pan))
    # the reference of these inputs is integer-valued and far inside fp32's exact range
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2.0 ** 24
    monkeypatch.setenv("ATE_GRAM_WG", "24")          # 4 chunks per segment, ~6 stages each
    G = _gram(monkeypatch, pan, sched)
    assert torch.equal(G.cpu(), ref)


def _byte_panel(gpu, monkeypatch):
    from ate_replication_causalml_amd.data import device_dgp
    monkeypatch.setattr(device_dgp, "BYTE_PANEL", True)
    pan = device_dgp.synthetic_panel(40000, p=500, folds=5, seed=5, dtype="bf16", blocked=True,
                                     device=gpu, dgp="tutorial", align=4096)
    assert pan.P == 512 and pan.bytes8 is not None
    return pan


@pytest.mark.parametrize("sched", NEW)
def test_byte_panel_default_exact_and_weighted(gpu, monkeypatch, sched):
    """The blocked64 + bytes8 panel (the bench layout): default and exact launches of the
    paired kernel match lockstep bit for bit. A weighted Gram needs an fp32 / fp64 panel and
    runs the 64-tile kernel: the schedule switch must leave it alone."""
    pan = _cached("byte", lambda: _byte_panel(gpu, monkeypatch))
    monkeypatch.setattr(gram_op, "BYTE_COLS", True)
    G0, X0 = _cached("byte0", lambda: (_gram(monkeypatch, pan, "lockstep"),
                                       _gram(monkeypatch, pan, "lockstep", exact=True)))
    assert torch.equal(_gram(monkeypatch, pan, sched), G0)
    assert torch.equal(_gram(monkeypatch, pan, sched, exact=True), X0)
    monkeypatch.setattr(gram_op, "BYTE_COLS", False)   # the same columns read as bf16
    assert torch.equal(_gram(monkeypatch, pan, sched), G0)

    def wpanel():
        rs = np.random.RandomState(29)
        n = 3001
        p32 = build_panel(rs.randn(n, 60), rs.randint(0, 2, n), rs.rand(n),
                          folds=rs.randint(0, 3, n), dtype="f32", device=gpu)
        w = torch.rand(p32.ld, dtype=torch.float32, device=gpu)
        return p32, w, _gram(monkeypatch, p32, "lockstep", w=w)
    p32, w, W0 = _cached("weighted", wpanel)
    assert torch.equal(_gram(monkeypatch, p32, sched, w=w), W0)


@pytest.mark.parametrize("sched", NEW)
def test_four_tiles_same_bits_as_lockstep(gpu, monkeypatch, sched):
    """p = 1000 (P = 1024, four 256-column tiles): two diagonal pairs with their off-diagonal
    tiles and four more off-diagonal tiles that have no sibling workgroup."""
    def make():
        rs = np.random.RandomState(3)
        n = 6000
        return build_panel(rs.randn(n, 1000), rs.rand(n), rs.randint(0, 2, n),
                           folds=rs.randint(0, 5, n), dtype="bf16", device=gpu)
    pan = _cached("wide", make)
    assert pan.P == 1024
    gram_op._plan_cache.clear()
    assert gram_op.plan_for(pan).pair and gram_op.plan_for(pan).ntiles == 8
    G0 = _cached("wide0", lambda: _gram(monkeypatch, pan, "lockstep"))
    assert torch.equal(_gram(monkeypatch, pan, sched), G0)


@pytest.mark.parametrize("sched", NEW)
def test_two_launches_same_bits(gpu, monkeypatch, sched):
    """An LDS race shows as flicker between launches."""
    pan = _cached("byte", lambda: _byte_panel(gpu, monkeypatch))
    monkeypatch.setattr(gram_op, "GRAM_SCHED", sched)
    gram_op._plan_cache.clear()
    a = gram_op.gram(pan).clone()
    b = gram_op.gram(pan).clone()
    gram_op._plan_cache.clear()
    assert torch.equal(a, b)
