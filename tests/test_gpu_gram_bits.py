"""Bit columns of the paired-tile Gram (csrc/gram.hip COL_BITS, DevicePanel.bits1): the 128
{0, 1} columns of a P = 512 blocked bf16 panel streamed as bits must give the SAME BITS as
the byte path (a panel built with ATE_PANEL_BITS=0) -- Gram, exact-mode limbs, DML result --
under both schedules, at chunks of one and of several stages, with tiles and reduce run split
and together; on integer panels the Gram must equal the fp64 reference. Run on the MI355X
box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.data import device_dgp
from ate_replication_causalml_amd.ops import gram as gram_op
from ate_replication_causalml_amd.ops.panel import empty_panel

pytestmark = pytest.mark.gpu

STAGES = (1, 2, 3, 4, 7)            # 64-row stages per segment (tests/test_gpu_gram_shapes.py)
ROWS = 64 * sum(STAGES)             # 1,088
SCHEDS = ["lockstep", "stagger"]
# ATE_GRAM_WG -> chunks per segment 1, 2 and 7: chunks of 1..7 stages, 1..4 stages, 1 stage
WGS = {10: [[1], [2], [3], [4], [7]], 20: [[1], [1, 1], [1, 2], [2, 2], [3, 4]],
       70: [[1] * k for k in STAGES]}

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _stage_segments(pan):
    """``pan`` (one segment of 1,088 real rows) cut into segments of 1, 2, 3, 4 and 7 stages;
    64-row blocks for the exact mode."""
    assert pan.ld == ROWS and pan.nseg == 1
    ends = np.cumsum([64 * k for k in STAGES])
    bounds = np.stack([ends - [64 * k for k in STAGES], ends], axis=1)
    return dataclasses.replace(pan, seg_bounds=bounds, seg_nreal=bounds[:, 1] - bounds[:, 0],
                               identity=False, exact_block=64)


def _synthetic(gpu, monkeypatch, bits, n=ROWS, folds=1, **kw):
    monkeypatch.setattr(device_dgp, "BYTE_PANEL", True)
    monkeypatch.setattr(device_dgp, "BIT_PANEL", bits)
    pan = device_dgp.synthetic_panel(n, p=500, folds=folds, seed=13, dtype="bf16", blocked=True,
                                     device=gpu, **kw)
    assert pan.P == 512 and pan.blocked and pan.bytes8 is not None
    assert (pan.bits1 is not None) == bits
    return pan


def _stage_pair(gpu, monkeypatch):
    """(bits panel, byte panel built with the switch off) on the 1,088-row stage shape."""
    def make():
        a = _stage_segments(_synthetic(gpu, monkeypatch, True, dgp="rct"))
        b = _stage_segments(_synthetic(gpu, monkeypatch, False, dgp="rct"))
        assert torch.equal(a.data, b.data) and torch.equal(a.bytes8, b.bytes8)
        return a, b
    return _cached("stage", make)


def _hand_panel(gpu, counts, seed=3):
    """Integer panel in the byte-panel layout made by hand: columns 0..383 in {-2..2}, columns
    384..511 in {0, 1}, padding rows zero; bytes8 in the order of csrc/dgp.hip x8_pos and
    bits1 packed from it. Every product is an integer of magnitude <= 4 and a segment has
    < 2,000 rows: every partial sum (scaled by 0.25 .. 4) is exact in fp32 in any order."""
    rs = np.random.RandomState(seed)
    pan = empty_panel(counts, 512, dtype="bf16", device=gpu, blocked=True)
    cm = np.zeros((512, pan.ld))
    for (r0, _), c in zip(pan.seg_bounds, counts):
        cm[:384, r0:r0 + c] = rs.randint(-2, 3, size=(384, c))
        cm[384:, r0:r0 + c] = rs.randint(0, 2, size=(128, c))
    t = torch.from_numpy(cm).to(gpu)
    data = t.reshape(512, -1, 64).permute(1, 0, 2).contiguous().to(torch.bfloat16)
    r = torch.arange(64, device=gpu)
    pos = ((r >> 3) & 3) * 16 + (r >> 5) * 8 + (r & 7)
    ones = (t[384:] != 0).reshape(128, -1, 64).permute(1, 0, 2)
    bytes8 = torch.zeros(ones.shape, dtype=torch.uint8, device=gpu)
    bytes8[:, :, pos] = ones.to(torch.uint8) * 0x3F
    bytes8 = bytes8.contiguous()
    return dataclasses.replace(pan, data=data, bytes8=bytes8, bits1=device_dgp.pack_bits(bytes8))


def _no_bits(pan):
    return dataclasses.replace(pan, bits1=None)


def _gram(monkeypatch, pan, sched, wg=None, stage="all", **kw):
    """The Gram of ``pan`` with a fresh plan (cloned: the plan owns its buffer; an ``out=``
    buffer comes back as it is). stage "split": tiles and reduce as two calls."""
    monkeypatch.setattr(gram_op, "GRAM_KERNEL", "pair")
    monkeypatch.setattr(gram_op, "GRAM_SCHED", sched)
    monkeypatch.setattr(gram_op, "BYTE_COLS", True)
    if wg is None:
        monkeypatch.delenv("ATE_GRAM_WG", raising=False)
    else:
        monkeypatch.setenv("ATE_GRAM_WG", str(wg))
    gram_op._plan_cache.clear()
    pl = gram_op.plan_for(pan, exact=kw.get("exact", False))
    assert pl.pair and pl.ntiles == 2
    if stage == "split":
        gram_op.gram(pan, stage="tiles", **kw)
        G = gram_op.gram(pan, stage="reduce", **kw)
    else:
        G = gram_op.gram(pan, **kw)
    if kw.get("out") is None:
        G = G.clone()
    gram_op._plan_cache.clear()
    return G, pl


def _chunk_stages(pl):
    ch = pl.chunks.cpu().numpy().view([("r0", "<i8"), ("r1", "<i8"), ("seg", "<i4"),
                                       ("pad", "<i4")])
    c0 = [int(v) for v in pl.seg_chunk0.cpu()]
    return [[int(c["r1"] - c["r0"]) // 64 for c in ch[c0[s]:c0[s + 1]]]
            for s in range(len(c0) - 1)]


# ---------------------------------------------------------------- the image itself
def test_bit_image_equals_byte_copy(gpu, monkeypatch):
    a, _ = _stage_pair(gpu, monkeypatch)
    big = _cached("dml", lambda: _synthetic(gpu, monkeypatch, True, n=20000, folds=5,
                                            dgp="tutorial"))
    r = torch.arange(64, device=gpu)
    pos = ((r >> 3) & 3) * 16 + (r >> 5) * 8 + (r & 7)       # csrc/dgp.hip x8_pos
    for pan in (a, big):
        assert pan.bits1.shape == (pan.ld // 64, 1024) and pan.bits1.dtype == torch.uint8
        want = (pan.bytes8[:, :, pos] != 0).to(torch.uint8)          # [block, column, row]
        assert torch.equal(device_dgp.unpack_bits(pan.bits1), want)
        assert int(want.sum()) > 0
    # the native pack against the host twin, one block
    blk = (a.bytes8[3][:, pos] != 0).to(torch.uint8).cpu().numpy()
    assert np.array_equal(a.bits1[3].cpu().numpy(), device_dgp.pack_bits_block(blk))


# ---------------------------------------------------------------- same bits as the byte path
@pytest.mark.parametrize("wg", sorted(WGS))
@pytest.mark.parametrize("sched", SCHEDS)
def test_gram_same_bits_as_byte_path(gpu, monkeypatch, sched, wg):
    a, b = _stage_pair(gpu, monkeypatch)
    G0, pl0 = _cached(("bytes", sched, wg), lambda: _gram(monkeypatch, b, sched, wg))
    assert _chunk_stages(pl0) == WGS[wg]
    G1, pl1 = _gram(monkeypatch, a, sched, wg)
    assert _chunk_stages(pl1) == WGS[wg]
    assert torch.equal(G1, G0)
    assert torch.equal(G1, G1.transpose(1, 2))
    G2, _ = _gram(monkeypatch, a, sched, wg, stage="split")
    assert torch.equal(G2, G0)
    # the same panel object with its bit image dropped takes the byte path as well
    G3, _ = _gram(monkeypatch, _no_bits(a), sched, wg)
    assert torch.equal(G3, G0)


@pytest.mark.parametrize("sched", SCHEDS)
def test_exact_limbs_same_as_byte_path(gpu, monkeypatch, sched):
    """Exact mode: one chunk per 64-row block, the partials summed as int64 limbs."""
    a, b = _stage_pair(gpu, monkeypatch)
    X0, pl = _gram(monkeypatch, b, sched, exact=True, checked=True)
    assert _chunk_stages(pl) == WGS[70]
    X1, _ = _gram(monkeypatch, a, sched, exact=True, checked=True)
    assert X1.dtype == torch.int64 and torch.equal(X1, X0)
    X2, _ = _gram(monkeypatch, a, sched, exact=True, checked=True, stage="split")
    assert torch.equal(X2, X0)


# ---------------------------------------------------------------- exact on integers
def _int_case(gpu, key, counts):
    def make():
        pan = _hand_panel(gpu, counts)
        ref = gram_op.gram_reference(pan)
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2.0 ** 15
        return pan, ref
    return _cached(("int", key), make)


@pytest.mark.parametrize("wg", sorted(WGS))
@pytest.mark.parametrize("sched", SCHEDS)
def test_integer_panel_equals_reference_and_is_fully_written(gpu, monkeypatch, sched, wg):
    pan, ref = _int_case(gpu, "stage", [64 * k for k in STAGES])
    out = torch.full((pan.nseg, 512, 512), float("nan"), dtype=torch.float64, device=gpu)
    G, pl = _gram(monkeypatch, pan, sched, wg, out=out)
    assert _chunk_stages(pl) == WGS[wg]
    assert G is out and not bool(torch.isnan(out).any())
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(out, out.transpose(1, 2))


@pytest.mark.parametrize("sched", SCHEDS)
def test_partial_last_block_and_empty_segment(gpu, monkeypatch, sched):
    """63 real rows (one block, one padding row), 65 (a second block with one real row) and
    an empty segment (one block of padding): padding rows hold zero bits."""
    pan, ref = _int_case(gpu, "partial", [63, 65, 0])
    assert [int(b - a) for a, b in pan.seg_bounds] == [64, 128, 64]
    assert int(device_dgp.unpack_bits(pan.bits1)[-1].sum()) == 0
    G1, _ = _gram(monkeypatch, pan, sched, 12)
    assert torch.equal(G1.cpu(), ref) and not bool(G1[2].any())
    G0, _ = _gram(monkeypatch, _no_bits(pan), sched, 12)
    assert torch.equal(G1, G0)


# ---------------------------------------------------------------- the estimator on top
def test_dml_call_same_result_as_byte_path(gpu, monkeypatch):
    from ate_replication_causalml_amd.estimators.lasso import dml_crossfit_panel
    a = _cached("dml", lambda: _synthetic(gpu, monkeypatch, True, n=20000, folds=5,
                                          dgp="tutorial"))
    b = _synthetic(gpu, monkeypatch, False, n=20000, folds=5, dgp="tutorial")
    monkeypatch.setattr(gram_op, "BYTE_COLS", True)
    out = []
    for pan in (a, b):
        gram_op._plan_cache.clear()
        res, mom, _ = dml_crossfit_panel(pan, 5)
        out.append((res.clone(), mom.clone()))
    gram_op._plan_cache.clear()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][0]).all()) and float(out[0][0][1]) > 0


def test_graph_replay_takes_the_new_panels_bits(gpu, monkeypatch):
    """A captured step replayed with a second panel of the same layout copies that panel's
    data, byte copy AND bit image into the captured buffers: its result is the second
    panel's own, not the first one's."""
    from ate_replication_causalml_amd.estimators.lasso import _dml_body, dml_crossfit_panel
    from ate_replication_causalml_amd.utils.graphs import GraphCache, layout_key
    monkeypatch.setattr(gram_op, "BYTE_COLS", True)
    kw = dict(p=500, folds=5, dtype="bf16", blocked=True, device=gpu, dgp="rct")
    monkeypatch.setattr(device_dgp, "BYTE_PANEL", True)
    monkeypatch.setattr(device_dgp, "BIT_PANEL", True)
    a = device_dgp.synthetic_panel(20000, seed=21, **kw)
    b = device_dgp.synthetic_panel(20000, seed=22, **kw)
    assert layout_key(a) == layout_key(b) and not torch.equal(a.bits1, b.bits1)
    want_a = dml_crossfit_panel(a, 5)[0].clone()
    want_b = dml_crossfit_panel(b, 5)[0].clone()
    assert not torch.equal(want_a, want_b)
    cache = GraphCache()
    args = (5, "min", None, None)
    r1, g1 = cache.run("dml_plr", _dml_body, (a,), *args)        # eager
    assert not g1 and torch.equal(r1, want_a)
    r2, g2 = cache.run("dml_plr", _dml_body, (a,), *args)        # captured and replayed
    assert g2 and torch.equal(r2, want_a)
    r3, g3 = cache.run("dml_plr", _dml_body, (b,), *args)        # replayed on b's copy
    assert g3 and torch.equal(r3, want_b)
    cache.clear()
    gram_op._plan_cache.clear()
