"""Row-chunk planners of the Gram (ops/gram.pair_chunks for the paired-tile bf16 kernel,
GramPlan's own loops for the other kernels and for the exact mode): pure host arithmetic,
so they are pinned on the CPU. The kernel's results do not depend on the plan beyond fp32
partial-sum order (tests/test_gpu.py and tests/test_gpu_gram_shapes.py check the Gram
values on a GPU; the latter relies on the stage counts pinned here)."""
import dataclasses

import numpy as np
import pytest

from ate_replication_causalml_amd.ops import gram as gram_op
from ate_replication_causalml_amd.ops.gram import pair_chunks
from ate_replication_causalml_amd.ops.panel import build_panel


def _check(seg_bounds, K, chunks, seg_chunk0):
    assert seg_chunk0[0] == 0 and seg_chunk0[-1] == len(chunks)
    for s, (r0, r1) in enumerate(seg_bounds):
        cs = chunks[seg_chunk0[s]:seg_chunk0[s + 1]]
        assert cs, "every segment gets at least one chunk"
        assert cs[0][0] == r0 and cs[-1][1] == r1
        for (a, e, seg, _), nxt in zip(cs, cs[1:] + [None]):
            assert seg == s and a <= e
            if nxt is not None:
                assert e == nxt[0] and (e - a) % K == 0   # contiguous, whole K-steps
        lens = [e - a for a, e, _, _ in cs[:-1]]
        if lens:
            assert max(lens) - min(lens) <= K              # near-equal


@pytest.mark.parametrize("nseg,rows,target,ncu,want", [
    (5, 2_000_000, 1280, 256, 1280),    # the bench shape: 5 whole rounds on 256 CUs
    (5, 2_000_000, 2048, 0, 2040),      # explicit target: 2 x 5 x 204
    (5, 2_000_000, 2048, 256, 1280),    # rounded down to whole rounds (k 204 -> 128)
    (10, 1_000_000, 1280, 256, 1280),
    (3, 3_000_000, 1280, 256, 768),
    (1, 10_000_000, 1280, 256, 1280),
])
def test_pair_chunks_counts(nseg, rows, target, ncu, want):
    segs = [(s * rows, (s + 1) * rows) for s in range(nseg)]
    chunks, c0 = pair_chunks(segs, 64, 2, target, ncu)
    assert 2 * len(chunks) == want
    _check(segs, 64, chunks, c0)


def test_pair_chunks_small_segments():
    # panels pad every segment to a positive multiple of 64 rows (ops/panel.py ROW_ALIGN)
    segs = [(0, 64), (64, 64 + 64 * 5), (384, 384 + 128)]
    chunks, c0 = pair_chunks(segs, 64, 2, 2048, 256)
    _check(segs, 64, chunks, c0)
    # a segment shorter than its chunk count gets one chunk per K-step
    assert [c0[s + 1] - c0[s] for s in range(3)] == [1, 5, 2]


@pytest.mark.parametrize("nt", [2, 3, 4])
def test_pair_tiles_cover_the_upper_triangle_once(nt):
    """Paired-tile slab table (csrc/gram.hip gram_bf16_pair_kernel): every 16-column block
    I <= J once (32 / 36 blocks per rectangle / triangle wave of a diagonal pair)."""
    from ate_replication_causalml_amd.ops.gram import PAIR_SLOTS, _pair_tiles
    tiles, blocks = _pair_tiles(nt)
    assert all(len(t) == PAIR_SLOTS for t in blocks)
    used = [b for t in blocks for b in t if b[0] >= 0]
    assert sorted(used) == [(i, j) for i in range(16 * nt) for j in range(i, 16 * nt)]


# ---------------------------------------------------------------- the non-pair and exact plans
STAGES = (1, 2, 3, 4, 7)            # 64-row stages per segment of the stage panel
# stages per chunk, segment by segment, at ATE_GRAM_WG = m x ntiles (64-row stages: the
# 64-tile kernels run four 16-row steps per stage)
STAGE_TABLE = {
    2: [[1], [2], [3], [4], [7]],
    5: [[1], [2], [3], [3, 1], [3, 3, 1]],
    8: [[1], [2], [2, 1], [2, 2], [2, 2, 2, 1]],
    17: [[1], [1] * 2, [1] * 3, [1] * 4, [1] * 7],
}
# the 64-tile kernels in 16-row steps: at m = 5 a chunk is 13 steps, no multiple of 64 rows
STEP_TABLE_M5 = [[4], [8], [12], [13, 3], [13, 13, 2]]
# (dtype, p, GRAM_KERNEL) -> (P, T, ntiles, K)
KERNELS = [
    ("bf16", 100, "pair", 128, 128, 1, 64),
    ("bf16", 150, "pair", 256, 256, 1, 64),
    ("bf16", 300, "pair", 384, 128, 6, 64),
    ("bf16", 700, "pair", 768, 256, 6, 64),
    ("bf16", 400, "tile256", 512, 256, 3, 64),
    ("f32", 150, "pair", 192, 64, 6, 16),
    ("f64", 20, "pair", 64, 64, 1, 16),
    ("f64", 150, "pair", 192, 64, 6, 16),
]


def _stage_panel(dtype, p):
    rs = np.random.RandomState(5)
    folds = np.repeat(np.arange(len(STAGES)), [64 * k for k in STAGES])
    n = len(folds)
    return build_panel(rs.randint(-2, 3, size=(n, p)), rs.randint(0, 2, n), rs.randint(-3, 4, n),
                       folds=folds, dtype=dtype, device="cpu")


def _plan_chunks(pl):
    """[(r0, r1, seg)] of a GramPlan's chunk table (the device struct, csrc/gram.hip Chunk)."""
    ch = pl.chunks.cpu().numpy().view([("r0", "<i8"), ("r1", "<i8"), ("seg", "<i4"),
                                       ("pad", "<i4")])
    return [(int(c["r0"]), int(c["r1"]), int(c["seg"])) for c in ch]


def _per_segment(pan, pl, unit):
    """Chunk lengths in ``unit`` rows, segment by segment, after checking that the chunks of a
    segment tile it in order (so none crosses a segment), that ``seg_chunk0`` names exactly
    them, and that every length is a whole number of the kernel's K-steps."""
    chunks = _plan_chunks(pl)
    c0 = [int(v) for v in pl.seg_chunk0.cpu()]
    assert len(c0) == pan.nseg + 1 and c0[0] == 0 and c0[-1] == len(chunks) == pl.nchunks
    out = []
    for s, (r0, r1) in enumerate(pan.seg_bounds):
        cs = chunks[c0[s]:c0[s + 1]]
        assert cs and cs[0][0] == r0 and cs[-1][1] == r1
        assert all(seg == s for _, _, seg in cs)
        assert all(a[1] == b[0] for a, b in zip(cs, cs[1:]))
        assert all(e > a and (e - a) % pl.K == 0 for a, e, _ in cs)
        out.append([(e - a) / unit for a, e, _ in cs])
    return out


@pytest.mark.parametrize("m", sorted(STAGE_TABLE))
@pytest.mark.parametrize("dtype,p,kernel,P,T,ntiles,K", KERNELS)
def test_stage_panel_plan(monkeypatch, dtype, p, kernel, P, T, ntiles, K, m):
    """The stage panel (segments of 1, 2, 3, 4 and 7 stages of 64 rows) under
    ATE_GRAM_WG = m x ntiles: the chunk lists that tests/test_gpu_gram_shapes.py runs the
    kernels at, for every kernel of the non-pair plan."""
    pan = _stage_panel(dtype, p)
    assert pan.P == P and [int(b - a) // 64 for a, b in pan.seg_bounds] == list(STAGES)
    monkeypatch.setattr(gram_op, "GRAM_KERNEL", kernel)
    monkeypatch.setenv("ATE_GRAM_WG", str(m * ntiles))
    pl = gram_op.GramPlan(pan, False)
    assert not pl.pair and (pl.T, pl.ntiles, pl.K) == (T, ntiles, K)
    if K == 16 and m == 5:
        assert _per_segment(pan, pl, 16) == STEP_TABLE_M5
    else:
        assert _per_segment(pan, pl, 64) == STAGE_TABLE[m]
    # workgroups: 5, 8, 10, 17 chunks x ntiles -- several below 8 or no multiple of 8
    assert pl.nchunks * ntiles == {2: 5, 5: 8, 8: 10, 17: 17}[m] * ntiles


@pytest.mark.parametrize("dtype,p,P,K", [("bf16", 100, 128, 64), ("bf16", 400, 512, 64),
                                         ("f32", 150, 192, 16), ("f64", 20, 64, 16)])
def test_exact_plan_blocks(dtype, p, P, K):
    """Exact mode: one chunk per 128-row block counted from the segment start, whatever the
    kernel (the paired-tile one at P = 512 included) -- two stages and a one-stage tail."""
    pan = dataclasses.replace(_stage_panel(dtype, p), exact_block=128)
    assert pan.P == P
    pl = gram_op.GramPlan(pan, False, exact=True)
    assert pl.K == K
    assert _per_segment(pan, pl, 64) == [[1], [2], [2, 1], [2, 2], [2, 2, 2, 1]]


@pytest.mark.parametrize("dtype,p,block", [("bf16", 100, 96), ("bf16", 400, 32), ("f64", 20, 24),
                                           ("f64", 20, 0)])
def test_exact_plan_refuses_unaligned_blocks(dtype, p, block):
    pan = dataclasses.replace(_stage_panel(dtype, p), exact_block=block)
    with pytest.raises(ValueError, match="block-aligned"):
        gram_op.GramPlan(pan, False, exact=True)


def test_weighted_bf16_plan_is_refused():
    with pytest.raises(ValueError, match="weighted Gram"):
        gram_op.GramPlan(_stage_panel("bf16", 100), True)
