"""The Gram kernels (csrc/gram.hip, ops/gram.py, K01) at their edge shapes, each against a
plain fp64 reference of the same operation.

The workload-shaped tests cut every chunk of the non-pair kernels to ONE 64-row stage (a
chunk holds more only above ~131,072 .. 393,216 rows), so the double-buffered K-loops of
``gram_bf16_kernel`` and ``gram_bf16_256_kernel`` -- the prefetch of stage s + 1, the store
into the other buffer, the wait before the barrier -- and the reduce over several chunks of
unequal length never ran. Here ATE_GRAM_WG cuts a 1,088-row panel whose segments hold
exactly 1, 2, 3, 4 and 7 stages into chunks of 1 .. 7 stages (tests/test_gram_plan.py pins
the same tables on the CPU), for every kernel of the family, one tile and six.

Integer panels make fp32 accumulation exact in any order, so the device Gram must EQUAL the
reference; a stale or half-written LDS stage, a dropped or doubled chunk, a tile written to
the wrong place would not. Gaussian panels are held entry by entry against the forward-error
bound of the accumulation. Run on the MI355X box: ``pytest -m gpu``."""
import dataclasses

import numpy as np
import pytest
import torch

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.ops import gram as gram_op
from ate_replication_causalml_amd.ops.exact import from_limbs
from ate_replication_causalml_amd.ops.panel import build_panel

pytestmark = pytest.mark.gpu

STAGES = (1, 2, 3, 4, 7)            # 64-row stages per segment: one segment per fold
# stages per chunk, segment by segment, at ATE_GRAM_WG = m x ntiles
STAGE_TABLE = {
    2: [[1], [2], [3], [4], [7]],
    5: [[1], [2], [3], [3, 1], [3, 3, 1]],
    8: [[1], [2], [2, 1], [2, 2], [2, 2, 2, 1]],
    17: [[1], [1] * 2, [1] * 3, [1] * 4, [1] * 7],
}
# the 64-tile kernels at m = 5, in 16-row steps: chunks that are no multiple of 64 rows
STEP_TABLE_M5 = [[4], [8], [12], [13, 3], [13, 13, 2]]
# id -> (dtype, p, GRAM_KERNEL, P, tile, ntiles)
KERNELS = {
    "bf16-P128": ("bf16", 100, "pair", 128, 128, 1),
    "bf16-P256": ("bf16", 150, "pair", 256, 256, 1),
    "bf16-P384": ("bf16", 300, "pair", 384, 128, 6),       # off-diagonal 128 tiles
    "bf16-P768": ("bf16", 700, "pair", 768, 256, 6),       # off-diagonal 256 tiles
    "bf16-P512-tile256": ("bf16", 400, "tile256", 512, 256, 3),
    "f32-P192": ("f32", 150, "pair", 192, 64, 6),
    "f64-P64": ("f64", 20, "pair", 64, 64, 1),
    "f64-P192": ("f64", 150, "pair", 192, 64, 6),
}
PAIR = {"pair-P512": (400, 512, 2), "pair-P1024": (1000, 1024, 8)}     # p, P, ntiles
DEFAULT_SCHED = gram_op.GRAM_SCHED
U = {"bf16": 2.0 ** -24, "f32": 2.0 ** -24, "f64": 2.0 ** -53}   # unit roundoff of the sums

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _stage_folds():
    return np.repeat(np.arange(len(STAGES)), [64 * k for k in STAGES])


def _int_panel(gpu, dtype, p, folds=None, seed=17, limbs=False, nseg=None):
    """Covariates in {-2..2}, W in {0, 1}, Y in {-3..3}: every product is an integer of
    magnitude <= 9 and a segment has < 2,000 rows, so every partial sum is an integer far
    below 2^24 and fp32 accumulation is exact in any order. ``limbs``: covariate columns
    j = 1 (mod 3) times 2^-13 -- entries between two of them are multiples of 2^-26 (non-zero
    lo limbs, the floor of negative values), every partial still exact in fp32."""
    rs = np.random.RandomState(seed)
    folds = _stage_folds() if folds is None else folds
    n = len(folds)
    X = rs.randint(-2, 3, size=(n, p)).astype(np.float64)
    if limbs:
        X[:, 1::3] *= 2.0 ** -13
    return build_panel(X, rs.randint(0, 2, n), rs.randint(-3, 4, n), folds=folds, dtype=dtype,
                       device=gpu, nseg=nseg)


def _gauss_panel(gpu, dtype, p):
    """The columns of test_gpu.test_gram_kernel_vs_fp64 on the stage layout."""
    rs = np.random.RandomState(0)
    folds = _stage_folds()
    n = len(folds)
    X = rs.randn(n, p) * np.linspace(0.5, 2, p) + np.linspace(-1, 1, p)
    return build_panel(X, rs.rand(n), rs.randint(0, 2, n), folds=folds, dtype=dtype, device=gpu)


def _shape(kid):
    """(dtype, p, GRAM_KERNEL, P) of a KERNELS or PAIR id."""
    if kid in KERNELS:
        return KERNELS[kid][:4]
    return "bf16", PAIR[kid][0], "pair", PAIR[kid][1]


def _int_case(gpu, kid):
    """(panel, fp64 reference) of a kernel's integer stage panel, made once."""
    def make():
        dtype, p, _, P = _shape(kid)
        pan = _int_panel(gpu, dtype, p)
        assert pan.P == P and [int(b - a) // 64 for a, b in pan.seg_bounds] == list(STAGES)
        ref = gram_op.gram_reference(pan)
        _assert_exact_inputs(ref)
        return pan, ref
    return _cached(("int", kid), make)


def _assert_exact_inputs(ref):
    # the precondition of the exact comparisons: an integer-valued reference far inside
    # fp32's exact range (every partial sum is bounded by the sum of magnitudes <= 9 x rows)
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2.0 ** 15


def _chunk_rows(pl):
    """Rows of every chunk of a plan, segment by segment (from the device chunk table)."""
    ch = pl.chunks.cpu().numpy().view([("r0", "<i8"), ("r1", "<i8"), ("seg", "<i4"),
                                       ("pad", "<i4")])
    c0 = [int(v) for v in pl.seg_chunk0.cpu()]
    assert c0[0] == 0 and c0[-1] == len(ch) == pl.nchunks
    out = []
    for s in range(len(c0) - 1):
        assert all(int(c["seg"]) == s for c in ch[c0[s]:c0[s + 1]])
        out.append([int(c["r1"] - c["r0"]) for c in ch[c0[s]:c0[s + 1]]])
    return out


def _run(monkeypatch, pan, kernel="pair", wg=None, sched=None, **kw):
    """(Gram, plan) of ``pan`` with a fresh plan under ATE_GRAM_WG = wg; the plan's own buffer
    is cloned (the plan owns it), an ``out=`` buffer is returned as it is."""
    monkeypatch.setattr(gram_op, "GRAM_KERNEL", kernel)
    if sched is not None:
        monkeypatch.setattr(gram_op, "GRAM_SCHED", sched)
    if wg is None:
        monkeypatch.delenv("ATE_GRAM_WG", raising=False)
    else:
        monkeypatch.setenv("ATE_GRAM_WG", str(wg))
    gram_op._plan_cache.clear()
    pl = gram_op.plan_for(pan, weighted=kw.get("w") is not None, exact=kw.get("exact", False))
    G = gram_op.gram(pan, **kw)
    assert len(gram_op._plan_cache) == 1           # the Gram ran the plan returned here
    if kw.get("out") is None:
        G = G.clone()
    gram_op._plan_cache.clear()
    return G, pl


def _run_kernel(monkeypatch, pan, kid, m, **kw):
    """One of KERNELS at chunking m, after asserting that the plan is the kernel and the
    stage counts this test is about (so a plan change cannot turn them into 1-stage tests)."""
    _, _, kernel, P, T, ntiles = KERNELS[kid]
    G, pl = _run(monkeypatch, pan, kernel, m * ntiles, **kw)
    assert not pl.pair and (pan.P, pl.T, pl.ntiles) == (P, T, ntiles)
    rows = _chunk_rows(pl)
    if T == 64 and m == 5:
        assert [[r // 16 for r in seg] for seg in rows] == STEP_TABLE_M5
    else:
        assert [[r / 64 for r in seg] for seg in rows] == STAGE_TABLE[m]
    assert pl.nchunks * ntiles == {2: 5, 5: 8, 8: 10, 17: 17}[m] * ntiles
    return G, pl


def _nan_like(pan, gpu):
    return torch.full((pan.nseg, pan.P, pan.P), float("nan"), dtype=torch.float64, device=gpu)


# ---------------------------------------------------------------- 1. exact on integers
@pytest.mark.parametrize("m", sorted(STAGE_TABLE))
@pytest.mark.parametrize("kid", list(KERNELS))
def test_integer_panel_exact_at_every_chunking(gpu, monkeypatch, kid, m):
    """Chunks of 1, 2, 3, 4 and 7 stages (m = 2), 3 + 1 and 3 + 3 + 1 (m = 5), 2 + 1 ..
    2 + 2 + 2 + 1 (m = 8) and 1 x 7 (m = 17) through every non-pair kernel, with 5 .. 102
    workgroups (several below 8 or no multiple of 8: xcd_remap's remainder branch)."""
    pan, ref = _int_case(gpu, kid)
    G, _ = _run_kernel(monkeypatch, pan, kid, m)
    assert torch.equal(G.cpu(), ref)
    assert torch.equal(G, G.transpose(1, 2))


# ---------------------------------------------------------------- 2. every entry written
@pytest.mark.parametrize("m", sorted(STAGE_TABLE))
@pytest.mark.parametrize("kid", list(KERNELS))
def test_every_entry_written(gpu, monkeypatch, kid, m):
    """The writers fill a torch.empty buffer under a one-writer-per-entry-plus-its-mirror
    rule (the reduce skips the lower half of a diagonal tile): no NaN of a pre-filled
    ``out`` may remain."""
    pan, ref = _int_case(gpu, kid)
    out = _nan_like(pan, gpu)
    G, _ = _run_kernel(monkeypatch, pan, kid, m, out=out)
    assert G is out and not bool(torch.isnan(out).any())
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("sched", ["lockstep", DEFAULT_SCHED])
@pytest.mark.parametrize("kid", list(PAIR))
def test_every_entry_written_pair(gpu, monkeypatch, kid, sched):
    """The paired-tile kernel's block table (gram_pair_reduce_kernel) at two and eight tiles,
    every segment cut in two chunks (1 .. 4 stages; the 1-stage segment stays whole)."""
    pan, ref = _int_case(gpu, kid)
    _, P, ntiles = PAIR[kid]
    out = _nan_like(pan, gpu)
    G, pl = _run(monkeypatch, pan, "pair", ntiles * len(STAGES) * 2, sched=sched, out=out)
    assert pl.pair and (pan.P, pl.ntiles) == (P, ntiles)
    assert [[r // 64 for r in seg] for seg in _chunk_rows(pl)] == \
        [[1], [1, 1], [1, 2], [2, 2], [3, 4]]
    assert G is out and not bool(torch.isnan(out).any())
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(out, out.transpose(1, 2))


# ---------------------------------------------------------------- 3. rounded data, entry-wise bound
def _abs_gram(pan, w=None):
    """S = |X_s|' diag(|w|) |X_s| in fp64 from the panel as stored."""
    X = pan.colmajor().double().cpu().abs()
    wv = None if w is None else w.double().cpu().abs()
    return torch.stack([(X[:, a:b] if wv is None else X[:, a:b] * wv[a:b]) @ X[:, a:b].T
                        for a, b in pan.seg_bounds])


def _reference(pan, w=None):
    """The reference of the bound tests. bf16 / f32 panels: the fp64 one, whose own error
    (rows x 2^-53 x S) is 2^-29 of the bound. f64 panels: extended precision (the fp64
    reference's error would be as large as the bound)."""
    if pan.dtype != torch.float64:
        return gram_op.gram_reference(pan, w)
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    X = pan.colmajor().cpu().numpy().astype(np.longdouble)
    wv = None if w is None else w.cpu().numpy().astype(np.longdouble)
    return [(X[:, a:b] if wv is None else X[:, a:b] * wv[a:b]) @ X[:, a:b].T
            for a, b in pan.seg_bounds]


def _worst_over_bound(G, ref, S, u, rows, weighted):
    """max over entries of |G - ref| / (c u S) with c = 2 (rows + 2), weighted 2 (rows + 3):
    rows + 2 bounds a sum of ``rows`` exactly representable products rounded once per add
    in any order (the fp64 sum over chunks is below that), + 1 for the rounding of x w; the
    factor 2 is margin, the order and rounding inside one MFMA being undocumented. Entries
    with S = 0 (padding columns) must be exact."""
    c = 2.0 * (rows + 2 + (1 if weighted else 0))
    if isinstance(ref, list):
        err = torch.from_numpy(np.stack([np.abs(g.astype(np.longdouble) - r).astype(np.float64)
                                         for g, r in zip(G.cpu().numpy(), ref)]))
    else:
        err = (G.cpu() - ref).abs()
    bound = c * u * S
    assert bool((err[S == 0] == 0).all())
    return float((err[S > 0] / bound[S > 0]).max())


@pytest.mark.parametrize("m", [2, 8])
@pytest.mark.parametrize("kid", list(KERNELS))
def test_gaussian_panel_forward_error_bound(gpu, monkeypatch, kid, m):
    """Worst observed / bound on the MI355X (the larger of m = 2 and m = 8): bf16 128 tile
    0.012, 256 tile 0.016, f32 0.034, f64 0.041 (COMPONENTS.md K01)."""
    dtype, p = KERNELS[kid][:2]

    def make():
        pan = _gauss_panel(gpu, dtype, p)
        return pan, _reference(pan), _abs_gram(pan)
    pan, ref, S = _cached(("gauss", dtype, p), make)
    G, pl = _run_kernel(monkeypatch, pan, kid, m)
    rows = max(max(seg) for seg in _chunk_rows(pl))
    ratio = _worst_over_bound(G, ref, S, U[dtype], rows, False)
    print(f"gram bound {kid} m={m} longest chunk {rows}: worst / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert torch.equal(G, G.transpose(1, 2))


# ---------------------------------------------------------------- 4. segment edges
EDGE_COUNTS = (63, 64, 0, 65, 1, 0)
EDGE_BOUNDS = [[0, 64], [64, 128], [128, 192], [192, 320], [320, 384], [384, 448]]


@pytest.mark.parametrize("kid", ["bf16-P128", "bf16-P256", "f64-P64", "pair-P512"])
def test_segment_edges(gpu, monkeypatch, kid):
    """Segments of 63, 64, 0, 65, 1 and 0 real rows (64-row padded; an empty segment is one
    all-zero stage): exact, the empty segments exactly zero even when ``out`` held another
    panel's Gram, and the one-one entry counts the real rows."""
    dtype, p, kernel, _ = _shape(kid)
    folds = np.repeat(np.arange(6), EDGE_COUNTS)
    pan = _int_panel(gpu, dtype, p, folds=folds, seed=31, nseg=6)
    assert pan.seg_bounds.tolist() == EDGE_BOUNDS and pan.seg_nreal.tolist() == list(EDGE_COUNTS)
    other = _int_panel(gpu, dtype, p, folds=np.arange(6 * 64) % 6, seed=37)
    assert other.nseg == 6 and other.P == pan.P
    ref = gram_op.gram_reference(pan)
    _assert_exact_inputs(ref)
    out = _nan_like(pan, gpu)
    G0, pl0 = _run(monkeypatch, other, kernel, out=out)
    assert torch.equal(G0.cpu(), gram_op.gram_reference(other)) and bool((G0[2] != 0).any())
    G, pl = _run(monkeypatch, pan, kernel, out=out)
    assert pl.pair == pl0.pair == (kid in PAIR)
    assert [sum(seg) for seg in _chunk_rows(pl)] == [64, 64, 64, 128, 64, 64]
    assert G is out and torch.equal(out.cpu(), ref)
    zero = torch.zeros_like(out[0])
    assert torch.equal(out[2], zero) and torch.equal(out[5], zero)
    one = pan.cols["one"]
    assert out[:, one, one].cpu().tolist() == [float(c) for c in pan.seg_nreal]


# ---------------------------------------------------------------- 5. weighted 64-tile kernels
@pytest.mark.parametrize("m", [2, 8])
@pytest.mark.parametrize("kid", ["f32-P192", "f64-P192"])
def test_weighted_integer_exact(gpu, monkeypatch, kid, m):
    """Integer weights in {0..3} (zero-weight rows included), six tiles: exact, and symmetric
    bit for bit -- on a diagonal tile (x_i w) x_j and (x_j w) x_i are different partials, and
    only one of them may be written (the single-writer rule of gram_reduce_kernel)."""
    pan, _ = _int_case(gpu, kid)
    w = _cached(("wint", kid), lambda: torch.from_numpy(
        np.random.RandomState(41).randint(0, 4, pan.ld)).to(device=gpu, dtype=pan.dtype))
    assert bool((w == 0).any()) and w.numel() == pan.ld
    ref = _cached(("wintref", kid), lambda: gram_op.gram_reference(pan, w))
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2.0 ** 17
    G, _ = _run_kernel(monkeypatch, pan, kid, m, w=w, out=_nan_like(pan, gpu))
    assert torch.equal(G.cpu(), ref)
    assert torch.equal(G, G.transpose(1, 2))


@pytest.mark.parametrize("m", [2, 8])
@pytest.mark.parametrize("kid", ["f32-P192", "f64-P192"])
def test_weighted_gaussian_forward_error_bound(gpu, monkeypatch, kid, m):
    """Weights in [0.1, 1.1] on the Gaussian panel. Worst observed / bound on the MI355X:
    f32 0.032, f64 0.035 (COMPONENTS.md K01)."""
    dtype, p = KERNELS[kid][:2]

    def make():
        pan = _gauss_panel(gpu, dtype, p)
        w = torch.from_numpy(0.1 + np.random.RandomState(43).rand(pan.ld)).to(
            device=gpu, dtype=pan.dtype)
        return pan, w, _reference(pan, w), _abs_gram(pan, w)
    pan, w, ref, S = _cached(("wgauss", kid), make)
    G, pl = _run_kernel(monkeypatch, pan, kid, m, w=w)
    rows = max(max(seg) for seg in _chunk_rows(pl))
    ratio = _worst_over_bound(G, ref, S, U[dtype], rows, True)
    print(f"gram bound weighted {kid} m={m} longest chunk {rows}: worst / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert torch.equal(G, G.transpose(1, 2))


# ---------------------------------------------------------------- 6. the IRLS latch
@pytest.mark.parametrize("kid", ["f32-P192", "f64-P192"])
def test_done_flag(gpu, monkeypatch, kid):
    """``done`` = 1: neither the tile kernel nor the reduce touches a bit of ``out``;
    ``done`` = 0: the bits of the call without ``done``."""
    dtype, p = KERNELS[kid][:2]
    pan = _cached(("gauss", dtype, p, "done"), lambda: _gauss_panel(gpu, dtype, p))
    w = torch.from_numpy(0.1 + np.random.RandomState(47).rand(pan.ld)).to(device=gpu,
                                                                         dtype=pan.dtype)
    G0, _ = _run_kernel(monkeypatch, pan, kid, 8, w=w)
    sentinel = torch.full_like(G0, -7.25)
    for flag in (1, 0):
        done = torch.full((1,), flag, dtype=torch.int32, device=gpu)
        out = sentinel.clone()
        G, _ = _run_kernel(monkeypatch, pan, kid, 8, w=w, done=done, out=out)
        assert G is out and torch.equal(out, sentinel if flag else G0)
        assert int(done) == flag


# ---------------------------------------------------------------- 7. exact-mode limbs
EXACT_CHUNKS = [[1], [2], [2, 1], [2, 2], [2, 2, 2, 1]]     # stages, exact_block = 128


def _cpu_copy(pan):
    return dataclasses.replace(pan, data=pan.data.cpu(), row_index=pan.row_index.cpu())


@pytest.mark.parametrize("kid,weighted", [
    ("bf16-P128", False), ("bf16-P256", False), ("bf16-P384", False), ("pair-P512", False),
    ("f32-P192", False), ("f64-P64", False), ("f64-P64", True)])
def test_exact_limbs_equal_cpu_twin(gpu, monkeypatch, kid, weighted):
    """The int64 limbs of the exact mode (the Gx branch of both reduces) against the CPU twin
    ``_gram_cpu_exact`` on chunks of 2 stages with 1-stage tails; columns scaled by 2^-13 give
    non-zero lo limbs and negative values to floor. Weighted: f64 with integer weights."""
    dtype, p, kernel, _ = _shape(kid)
    pan = dataclasses.replace(_int_panel(gpu, dtype, p, limbs=True), exact_block=128)
    w = None
    if weighted:
        w = torch.from_numpy(np.random.RandomState(53).randint(0, 4, pan.ld)).to(
            device=gpu, dtype=pan.dtype)
    ref = gram_op.gram_reference(pan, w)
    assert torch.equal(ref * 2.0 ** 26, (ref * 2.0 ** 26).round())
    assert float(ref.abs().max()) < 2.0 ** 17
    Gx, pl = _run(monkeypatch, pan, kernel, exact=True, w=w)
    assert pl.pair == (kid in PAIR)
    assert [[r // 64 for r in seg] for seg in _chunk_rows(pl)] == EXACT_CHUNKS
    assert Gx.dtype == torch.int64 and tuple(Gx.shape) == (2, pan.nseg, pan.P, pan.P)
    twin = gram_op._gram_cpu_exact(_cpu_copy(pan), None if w is None else w.cpu())
    assert bool((twin[1] != 0).any()) and bool((twin[0] < 0).any())
    assert torch.equal(Gx.cpu(), twin)
    assert torch.equal(from_limbs(Gx.cpu()), ref)


@pytest.mark.parametrize("kid,block", [("bf16-P128", 96), ("pair-P512", 32), ("f32-P192", 24)])
def test_exact_refuses_unaligned_block(gpu, monkeypatch, kid, block):
    pan = dataclasses.replace(_int_case(gpu, kid)[0], exact_block=block)
    gram_op._plan_cache.clear()
    with pytest.raises(ValueError, match="block-aligned"):
        gram_op.gram(pan, exact=True)
    assert not gram_op._plan_cache


# ---------------------------------------------------------------- 8. stage split
def test_stage_split_pair(gpu, monkeypatch):
    """Paired-tile kernel: "tiles" then "reduce" into ``out`` gives the bits of "all"."""
    pan, ref = _int_case(gpu, "pair-P512")
    Gall, pl = _run(monkeypatch, pan, "pair", 20)
    assert pl.pair and torch.equal(Gall.cpu(), ref)
    out = _nan_like(pan, gpu)
    gram_op._plan_cache.clear()
    gram_op.gram(pan, stage="tiles")
    G = gram_op.gram(pan, stage="reduce", out=out)           # the same plan: its slab
    assert len(gram_op._plan_cache) == 1
    gram_op._plan_cache.clear()
    assert G is out and torch.equal(out, Gall)


def test_stage_split_other_kernels(gpu, monkeypatch):
    """The other kernels do everything at "tiles" and nothing at "reduce"."""
    pan, ref = _int_case(gpu, "bf16-P128")
    out = _nan_like(pan, gpu)
    G, pl = _run_kernel(monkeypatch, pan, "bf16-P128", 8, stage="tiles", out=out)
    assert G is out and torch.equal(out.cpu(), ref)
    sentinel = torch.full_like(out, -7.25)
    out2 = sentinel.clone()
    G2, _ = _run_kernel(monkeypatch, pan, "bf16-P128", 8, stage="reduce", out=out2)
    assert G2 is out2 and torch.equal(out2, sentinel)


# ---------------------------------------------------------------- 9. refusals
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _refused(name, *args):
    with pytest.raises(_native.NativeError) as ei:
        _native.call(name, *args)
    assert ei.value.status < 0


def test_gram_argument_checks(gpu, monkeypatch):
    """Each refusal returns before any launch (status < 0): a tile size no kernel has, P no
    multiple of the tile, and for the paired-tile entry point P % 512, ``what`` outside 1..3,
    one-byte columns at P != 512, an unknown schedule, ``prio`` > 2, and a column stride of
    2^28 elements under the stagger schedule (32-bit byte offsets)."""
    pan, ref = _int_case(gpu, "bf16-P128")
    monkeypatch.delenv("ATE_GRAM_WG", raising=False)
    gram_op._plan_cache.clear()
    pl = gram_op.plan_for(pan)

    def bf16(P, tile):
        return ("ate_gram_bf16", pan.data.data_ptr(), pan.cm_ld, P, tile, pl.tiles.data_ptr(),
                pl.ntiles, pl.chunks.data_ptr(), pl.nchunks, pl.seg_chunk0.data_ptr(), pan.nseg,
                pl.slab.data_ptr(), pl.G.data_ptr(), None, _stream())
    _refused(*bf16(128, 64))
    _refused(*bf16(192, 128))
    _refused(*bf16(384, 256))

    for dtype, name in (("f32", "ate_gram_f32"), ("f64", "ate_gram_f64")):
        ps = _int_panel(gpu, dtype, 20)
        gram_op._plan_cache.clear()
        pls = gram_op.plan_for(ps)
        assert ps.P == 64
        _refused(name, ps.data.data_ptr(), ps.cm_ld, 96, 0, pls.tiles.data_ptr(), pls.ntiles,
                 pls.chunks.data_ptr(), pls.nchunks, pls.seg_chunk0.data_ptr(), ps.nseg,
                 pls.slab.data_ptr(), pls.G.data_ptr(), 0, None, _stream())

    pp, pref = _int_case(gpu, "pair-P512")
    monkeypatch.setattr(gram_op, "GRAM_KERNEL", "pair")
    gram_op._plan_cache.clear()
    plp = gram_op.plan_for(pp)
    assert plp.pair
    cs, bs = pp.strides()

    def pair(P=512, what=3, x8=None, sched=gram_op.SCHEDULES["lockstep"], prio=-1, cs=cs):
        return ("ate_gram_bf16_pair", pp.data.data_ptr(), cs, bs, P, plp.tiles.data_ptr(),
                plp.ntiles, plp.blocks.data_ptr(), plp.chunks.data_ptr(), plp.nchunks,
                plp.seg_chunk0.data_ptr(), pp.nseg, plp.slab.data_ptr(), plp.G.data_ptr(), what,
                None, x8, sched, prio, _stream())
    byte_like = torch.zeros(64, dtype=torch.uint8, device=gpu)
    _refused(*pair(P=768))
    _refused(*pair(what=0))
    _refused(*pair(what=4))
    _refused(*pair(P=1024, x8=byte_like.data_ptr()))
    _refused(*pair(sched=7))
    _refused(*pair(prio=3))
    _refused(*pair(sched=gram_op.SCHEDULES["stagger"], cs=1 << 28))
    gram_op._plan_cache.clear()

    # the plan's own refusal: a weighted Gram needs an fp32 / fp64 panel
    with pytest.raises(ValueError, match="weighted Gram"):
        gram_op.gram(pan, w=torch.ones(pan.ld, dtype=torch.float32, device=gpu))
    gram_op._plan_cache.clear()

    # nothing is left pending: a synchronize, then good Grams through both entry points
    torch.cuda.synchronize()
    assert torch.equal(_run(monkeypatch, pan)[0].cpu(), ref)
    assert torch.equal(_run(monkeypatch, pp)[0].cpu(), pref)
    torch.cuda.synchronize()
