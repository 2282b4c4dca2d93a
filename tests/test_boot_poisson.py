"""CPU twin of the Poisson(1) streaming bootstrap (ops/stats.bootstrap_poisson_partial,
poisson1_counts; kernel: csrc/stats.hip boot_poisson_kernel, K20): the inverse-CDF table,
the shard and replicate-offset contracts, and the distribution of the draws."""
import math

import numpy as np
import torch

from ate_replication_causalml_amd.ops import stats as S

SEED = 1991


def _scores(n, seed=0):
    rs = np.random.RandomState(seed)
    e1 = rs.randint(-64, 65, n) / 8.0          # 1/8 grid: every c * e sum is exact
    e2 = rs.randint(-64, 65, n) / 8.0
    e1[::17] = np.nan
    return torch.as_tensor(e1), torch.as_tensor(e2)


def test_table_is_the_poisson1_cdf_in_float32():
    pmf = [math.exp(-1.0) / math.factorial(q) for q in range(8)]
    cdf = np.cumsum(np.asarray(pmf, dtype=np.float64)).astype(np.float32)
    got = np.asarray(S.POISSON1_CDF, dtype=np.float32)
    np.testing.assert_array_equal(got, cdf)
    assert np.all(np.diff(got) > 0) and got[-1] < 1


def test_output_layout_and_nan_rows():
    e1, e2 = _scores(300)
    out = S.bootstrap_poisson_partial(e1, e2, 5, SEED)
    assert out.shape == (5, 4) and out.dtype == torch.float64
    ok = ~torch.isnan(e1)
    for b in range(5):
        c = torch.as_tensor(S.poisson1_counts(300, SEED, b)).double()
        want = [(c[ok] * e1[ok]).sum(), c[ok].sum(), (c * e2).sum(), c.sum()]
        assert out[b].tolist() == [float(v) for v in want]
    assert (out[:, 1] < out[:, 3]).any()           # NaN rows are out of column 1 only


def test_rows_with_count_zero_are_not_read():
    e1, e2 = _scores(200)
    c = S.poisson1_counts(200, SEED, 0)
    e2b = e2.clone()
    e2b[torch.as_tensor(c == 0)] = float("nan")
    a = S.bootstrap_poisson_partial(e1, e2, 1, SEED)
    b = S.bootstrap_poisson_partial(e1, e2b, 1, SEED)
    assert torch.equal(a, b)


def test_shard_invariance():
    n, m = 1000, 377
    e1, e2 = _scores(n)
    full = S.bootstrap_poisson_partial(e1, e2, 9, SEED)
    lo = S.bootstrap_poisson_partial(e1[:m], e2[:m], 9, SEED, row_offset=0)
    hi = S.bootstrap_poisson_partial(e1[m:], e2[m:], 9, SEED, row_offset=m)
    assert torch.equal(full, lo + hi)              # exact: 1/8-grid scores
    # the offset matters: the same rows keyed from 0 draw other counts
    assert not torch.equal(hi, S.bootstrap_poisson_partial(e1[m:], e2[m:], 9, SEED))


def test_replicate_offset():
    e1, e2 = _scores(500)
    full = S.bootstrap_poisson_partial(e1, e2, 9, SEED)
    part = S.bootstrap_poisson_partial(e1, e2, 2, SEED, b0=7)
    assert torch.equal(part, full[7:9])
    assert not torch.equal(full[0], full[1])


def test_draws_are_disjoint_from_the_multinomial_stream():
    from ate_replication_causalml_amd.parallel import rng
    i = np.arange(64, dtype=np.uint64)
    a = rng.random_u32(SEED, rng.P_BOOT, 3, i)[:, 0]
    b = rng.random_u32(SEED, rng.P_BOOT, 3, i | (np.uint64(1) << np.uint64(62)))[:, 0]
    assert not np.any(a == b)


def test_mean_and_variance_of_the_counts():
    """2 * 10^5 draws (seed 1991, replicates 0..3 of 50,000 rows): mean and variance of
    Poisson(1) are 1; the standard error of the mean is sqrt(1 / N) and that of the
    variance sqrt((mu4 - 1) / N) with mu4 = lambda (1 + 3 lambda) = 4. The table's cut at 8
    moves either by less than 1e-5. Fixed margin: 5 standard errors."""
    N = 200000
    c = np.concatenate([S.poisson1_counts(50000, SEED, b) for b in range(4)]).astype(float)
    assert c.size == N and c.min() == 0 and c.max() <= 8
    zm = (c.mean() - 1.0) / math.sqrt(1.0 / N)
    zv = (c.var(ddof=1) - 1.0) / math.sqrt(3.0 / N)
    print("poisson1 z(mean) = %.2f z(var) = %.2f" % (zm, zv))
    assert abs(zm) < 5 and abs(zv) < 5
    # P(K = 0) = exp(-1)
    z0 = ((c == 0).mean() - math.exp(-1)) / math.sqrt(math.exp(-1) * (1 - math.exp(-1)) / N)
    assert abs(z0) < 5
