"""K02 column moments / R scale() and K21 interaction expansion (ops/prep.py): CPU
formulas vs numpy, and the HIP kernels (csrc/prep.hip) vs the fp64 CPU path."""
import numpy as np
import pytest
import torch

from ate_replication_causalml_amd.data.dgp import r_scale as np_r_scale
from ate_replication_causalml_amd.ops import prep


def _x(n=1000, p=7, seed=0, nan=False):
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, p)) * r.uniform(0.5, 5, size=p) + r.uniform(-3, 3, size=p)
    if nan:
        X[r.random((n, p)) < 0.02] = np.nan
    return X


def test_col_moments_cpu_matches_numpy():
    X = _x(nan=True)
    m = prep.col_moments(torch.as_tensor(X)).numpy()
    np.testing.assert_allclose(m[:, 0], (~np.isnan(X)).sum(0))
    np.testing.assert_allclose(m[:, 1], np.nanmean(X, 0), rtol=1e-13)
    np.testing.assert_allclose(m[:, 2], np.nanstd(X, 0, ddof=1), rtol=1e-12)


def test_r_scale_cpu_matches_dgp_scale():
    X = _x()
    np.testing.assert_allclose(prep.r_scale(torch.as_tensor(X)).numpy(), np_r_scale(X),
                               rtol=1e-12, atol=1e-12)
    part = prep.r_scale(torch.as_tensor(X), cols=[0, 3]).numpy()
    np.testing.assert_array_equal(part[:, 1], X[:, 1])


def test_interactions_cpu_layout():
    X = _x(50, 4)
    Z = prep.interactions(torch.as_tensor(X)).numpy()
    assert Z.shape == (50, 4 + 16)
    np.testing.assert_array_equal(Z[:, :4], X)
    np.testing.assert_allclose(Z[:, 4 + 2 * 4 + 3], X[:, 2] * X[:, 3])


@pytest.mark.gpu
def test_prep_kernels_match_cpu(gpu):
    X = _x(20000, 9, nan=True)
    m_cpu = prep.col_moments(torch.as_tensor(X)).numpy()
    m_gpu = prep.col_moments(torch.as_tensor(X, device=gpu)).cpu().numpy()
    np.testing.assert_allclose(m_gpu, m_cpu, rtol=1e-12)
    Xs = _x(20000, 9)
    s_cpu = prep.r_scale(torch.as_tensor(Xs), cols=[0, 1, 2, 5]).numpy()
    s_gpu = prep.r_scale(torch.as_tensor(Xs, device=gpu), cols=[0, 1, 2, 5]).cpu().numpy()
    np.testing.assert_allclose(s_gpu, s_cpu, rtol=1e-12, atol=1e-12)
    Z_cpu = prep.interactions(torch.as_tensor(Xs[:, :5])).numpy()
    Z_gpu = prep.interactions(torch.as_tensor(Xs[:, :5], device=gpu)).cpu().numpy()
    np.testing.assert_array_equal(Z_gpu, Z_cpu)


@pytest.mark.gpu
def test_loader_device_scale_matches_host(gpu, tmp_path):
    import pandas as pd
    from ate_replication_causalml_amd.data.dgp import BIN_NAMES, CTS_NAMES
    from ate_replication_causalml_amd.data.loader import OUTCOME, TREATMENT, load_social_pressure
    r = np.random.default_rng(4)
    n = 3000
    df = pd.DataFrame({c: r.normal(size=n) * 7 + 3 for c in CTS_NAMES})
    for c in BIN_NAMES:
        df[c] = (r.random(n) < 0.4).astype(float)
    df[OUTCOME] = (r.random(n) < 0.3).astype(float)
    df[TREATMENT] = (r.random(n) < 0.2).astype(float)
    df.loc[5, CTS_NAMES[2]] = np.nan
    f = tmp_path / "gotv.csv"
    df.to_csv(f, index=False)
    a = load_social_pressure(f, n_obs=2500)
    b = load_social_pressure(f, n_obs=2500, device=gpu)
    np.testing.assert_allclose(b.X, a.X, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(b.Y, a.Y)


# ---------------------------------------------------------------- edge shapes (K02, K21)
# Dyadic inputs whose column means are dyadic too (values paired around a centre), so every
# sum is exact in any order and the kernels must give the CPU path's bits.
def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    np.testing.assert_array_equal(na, nb)
    np.testing.assert_array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def _paired(n, p, seed=0):
    """[n, p], n odd: column j = centre_j +- d (d on a 1/8 grid) plus the centre itself."""
    assert n % 2 == 1
    r = np.random.default_rng(seed)
    c = r.integers(-16, 17, size=p) / 4.0
    d = r.integers(1, 64, size=(n // 2, p)) / 8.0
    X = np.concatenate([c + d, c - d, c[None, :]], 0)
    return X[r.permutation(n)]


def test_col_moments_cpu_degenerate_columns():
    X = _paired(9, 3)
    X[:, 1] = np.nan
    X[1:, 2] = np.nan
    m = prep.col_moments(torch.as_tensor(X)).numpy()
    np.testing.assert_array_equal(m[:, 0], [9, 0, 1])
    assert np.isnan(m[1, 1]) and np.isnan(m[1, 2]) and np.isnan(m[2, 2]) and m[2, 1] == X[0, 2]
    assert m[0, 2] == np.std(X[:, 0], ddof=1)


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(1, 3), (63, 4), (65, 4), (65, 70)])
def test_col_moments_edge_shapes(gpu, n, p):
    """n < 64: most of the 64 row chunks are empty; n = 1: count 1, NaN SD; p = 70: the
    second block of colmom_final_kernel; an all-NaN and a constant column."""
    X = _paired(n, p, seed=n + p)
    X[:, 1] = np.nan
    X[:, 2] = 2.5
    m_cpu = prep.col_moments(torch.as_tensor(X)).numpy()
    m_gpu = prep.col_moments(torch.as_tensor(X, device=gpu)).cpu().numpy()
    _same_bits(m_gpu, m_cpu)
    np.testing.assert_array_equal(m_gpu[:, 0], np.where(np.arange(p) == 1, 0, n))
    assert np.isnan(m_gpu[1, 1]) and np.isnan(m_gpu[1, 2])
    assert m_gpu[2, 1] == 2.5
    if n == 1:
        assert np.isnan(m_gpu[:, 2]).all()
    else:
        assert m_gpu[2, 2] == 0.0
        np.testing.assert_array_equal(m_gpu[0], [n, np.mean(X[:, 0]), np.std(X[:, 0], ddof=1)])


@pytest.mark.gpu
@pytest.mark.parametrize("constant_to_one", [False, True])
@pytest.mark.parametrize("n,p", [(1, 3), (63, 4), (65, 70), (65536 + 5, 3)])
def test_r_scale_edge_shapes(gpu, n, p, constant_to_one):
    """n = 65,536 + 5: the second trip of standardize_kernel's 256-block grid."""
    X = _paired(n, p, seed=n + p)
    X[:, 2] = 2.5                                   # zero SD: NaN, or 0 with the guard
    # the centre row (the median) of column 0: stays NaN and is out of the moments, and the
    # remaining pairs keep the mean dyadic
    i0 = int(np.flatnonzero(X[:, 0] == np.median(X[:, 0]))[0])
    X[i0, 0] = np.nan
    kw = dict(cols=[0, 2, p - 1], constant_to_one=constant_to_one)
    s_cpu = prep.r_scale(torch.as_tensor(X), **kw).numpy()
    s_gpu = prep.r_scale(torch.as_tensor(X, device=gpu), **kw).cpu().numpy()
    _same_bits(s_gpu, s_cpu)
    np.testing.assert_array_equal(s_gpu[:, 1], X[:, 1])          # not selected
    if n > 1:
        assert np.isnan(s_gpu[i0, 0]) and np.isnan(s_gpu[:, 0]).sum() == 1
        if constant_to_one:
            np.testing.assert_array_equal(s_gpu[:, 2], np.zeros(n))
        else:
            assert np.isnan(s_gpu[:, 2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n,p", [(1, 2), (16384 + 3, 3), (8, 255)])
def test_interactions_edge_shapes(gpu, n, p):
    """n = 16,384 + 3: the second trip of the 64-block grid; p = 255: p (p + 1) = 65,280,
    the largest grid.y the entry point accepts."""
    r = np.random.default_rng(n + p)
    X = r.integers(-32, 33, size=(n, p)) / 8.0
    Z_cpu = prep.interactions(torch.as_tensor(X)).numpy()
    Z_gpu = prep.interactions(torch.as_tensor(X, device=gpu)).cpu().numpy()
    assert Z_gpu.shape == (n, p + p * p)
    _same_bits(Z_gpu, Z_cpu)
    np.testing.assert_array_equal(Z_gpu[:, p + (p - 1) * p + 1], X[:, p - 1] * X[:, 1])


@pytest.mark.gpu
def test_interactions_rejects_p_256(gpu):
    from ate_replication_causalml_amd import _native
    X = torch.zeros((2, 256), dtype=torch.float64, device=gpu)
    with pytest.raises(_native.NativeError) as ei:
        prep.interactions(X)
    assert ei.value.status < 0
