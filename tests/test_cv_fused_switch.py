"""``ATE_CV_FUSED`` (ops/enet.py, read at import) selects between the fused launches and the
chain of separate ones on the GPU only: the problem tables, the CPU path and the phase list
of the DML step are the same under both settings."""
import importlib

import numpy as np

from ate_replication_causalml_amd import _native
from ate_replication_causalml_amd.estimators import lasso
from ate_replication_causalml_amd.ops import enet
from ate_replication_causalml_amd.ops.panel import build_panel


def _panel():
    rs = np.random.RandomState(4)
    n, p, K = 240, 6, 3
    X = rs.randn(n, p)
    W = (rs.rand(n) < 0.5).astype(float)
    Y = X[:, 0] - 0.5 * X[:, 1] + 0.7 * W + rs.randn(n)
    return build_panel(X, W, Y, folds=np.arange(n) % K, dtype="f64", device="cpu"), K


def _observe(monkeypatch, value):
    monkeypatch.setenv("ATE_CV_FUSED", value)
    importlib.reload(enet)
    assert enet.CV_FUSED is (value != "0")
    calls = []
    monkeypatch.setattr(_native, "call", lambda name, *a: calls.append(name))
    counts = [enet.cv_problem_count(5), enet.cv_problem_count(5, ny=2),
              enet.cv_problem_count(5, [[s for s in range(5) if s != k] for k in range(5)], ny=2),
              enet.cv_problem_count(4, [[0, 1], [2, 3]], ny=2, full_y=[0, 1])]
    tables = enet._cv_tables(5, [[0, 1, 2, 3], [1, 2, 3, 4]], [7, 8], np.arange(5.0) + 10, 20, None)
    pan, K = _panel()
    phases = [ph.__name__ if hasattr(ph, "__name__") else type(ph).__name__
              for ph in lasso.dml_phases(pan, K)]
    res, mom, cv = lasso.dml_crossfit_panel(pan, K)
    return dict(counts=counts, tables=tables, phases=phases, calls=calls, res=res.numpy(),
                mom=mom.numpy(), sel=cv.sel.numpy(), cvm=cv.cvm.numpy())


def test_switch_leaves_tables_and_cpu_path_alone(monkeypatch):
    try:
        a, b = _observe(monkeypatch, "0"), _observe(monkeypatch, "1")
    finally:
        monkeypatch.undo()
        importlib.reload(enet)
    assert a["counts"] == b["counts"] == [6, 12, 50, 6]
    for x, y in zip(a["tables"], b["tables"]):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    assert a["phases"] == b["phases"]
    assert a["calls"] == b["calls"] == []           # no native kernel on the CPU path
    for k in ("res", "mom", "sel", "cvm"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_default_is_fused(monkeypatch):
    monkeypatch.delenv("ATE_CV_FUSED", raising=False)
    try:
        importlib.reload(enet)
        assert enet.CV_FUSED is True
    finally:
        monkeypatch.undo()
        importlib.reload(enet)
