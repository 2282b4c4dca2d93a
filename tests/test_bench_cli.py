"""bench.py's command line, on the CPU (a small float64 panel): a plain run times the
``--steps`` calls and nothing else, ``--dump-outputs`` writes what the last timed call
returned (the same arrays from run to run), ``--full`` adds the secondary blocks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--rows", "1000", "--p", "21", "--folds", "3", "--dtype", "f64",
        "--steps", "2", "--warmup", "0"]


def _bench(*args, cpu=False):
    env = dict(os.environ)
    if cpu:
        env.update(OMP_NUM_THREADS="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    dirs = [str(tmp_path_factory.mktemp("dump") / "out") for _ in range(2)]
    return [(_bench(*ARGS, "--dump-outputs", d, cpu=True), d) for d in dirs]


def test_plain_run_times_the_steps_only(plain):
    out, _ = plain[0]
    assert out["steps"] == 2 and out["warmup"] == 0 and not out["full"]
    assert out["ms_per_step"] > 0 and out["unit"] == "rows/s" and out["higher_is_better"]
    assert out["value"] == pytest.approx(1000 / (out["ms_per_step"] / 1e3), rel=1e-9)
    assert np.isfinite(out["ate"]) and out["se"] > 0
    for k in ("single_fit_ms", "single_fit_ms_all", "single_fit_rows_per_s",
              "throughput_inflight", "parity", "repeated", "rct"):
        assert out[k] is None, k


def test_dump_outputs_repeatable(plain):
    (a, da), (b, db) = plain
    assert a["ate_hex"] == b["ate_hex"] and a["se_hex"] == b["se_hex"]
    names = sorted(os.listdir(da))
    assert names == sorted(os.listdir(db))
    assert {"res.npy", "mom.npy", "gram.npy", "coef_min.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(os.path.join(da, n)), np.load(os.path.join(db, n))
        assert x.dtype in (np.float32, np.float64) and x.size > 0
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), n
        total += x.nbytes
    assert total <= 64 << 20
    res = np.load(os.path.join(da, "res.npy"))
    assert res.shape == (2,) and res[0].item().hex() == a["ate_hex"] \
        and res[1].item().hex() == a["se_hex"]
    assert np.load(os.path.join(da, "coef_min.npy")).shape == (6, 22)   # 3 folds x {Y, W}


@pytest.mark.gpu
def test_full_adds_the_secondary_blocks(gpu):
    """--full on the GPU (bf16, p=500, 1e6 rows): the timed step as in a plain run, then
    every secondary block."""
    args = ["--gpus", "1", "--rows", "1000000", "--steps", "3", "--warmup", "1"]
    lean, full = _bench(*args), _bench(*args, "--full")
    assert not lean["full"] and lean["rct"] is None and lean["parity"] is None
    assert full["full"] and full["steps"] == 3 and full["hipgraph"]
    assert full["ate_hex"] == lean["ate_hex"] and full["se_hex"] == lean["se_hex"]
    assert full["single_fit_ms"] > 0 and len(full["single_fit_ms_all"]) == 5
    assert full["throughput_inflight"]["inflight"] == 3
    assert full["repeated"]["repeats"] == 3 and len(full["repeated"]["splits"]) == 3
    assert np.isfinite(full["parity"]["abs_diff_ate_in_se"])
    assert full["rct"]["ms_per_step"] > 0 and np.isfinite(full["rct"]["ate"])
