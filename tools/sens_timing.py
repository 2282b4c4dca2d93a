#!/usr/bin/env python3
"""The DML-IRM sensitivity call beside plain DML-IRM on one GPU: ms per captured call of
``irm_phases`` (the estimator), ``sens_phases`` without benchmarks and ``sens_phases`` with
``--sets`` benchmark covariate sets, on one arm-split panel (tutorial DGP, bf16 blocked),
alternated in one process and timed with device events; then the 14-moment pass beside the
8-moment pass, eager launches in alternated batches between device events. Recorded, not
gated: profiles/sens/README.md.

  python tools/sens_timing.py --n 1e7 --p 500 --calls 20

``--pass-only``: one eager fit, then a few eager launches of each of the two passes and nothing
else, for a separate ``rocprofv3 --kernel-trace --stats -- python tools/sens_timing.py
--pass-only`` run that splits each pass into its score kernel and its sum kernel."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7)
    ap.add_argument("--p", type=int, default=500)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--blocked", type=int, default=1)
    ap.add_argument("--dgp", default="tutorial")
    ap.add_argument("--seed", type=int, default=1991)
    ap.add_argument("--clip", type=float, default=0.01)
    ap.add_argument("--calls", type=int, default=20, help="timed calls of each step")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=1, help="benchmark sets of the third step")
    ap.add_argument("--batch", type=int, default=10, help="kernel launches per timed batch")
    ap.add_argument("--pass-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators.irm import irm_phases, irm_score_moments
    from ate_replication_causalml_amd.estimators.sensitivity import irm_sens_moments, sens_phases
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.result import SensitivityResult
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    dev = torch.device("cuda:0")
    n, K = int(a.n), a.folds
    blocked = bool(a.blocked) and a.dtype == "bf16"
    pan = synthetic_panel(n, p=a.p, folds=K, seed=a.seed, dtype=a.dtype, device=dev,
                          blocked=blocked, dgp=a.dgp, arm_split=True)
    torch.cuda.synchronize()
    if a.pass_only:
        st = None
        for ph in irm_phases(pan, K, "min", a.clip):
            st = ph(st)
        torch.cuda.synchronize()
        for _ in range(5):
            m8 = irm_score_moments(pan, st["coef"], a.clip, 2)
            m14 = irm_sens_moments(pan, st["coef"], a.clip, 2)
        torch.cuda.synchronize()
        print(json.dumps({"mode": "pass-only", "n": n, "p": a.p, "launches_each": 5,
                          "mom8": m8.cpu().tolist(), "mom14": m14.cpu().tolist()}))
        return
    bench = tuple((3 * j, 3 * j + 1, 3 * j + 2) for j in range(a.sets))
    steps = {}
    with plan_slot(0):
        steps["irm"] = SegmentedStep(irm_phases(pan, K, "min", a.clip), graph=True, warmup=1)
    with plan_slot(1):
        steps["sens"] = SegmentedStep(sens_phases(pan, K, "min", a.clip), graph=True, warmup=1)
    with plan_slot(2):
        steps["sens_bench"] = SegmentedStep(sens_phases(pan, K, "min", a.clip, bench), graph=True,
                                            warmup=1)
    for _ in range(a.warmup):
        for step in steps.values():
            step()
    torch.cuda.synchronize()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    ms = {name: [] for name in steps}
    for _ in range(a.calls):                      # alternate: all see the same clocks
        for name, step in steps.items():
            ms[name].append(timed(step)[0])
    out = {"n": n, "p": a.p, "folds": K, "dtype": a.dtype, "blocked": blocked, "dgp": a.dgp,
           "calls": a.calls, "benchmarks": [list(b) for b in bench],
           "graphed": [s.graphed for s in steps.values()]}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v)}
    out["ratio_sens_over_irm"] = out["sens"]["median_ms"] / out["irm"]["median_ms"]
    out["ms_per_benchmark_set"] = (out["sens_bench"]["median_ms"] - out["sens"]["median_ms"]) \
        / max(a.sets, 1)
    st = steps["irm"]()
    out["irm_res"], irm_mom = st["res"].cpu().tolist(), st["mom"].cpu()
    coef = st["coef"].clone()
    mom = steps["sens_bench"]()["mom"].cpu()
    out["sens_mom"] = mom.tolist()
    out["shared_bits_equal"] = bool(torch.equal(mom[0][[0, 1, 2, 3, 13]], irm_mom[[0, 1, 2, 3, 7]]))
    r = SensitivityResult.from_moments("DML-IRM sensitivity (LASSO)", mom[0].numpy(), short=[
        (c, mom[1 + j].numpy()) for j, c in enumerate(bench)])
    out["table"] = r.table().splitlines()

    # the two passes alone: eager launches, `batch` per timing, alternated
    passes = {"score_moments_8": lambda: irm_score_moments(pan, coef, a.clip, 2),
              "sens_moments_14": lambda: irm_sens_moments(pan, coef, a.clip, 2)}
    for f in passes.values():
        f()
    torch.cuda.synchronize()
    us = {name: [] for name in passes}
    for _ in range(a.calls):
        for name, f in passes.items():
            t, _ = timed(lambda: [f() for _ in range(a.batch)])
            us[name].append(1e3 * t / a.batch)
    for name, v in us.items():
        out[name] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
    out["ratio_14_over_8"] = out["sens_moments_14"]["median_us"] / out["score_moments_8"]["median_us"]
    nnz = (coef[:, :, 1:] != 0).any(1).sum(1).cpu().numpy()
    rows = np.asarray(pan.seg_nreal).reshape(K, 2).sum(1)
    out["union_support"] = nnz.tolist()
    out["score_bytes"] = int((rows * (nnz + 5) * 2).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
