#!/usr/bin/env python3
"""The CATE curve with a uniform band beside the group ATEs on one GPU: ms per captured call
of the ``cate_phases`` step and of the ``gate_phases`` step on the same arm-split panel
(tutorial DGP, bf16 blocked), alternated in one process and timed with device events, plus
the two new entry points alone (``ate_cate_moments``, ``ate_cate_boot``) and the group
bootstrap (``ate_group_boot``) timed as eager launches between events. Recorded, not gated:
profiles/cate/README.md.

  python tools/cate_timing.py --n 1e7 --p 500 --df 8 --degree 3 --boot 1024 --groups 8 --calls 20

The JSON line carries the three bounds of the bootstrap kernel for these sizes: the bytes it
reads (rows x 24: psi, x, row id), the (row, replicate, basis function) accumulations
(rows x boot x (degree + 1)) and the Philox calls (rows x ceil(boot / 128))."""
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
    ap.add_argument("--col", type=int, default=0, help="the covariate x{J} of both steps")
    ap.add_argument("--df", type=int, default=8)
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--boot", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20, help="timed calls of each step")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true",
                    help="one eager fit, then 5 eager launches of each kernel: for a separate "
                         "rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators import cate as DC
    from ate_replication_causalml_amd.estimators.gate import (boot_geometry, gate_phases,
                                                               group_boot, quantile_groups)
    from ate_replication_causalml_amd.estimators.irm import irm_scores
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    dev = torch.device("cuda:0")
    n, K, G, B, d, q, m = int(a.n), a.folds, a.groups, a.boot, a.df, a.degree, a.grid
    blocked = bool(a.blocked) and a.dtype == "bf16"
    pan = synthetic_panel(n, p=a.p, folds=K, seed=a.seed, dtype=a.dtype, device=dev,
                          blocked=blocked, dgp=a.dgp, arm_split=True)
    gid, _ = quantile_groups(pan, a.col, G)
    rid = pan.row_index
    x = pan.col(f"x{a.col}").double().contiguous()
    knots = DC.spline_knots(pan, a.col, d, q)
    xs = torch.sort(x[rid >= 0]).values
    grid = np.linspace(float(xs[(5 * xs.numel()) // 100]), float(xs[(95 * xs.numel()) // 100]), m)
    gbasis = DC.bspline_basis(grid, knots.cpu(), q).to(dev)
    spans = DC.span_counts(x, rid, knots, q)
    DC.check_spans(spans)
    del xs
    torch.cuda.synchronize()
    cate_ph = lambda: DC.cate_phases(pan, x, rid, knots, gbasis, q, K, "min", a.clip, B, 0.95,
                                     a.seed)
    if a.kernels_only:
        st = None
        for ph in cate_ph():
            st = ph(st)
        torch.cuda.synchronize()
        for _ in range(5):
            psi = irm_scores(pan, st["coef"], a.clip, 2)
            mom = DC.cate_moments(psi, x, rid, knots, q)
            buf = DC.cate_boot(psi, x, rid, knots, q, st["beta"], B, a.seed)
            group_boot(psi, gid, rid, G, B, a.seed)
        torch.cuda.synchronize()
        print(json.dumps({"mode": "kernels-only", "n": n, "p": a.p, "df": d, "degree": q,
                          "boot": B, "groups": G, "launches": 6,
                          "geometry": DC.boot_geometry(B, d, pan.ld),
                          "same_bits": bool(torch.equal(buf, st["boot"]) and
                                            torch.equal(mom, st["mom"]))}))
        return
    with plan_slot(0):
        gate = SegmentedStep(gate_phases(pan, gid, rid, G, K, "min", a.clip, B, 0.95, a.seed),
                             graph=True, warmup=1)
    with plan_slot(1):
        cate = SegmentedStep(cate_ph(), graph=True, warmup=1)
    for _ in range(a.warmup):
        gate()
        cate()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    ms = {"gate": [], "cate": [], "moments_kernel": [], "boot_kernel": [], "gate_boot_kernel": []}
    for _ in range(a.calls):                      # alternate: both see the same clocks
        ms["gate"].append(timed(gate)[0])
        ms["cate"].append(timed(cate)[0])
    st = cate()
    fin = st["fin"].cpu().numpy()
    beta = st["beta"].clone()
    psi = irm_scores(pan, st["coef"], a.clip, 2)
    DC.cate_moments(psi, x, rid, knots, q)
    DC.cate_boot(psi, x, rid, knots, q, beta, B, a.seed)
    group_boot(psi, gid, rid, G, B, a.seed)
    torch.cuda.synchronize()
    for _ in range(a.calls):
        ms["moments_kernel"].append(timed(lambda: DC.cate_moments(psi, x, rid, knots, q))[0])
        ms["boot_kernel"].append(
            timed(lambda: DC.cate_boot(psi, x, rid, knots, q, beta, B, a.seed))[0])
        ms["gate_boot_kernel"].append(timed(lambda: group_boot(psi, gid, rid, G, B, a.seed))[0])
    out = {"n": n, "p": a.p, "folds": K, "dtype": a.dtype, "blocked": blocked, "dgp": a.dgp,
           "df": d, "degree": q, "grid": m, "groups": G, "boot": B, "calls": a.calls,
           "graphed": [gate.graphed, cate.graphed], "geometry": DC.boot_geometry(B, d, pan.ld),
           "gate_geometry": boot_geometry(B, G, pan.ld), "span_rows": spans.tolist(),
           "knots": knots.cpu().tolist()}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v)}
    out["ratio_cate_over_gate"] = out["cate"]["median_ms"] / out["gate"]["median_ms"]
    out["ratio_boot_over_gate_boot"] = (out["boot_kernel"]["median_ms"] /
                                        out["gate_boot_kernel"]["median_ms"])
    out["boot_bytes"] = pan.ld * 24
    out["boot_accumulations"] = n * B * (q + 1)
    out["boot_philox_calls"] = n * (-(-B // 128))
    cv, se, crit, o_ate, o_se, nn, b, _ = DC.read_fin(fin, d, m)
    out["cate_minmax"] = [float(cv.min()), float(cv.max())]
    out["se_minmax"] = [float(se.min()), float(se.max())]
    out["crit"], out["overall"], out["coef"] = float(crit), [float(o_ate), float(o_se)], b.tolist()
    out["gate_fin"] = gate()["fin"].cpu().tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
