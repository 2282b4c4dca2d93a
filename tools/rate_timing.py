#!/usr/bin/env python3
"""RATE (AUTOC, QINI, the TOC curve) beside plain DML-IRM on one GPU: ms per captured call of
the ``rate_phases`` step and of ``irm_phases`` on the same arm-split panel (tutorial DGP, bf16
blocked), alternated in one process and timed with device events, plus the entry points alone
as eager launches between events: ``ate_rate_boot`` for a priority of distinct values (every
position ends a run: one fp64 division per position and replicate) and for one of ``--values``
distinct values (that many divisions per replicate in all), and beside them the project's
comparable passes over the same rows -- ``ate_group_boot`` with one group at the same number
of replicates, and the score pass ``ate_irm_scores``. Recorded, not gated:
profiles/rate/README.md.

  python tools/rate_timing.py --n 1e7 --p 500 --boot 200 --grid 10 --calls 20
  rocprofv3 --kernel-trace --stats -- python tools/rate_timing.py ... --kernels-only --case distinct

The JSON line carries the counts that bound the walk for these sizes: the (row, replicate)
updates of one launch (rows x (boot + 1)), the divisions (run ends x included replicates, at
most) and the Philox calls (rows x streams, twice: both walks draw the words)."""
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
    ap.add_argument("--boot", type=int, default=200)
    ap.add_argument("--grid", type=int, default=10, help="points of the TOC curve")
    ap.add_argument("--values", type=int, default=32, help="distinct values of the tied priority")
    ap.add_argument("--calls", type=int, default=20, help="timed calls of each step")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--case", default="both", choices=["both", "distinct", "valued"],
                    help="--kernels-only: which priority the launches walk")
    ap.add_argument("--kernels-only", action="store_true",
                    help="one eager fit, then 5 eager launches of each entry point: for a "
                         "separate rocprofv3 run (kernel trace, or counters)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators import rate as DR
    from ate_replication_causalml_amd.estimators.gate import boot_geometry, group_boot
    from ate_replication_causalml_amd.estimators.irm import irm_phases, irm_scores, run_phases
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    dev = torch.device(a.device)
    n, K, B, Q = int(a.n), a.folds, a.boot, a.grid
    blocked = bool(a.blocked) and a.dtype == "bf16"
    pan = synthetic_panel(n, p=a.p, folds=K, seed=a.seed, dtype=a.dtype, device=dev,
                          blocked=blocked, dgp=a.dgp, arm_split=True)
    rid = pan.row_index
    grid = np.arange(1, Q + 1) / Q
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    prio = {"distinct": torch.randperm(pan.ld, generator=gen, device=dev).double(),
            "valued": torch.randint(0, a.values, (pan.ld,), generator=gen, device=dev).double()}
    ranks = {k: DR.rate_order(v, rid, None, grid) for k, v in prio.items()}
    gid1 = torch.where(rid >= 0, 0, -1).to(torch.int32)          # one group: every real row

    def phases(case):
        return DR.rate_phases(pan, rid, *ranks[case], Q, K, "min", a.clip, B, 0.95, a.seed)

    st = run_phases(phases("distinct"))
    coef, psi = st["coef"], st["psi"] - st["shift"]
    cases = ("distinct", "valued") if a.case == "both" else (a.case,)
    info = {"n": n, "p": a.p, "folds": K, "dtype": a.dtype, "blocked": blocked, "dgp": a.dgp,
            "boot": B, "grid": Q, "values": a.values, "ld": pan.ld,
            "geometry": DR.rate_geometry(B, n), "group_geometry": boot_geometry(B, 1, pan.ld),
            "runs": {k: int((f & 1).sum().item()) for k, (_, f) in ranks.items()},
            "walk_updates": n * (B + 1), "philox_calls": 2 * n * (B // 128 + 1)}
    if dev.type != "cuda":
        raise SystemExit("the set-up runs anywhere; the timings need the GPU")
    torch.cuda.synchronize()
    if a.kernels_only:
        for _ in range(5):
            irm_scores(pan, coef, a.clip, 2)
            group_boot(psi, gid1, rid, 1, B, a.seed)
            for c in cases:
                buf = DR.rate_boot(psi, *ranks[c], rid, Q, B, a.seed)
        torch.cuda.synchronize()
        print(json.dumps({"mode": "kernels-only", "cases": cases, "launches": 5, **info,
                          "same_bits": bool(torch.equal(buf, st["boot"])) if
                          cases[-1] == "distinct" else None,
                          "fin": DR.rate_finalize(buf, st["shift"], B).cpu().tolist()}))
        return
    with plan_slot(0):
        irm = SegmentedStep(irm_phases(pan, K, "min", a.clip), graph=True, warmup=1)
    with plan_slot(1):
        rate = SegmentedStep(phases("distinct"), graph=True, warmup=1)
    for _ in range(a.warmup):
        irm()
        rate()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    steps = {"irm": irm, "rate": rate,
             "scores_kernel": lambda: irm_scores(pan, coef, a.clip, 2),
             "group_boot_g1": lambda: group_boot(psi, gid1, rid, 1, B, a.seed),
             "rate_boot_distinct": lambda: DR.rate_boot(psi, *ranks["distinct"], rid, Q, B, a.seed),
             "rate_boot_valued": lambda: DR.rate_boot(psi, *ranks["valued"], rid, Q, B, a.seed),
             "rate_order_distinct": lambda: DR.rate_order(prio["distinct"], rid, None, grid)}
    for fn in steps.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(a.calls):                      # alternate: all see the same clocks
        for k, fn in steps.items():
            ms[k].append(timed(fn)[0])
    out = {**info, "calls": a.calls, "graphed": [irm.graphed, rate.graphed]}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v)}
    out["ratio_rate_over_irm"] = out["rate"]["median_ms"] / out["irm"]["median_ms"]
    out["irm_res"] = irm()["res"].cpu().tolist()
    out["rate_fin"] = rate()["fin"].cpu().tolist()
    out["valued_fin"] = DR.rate_finalize(steps["rate_boot_valued"](), st["shift"], B).cpu().tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
