#!/usr/bin/env python3
"""Group ATEs with a joint band beside plain DML-IRM on one GPU: ms per captured call of
``irm_gate_panel`` and ``irm_crossfit_panel`` on the same arm-split panel (tutorial DGP,
bf16 blocked), alternated in one process and timed with device events, plus the two new
kernels alone (``ate_irm_scores``, ``ate_group_boot``) timed as eager launches between
events. Recorded, not gated: profiles/gate/README.md.

  python tools/gate_timing.py --n 1e7 --p 500 --groups 8 --boot 1024 --calls 20

The JSON line carries the three bounds of the bootstrap kernel for these sizes: the bytes it
reads (rows x 20: psi, group, row id), the (row, replicate) accumulations and the Philox
calls (rows x ceil(boot / 128))."""
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
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--gate-col", type=int, default=0)
    ap.add_argument("--boot", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20, help="timed calls of each step")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true",
                    help="one eager fit, then 5 eager launches of each new kernel: for a "
                         "separate rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators.gate import (boot_geometry, gate_phases,
                                                               group_boot, group_counts,
                                                               quantile_groups)
    from ate_replication_causalml_amd.estimators.irm import irm_phases, irm_scores
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    dev = torch.device("cuda:0")
    n, K, G, B = int(a.n), a.folds, a.groups, a.boot
    blocked = bool(a.blocked) and a.dtype == "bf16"
    pan = synthetic_panel(n, p=a.p, folds=K, seed=a.seed, dtype=a.dtype, device=dev,
                          blocked=blocked, dgp=a.dgp, arm_split=True)
    gid, _ = quantile_groups(pan, a.gate_col, G)
    rid = pan.row_index
    counts = group_counts(gid, G)
    torch.cuda.synchronize()
    if a.kernels_only:
        st = None
        for ph in gate_phases(pan, gid, rid, G, K, "min", a.clip, B, 0.95, a.seed):
            st = ph(st)
        torch.cuda.synchronize()
        for _ in range(5):
            psi = irm_scores(pan, st["coef"], a.clip, 2)
            buf = group_boot(psi, gid, rid, G, B, a.seed)
        torch.cuda.synchronize()
        print(json.dumps({"mode": "kernels-only", "n": n, "p": a.p, "groups": G, "boot": B,
                          "launches": 6, "geometry": boot_geometry(B, G, pan.ld),
                          "same_bits": bool(torch.equal(buf, st["boot"])),
                          "fin": st["fin"].cpu().tolist()}))
        return
    with plan_slot(0):
        irm = SegmentedStep(irm_phases(pan, K, "min", a.clip), graph=True, warmup=1)
    with plan_slot(1):
        gate = SegmentedStep(gate_phases(pan, gid, rid, G, K, "min", a.clip, B, 0.95, a.seed),
                             graph=True, warmup=1)
    for _ in range(a.warmup):
        irm()
        gate()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    ms = {"irm": [], "gate": [], "scores_kernel": [], "boot_kernel": []}
    for _ in range(a.calls):                      # alternate: both see the same clocks
        ms["irm"].append(timed(irm)[0])
        ms["gate"].append(timed(gate)[0])
    st = gate()
    coef = st["coef"]
    psi = irm_scores(pan, coef, a.clip, 2)
    group_boot(psi, gid, rid, G, B, a.seed)
    torch.cuda.synchronize()
    for _ in range(a.calls):
        ms["scores_kernel"].append(timed(lambda: irm_scores(pan, coef, a.clip, 2))[0])
        ms["boot_kernel"].append(timed(lambda: group_boot(psi, gid, rid, G, B, a.seed))[0])
    out = {"n": n, "p": a.p, "folds": K, "dtype": a.dtype, "blocked": blocked, "dgp": a.dgp,
           "groups": G, "boot": B, "calls": a.calls, "graphed": [irm.graphed, gate.graphed],
           "geometry": boot_geometry(B, G, pan.ld), "group_rows": counts.tolist()}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v)}
    out["ratio_gate_over_irm"] = out["gate"]["median_ms"] / out["irm"]["median_ms"]
    out["boot_bytes"] = pan.ld * 20
    out["boot_accumulations"] = n * B
    out["boot_philox_calls"] = n * (-(-B // 128))
    out["irm_res"] = irm()["res"].cpu().tolist()
    out["gate_fin"] = gate()["fin"].cpu().tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
