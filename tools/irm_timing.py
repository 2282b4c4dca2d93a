#!/usr/bin/env python3
"""DML-IRM beside DML-PLR on one GPU: ms per captured call of ``irm_crossfit_panel`` and
``dml_crossfit_panel`` on the same rows (tutorial DGP, bf16 blocked panels), alternated in
one process and timed with device events. Recorded, not gated: profiles/irm/README.md.

  python tools/irm_timing.py --n 1e7 --p 500 --calls 20

``--score-only``: a few eager launches of the fused score pass alone after one fit, for a
separate ``rocprofv3 --kernel-trace --stats -- python tools/irm_timing.py --score-only``
run; the JSON line carries the bytes the pass reads, rows x (union support + 5 columns) x 2
summed over the folds, to turn the kernel's time into bytes/s.

``--repeats S``: repeated cross-fitting (``irm_repeated_phases`` on the 2 K*K micro-arm panel)
beside what a user without it must do, S single-partition calls of ``irm_phases`` on the
same rows: one captured repeated call and S captured single calls, alternated. With
``--score-only``: after one repeated fit, the fused multi-split score pass
(``irm_score_multi*`` kernels) and S launches of ``ate_irm_score_moments`` on the same panel
and coefficients, for the kernel trace; the JSON line carries each side's unique bytes.
Recorded in profiles/irm_repeated/README.md.

``--targets T,T,...``: the target populations (``estimators/targets.py``) beside the plain ATE
on the same arm-split panel: one captured ``target_phases`` call (only the nuisances the
targets need) and one captured ``irm_phases`` call, alternated; then, on the coefficients of
one full fit, the 12-moment pass (``ate_irm_target_moments``) and the 8-moment pass
(``ate_irm_score_moments``), alternated in batches of ``--pass-batch`` back-to-back launches
between two device events (one launch is ~0.1 ms: too short a window on its own). With
``--score-only``: after one full fit, 5 launches of each pass, alternated, for a separate
``rocprofv3 --kernel-trace --stats`` run (the two instantiations are told apart by their
template argument: 0 = the 8 moments, 3 = the 12). Recorded in profiles/irm_targets/README.md.

``--iivm``: the LATE of the interactive IV model (``estimators/late.py``) beside the plain ATE
on the same arm-split panel, whose W is taken as the instrument and whose binary covariate
x{--iivm-col} as the treatment taken (removed from the covariates): one captured
``late_phases`` call and one captured ``irm_phases`` call, alternated; then the 15-moment pass
(``ate_iivm_moments``) and the 8-moment pass on the coefficients of those fits, alternated in
batches as for ``--targets``. The JSON line carries both union sizes and the bytes each pass
reads. Recorded in profiles/iivm/README.md.

``--propensity logit``: the binomial CV-LASSO propensity (fp32 / fp64 panels, p <= 96) beside
the linear one on the same arm-split panel: one captured ``irm_phases`` call each, alternated;
the grouped path launch of ``cv_lognet_groups`` (K * K problems, one launch) beside what there
was without it, K ``cv_lognet`` calls back to back on the K training panels (plain K-fold
panels of the same rows without fold k), alternated; and the logistic-link score pass beside
the identity one on the same coefficients, alternated in batches as for ``--targets``.
Recorded in profiles/irm_logit/README.md.

``--apos L``: the mean potential outcomes of an L-arm treatment (``estimators/apos.py``) on a
host-built level-split panel of ``data.dgp.make_multiarm_data`` (n rows, p covariates, --dtype;
column-major): the captured ``apos_phases`` call, its fit phase alone (the path launch or
launches with their glue) on the call's Gram stack, and the potential-outcome pass
(``ate_apo_moments``) in batches as for ``--targets``. At L = 2 the 8-moment pass
(``ate_irm_score_moments``) runs on the same panel with the rows (g_0, g_1, m_1), alternated
with it in the same process, and the JSON line says whether the shared sums have the same
bits. Recorded in profiles/apos/README.md.

``--pliv q``: the partially linear IV model with q instruments (``estimators/pliv.py``) beside
PLR on the same plain K-fold panel (the covariates x0..x{q-1} are the instruments and leave the
covariates; the panel's W is the treatment): one captured ``pliv_phases`` call and one captured
``dml_phases`` call, alternated; the PLIV fit phase alone (its path launch or launches); then
the PLIV pass (``ate_pliv_moments``, its finishing launch included) and PLR's 7-moment pass
(``ate_dml_resid_moments``) with the picked coefficients, in batches as for ``--targets``. The
JSON line carries the pass's byte model (rows x (union of supports + 2 (2 + q) + 1 target and
valid columns) x element size) and its rate. Recorded in profiles/pliv/README.md.

``--clusters``: the cluster-robust call (``estimators/cluster.py``) beside the plain ATE on the
same arm-split panel, for four cluster-size profiles over the panel's real rows (singletons,
households of 1-6, 50 equal clusters, one cluster of half the rows plus singletons; clusters
are consecutive runs of panel rows, the shape the front end produces): per profile the two
launches of the cluster pass (``ate_cluster_moments``) and, once, the per-row score pass
(``ate_irm_scores``) and the 8-moment pass, in batches as for ``--targets``; then one captured
clustered call per profile and one captured ``irm_phases`` call, alternated. The JSON line
carries the pass's byte model (12 n + 8 J) and its rate. With ``--score-only``: after one fit, 5
launches of the cluster pass per profile and of the score pass, for a separate ``rocprofv3
--kernel-trace --stats`` run (the two cluster kernels are told apart by name). Recorded in
profiles/cluster/README.md."""
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
    ap.add_argument("--calls", type=int, default=20, help="timed calls of each estimator")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--score-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=0, help="S > 0: time repeated cross-fitting")
    ap.add_argument("--targets", default=None, metavar="T,T,...",
                    help="time the target populations (all, treated, control) beside the ATE")
    ap.add_argument("--pass-batch", type=int, default=20,
                    help="--targets / --iivm: back-to-back launches per timed sample of a pass")
    ap.add_argument("--iivm", action="store_true",
                    help="time the LATE of the interactive IV model beside the ATE")
    ap.add_argument("--iivm-col", type=int, default=16,
                    help="--iivm: the exactly-binary covariate x{J} taken as the treatment D")
    ap.add_argument("--apos", type=int, default=0, metavar="L",
                    help="time the potential outcomes of an L-arm treatment (2..8)")
    ap.add_argument("--pliv", type=int, default=0, metavar="q",
                    help="time the partially linear IV model with q instruments (1..4)")
    ap.add_argument("--propensity", default="linear", choices=["linear", "logit"],
                    help="logit: time the binomial CV-LASSO propensity beside the linear one")
    ap.add_argument("--clusters", action="store_true",
                    help="time the cluster-robust call for four cluster-size profiles")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators.irm import irm_phases, irm_score_moments
    from ate_replication_causalml_amd.estimators.lasso import dml_phases
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    dev = torch.device("cuda:0")
    n, K = int(a.n), a.folds
    blocked = bool(a.blocked) and a.dtype == "bf16"
    kw = dict(p=a.p, folds=K, seed=a.seed, dtype=a.dtype, device=dev, blocked=blocked, dgp=a.dgp)
    if a.apos:
        return apos(a, n, K)
    if a.pliv:
        return pliv(a, n, K, kw)
    if a.clusters:
        return clusters(a, n, K, kw)
    if a.repeats > 0:
        return repeated(a, n, K, kw)
    if a.targets is not None:
        return targets(a, n, K, kw)
    if a.iivm:
        return iivm(a, n, K, kw)
    if a.propensity == "logit":
        return propensity(a, n, K, kw)
    split = synthetic_panel(n, arm_split=True, **kw)
    torch.cuda.synchronize()

    def support_bytes(coef):
        # rows x (union support + 5 columns: one, Y hi / lo, W hi / lo) x 2 bytes, per fold
        nnz = (coef[:, :, 1:] != 0).any(1).sum(1).cpu().numpy()
        rows = np.asarray(split.seg_nreal).reshape(K, 2).sum(1)
        return nnz.tolist(), int((rows * (nnz + 5) * 2).sum())

    if a.score_only:
        st = None
        for ph in irm_phases(split, K, "min", a.clip):
            st = ph(st)
        torch.cuda.synchronize()
        for _ in range(5):
            mom = irm_score_moments(split, st["coef"], a.clip, 2)
        torch.cuda.synchronize()
        nnz, nbytes = support_bytes(st["coef"])
        print(json.dumps({"mode": "score-only", "n": n, "p": a.p, "launches": 6,
                          "union_support": nnz, "score_bytes": nbytes,
                          "res": st["res"].cpu().tolist(), "mom": mom.cpu().tolist()}))
        return
    plain = synthetic_panel(n, selection=split.selection, **kw)
    with plan_slot(0):
        plr = SegmentedStep(dml_phases(plain, K, "min"), graph=True, warmup=1)
    with plan_slot(1):
        irm = SegmentedStep(irm_phases(split, K, "min", a.clip), graph=True, warmup=1)
    for _ in range(a.warmup):
        plr()
        irm()
    torch.cuda.synchronize()
    ms = {"plr": [], "irm": []}
    for _ in range(a.calls):                      # alternate: both see the same clocks
        for name, step in (("plr", plr), ("irm", irm)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st = step()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    nnz, nbytes = support_bytes(irm()["coef"])
    torch.cuda.synchronize()
    out = {"n": n, "p": a.p, "folds": K, "dtype": a.dtype, "blocked": blocked, "dgp": a.dgp,
           "calls": a.calls, "graphed": [plr.graphed, irm.graphed]}
    for name in ms:
        v = ms[name]
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v)}
    out["ratio_irm_over_plr"] = out["irm"]["median_ms"] / out["plr"]["median_ms"]
    out["plr_res"] = plr()["res"].cpu().tolist()
    out["irm_res"] = irm()["res"].cpu().tolist()
    out["irm_mom"] = irm()["mom"].cpu().tolist()
    out["union_support"], out["score_bytes"] = nnz, nbytes
    print(json.dumps(out))


def repeated(a, n, K, kw):
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators import irm as DI
    from ate_replication_causalml_amd.estimators.lasso import micro_fold_map
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    S = a.repeats
    micro = synthetic_panel(n, arm_split=True, **{**kw, "folds": K * K})
    torch.cuda.synchronize()
    out = {"n": n, "p": a.p, "folds": K, "repeats": S, "dtype": a.dtype,
           "blocked": kw["blocked"], "dgp": a.dgp}
    if a.score_only:
        st = DI.run_phases(DI.irm_repeated_phases(micro, K, S, "min", a.clip))
        torch.cuda.synchronize()
        coef = st["coef"]
        blk = np.stack([s * K + micro_fold_map(K, s) for s in range(S)])
        gathered = [coef.index_select(0, torch.as_tensor(b, device=coef.device)).contiguous()
                    for b in blk]
        for _ in range(5):                      # alternate: both see the same clocks
            fused = DI.irm_score_moments_multi(micro, coef, blk, a.clip, 2)
            single = torch.stack([DI.irm_score_moments(micro, c, a.clip, 2) for c in gathered])
        torch.cuda.synchronize()
        rows = np.asarray(micro.seg_nreal).reshape(K * K, 2).sum(1)
        sup = np.stack([(c[:, :, 1:] != 0).any(1).cpu().numpy() for c in gathered])  # [S, K*K, p]
        out.update(mode="score-only", launches_each=5, smax=DI.score_multi_smax(),
                   fused_bytes=int((rows * (sup.any(0).sum(1) + 5) * 2).sum()),
                   single_bytes=int((rows[None] * (sup.sum(2) + 5) * 2).sum()),
                   union_support_mean=float(sup.any(0).sum(1).mean()),
                   split_support_mean=float(sup.sum(2).mean()),
                   same_bits=bool(torch.equal(fused, single)),
                   splits=st["splits"].cpu().tolist(), mom=fused.cpu().tolist())
        print(json.dumps(out))
        return
    split = synthetic_panel(n, arm_split=True, selection=micro.selection, **kw)
    torch.cuda.synchronize()
    with plan_slot(0):
        one = SegmentedStep(DI.irm_phases(split, K, "min", a.clip), graph=True, warmup=1)
    with plan_slot(1):
        rep = SegmentedStep(DI.irm_repeated_phases(micro, K, S, "min", a.clip), graph=True,
                            warmup=1)
    for _ in range(a.warmup):
        one()
        rep()
    torch.cuda.synchronize()
    ms = {"single_x_S": [], "single": [], "repeated": []}
    for _ in range(a.calls):                      # alternate: both see the same clocks
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(S + 3)]
        ev[0].record()
        for s in range(S):
            one()
            ev[1 + s].record()
        rep()
        ev[S + 1].record()
        torch.cuda.synchronize()
        ms["single_x_S"].append(ev[0].elapsed_time(ev[S]))
        ms["single"] += [ev[s].elapsed_time(ev[s + 1]) for s in range(S)]
        ms["repeated"].append(ev[S].elapsed_time(ev[S + 1]))
    out.update(calls=a.calls, graphed=[one.graphed, rep.graphed])
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v), "spread_ms": max(v) - min(v)}
    out["saved_ms"] = out["single_x_S"]["median_ms"] - out["repeated"]["median_ms"]
    st = rep()
    out["res"], out["splits"] = st["res"].cpu().tolist(), st["splits"].cpu().tolist()
    out["single_res"] = one()["res"].cpu().tolist()
    print(json.dumps(out))


def targets(a, n, K, kw):
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators import irm as DI
    from ate_replication_causalml_amd.estimators import targets as DT
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.result import TargetResult, check_targets
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    tg = check_targets([t for t in a.targets.split(",") if t])
    split = synthetic_panel(n, arm_split=True, **kw)
    torch.cuda.synchronize()
    if a.score_only:
        coef = DI.run_phases(DI.irm_phases(split, K, "min", a.clip))["coef"]
        torch.cuda.synchronize()
        for _ in range(5):                        # alternate: both see the same clocks
            m8 = DI.irm_score_moments(split, coef, a.clip, 2)
            m12 = DI.irm_target_moments(split, coef, a.clip, 2)
        torch.cuda.synchronize()
        print(json.dumps({"mode": "score-only", "n": n, "p": a.p, "launches_each": 5,
                          "union_support": (coef[:, :, 1:] != 0).any(1).sum(1).cpu().tolist(),
                          "shared_bits": bool(torch.equal(m12[[0, 1, 2, 3, 11]],
                                                          m8[[0, 1, 2, 3, 7]])),
                          "mom8": m8.cpu().tolist(), "mom12": m12.cpu().tolist()}))
        return
    with plan_slot(0):
        ate = SegmentedStep(DI.irm_phases(split, K, "min", a.clip), graph=True, warmup=1)
    with plan_slot(1):
        tar = SegmentedStep(DT.target_phases(split, K, tg, "min", a.clip), graph=True, warmup=1)
    for _ in range(a.warmup):
        ate()
        tar()
    torch.cuda.synchronize()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    ms = {"irm_call": [], "targets_call": [], "pass8": [], "pass12": []}
    for _ in range(a.calls):                      # alternate: both see the same clocks
        ms["irm_call"].append(timed(ate)[0])
        ms["targets_call"].append(timed(tar)[0])
    coef = ate()["coef"].clone()                  # every nuisance: both passes read the same columns
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        DI.irm_score_moments(split, coef, a.clip, 2)
        DI.irm_target_moments(split, coef, a.clip, 2)
    torch.cuda.synchronize()
    nb = max(a.pass_batch, 1)

    def batch(f):
        def g():
            for _ in range(nb):
                out = f(split, coef, a.clip, 2)
            return out
        return g

    for _ in range(a.calls):                      # per launch: a batch's time over its size
        t8, m8 = timed(batch(DI.irm_score_moments))
        t12, m12 = timed(batch(DI.irm_target_moments))
        ms["pass8"].append(t8 / nb)
        ms["pass12"].append(t12 / nb)
    out = {"n": n, "p": a.p, "folds": K, "dtype": a.dtype, "blocked": kw["blocked"],
           "dgp": a.dgp, "targets": list(tg), "nuisances": list(DT.target_nuisances(tg)),
           "calls": a.calls, "pass_batch": nb, "graphed": [ate.graphed, tar.graphed]}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v)}
    out["ratio_targets_over_irm_call"] = out["targets_call"]["median_ms"] / out["irm_call"]["median_ms"]
    out["ratio_pass12_over_pass8"] = out["pass12"]["median_ms"] / out["pass8"]["median_ms"]
    out["shared_bits"] = bool(torch.equal(m12[[0, 1, 2, 3, 11]], m8[[0, 1, 2, 3, 7]]))
    r = TargetResult.from_moments("targets", tar()["mom"].cpu().numpy(), tg)
    out["estimates"] = r.rows()
    out["irm_res"] = ate()["res"].cpu().tolist()
    print(json.dumps(out))


def propensity(a, n, K, kw):
    import dataclasses
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators import irm as DI
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.ops.lognet import cv_lognet, cv_lognet_groups
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    split = synthetic_panel(n, arm_split=True, **kw)
    plain = synthetic_panel(n, selection=split.selection, **kw)
    torch.cuda.synchronize()
    with plan_slot(0):
        lin = SegmentedStep(DI.irm_phases(split, K, "min", a.clip), graph=True, warmup=1)
    with plan_slot(1):
        logit = SegmentedStep(DI.irm_phases(split, K, "min", a.clip, propensity="logit"),
                              graph=True, warmup=1)
    for _ in range(a.warmup):
        lin()
        logit()
    torch.cuda.synchronize()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    ms = {"linear_call": [], "logit_call": [], "grouped_path": [], "k_launches": [],
          "pass_identity": [], "pass_logistic": []}
    for _ in range(a.calls):                      # alternate: both see the same clocks
        ms["linear_call"].append(timed(lin)[0])
        ms["logit_call"].append(timed(logit)[0])
    # the K training panels of the alternative: the plain K-fold panel without fold k
    keep = [[j for j in range(K) if j != k] for k in range(K)]
    trains = [dataclasses.replace(plain, seg_bounds=np.asarray(plain.seg_bounds)[kk],
                                  seg_nreal=np.asarray(plain.seg_nreal)[kk]) for kk in keep]
    sets = DI.logit_fold_sets(K)
    wcol = split.cols["W"]

    def grouped():
        return cv_lognet_groups(split, split.xcols, wcol, sets)

    def k_launches():
        return [cv_lognet(t, t.xcols, t.cols["W"]) for t in trains]

    for _ in range(a.warmup):
        g = grouped()
        kl = k_launches()
    torch.cuda.synchronize()
    for _ in range(a.calls):
        ms["grouped_path"].append(timed(grouped)[0])
        ms["k_launches"].append(timed(k_launches)[0])
    same_sel = [g.sel[k].cpu().tolist() == kl[k].sel.cpu().tolist() for k in range(K)]
    coef = logit()["coef"].clone()
    torch.cuda.synchronize()
    nb = max(a.pass_batch, 1)

    def batch(link):
        def f():
            for _ in range(nb):
                out = DI.irm_score_moments(split, coef, a.clip, 2, link=link)
            return out
        return f

    for _ in range(a.warmup):
        batch("identity")()
        batch("logistic")()
    torch.cuda.synchronize()
    for _ in range(a.calls):                      # per launch: a batch's time over its size
        ms["pass_identity"].append(timed(batch("identity"))[0] / nb)
        ms["pass_logistic"].append(timed(batch("logistic"))[0] / nb)
    out = {"n": n, "p": a.p, "folds": K, "dtype": a.dtype, "dgp": a.dgp, "calls": a.calls,
           "pass_batch": nb, "graphed": [lin.graphed, logit.graphed],
           "grouped_equals_k_launches_sel": same_sel}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v)}
    out["ratio_logit_over_linear_call"] = out["logit_call"]["median_ms"] / out["linear_call"]["median_ms"]
    out["ratio_k_launches_over_grouped"] = out["k_launches"]["median_ms"] / out["grouped_path"]["median_ms"]
    out["ratio_pass_logistic_over_identity"] = (out["pass_logistic"]["median_ms"]
                                                / out["pass_identity"]["median_ms"])
    out["linear_res"] = lin()["res"].cpu().tolist()
    out["logit_res"] = logit()["res"].cpu().tolist()
    out["logit_mom"] = logit()["mom"].cpu().tolist()
    print(json.dumps(out))


def iivm(a, n, K, kw):
    import dataclasses
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators import irm as DI
    from ate_replication_causalml_amd.estimators import late as DL
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.result import LateResult
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    split = synthetic_panel(n, arm_split=True, **kw)
    torch.cuda.synchronize()
    # the panel's W is the instrument; the binary covariate x{iivm_col} (vote history, so the
    # first stage has covariates to select) is the treatment taken and leaves the covariates.
    # A binary column is its own hi part; its lo part is W's, which is all zero.
    c = split.cols[f"x{a.iivm_col}"]
    d = split.col(f"x{a.iivm_col}")
    assert bool(((d == 0) | (d == 1)).all()), "the D column must be exactly binary"
    cols = {**split.cols, "D": c}
    if split.dtype == torch.bfloat16:
        cols.update(D_hi=c, D_lo=split.cols["W_lo"])
    pan = dataclasses.replace(split, cols=cols, xcols=[x for x in split.xcols if x != c])
    rows = np.asarray(split.seg_nreal).reshape(K, 2).sum(1)

    def nbytes(coef, ntarget):
        # rows x (union support + target columns incl. `one`) x 2 bytes, per fold
        nnz = (coef[:, :, 1:] != 0).any(1).sum(1).cpu().numpy()
        return nnz.tolist(), int((rows * (nnz + ntarget) * 2).sum())

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    with plan_slot(0):
        ate = SegmentedStep(DI.irm_phases(split, K, "min", a.clip), graph=True, warmup=1)
    with plan_slot(1):
        lat = SegmentedStep(DL.late_phases(pan, K, "min", a.clip), graph=True, warmup=1)
    for _ in range(a.warmup):
        ate()
        lat()
    torch.cuda.synchronize()
    ms = {"irm_call": [], "iivm_call": [], "pass8": [], "pass15": []}
    for _ in range(a.calls):                      # alternate: both see the same clocks
        ms["irm_call"].append(timed(ate)[0])
        ms["iivm_call"].append(timed(lat)[0])
    c3, c5 = ate()["coef"].clone(), lat()["coef"].clone()
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        DI.irm_score_moments(split, c3, a.clip, 2)
        DL.iivm_moments(pan, c5, a.clip, 2)
    torch.cuda.synchronize()
    nb = max(a.pass_batch, 1)

    def batch(f, *args):
        def g():
            for _ in range(nb):
                out = f(*args, a.clip, 2)
            return out
        return g

    for _ in range(a.calls):                      # per launch: a batch's time over its size
        t8, m8 = timed(batch(DI.irm_score_moments, split, c3))
        t15, m15 = timed(batch(DL.iivm_moments, pan, c5))
        ms["pass8"].append(t8 / nb)
        ms["pass15"].append(t15 / nb)
    out = {"n": n, "p": a.p, "folds": K, "dtype": a.dtype, "blocked": kw["blocked"],
           "dgp": a.dgp, "iivm_col": a.iivm_col, "calls": a.calls, "pass_batch": nb,
           "graphed": [ate.graphed, lat.graphed]}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v)}
    out["union8"], out["bytes8"] = nbytes(c3, 5)       # one, Y hi / lo, W hi / lo
    out["union15"], out["bytes15"] = nbytes(c5, 7)     # and D hi / lo
    for k, b in (("pass8", "bytes8"), ("pass15", "bytes15")):
        out[k]["TB_per_s"] = out[b] / (out[k]["median_ms"] * 1e-3) / 1e12
    # the moments shared with the AIPW pass on the same covariates, bit for bit
    base = DI.irm_score_moments(pan, c5[:, [0, 1, 4]].contiguous(), a.clip, 2)
    out["shared_bits"] = bool(torch.equal(m15[[0, 1, 2, 3, 7, 10, 11, 14]],
                                          base[[0, 1, 2, 3, 7, 4, 5, 6]]))
    r = LateResult.from_moments("iivm", lat()["mom"].cpu().numpy())
    out["late"] = json.loads(r.json())
    out["irm_res"] = ate()["res"].cpu().tolist()
    print(json.dumps(out))


def cluster_profiles(nv, seed):
    """name -> cluster sizes summing to nv, the four profiles of ``--clusters``."""
    import numpy as np
    rs = np.random.default_rng(seed)
    hh = rs.integers(1, 7, size=nv // 3 + 8)
    hh = hh[:int(np.searchsorted(np.cumsum(hh), nv)) + 1]
    hh[-1] -= hh.sum() - nv
    eq = np.full(50, nv // 50)
    eq[:nv % 50] += 1
    return {"singletons": np.ones(nv, dtype=np.int64), "households_1_6": hh[hh > 0],
            "equal_50": eq, "half_plus_singletons": np.r_[nv // 2, np.ones(nv - nv // 2,
                                                                           dtype=np.int64)]}


def clusters(a, n, K, kw):
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators import cluster as DC
    from ate_replication_causalml_amd.estimators import irm as DI
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.utils.graphs import GraphedStep, SegmentedStep
    split = synthetic_panel(n, arm_split=True, **kw)
    torch.cuda.synchronize()
    dev = split.device
    order = torch.nonzero(split.row_index >= 0).flatten().to(torch.int32)   # panel rows, ascending
    nv = order.numel()
    prof = {}
    for name, sizes in cluster_profiles(nv, a.seed).items():
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        assert starts[-1] == nv
        prof[name] = (torch.from_numpy(starts).to(dev), len(sizes), int(sizes.max()))
    counts = tuple(float(c) for c in split.seg_nreal)
    st = DI.run_phases(DI.irm_phases(split, K, "min", a.clip))
    coef, theta = st["coef"].clone(), st["res"][:1].clone()
    psi = DI.irm_scores(split, coef, a.clip, 2)
    torch.cuda.synchronize()
    out = {"mode": "clusters", "n": nv, "p": a.p, "folds": K, "dtype": a.dtype,
           "blocked": kw["blocked"], "dgp": a.dgp, "chunk": DC.cluster_chunk(),
           "irm_res": st["res"].cpu().tolist(), "profiles": {}}
    if a.score_only:
        for name, (starts, J, _) in prof.items():
            for _ in range(5):
                mom = DC.cluster_moments(psi, None, starts, order, J, theta)
            out["profiles"][name] = {"J": J, "moments": mom.cpu().tolist()}
        for _ in range(5):
            DI.irm_scores(split, coef, a.clip, 2)
        torch.cuda.synchronize()
        out["launches_each"] = 5
        print(json.dumps(out))
        return

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    nb = max(a.pass_batch, 1)

    def batch(f):
        def g():
            for _ in range(nb):
                r = f()
            return r
        return g

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                "mean_ms": statistics.fmean(v)}

    passes = {name: batch(lambda s=starts, J=J: DC.cluster_moments(psi, None, s, order, J, theta))
              for name, (starts, J, _) in prof.items()}
    passes["scores"] = batch(lambda: DI.irm_scores(split, coef, a.clip, 2))
    passes["moments8"] = batch(lambda: DI.irm_score_moments(split, coef, a.clip, 2))
    for _ in range(a.warmup):
        for f in passes.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in passes}
    for _ in range(a.calls):                      # alternate: all see the same clocks
        for k, f in passes.items():
            ms[k].append(timed(f)[0] / nb)
    out["pass_batch"], out["calls"] = nb, a.calls
    out["scores_pass"], out["moments8_pass"] = stats(ms["scores"]), stats(ms["moments8"])
    with plan_slot(0):
        plain = SegmentedStep(DI.irm_phases(split, K, "min", a.clip), graph=True, warmup=1)
    calls = {}
    with plan_slot(1):
        for name, (starts, J, _) in prof.items():
            calls[name] = GraphedStep(lambda s=starts, J=J: DC._irm_cluster_body(
                split, s, order, K, "min", a.clip, J, counts), warmup=1)
    for _ in range(a.warmup):
        plain()
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    cms = {k: [] for k in ("plain", *calls)}
    for _ in range(a.calls):
        cms["plain"].append(timed(plain)[0])
        for k, c in calls.items():
            cms[k].append(timed(c)[0])
    out["plain_call"] = stats(cms["plain"])
    out["graphed"] = plain.graphed
    for name, (starts, J, nmax) in prof.items():
        r = calls[name]().cpu().tolist()
        p_ms = statistics.median(ms[name])
        model = 12 * nv + 8 * J
        out["profiles"][name] = {
            "J": J, "max_cluster": nmax, "cluster_pass": stats(ms[name]), "call": stats(cms[name]),
            "added_ms_over_plain_call": statistics.median(cms[name]) - out["plain_call"]["median_ms"],
            "model_bytes": model, "TB_per_s": model / (p_ms * 1e-3) / 1e12,
            "theta_se_se0": r[:3], "cluster_moments": r[3:7]}
    base = out["profiles"]["singletons"]["cluster_pass"]["median_ms"]
    for v in out["profiles"].values():
        v["pass_over_singletons"] = v["cluster_pass"]["median_ms"] / base
    print(json.dumps(out))


def apos(a, n, K):
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.dgp import make_multiarm_data
    from ate_replication_causalml_amd.estimators import apos as DA
    from ate_replication_causalml_amd.estimators import irm as DI
    from ate_replication_causalml_amd.ops.panel import build_panel
    from ate_replication_causalml_amd.parallel import rng
    from ate_replication_causalml_amd.result import ApoResult, apo_layout
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    L = a.apos
    dev = torch.device("cuda:0")
    d = make_multiarm_data(n, a.seed, levels=L, p_extra=max(a.p - 21, 0))
    level = d.D.astype(np.int64)
    seg = L * rng.fold_ids(n, K, a.seed, 0) + level
    # the panel of level_split_panel with the level in column W too, for the 8-moment pass
    tg = {"D": d.D, **{f"I{c}": (level == c).astype(np.float64) for c in range(L)}}
    pan = build_panel(d.X, d.D, d.Y, folds=seg, dtype=a.dtype, device=dev, nseg=L * K, targets=tg)
    counts = np.asarray(pan.seg_nreal, dtype=np.float64)
    torch.cuda.synchronize()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    phases = DA.apos_phases(pan, K, L, "min", a.clip, seg_counts=counts)
    call = SegmentedStep(phases, graph=True, warmup=1)
    for _ in range(a.warmup):
        st = call()
    torch.cuda.synchronize()
    coef, G = st["coef"].clone(), st["G"].clone()
    fit_phase = DA.apos_fit_phases(pan, K, L, "min", seg_counts=counts)[0][-1]
    c3 = coef[:, [0, 1, 3]].contiguous() if L == 2 else None
    nb = max(a.pass_batch, 1)

    def batch(f, *args):
        def g():
            for _ in range(nb):
                out = f(*args)
            return out
        return g

    p_apo = batch(DA.apo_moments, pan, coef, L, a.clip)
    p_irm = batch(DI.irm_score_moments, pan, c3, a.clip, 2) if L == 2 else None
    for _ in range(a.warmup):
        fit_phase({"G": G})
        p_apo()
        if p_irm:
            p_irm()
    torch.cuda.synchronize()
    ms = {"call": [], "fit": [], "pass_apo": []}
    if p_irm:
        ms["pass8"] = []
    for _ in range(a.calls):                      # alternate: all see the same clocks
        ms["call"].append(timed(call)[0])
        ms["fit"].append(timed(lambda: fit_phase({"G": G}))[0])
        t, mom = timed(p_apo)
        ms["pass_apo"].append(t / nb)
        if p_irm:
            t, m8 = timed(p_irm)
            ms["pass8"].append(t / nb)
    esz = pan.data.element_size()
    rows = counts.reshape(K, L)
    ntarget = 5 if a.dtype == "bf16" else 3                      # one, Y (hi / lo), D (hi / lo)
    union = [[int(((coef[k, :L, 1:] != 0).any(0) | (coef[k, L + c, 1:] != 0)).sum())
              for c in range(L)] for k in range(K)]
    out = {"mode": "apos", "levels": L, "n": n, "p": len(pan.xcols), "folds": K, "dtype": a.dtype,
           "calls": a.calls, "pass_batch": nb, "graphed": call.graphed,
           "path_launches": len(DA.path_launches(2 * L * K, K)), "moments": apo_layout(L).size,
           "union": union, "nbx_apo": DA.default_nbx(pan, L),
           "bytes_apo": int(sum(rows[k, c] * (union[k][c] + ntarget) * esz
                                for k in range(K) for c in range(L)))}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v), "spread_ms": max(v) - min(v)}
    out["pass_apo"]["TB_per_s"] = out["bytes_apo"] / (out["pass_apo"]["median_ms"] * 1e-3) / 1e12
    if p_irm:
        lay = apo_layout(2)
        mine = [lay.level + 2, lay.level + 6, 0, lay.level + 4]
        # each pass is timed on its own default grid; the shared sums are compared at one nbx
        same = DA.apo_moments(pan, coef, 2, a.clip, nbx=512 if a.dtype == "bf16" else 256)
        out["shared_bits"] = bool(torch.equal(same[mine], m8[[5, 4, 2, 7]]))
        out["nbx"] = [DA.default_nbx(pan, 2), 512 if a.dtype == "bf16" else 256]
        out["ratio_pass_apo_over_pass8"] = out["pass_apo"]["median_ms"] / out["pass8"]["median_ms"]
    r = ApoResult.from_moments("apos", call()["mom"].cpu().numpy(), list(range(L)), n=n)
    out["apo"] = [x.ate for x in r.apo]
    out["apo_true"] = [float(v) for v in d.apo_true]
    out["contrasts"] = [(c.effect, c.se) for c in r.contrasts()]
    out["crit"] = r.crit
    print(json.dumps(out))


def pliv(a, n, K, kw):
    import dataclasses
    import numpy as np
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators import lasso as DL
    from ate_replication_causalml_amd.estimators import pliv as DP
    from ate_replication_causalml_amd.ops.gram import plan_slot
    from ate_replication_causalml_amd.result import PlivResult, pliv_layout
    from ate_replication_causalml_amd.utils.graphs import SegmentedStep
    q = a.pliv
    plain = synthetic_panel(n, **kw)
    torch.cuda.synchronize()
    # the covariates x0..x{q-1} (continuous) are the instruments and leave the covariates. A
    # bf16 covariate is its own hi part; its lo part is W's, which is all zero (W is binary).
    cols = dict(plain.cols)
    zc = [plain.cols[f"x{j}"] for j in range(q)]
    for j, c in enumerate(zc):
        cols[f"Z{j}"] = c
        if plain.dtype == torch.bfloat16:
            cols.update({f"Z{j}_hi": c, f"Z{j}_lo": plain.cols["W_lo"]})
    pan = dataclasses.replace(plain, cols=cols, xcols=[x for x in plain.xcols if x not in zc])
    rows = np.asarray(plain.seg_nreal, dtype=np.float64)
    esz = plain.data.element_size()

    def nbytes(coef, ntarget):
        nnz = (coef[:, :, 1:] != 0).any(1).sum(1).cpu().numpy()
        return nnz.tolist(), int((rows * (nnz + ntarget) * esz).sum())

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    with plan_slot(0):
        plr = SegmentedStep(DL.dml_phases(plain, K, "min"), graph=True, warmup=1)
    with plan_slot(1):
        piv = SegmentedStep(DP.pliv_phases(pan, K, q, "min"), graph=True, warmup=1)
    for _ in range(a.warmup):
        plr()
        st = piv()
    torch.cuda.synchronize()
    coef, G = st["coef"].clone(), st["G"].clone()
    cv = plr()["cv"]
    c2 = cv.coef_min.reshape(K, 2, -1).double().contiguous().clone()
    fit_phase = DP.pliv_fit_phases(pan, K, q, "min")[-1]
    nb = max(a.pass_batch, 1)

    def batch(f, *args, **kws):
        def g():
            for _ in range(nb):
                out = f(*args, **kws)
            return out
        return g

    p_piv = batch(DP.pliv_moments, pan, coef, q, finish=True)
    p_plr = batch(DL.dml_residual_moments, plain, c2)
    for _ in range(a.warmup):
        fit_phase({"G": G})
        p_piv()
        p_plr()
    torch.cuda.synchronize()
    ms = {"plr_call": [], "pliv_call": [], "pliv_fit": [], "pass7": [], "pass_pliv": []}
    for _ in range(a.calls):                      # alternate: all see the same clocks
        ms["plr_call"].append(timed(plr)[0])
        ms["pliv_call"].append(timed(piv)[0])
        ms["pliv_fit"].append(timed(lambda: fit_phase({"G": G}))[0])
        ms["pass7"].append(timed(p_plr)[0] / nb)
        ms["pass_pliv"].append(timed(p_piv)[0] / nb)
    split = plain.dtype == torch.bfloat16
    out = {"mode": "pliv", "instruments": q, "n": n, "p": len(pan.xcols), "folds": K,
           "dtype": a.dtype, "blocked": kw["blocked"], "dgp": a.dgp, "calls": a.calls,
           "pass_batch": nb, "graphed": [plr.graphed, piv.graphed],
           "path_launches": len(DP.path_launches((2 + q) * K, K)), "moments": pliv_layout(q).size,
           "nbx_pliv": DP.default_nbx(pan, q)}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "mean_ms": statistics.fmean(v), "spread_ms": max(v) - min(v)}
    # target and valid columns per row: one, and Y, D, Z.. once each (hi + lo pairs on bf16)
    out["union7"], out["bytes7"] = nbytes(c2, 5 if split else 3)
    out["union_pliv"], out["bytes_pliv"] = nbytes(coef, (2 * (2 + q) if split else 2 + q) + 1)
    for k, b in (("pass7", "bytes7"), ("pass_pliv", "bytes_pliv")):
        out[k]["TB_per_s"] = out[b] / (out[k]["median_ms"] * 1e-3) / 1e12
    out["ratio_pass_pliv_over_pass7"] = out["pass_pliv"]["median_ms"] / out["pass7"]["median_ms"]
    st = piv()
    r = PlivResult.from_moments("pliv", st["mom"].cpu().numpy())
    out["pliv"] = {"theta": r.theta, "se": r.se, "pi": r.pi, "F": r.first_stage_F,
                   "res": st["res"].cpu().tolist()}
    out["plr_res"] = plr()["res"].cpu().tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
