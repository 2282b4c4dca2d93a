"""Command line: ``python -m ate_replication_causalml_amd <command>``.

  replicate  run the 14-row driver (ate_replication.Rmd) and print/log/plot it
  dml        K-fold DML cross-fit on a synthetic N x p panel (the north-star job)
  late       the LATE of the interactive IV model (DML-IIVM) on a synthetic encouragement design
  pliv       the partially linear IV model (DML-PLIV) on a synthetic endogenous-dose design
  apos       the mean potential outcomes of a multi-arm treatment (DML-APOS) on a synthetic mailing design
  cluster    cluster-robust DML (PLR or IRM) on synthetic data with a cluster random effect
  build      compile the gfx950 HIP library and the host C++ library
"""
from __future__ import annotations

import argparse
import json
import sys


def _replicate(a):
    from .api import replicate
    from .config import ReplicateConfig, RunConfig
    from .utils import tracing
    data = None
    if a.csv:
        from .data.loader import load_social_pressure
        data = load_social_pressure(a.csv, a.n_obs, a.seed)
    cfg = ReplicateConfig(n_obs=a.n_obs, dr_trees=a.dr_trees, dml_trees=a.dml_trees,
                          cf_trees=a.cf_trees, bootstrap_se=a.bootstrap_se,
                          include=tuple(a.only) if a.only else None,
                          run=RunConfig(backend=a.backend, dtype=a.dtype, compat=a.compat,
                                        seed=a.seed))
    rep = replicate(data, cfg, log_path=a.log, plot_path=a.plot, verbose=a.verbose,
                    checkpoint_dir=a.checkpoint)
    print(f"rows dropped by selection bias: {rep.n_dropped}  (df_mod n={rep.n_mod})")
    print(rep.table())
    if a.trace:
        tracing.export_jsonl(a.trace)
    if a.json:
        print(json.dumps({"seconds": rep.seconds}))
    return 0


def _dml(a):
    import torch
    from .data.device_dgp import synthetic_panel
    from .estimators.lasso import dml_crossfit_panel, dml_repeated_panel
    from .estimators.common import read_result
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    if a.model == "irm":
        # interactive model: arm-split panel (segment 2k + a = fold k, W = a), AIPW score
        from .estimators.irm import check_logit_scope, irm_crossfit_panel
        pk = {} if a.propensity == "linear" else {"propensity": a.propensity}
        try:
            check_logit_scope(a.propensity, a.p, a.folds, a.dtype, repeats=a.repeats)
        except ValueError as e:
            raise SystemExit(str(e))
        if pk and a.sensitivity:
            raise SystemExit("--propensity logit is not available with --sensitivity")
        if a.rate_col is not None and (
                a.repeats > 1 or a.gate_col is not None or a.cate_col is not None
                or a.policy_cols is not None or a.sensitivity or a.targets is not None):
            raise SystemExit("--rate-col is an analysis of its own: not with --repeats, "
                             "--gate-col, --cate-col, --policy-cols, --sensitivity or --targets")
        if a.repeats > 1:
            # repeated cross-fitting: 2 K*K micro-arm segments, `repeats` K-fold partitions
            if (a.gate_col is not None or a.cate_col is not None or a.policy_cols is not None
                    or a.sensitivity or a.targets is not None):
                raise SystemExit("--repeats applies to the ATE only: not with --gate-col, "
                                 "--cate-col, --policy-cols, --sensitivity or --targets")
            from .estimators.irm import irm_repeated_panel
            pan = synthetic_panel(a.n, p=a.p, folds=a.folds * a.folds, seed=a.seed,
                                  dtype=a.dtype, device=dev, arm_split=True)
            try:
                res, splits, mom = irm_repeated_panel(pan, a.folds, a.repeats, a.lambda_rule,
                                                      a.clip, aggregate=a.aggregate)
            except ValueError as e:
                raise SystemExit(str(e))
            r = read_result(res, "DML-IRM cross-fit (LASSO, repeated)", n=a.n)
            print(json.dumps({"ate": r.ate, "se": r.se, "lower_ci": r.lower_ci,
                              "upper_ci": r.upper_ci, "repeats": a.repeats,
                              "aggregate": a.aggregate, "splits": splits.cpu().tolist(),
                              "n_clipped": [int(round(v)) for v in mom[:, 3].cpu().tolist()]}))
            return 0
        if a.targets is not None and (a.gate_col is not None or a.cate_col is not None
                                      or a.policy_cols is not None or a.sensitivity):
            raise SystemExit("--targets is an analysis of its own: not with --gate-col, "
                             "--cate-col, --policy-cols or --sensitivity")
        pan = synthetic_panel(a.n, p=a.p, folds=a.folds, seed=a.seed, dtype=a.dtype, device=dev,
                              arm_split=True)
        if a.targets is not None:
            # the effect over everyone, on the treated and on the controls, joint covariance
            from .estimators.targets import irm_targets_panel
            from .result import TARGETS, TargetResult, check_targets
            try:
                tg = check_targets([t for t in a.targets.split(",") if t])
            except ValueError as e:
                raise SystemExit(str(e))
            tg = tuple(t for t in TARGETS if t in tg)
            mom, _ = irm_targets_panel(pan, a.folds, tg, a.lambda_rule, a.clip, **pk)
            v = mom.double().cpu().numpy()
            r = TargetResult.from_moments("DML-IRM target populations (LASSO)", v, tg, n=a.n)
            out = {"targets": list(r.targets), "estimates": r.rows(), "cov": r.cov,
                   "n_treated": int(round(float(v[11]))), "n_clipped": int(round(float(v[3]))),
                   **pk}
            if "treated" in tg and "control" in tg:
                from dataclasses import asdict
                out["contrast"] = asdict(r.contrast("treated", "control"))
            print(json.dumps(out))
            return 0
        if a.rate_col is not None:
            # does treating by covariate x{rate_col}, largest first, find the large effects:
            # AUTOC, QINI and the TOC curve with half-sample bootstrap SEs
            import numpy as np
            from .estimators import rate as DR
            from .estimators.irm import run_phases
            from .result import RateResult
            if not 0 <= a.rate_col < a.p:
                raise SystemExit(f"--rate-col must index the {a.p} covariates")
            if not 1 <= a.rate_grid <= DR.GRID_MAX:
                raise SystemExit(f"--rate-grid must be in [1, {DR.GRID_MAX}]")
            grid = np.arange(1, a.rate_grid + 1) / a.rate_grid
            rid = pan.row_index
            try:
                DR.check_boot(a.boot)
                order, flags = DR.rate_order(pan.col(f"x{a.rate_col}").double(), rid, None, grid)
                if order.numel() < DR.ROWS_MIN or int(DR.rate_entered(flags)[0]) < DR.FIRST_MIN:
                    raise ValueError(f"RATE needs at least {DR.ROWS_MIN} rows and a first grid "
                                     f"point entering at least {DR.FIRST_MIN}")
                st = run_phases(DR.rate_phases(pan, rid, order, flags, a.rate_grid, a.folds,
                                               a.lambda_rule, a.clip, a.boot, 0.95, a.seed, **pk))
            except ValueError as e:
                raise SystemExit(str(e))
            r = RateResult.make("DML-IRM RATE (LASSO)", grid, DR.rate_entered(flags).cpu().numpy(),
                                st["fin"].double().cpu().numpy(), order.numel(),
                                int((flags & 1).sum().item()), a.boot, 0.95)
            print(json.dumps({**json.loads(r.json()), **pk}))
            return 0
        if a.gate_col is not None and a.sensitivity:
            raise SystemExit("--gate-col and --sensitivity are separate analyses: pick one")
        if a.cate_col is not None and (a.gate_col is not None or a.sensitivity):
            raise SystemExit("--cate-col, --gate-col and --sensitivity are separate analyses: "
                             "pick one")
        if a.policy_cols is not None:
            # whom to treat: the exact policy tree over the covariates x{J}, ...
            if a.cate_col is not None or a.gate_col is not None or a.sensitivity:
                raise SystemExit("--policy-cols, --cate-col, --gate-col and --sensitivity are "
                                 "separate analyses: pick one")
            from .estimators import policy as DP
            from .result import PolicyTreeResult
            try:
                cols = [int(c) for c in a.policy_cols.split(",")]
            except ValueError:
                raise SystemExit("--policy-cols takes comma-separated column indices")
            try:
                cols = DP.check_features(cols, a.p)
                DP.check_tree_args(a.policy_depth, a.policy_bins, 1)
            except ValueError as e:
                raise SystemExit(str(e))
            real = pan.row_index >= 0
            xs = [pan.col(f"x{j}").double() for j in cols]
            edges = [DP.feature_edges(x[real].cpu().numpy(), a.policy_bins) for x in xs]
            codes = torch.stack([torch.bucketize(x, torch.as_tensor(ed, device=x.device),
                                                 right=True).to(torch.uint8)
                                 for x, ed in zip(xs, edges)])
            use = torch.where(real, 0, -1).to(torch.int8)
            fin, rec, e, _ = DP.irm_policy_panel(pan, codes, use, [len(ed) + 1 for ed in edges],
                                                 a.policy_cost, a.folds, a.policy_depth, 1,
                                                 a.lambda_rule, a.clip, n_rows=a.n, **pk)
            r = PolicyTreeResult.make("DML-IRM policy tree (LASSO)", rec.cpu().numpy(),
                                      fin.double().cpu().numpy(), cols, edges, a.policy_cost,
                                      a.policy_depth, e=int(e.item()))
            ev = r.in_sample
            out = {"nodes": r.nodes, "actions": r.actions, "leaves": ev["leaves"],
                   **{k: v for k, v in ev.items() if k != "leaves"}, "honest": False,
                   "depth": r.depth, "cost": r.cost, "features": r.features, "edges": r.edges,
                   **pk}
            print(json.dumps(out))
            return 0
        if a.cate_col is not None:
            # the effect curve along covariate x{cate_col} on a B-spline basis, uniform band
            import numpy as np
            from .estimators import cate as DC
            from .result import AteResult, CateResult
            if not 1 <= a.cate_grid <= DC.GRID_MAX:
                raise SystemExit(f"--cate-grid must be in [1, {DC.GRID_MAX}]")
            knots = DC.spline_knots(pan, a.cate_col, a.cate_df, a.cate_degree)
            x = pan.col(f"x{a.cate_col}").double()
            xs = torch.sort(x[pan.row_index >= 0]).values
            n = xs.numel()
            grid = np.linspace(float(xs[(5 * n) // 100]), float(xs[min((95 * n) // 100, n - 1)]),
                               a.cate_grid)
            fin, _, _, _ = DC.irm_cate_panel(pan, x, knots, a.cate_degree, grid, a.folds,
                                             a.lambda_rule, a.clip, n_boot=a.boot, seed=a.seed,
                                             **pk)
            cate, se, crit, o_ate, o_se, nn, beta, omega = DC.read_fin(
                fin.double().cpu().numpy(), a.cate_df, a.cate_grid)
            r = CateResult.make("DML-IRM CATE curve (LASSO)", grid, cate, se, crit, beta, omega,
                                knots.cpu().numpy(), a.cate_degree, a.boot, 0.95,
                                AteResult.make("DML-IRM cross-fit (LASSO)", o_ate, o_se, n=a.n))
            out = {"curve": r.rows(), "crit": r.crit, "n_boot": r.n_boot, "level": r.level,
                   "knots": r.knots, "degree": r.degree, "coef": r.coef, "n": int(round(nn)),
                   "ate": r.overall.ate, "se": r.overall.se, **pk}
            print(json.dumps(out))
            return 0
        if a.gate_col is not None:
            # group effects over quantile bins of covariate x{gate_col}, with a joint band
            from .estimators.gate import irm_gate_panel, quantile_groups
            from .result import AteResult, GateResult
            gid, edges = quantile_groups(pan, a.gate_col, a.gate_bins)
            fin, _, _ = irm_gate_panel(pan, gid, a.folds, a.lambda_rule, a.clip, n_boot=a.boot,
                                       seed=a.seed, **pk)
            v = fin.double().cpu().numpy()
            G = a.gate_bins
            r = GateResult.make("DML-IRM group ATEs (LASSO)", list(range(G)), v[2 * G:3 * G],
                                v[:G], v[G:2 * G], v[3 * G], a.boot, 0.95,
                                AteResult.make("DML-IRM cross-fit (LASSO)", v[3 * G + 1],
                                               v[3 * G + 2], n=a.n))
            out = {"groups": r.rows(), "crit": r.crit, "n_boot": r.n_boot, "level": r.level,
                   "edges": edges.cpu().tolist(), "ate": r.overall.ate, "se": r.overall.se,
                   **pk}
            print(json.dumps(out))
            return 0
        if a.sensitivity:
            # bounds under a confounder of strength (cf_y, cf_d, rho), RV / RVa, benchmarks
            from dataclasses import asdict
            from .estimators.sensitivity import irm_sens_panel
            from .result import SensitivityResult, check_benchmarks, check_scenario
            check_scenario(a.cf_y, a.cf_d, a.rho)
            try:
                sets = [[int(c) for c in s.split(",")] for s in a.benchmark_cols or []]
            except ValueError:
                raise SystemExit("--benchmark-cols takes comma-separated column indices")
            bench = check_benchmarks(sets or None, a.p)
            mom, _ = irm_sens_panel(pan, a.folds, a.lambda_rule, a.clip, bench)
            v = mom.double().cpu().numpy()
            r = SensitivityResult.from_moments(
                "DML-IRM sensitivity (LASSO)", v[0], a.cf_y, a.cf_d, a.rho, 0.95, a.null,
                short=[(cols, v[1 + j]) for j, cols in enumerate(bench)], n=a.n)
            out = {"ate": r.theta, "se": r.se, "sigma2": r.sigma2, "nu2": r.nu2,
                   **{k: val for k, val in asdict(r.scenario).items()}, "null": r.null,
                   "rv": r.rv, "rva": r.rva, "benchmarks": [asdict(b) for b in r.benchmarks]}
            print(json.dumps(out))
            return 0
        res, mom, cv = irm_crossfit_panel(pan, a.folds, a.lambda_rule, a.clip, **pk)
        r = read_result(res, "DML-IRM cross-fit (LASSO)", n=a.n)
        out = {"ate": r.ate, "se": r.se, "lower_ci": r.lower_ci, "upper_ci": r.upper_ci,
               "n_clipped": int(round(float(mom[3]))), **pk}
    elif a.repeats > 1:
        # repeated cross-fitting: K*K micro-segments, `repeats` distinct K-fold partitions
        pan = synthetic_panel(a.n, p=a.p, folds=a.folds * a.folds, seed=a.seed, dtype=a.dtype,
                              device=dev)
        res, splits = dml_repeated_panel(pan, a.folds, a.repeats, a.lambda_rule,
                                         aggregate=a.aggregate)
        r = read_result(res, "DML cross-fit (LASSO, repeated)", n=a.n)
        out = {"ate": r.ate, "se": r.se, "lower_ci": r.lower_ci, "upper_ci": r.upper_ci,
               "repeats": a.repeats, "splits": splits.cpu().tolist()}
    else:
        pan = synthetic_panel(a.n, p=a.p, folds=a.folds, seed=a.seed, dtype=a.dtype, device=dev)
        res, mom, cv = dml_crossfit_panel(pan, a.folds, a.lambda_rule)
        r = read_result(res, "DML cross-fit (LASSO)", n=a.n)
        out = {"ate": r.ate, "se": r.se, "lower_ci": r.lower_ci, "upper_ci": r.upper_ci}
    print(json.dumps(out))
    return 0


def _late(a):
    # the LATE of the interactive IV model on the encouragement design of data.dgp
    from .api import ate_dml_iivm
    from .config import RunConfig
    from .data.dgp import make_late_data
    at, nt = not a.no_always_takers, not a.no_never_takers
    d = make_late_data(a.n, a.seed, always_takers=at, never_takers=nt)
    try:
        r = ate_dml_iivm(d.Y, d.D, d.Z, d.X, folds=a.folds, lambda_rule=a.lambda_rule,
                         clip=a.clip, always_takers=at, never_takers=nt,
                         run=RunConfig(backend=a.backend, dtype=a.dtype, seed=a.seed))
    except ValueError as e:
        raise SystemExit(str(e))
    out = json.loads(r.json())
    out["late_true"] = d.late_true
    print(json.dumps(out))
    return 0


def _apos(a):
    # the mean potential outcomes of every arm on the multi-arm mailing design of data.dgp
    from .api import ate_dml_apos
    from .config import RunConfig
    from .data.dgp import make_multiarm_data
    try:
        d = make_multiarm_data(a.n, a.seed, levels=a.levels)
        r = ate_dml_apos(d.Y, d.D, d.X, folds=a.folds, seed=a.seed, lambda_rule=a.lambda_rule,
                         clip=a.clip, run=RunConfig(backend=a.backend, dtype=a.dtype, seed=a.seed))
    except ValueError as e:
        raise SystemExit(str(e))
    out = json.loads(r.json())
    out["arms"] = d.arms
    out["apo_true"] = [float(v) for v in d.apo_true]
    print(json.dumps(out))
    return 0


def _cluster(a):
    # cluster-level cross-fitting and the cluster-robust SE on the clustered design of data.dgp
    from .api import ate_dml, ate_dml_irm
    from .config import RunConfig
    from .data.dgp import make_clustered_data
    run = RunConfig(backend=a.backend, dtype=a.dtype, seed=a.seed)
    try:
        d = make_clustered_data(a.n, a.cluster_size, a.icc, a.seed, assign=a.assign)
        if a.model == "irm":
            r = ate_dml_irm(d.Y, d.W, d.X, folds=a.folds, lambda_rule=a.lambda_rule, clip=a.clip,
                            run=run, clusters=d.clusters)
        else:
            r = ate_dml(d.Y, d.W, d.X, folds=a.folds, lambda_rule=a.lambda_rule, run=run,
                        clusters=d.clusters)
    except ValueError as e:
        raise SystemExit(str(e))
    out = json.loads(r.to_json())
    out["se_unclustered"] = r.diagnostics["se_unclustered"]
    out["tau_true"] = d.tau_true
    print(json.dumps(out))
    return 0


def _pliv(a):
    # the partially linear IV model on the endogenous-dose design of data.dgp, with the truth
    # and the (biased) partially linear regression beside it
    import numpy as np
    from .api import ate_dml, ate_dml_pliv
    from .config import RunConfig
    from .data.dgp import make_pliv_data
    run = RunConfig(backend=a.backend, dtype=a.dtype, seed=a.seed)
    try:
        d = make_pliv_data(a.n, a.seed, a.instruments, strength=a.strength)
        cl = None if a.cluster_size is None else np.arange(d.n) // max(a.cluster_size, 1)
        r = ate_dml_pliv(d.Y, d.D, d.Z, d.X, folds=a.folds, seed=a.seed,
                         lambda_rule=a.lambda_rule, clusters=cl, run=run)
        plr = ate_dml(d.Y, d.D, d.X, folds=a.folds, lambda_rule=a.lambda_rule, run=run)
    except ValueError as e:
        raise SystemExit(str(e))
    out = json.loads(r.json())
    out["theta_true"] = d.theta_true
    out["plr"] = {"estimate": plr.ate, "se": plr.se}
    print(json.dumps(out))
    return 0


def _build(a):
    from . import _build as b
    b.build_all()
    print("built")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="ate_replication_causalml_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("replicate")
    r.add_argument("--csv", help="socialpresswgeooneperhh_NEIGH.csv (else synthetic DGP)")
    r.add_argument("--n-obs", type=int, default=50000)
    r.add_argument("--seed", type=int, default=1991)
    r.add_argument("--backend", default="auto", choices=["auto", "gpu", "cpu", "reference"])
    r.add_argument("--dtype", default="f64", choices=["f64", "f32", "bf16"])
    r.add_argument("--compat", default="reference", choices=["reference", "textbook"])
    r.add_argument("--dr-trees", type=int, default=2500)
    r.add_argument("--dml-trees", type=int, default=2000)
    r.add_argument("--cf-trees", type=int, default=2000)
    r.add_argument("--bootstrap-se", action="store_true")
    r.add_argument("--only", nargs="*", help="subset of method labels")
    r.add_argument("--log", help="append results as JSONL")
    r.add_argument("--plot", help="write the pointrange plot (png)")
    r.add_argument("--trace", help="append tracing spans as JSONL")
    r.add_argument("--checkpoint", help="directory for per-row results (resume)")
    r.add_argument("--json", action="store_true")
    r.add_argument("-v", "--verbose", action="store_true")
    r.set_defaults(fn=_replicate)
    d = sub.add_parser("dml")
    d.add_argument("--n", type=int, default=1_000_000)
    d.add_argument("--p", type=int, default=500)
    d.add_argument("--folds", type=int, default=5)
    d.add_argument("--dtype", default="bf16")
    d.add_argument("--seed", type=int, default=7)
    d.add_argument("--lambda-rule", default="min", choices=["min", "1se"])
    d.add_argument("--repeats", type=int, default=1,
                   help="> 1: repeated cross-fitting over that many distinct K-fold partitions")
    d.add_argument("--aggregate", default="median", choices=["median", "mean"])
    d.add_argument("--model", default="plr", choices=["plr", "irm"],
                   help="plr: partially linear model; irm: interactive model (cross-fitted AIPW)")
    d.add_argument("--clip", type=float, default=0.01,
                   help="irm: the propensity is clipped to [clip, 1 - clip]")
    d.add_argument("--propensity", default="linear", choices=["linear", "logit"],
                   help="irm: the propensity fit -- linear-probability LASSO, or the binomial "
                        "CV-LASSO (logit: --repeats 1, f32/f64, p <= 96, folds <= 16; not with "
                        "--sensitivity)")
    d.add_argument("--gate-col", type=int, default=None,
                   help="irm: group ATEs over quantile bins of covariate x{J}, with a joint band")
    d.add_argument("--gate-bins", type=int, default=4, help="irm --gate-col: quantile groups")
    d.add_argument("--boot", type=int, default=999,
                   help="irm --gate-col / --cate-col: multiplier-bootstrap draws of the joint band")
    d.add_argument("--cate-col", type=int, default=None,
                   help="irm: the effect curve along covariate x{J} (B-splines), uniform band")
    d.add_argument("--cate-df", type=int, default=5, help="irm --cate-col: basis functions")
    d.add_argument("--cate-degree", type=int, default=3, help="irm --cate-col: spline degree 0..3")
    d.add_argument("--cate-grid", type=int, default=100,
                   help="irm --cate-col: points of the curve, between the 5 %% and 95 %% quantiles")
    d.add_argument("--rate-col", type=int, default=None,
                   help="irm: AUTOC, QINI and the TOC curve of treating by covariate x{J}, largest "
                        "first (half-sample bootstrap SEs; --boot replicates)")
    d.add_argument("--rate-grid", type=int, default=10,
                   help="irm --rate-col: points of the TOC curve, u = 1/Q, ..., 1")
    d.add_argument("--policy-cols", default=None, metavar="J,J,...",
                   help="irm: the exact policy tree (whom to treat) over the covariates x{J}, ...")
    d.add_argument("--policy-depth", type=int, default=2, help="irm --policy-cols: depth 0..2")
    d.add_argument("--policy-bins", type=int, default=32,
                   help="irm --policy-cols: bins per covariate, 2..64")
    d.add_argument("--policy-cost", type=float, default=0.0,
                   help="irm --policy-cols: the cost of treating one row, taken off every score")
    d.add_argument("--sensitivity", action="store_true",
                   help="irm: bounds under unobserved confounding, robustness values")
    d.add_argument("--cf-y", type=float, default=0.03, help="irm --sensitivity: outcome strength")
    d.add_argument("--cf-d", type=float, default=0.03,
                   help="irm --sensitivity: treatment (Riesz representer) strength")
    d.add_argument("--rho", type=float, default=1.0, help="irm --sensitivity: bias correlation")
    d.add_argument("--null", type=float, default=0.0,
                   help="irm --sensitivity: the hypothesis of the robustness values")
    d.add_argument("--benchmark-cols", action="append", metavar="J,J,...",
                   help="irm --sensitivity: benchmark the covariate set x{J}, ... (repeatable)")
    d.add_argument("--targets", default=None, metavar="T,T,...",
                   help="irm: the effect over these target populations (all, treated, control) "
                        "with their joint covariance")
    d.set_defaults(fn=_dml)
    l = sub.add_parser("late")
    l.add_argument("--n", type=int, default=50_000)
    l.add_argument("--seed", type=int, default=1991)
    l.add_argument("--folds", type=int, default=5)
    l.add_argument("--clip", type=float, default=0.01,
                   help="the instrument propensity is clipped to [clip, 1 - clip]")
    l.add_argument("--lambda-rule", default="min", choices=["min", "1se"])
    l.add_argument("--no-always-takers", action="store_true",
                   help="one-sided noncompliance: nobody takes the treatment unassigned (r0 = 0)")
    l.add_argument("--no-never-takers", action="store_true",
                   help="one-sided noncompliance: everybody assigned takes it (r1 = 1)")
    l.add_argument("--backend", default="auto", choices=["auto", "gpu", "cpu", "reference"])
    l.add_argument("--dtype", default="f64", choices=["f64", "f32", "bf16"])
    l.set_defaults(fn=_late)
    m = sub.add_parser("apos")
    m.add_argument("--n", type=int, default=50_000)
    m.add_argument("--levels", type=int, default=5,
                   help="arms of the design, the control included (2..8)")
    m.add_argument("--seed", type=int, default=1991)
    m.add_argument("--folds", type=int, default=5)
    m.add_argument("--clip", type=float, default=0.01,
                   help="every arm's propensity is clipped to [clip, 1 - clip]")
    m.add_argument("--lambda-rule", default="min", choices=["min", "1se"])
    m.add_argument("--backend", default="auto", choices=["auto", "gpu", "cpu", "reference"])
    m.add_argument("--dtype", default="f64", choices=["f64", "f32", "bf16"])
    m.set_defaults(fn=_apos)
    c = sub.add_parser("cluster")
    c.add_argument("--n", type=int, default=50_000)
    c.add_argument("--cluster-size", type=int, default=5, help="rows per cluster")
    c.add_argument("--icc", type=float, default=0.3,
                   help="intra-cluster correlation of the outcome noise, in [0, 1]")
    c.add_argument("--assign", default="cluster", choices=["cluster", "row"],
                   help="the treatment is drawn once per cluster, or once per row")
    c.add_argument("--model", default="irm", choices=["irm", "plr"])
    c.add_argument("--seed", type=int, default=1991)
    c.add_argument("--folds", type=int, default=5)
    c.add_argument("--clip", type=float, default=0.01,
                   help="irm: the propensity is clipped to [clip, 1 - clip]")
    c.add_argument("--lambda-rule", default="min", choices=["min", "1se"])
    c.add_argument("--backend", default="auto", choices=["auto", "gpu", "cpu", "reference"])
    c.add_argument("--dtype", default="f64", choices=["f64", "f32", "bf16"])
    c.set_defaults(fn=_cluster)
    v = sub.add_parser("pliv")
    v.add_argument("--n", type=int, default=50_000)
    v.add_argument("--instruments", type=int, default=1, help="instruments of the design (1..4)")
    v.add_argument("--strength", type=float, default=0.5, help="scale of the first stage")
    v.add_argument("--seed", type=int, default=1991)
    v.add_argument("--folds", type=int, default=5)
    v.add_argument("--cluster-size", type=int, default=None,
                   help="rows per cluster: cluster-level folds and the cluster-robust SE")
    v.add_argument("--lambda-rule", default="min", choices=["min", "1se"])
    v.add_argument("--backend", default="auto", choices=["auto", "gpu", "cpu", "reference"])
    v.add_argument("--dtype", default="f64", choices=["f64", "f32", "bf16"])
    v.set_defaults(fn=_pliv)
    b = sub.add_parser("build")
    b.set_defaults(fn=_build)
    a = ap.parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
