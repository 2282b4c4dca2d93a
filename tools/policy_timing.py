#!/usr/bin/env python3
"""The policy-tree step on one GPU: ms per eager launch, between device events, of the
feature-pair histogram kernel (``ate_policy_pair_hist``) on a device-generated arm-split panel
for three sets of features -- 16 features of 64 bins, 16 binary features with the per-lane
small-tile path and with the plain one, and the panel's first 21 covariates (the tutorial's:
15 continuous at ``--bins`` quantile bins, 6 binary) -- beside the ``ate_irm_scores`` pass
that feeds it, the search launches (``ate_policy_search``) and the torch evaluation sums and
finalisation, alternated in one process. Recorded, not gated: profiles/r07_policy/README.md.

  python tools/policy_timing.py --n 1e7 --p 500 --calls 20

The JSON line carries, per feature set, the bytes the histogram kernel reads (every workgroup
row block reads psi 8 + use 1 + its j1 codes 1 + one byte per tile it owns, per row) and their
time at ``--hbm-tbs`` (the register-load stream rate recorded with tools/hbm_stream.hip), and
the LDS atomics it issues (2 per row and tile). ``--kernels-only``: one eager fit, then two
eager passes of the policy phases after the score pass, for a separate
rocprofv3 --kernel-trace --stats run that shows the launches."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_edges(x, bins):
    """estimators.policy.feature_edges with torch ops on the device (same rule)."""
    import torch
    xs = torch.sort(x).values
    u = torch.unique_consecutive(xs)
    if u.numel() <= bins:
        return u[1:]
    at = torch.as_tensor([(k * xs.numel()) // bins for k in range(1, bins)], device=x.device)
    return torch.unique_consecutive(xs[at])


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
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--calls", type=int, default=20, help="timed launches of each kernel")
    ap.add_argument("--hbm-tbs", type=float, default=6.9,
                    help="stream rate of tools/hbm_stream.hip (profiles/README.md r02c_gram)")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch
    from ate_replication_causalml_amd.data.device_dgp import synthetic_panel
    from ate_replication_causalml_amd.estimators import policy as DP
    from ate_replication_causalml_amd.estimators.irm import irm_scores
    assert torch.cuda.is_available(), "policy_timing.py measures on a GPU"
    dev = torch.device("cuda:0")
    n, K = int(a.n), a.folds
    blocked = bool(a.blocked) and a.dtype == "bf16"
    pan = synthetic_panel(n, p=a.p, folds=K, seed=a.seed, dtype=a.dtype, device=dev,
                          blocked=blocked, dgp=a.dgp, arm_split=True)
    ld = pan.ld
    real = pan.row_index >= 0
    use = torch.where(real, 0, -1).to(torch.int8)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    sets = {}
    codes = torch.randint(0, 64, (16, ld), device=dev, generator=gen, dtype=torch.uint8)
    sets["d16_nb64"] = (codes, [64] * 16)
    codes = torch.randint(0, 2, (16, ld), device=dev, generator=gen, dtype=torch.uint8)
    sets["d16_binary"] = (codes, [2] * 16)
    cols, nb = [], []
    for j in range(min(21, a.p)):
        x = pan.col(f"x{j}").double()
        ed = device_edges(x[real], a.bins)
        cols.append(torch.bucketize(x, ed, right=True).to(torch.uint8))
        nb.append(int(ed.numel()) + 1)
        del x
    sets["tutorial21"] = (torch.stack(cols), nb)
    del cols
    cost = torch.zeros(1, dtype=torch.float64, device=dev)
    tcodes, tnb = sets["tutorial21"]
    tnbt = torch.tensor(tnb, dtype=torch.int32, device=dev)
    phases = DP.policy_phases(pan, tcodes, use, tnbt, cost, K, 2, 1, "min", a.clip, n_rows=n)
    st = None
    for ph in phases:
        st = ph(st)
    torch.cuda.synchronize()
    if a.kernels_only:
        for _ in range(2):
            s2 = {k: st[k] for k in ("G", "cv", "coef")}
            for ph in phases[-6:]:            # scores, range, hist, search, eval, final
                s2 = ph(s2)
        torch.cuda.synchronize()
        print(json.dumps({"mode": "kernels-only", "n": n, "p": a.p, "d": len(tnb), "passes": 3,
                          "same_bits": bool(torch.equal(s2["rec"], st["rec"]) and
                                            torch.equal(s2["hist"], st["hist"]))}))
        return
    psi, e, coef = st["psi"], st["e"], st["coef"]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    runs = {"scores": lambda: irm_scores(pan, coef, a.clip, 2)}
    for name, (c, b) in sets.items():
        bt = torch.tensor(b, dtype=torch.int32, device=dev)
        runs[f"hist_{name}"] = lambda c=c, bt=bt: DP.pair_hist(psi, cost, e, use, c, bt)
        if name == "d16_binary":
            runs[f"hist_{name}_plain"] = lambda c=c, bt=bt: DP.pair_hist(psi, cost, e, use, c, bt,
                                                                        priv=False)
    hists = {name: DP.pair_hist(psi, cost, e, use, c, b) for name, (c, b) in sets.items()}
    same = bool(torch.equal(hists["d16_binary"], runs["hist_d16_binary_plain"]()))
    for name, (c, b) in sets.items():
        bt = torch.tensor(b, dtype=torch.int32, device=dev)
        runs[f"search_{name}"] = lambda h=hists[name], bt=bt: DP.tree_search(h, bt, 2, 1)
    rec = st["rec"]
    runs["eval_final_tutorial21"] = lambda: DP.policy_finalize(
        DP.eval_sums(psi, cost, use, tcodes, rec), st["range"][1])
    ms = {k: [] for k in runs}
    for k, fn in runs.items():                    # warm every shape
        fn()
    torch.cuda.synchronize()
    for _ in range(a.calls):                      # alternate: all see the same clocks
        for k, fn in runs.items():
            ms[k].append(timed(fn)[0])
    out = {"n": n, "ld": ld, "p": a.p, "folds": K, "dtype": a.dtype, "blocked": blocked,
           "dgp": a.dgp, "bins": a.bins, "calls": a.calls, "e": int(e),
           "binary_paths_same_bits": same, "tutorial_nb": tnb, "tree": rec.cpu().tolist(),
           "fin_in_sample": st["fin"][0, :8].cpu().tolist()}
    for k, v in ms.items():
        out[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    for name, (c, b) in sets.items():
        d = len(b)
        tiles = [min(3, d - j2) for j1 in range(d) for j2 in range(j1, d, 3)]
        nbytes = ld * sum(10 + t for t in tiles)
        out[f"hist_{name}"].update(
            workgroup_groups=len(tiles), nbx=DP.hist_geometry(d, ld), bytes_read=nbytes,
            stream_bound_ms=nbytes / (a.hbm_tbs * 1e12) * 1e3,
            lds_atomics=2 * n * d * (d + 1) // 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
