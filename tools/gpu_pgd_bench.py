#!/usr/bin/env python3
"""Time the iterated attack in one process, at the ml-1m shape (6,041 x 3,707 rows,
993,792 triplets of one sampled epoch) and the pinterest-20 shape, d = 64, K = 10
steps from zero, eps = 0.5, step 2.5 eps / K:

  adv_pgd           ops.adv_pgd: one plan, then per step the planned direction and
                    the projected step on both tables, all inside one native call
  adv_pgd_planned   the same with a plan built beforehand (ops.adv_plan)
  composed          the same ten steps from what there was before adv_pgd: per step
                    ops.adv_direction on (P + dP, Q + dQ) (it sorts every time),
                    torch for v = delta + alpha n and the projection, ops.adv_apply
                    for the perturbed tables
  adv_plan          ops.adv_plan alone

Call times are device events around `iters` back-to-back calls after a warm-up
(alternating the variants, repeated `rounds` times; the median is reported, with
the minimum and maximum as the spread).  Needs a HIP device; writes one JSON
document (default profiles/pgd_bench.json).

    python tools/gpu_pgd_bench.py [--out FILE] [--shapes ml-1m,pinterest-20] [--iters N]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "adversarial-collaborative-filtering_amd"
sys.path.insert(0, REPO)


def timed(fn, iters, torch):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def composed(ops, torch, P, Q, u, i, j, eps, steps, alpha):
    """adv_pgd's loop from adv_direction, adv_apply and torch (check=False: no sync per step)."""
    dP, dQ = torch.zeros_like(P), torch.zeros_like(Q)
    Pa, Qa = P, Q
    for _ in range(steps):
        nP, nQ = ops.adv_direction(Pa, Qa, u, i, j, check=False)
        out = []
        for W, dl, n in ((P, dP, nP), (Q, dQ, nQ)):
            v = dl + alpha * n
            s = v.norm(dim=1, keepdim=True)
            v = torch.where(s <= eps, v, v * (eps / s.clamp_min(1e-30)))
            out.append((v, ops.adv_apply(W, v, 1.0)))
        (dP, Pa), (dQ, Qa) = out
    return dP, dQ


def bench_shape(name, ds, d, steps, iters, rounds, torch, ops, sampler_mod):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    U, I = ds.num_users, ds.num_items
    P = (torch.randn(U + 1, d, generator=g) * 0.1).to(dev)
    Q = (torch.randn(I + 1, d, generator=g) * 0.1).to(dev)
    ep = sampler_mod.DeviceSampler(ds, 512, dev, seed=0).epoch(0)
    u, i, j = ep.user, ep.item_pos, ep.item_neg
    n = int(u.numel())
    eps = 0.5
    alpha = 2.5 * eps / steps
    plan = ops.adv_plan(u, i, j, U + 1, I + 1)
    variants = {
        "adv_pgd": lambda: ops.adv_pgd(P, Q, u, i, j, eps, iters=steps, alpha=alpha, check=False),
        "adv_pgd_planned": lambda: ops.adv_pgd(P, Q, u, i, j, eps, iters=steps, alpha=alpha, plan=plan, check=False),
        "composed": lambda: composed(ops, torch, P, Q, u, i, j, eps, steps, alpha),
        "adv_plan": lambda: ops.adv_plan(u, i, j, U + 1, I + 1, check=False),
    }
    a, b = variants["adv_pgd"](), variants["adv_pgd"]()
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]))
    c = variants["composed"]()
    diff = max(float((a[0] - c[0]).abs().max()), float((a[1] - c[1]).abs().max()))
    for fn in variants.values():  # warm-up of every variant
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, iters, torch))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    out = {"shape": name, "user_rows": U + 1, "item_rows": I + 1, "dim": d, "triplets": n, "steps": steps,
           "eps": eps, "alpha": alpha, "iters": iters, "rounds": rounds, "repeat_is_bit_identical": same,
           "max_abs_diff_vs_composed": diff, "losses": a[2].tolist(),
           "workspace_bytes": ops.adv_pgd_workspace(n, U + 1, I + 1, d), "plan_bytes": plan.nbytes,
           "ms_median": med, "ms_min": {k: min(v) for k, v in ms.items()},
           "ms_max": {k: max(v) for k, v in ms.items()}, "ms_spread": spread,
           "composed_over_adv_pgd": med["composed"] / med["adv_pgd"],
           "faster_by_more_than_the_composed_spread": med["composed"] - med["adv_pgd"] > spread["composed"]}
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pgd_bench.json"))
    ap.add_argument("--shapes", default="ml-1m,pinterest-20")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        print("gpu_pgd_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    data = importlib.import_module(PKG + ".data")
    sampler_mod = importlib.import_module(PKG + ".sampler")
    results = []
    for name in args.shapes.split(","):
        ds = data.get_dataset(name + "-synthetic", seed=2019)
        results.append(bench_shape(name, ds, args.dim, args.steps, args.iters, args.rounds, torch, ops, sampler_mod))
    doc = {"tool": "tools/gpu_pgd_bench.py", "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
