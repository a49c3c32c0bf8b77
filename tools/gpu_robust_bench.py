#!/usr/bin/env python3
"""Time the robustness evaluation in one process, at the ml-1m shape (6,041 x 3,707
rows, 993,792 triplets of one sampled epoch) and the pinterest-20 shape, d = 64:

  adv_direction_grad    ops.adv_direction over the whole epoch as one batch
  torch_index_add       the same direction restated with torch on the GPU
                        (gathers, index_add_ of the four term sets, F.normalize)
  robustness_3eps       evaluate.robustness, one mode ("grad"), three eps: one
                        direction, then per eps two adv_apply and one all-items
                        positions sweep
  adv_apply_both        the two adv_apply calls of one eps alone

Call times are device events around `iters` back-to-back calls after a warm-up
(alternating the variants, repeated `rounds` times; the median is reported).
Needs a HIP device; writes one JSON document (default profiles/robust_bench.json).

    python tools/gpu_robust_bench.py [--out FILE] [--shapes ml-1m,pinterest-20] [--iters N]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
from types import SimpleNamespace

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


def torch_direction(P, Q, u, i, j, torch):
    """The grad direction with torch ops (float atomics inside index_add_: the
    order of a row's terms, and so the bits, vary from run to run)."""
    F = torch.nn.functional
    p, qi, qj = P[u], Q[i], Q[j]
    x = (p * qi).sum(1) - (p * qj).sum(1)
    g = -torch.sigmoid(-x.clamp(-80.0, 1e8)) * ((x >= -80.0) & (x <= 1e8))
    g = g[:, None]
    gP = torch.zeros_like(P).index_add_(0, u, g * qi).index_add_(0, u, -g * qj)
    gQ = torch.zeros_like(Q).index_add_(0, i, g * p).index_add_(0, j, -g * p)
    return F.normalize(gP, dim=1, eps=1e-6), F.normalize(gQ, dim=1, eps=1e-6)


def bench_shape(name, ds, d, iters, rounds, torch, ops, ev, sampler_mod):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    U, I = ds.num_users, ds.num_items
    P = (torch.randn(U + 1, d, generator=g) * 0.1).to(dev)
    Q = (torch.randn(I + 1, d, generator=g) * 0.1).to(dev)
    ep = sampler_mod.DeviceSampler(ds, 512, dev, seed=0).epoch(0)
    u, i, j = ep.user, ep.item_pos, ep.item_neg
    ul, il, jl = u.long(), i.long(), j.long()
    n = int(u.numel())
    plan = ev.init_eval_model(ds, SimpleNamespace(eval_mode="all"))
    model = SimpleNamespace(embedding_P=P, embedding_Q=Q)
    eps3 = [0.5, 1.0, 2.0]
    nP, nQ = ops.adv_direction(P, Q, u, i, j)
    variants = {
        "adv_direction_grad": lambda: ops.adv_direction(P, Q, u, i, j),
        "torch_index_add": lambda: torch_direction(P, Q, ul, il, jl, torch),
        "robustness_3eps": lambda: ev.robustness(model, ds, plan, ep, eps3, modes=("grad",)),
        "adv_apply_both": lambda: (ops.adv_apply(P, nP, 0.5), ops.adv_apply(Q, nQ, 0.5)),
    }
    again = ops.adv_direction(P, Q, u, i, j)
    same = bool(torch.equal(nP, again[0]) and torch.equal(nQ, again[1]))
    tP, tQ = torch_direction(P, Q, ul, il, jl, torch)
    diff = max(float((tP - nP).abs().max()), float((tQ - nQ).abs().max()))
    rows = variants["robustness_3eps"]()
    for fn in variants.values():  # warm-up of every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, iters, torch))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"shape": name, "user_rows": U + 1, "item_rows": I + 1, "dim": d, "triplets": n,
           "iters": iters, "rounds": rounds, "repeat_is_bit_identical": same,
           "max_abs_diff_vs_torch": diff,
           "workspace_bytes": ops.adv_direction_workspace(n, U + 1, I + 1, d),
           "robustness_rows": [list(r) for r in rows],
           "ms_median": med, "ms_min": {k: min(v) for k, v in ms.items()},
           "ms_max": {k: max(v) for k, v in ms.items()},
           "adv_direction_over_torch": med["adv_direction_grad"] / med["torch_index_add"]}
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "robust_bench.json"))
    ap.add_argument("--shapes", default="ml-1m,pinterest-20")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        print("gpu_robust_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    sampler_mod = importlib.import_module(PKG + ".sampler")
    results = []
    for name in args.shapes.split(","):
        ds = data.get_dataset(name + "-synthetic", seed=2019)
        results.append(bench_shape(name, ds, args.dim, args.iters, args.rounds, torch, ops, ev, sampler_mod))
    doc = {"tool": "tools/gpu_robust_bench.py", "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
