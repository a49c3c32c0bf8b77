#!/usr/bin/env python3
"""Time ops.recommend_topk (MFMA and VALU sweeps) against two baselines in one
process, at the ml-1m and pinterest-20 shapes (every user, d = 64, K = 100, the
synthetic datasets' train lists excluded):

  eval_positions_all   the all-items sweep without selection: the floor
  torch.topk           of the masked P[users] @ Q.T (materialises U x I scores)

Call times are device events around `iters` back-to-back calls after a warm-up
(alternating the variants, repeated `rounds` times; the median is reported).
Needs a HIP device; writes one JSON document (default profiles/topk_bench.json).

    python tools/gpu_topk_bench.py [--out FILE] [--shapes ml-1m,pinterest-20] [--iters N]
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


def bench_shape(name, ds, d, K, iters, rounds, torch, ops, ev):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    U, I = ds.num_users, ds.num_items
    P = (torch.randn(U + 1, d, generator=g) * 0.1).to(dev)
    Q = (torch.randn(I + 1, d, generator=g) * 0.1).to(dev)
    import numpy as np
    users_np = np.arange(U, dtype=np.int32)
    off_np, ex_np = ev.train_exclusions(ds, users_np)
    users = torch.as_tensor(users_np, device=dev)
    off = torch.as_tensor(off_np, device=dev)
    ex = torch.as_tensor(ex_np, device=dev)
    tests = torch.as_tensor(np.asarray(ds.test_items, dtype=np.int32), device=dev)
    owner = torch.repeat_interleave(torch.arange(U, device=dev), off[1:] - off[:-1])
    ex_long = ex.long()

    def torch_topk():
        s = P[users.long()] @ Q[:I].T
        s[owner, ex_long] = float("-inf")
        return torch.topk(s, K, dim=1)

    variants = {
        "recommend_topk_mfma": lambda: ops.recommend_topk(P, Q, users, K, I, off, ex, kernel="mfma"),
        "recommend_topk_valu": lambda: ops.recommend_topk(P, Q, users, K, I, off, ex, kernel="valu"),
        "eval_positions_all": lambda: ops.eval_positions_all(P, Q, users, tests, I, off, ex, unique_lists=True),
        "torch_topk_masked_gemm": torch_topk,
    }
    # same items from both sweeps at the timed size (scores are bit-equal by the tests)
    a = variants["recommend_topk_mfma"]()
    b = variants["recommend_topk_valu"]()
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
    t = torch_topk()
    agree = float((t.indices.int() == a[0]).float().mean())
    for fn in variants.values():  # warm-up of every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, iters, torch))
    out = {"shape": name, "users": U, "items": I, "dim": d, "k": K, "excluded_pairs": int(ex_np.size),
           "iters": iters, "rounds": rounds, "mfma_equals_valu": same,
           "torch_topk_item_agreement": agree,
           "workspace_bytes": {k: ops.recommend_topk_workspace(U, I, K, k) for k in ("mfma", "valu")},
           "score_matrix_bytes": U * I * 4,
           "ms_median": {k: statistics.median(v) for k, v in ms.items()},
           "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()}}
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "topk_bench.json"))
    ap.add_argument("--shapes", default="ml-1m,pinterest-20")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        print("gpu_topk_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    results = []
    for name in args.shapes.split(","):
        ds = data.get_dataset(name + "-synthetic", seed=2019)
        results.append(bench_shape(name, ds, args.dim, args.k, args.iters, args.rounds, torch, ops, ev))
    doc = {"tool": "tools/gpu_topk_bench.py", "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
