#!/usr/bin/env python3
"""Time the list-level robustness ops against the same quantities composed in
torch, in one process, at the pinterest-20 shape (every user, d = 64, K = 100, the
synthetic dataset's train lists excluded):

  list_compare                      vs  the [n, K, K] broadcast comparison + cumsum
  list_exposure + exposure_metrics  vs  bincount + sort

beside the two ops.recommend_topk sweeps (clean and attacked tables) they follow.
Call times are device events around `iters` back-to-back calls after a warm-up
(alternating the variants, repeated `rounds` times; the median is reported); peak
memory is torch's allocator peak over one call of each variant.
Needs a HIP device; writes one JSON document (default profiles/lists_bench.json).

    python tools/gpu_lists_bench.py [--out FILE] [--shapes pinterest-20] [--iters N]
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


def peak_bytes(fn, torch):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def bench_shape(name, ds, d, K, cutoffs, p, iters, rounds, torch, ops, ev):
    import numpy as np
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    U, I = ds.num_users, ds.num_items
    P = (torch.randn(U + 1, d, generator=g) * 0.1).to(dev)
    Q = (torch.randn(I + 1, d, generator=g) * 0.1).to(dev)
    Pa = P + 0.01 * torch.randn(U + 1, d, generator=g).to(dev)  # a stand-in for attacked tables
    Qa = Q + 0.01 * torch.randn(I + 1, d, generator=g).to(dev)
    users_np = np.arange(U, dtype=np.int32)
    off_np, ex_np = ev.train_exclusions(ds, users_np)
    users, off, ex = (torch.as_tensor(x, device=dev) for x in (users_np, off_np, ex_np))
    pop_np, tail_np = ev.item_popularity(ds)
    pop, tail = torch.as_tensor(pop_np, device=dev), torch.as_tensor(tail_np.astype(np.uint8), device=dev)
    A = ops.recommend_topk(P, Q, users, K, I, off, ex)[0]
    B = ops.recommend_topk(Pa, Qa, users, K, I, off, ex)[0]
    cuts = torch.tensor(cutoffs, device=dev)
    depth = torch.arange(1, K + 1, device=dev, dtype=torch.float64)
    pw = torch.tensor(p, dtype=torch.float64, device=dev) ** depth

    def torch_compare():
        """per-user (overlap, jaccard, rbo) [n, n_cut, 3] for full lists (no -1 entries at this shape)"""
        eq = A[:, :, None] == B[:, None, :]                               # [n, K, K] bools
        i = torch.arange(K, device=dev)
        m = torch.maximum(i[:, None], i[None, :]).expand_as(eq)[eq]       # the depth of every match
        row = torch.arange(A.shape[0], device=dev)[:, None, None].expand_as(eq)[eq]
        hist = torch.zeros((A.shape[0], K), dtype=torch.int32, device=dev)
        hist.index_put_((row, m), torch.ones_like(m, dtype=torch.int32), accumulate=True)
        X = hist.cumsum(1).double()                                       # X_d, d = 1..K
        run = (X / depth * pw).cumsum(1)
        Xc, runc = X[:, cuts - 1], run[:, cuts - 1]
        rbo = Xc / cuts * pw[cuts - 1] + (1 - p) / p * runc
        return torch.stack([Xc, Xc / (2 * cuts - Xc), rbo], dim=2)

    def torch_exposure():
        out = []
        for c in cutoffs:
            cnt = torch.bincount(B[:, :c].reshape(-1).long(), minlength=I)[:I]
            T = cnt.sum()
            s = torch.sort(cnt).values
            j = torch.arange(1, I + 1, device=dev)
            f = cnt[cnt > 0].double() / T
            T = T.double()
            out.append(torch.stack([T, (cnt > 0).sum().double() / I, ((2 * j - I - 1) * s).sum().double() / (I * T),
                                    -(f * torch.log2(f)).sum(), (cnt * pop).sum().double() / T,
                                    cnt[tail.bool()].sum().double() / T]))
        return torch.stack(out)

    variants = {
        "recommend_topk_clean": lambda: ops.recommend_topk(P, Q, users, K, I, off, ex),
        "recommend_topk_attacked": lambda: ops.recommend_topk(Pa, Qa, users, K, I, off, ex),
        "list_compare": lambda: ops.list_compare(A, B, cutoffs, p),
        "torch_compare": torch_compare,
        "list_exposure_metrics": lambda: ops.exposure_metrics(ops.list_exposure(B, I, cutoffs), pop, tail),
        "torch_exposure": torch_exposure,
    }
    # the two sides agree at the timed size (the tests hold the ops to the numpy yardstick)
    got, ref = variants["list_compare"]().per_user, torch_compare()
    cmp_err = float((got - ref).abs().max())
    exp_err = float((variants["list_exposure_metrics"]() - torch_exposure()).abs().max())
    for fn in variants.values():  # warm-up of every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, iters, torch))
    out = {"shape": name, "users": U, "items": I, "dim": d, "k": K, "cutoffs": list(cutoffs), "p": p, "iters": iters,
           "rounds": rounds, "compare_max_abs_diff_vs_torch": cmp_err, "exposure_max_abs_diff_vs_torch": exp_err,
           "mean_jaccard_at_k": float(got[:, -1, 1].mean()),
           "peak_bytes": {k: peak_bytes(variants[k], torch) for k in ("list_compare", "torch_compare",
                                                                       "list_exposure_metrics", "torch_exposure")},
           "ms_median": {k: statistics.median(v) for k, v in ms.items()},
           "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()}}
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lists_bench.json"))
    ap.add_argument("--shapes", default="pinterest-20")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--cutoffs", default="1,10,100")
    ap.add_argument("--p", type=float, default=0.9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        print("gpu_lists_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    cutoffs = tuple(int(c) for c in args.cutoffs.split(","))
    results = []
    for name in args.shapes.split(","):
        ds = data.get_dataset(name + "-synthetic", seed=2019)
        results.append(bench_shape(name, ds, args.dim, args.k, cutoffs, args.p, args.iters, args.rounds, torch, ops,
                                   ev))
    doc = {"tool": "tools/gpu_lists_bench.py", "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
