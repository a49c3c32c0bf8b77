#!/usr/bin/env python3
"""Time ops.neighbors_topk (cosine and Euclidean, the query itself excluded)
against the two routes that existed before it, in one process, at d = 64, K = 100:

  ml-1m         every one of 3,706 items against the 3,706-row table
  pinterest-20  every one of 9,916 items against the 9,916-row table
  5m            1,024 queries against a 5,000,000-row table

  topk_on_normalized_copy  (cosine) torch.nn.functional.normalize(T) -- a copy of
                           the table, made inside the timed call -- then
                           ops.recommend_topk(Tn, Tn, ...) with a one-entry
                           exclusion list per query for the query itself
  torch_matmul_topk        torch: normalize + matmul + topk for cosine, the
                           2ab - |a|^2 - |b|^2 matmul form + topk for Euclid; it
                           materialises the [queries, rows] score matrix

and, as a check of what the score policy costs, dot without self-exclusion
against ops.recommend_topk(T, T, ...), the same sweep (dot_vs_recommend_topk;
the *_nocheck variants pass check=False, which drops the one synchronising
read-back of the range flag that recommend_topk does not have).

Call times are device events around `iters` back-to-back calls after a warm-up,
the variants alternating, repeated `rounds` times; the median is reported.  A
variant whose single call takes longer than --slow_ms is timed with fewer calls
per round (recorded as iters_used) so that the torch route at the 5m shape does
not take minutes.  Peak extra memory is torch's peak allocation during one call
above what was allocated before it (the workspace of the ops included).  Needs a
HIP device; writes one JSON document (default profiles/neighbors_bench.json).

    python tools/gpu_neighbors_bench.py [--out FILE] [--shapes ml-1m,pinterest-20,5m] [--iters N]
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

SHAPES = {"ml-1m": (3706, 3706), "pinterest-20": (9916, 9916), "5m": (5_000_000, 1024)}  # rows, queries


def timed(fn, iters, torch):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def peak_extra(fn, torch):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def bench_shape(name, rows, n_q, d, K, iters, rounds, slow_ms, torch, ops):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    T = (torch.randn(rows, d, generator=g) * 0.1).to(dev)
    q = torch.randperm(rows, generator=g)[:n_q].to(torch.int32).to(dev)
    ql = q.long()
    row = torch.arange(n_q, device=dev)
    off = torch.arange(n_q + 1, dtype=torch.int64, device=dev)  # one exclusion per query: itself
    F = torch.nn.functional

    def normalized_copy():
        Tn = F.normalize(T, dim=1)
        return ops.recommend_topk(Tn, Tn, q, K, rows, off, q)

    def torch_cosine():
        Tn = F.normalize(T, dim=1)
        s = Tn[ql] @ Tn.T
        s[row, ql] = float("-inf")
        return torch.topk(s, K, dim=1)

    def torch_euclid():
        n2 = (T * T).sum(1)
        s = (T[ql] @ T.T).mul_(2.0).sub_(n2[ql, None]).sub_(n2[None, :])  # in place: one score matrix, not three
        s[row, ql] = float("-inf")
        return torch.topk(s, K, dim=1)

    variants = {
        "neighbors_cosine": lambda: ops.neighbors_topk(T, q, K, "cosine"),
        "neighbors_euclid": lambda: ops.neighbors_topk(T, q, K, "euclid"),
        "topk_on_normalized_copy": normalized_copy,
        "torch_matmul_topk_cosine": torch_cosine,
        "torch_matmul_topk_euclid": torch_euclid,
        "neighbors_dot_noself": lambda: ops.neighbors_topk(T, q, K, "dot", exclude_self=False),
        "recommend_topk_TT": lambda: ops.recommend_topk(T, T, q, K),
        # check=False: no read-back of the range flag, so back-to-back calls queue up like recommend_topk's
        "neighbors_dot_noself_nocheck": lambda: ops.neighbors_topk(T, q, K, "dot", exclude_self=False, check=False),
        "neighbors_cosine_nocheck": lambda: ops.neighbors_topk(T, q, K, "cosine", check=False),
    }
    a, b = variants["neighbors_dot_noself"](), variants["recommend_topk_TT"]()
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
    agree = {"cosine": float((variants["neighbors_cosine"]()[0] == torch_cosine().indices.int()).float().mean()),
             "euclid": float((variants["neighbors_euclid"]()[0] == torch_euclid().indices.int()).float().mean())}
    del a, b
    mem = {k: peak_extra(fn, torch) for k, fn in variants.items()}
    used = {}
    for k, fn in variants.items():  # warm-up; a slow variant gets fewer calls per round
        fn()
        one = timed(fn, 1, torch)
        used[k] = iters if one <= slow_ms else max(1, min(iters, int(slow_ms * iters / one / 4)))
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, used[k], torch))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"shape": name, "rows": rows, "queries": n_q, "dim": d, "k": K, "iters": iters, "rounds": rounds,
           "iters_used": used, "dot_equals_recommend_topk": same, "torch_item_agreement": agree,
           "workspace_bytes": ops.neighbors_topk_workspace(n_q, rows, K), "table_bytes": rows * d * 4,
           "score_matrix_bytes": n_q * rows * 4, "peak_extra_bytes": mem, "ms_median": med,
           "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
           "dot_vs_recommend_topk": med["neighbors_dot_noself"] / med["recommend_topk_TT"],
           "dot_nocheck_vs_recommend_topk": med["neighbors_dot_noself_nocheck"] / med["recommend_topk_TT"],
           "cosine_vs_normalized_copy": med["neighbors_cosine"] / med["topk_on_normalized_copy"]}
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "neighbors_bench.json"))
    ap.add_argument("--shapes", default="ml-1m,pinterest-20,5m")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slow_ms", type=float, default=200.0)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        print("gpu_neighbors_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    results = []
    for name in args.shapes.split(","):
        rows, n_q = SHAPES[name]
        results.append(bench_shape(name, rows, n_q, args.dim, args.k, args.iters, args.rounds, args.slow_ms, torch,
                                   ops))
        torch.cuda.empty_cache()
    doc = {"tool": "tools/gpu_neighbors_bench.py", "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
