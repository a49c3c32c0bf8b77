#!/usr/bin/env python3
"""Time the diversity calls (ops.rerank_mmr, ops.list_similarity) at the shapes of
ml1m_like() and pinterest_like(), d = 64, random sigma = 0.1 tables, pool 128,
k = 100, cosine, against a torch restatement on the same GPU in the same process.

Every user is one row: its pool is ops.recommend_topk's 128 best items (train
items excluded), the relevances are evaluate.normalise_relevance's min-max.

  mmr        ops.rerank_mmr(Q, pool, rel, 100, lam = 0.7, check=False)
  mmr_torch  gather the pool's rows [n, 128, d], normalise, one bmm into
             [n, 128, 128], then the greedy loop: 100 steps of a masked batched
             argmax, a gather of the picked column and a running maximum
  ils        ops.list_similarity(Q, lists, (10, 100), check=False) on the plain
             top-100 lists
  ils_torch  gather, normalise, bmm into [n, 100, 100], a masked sum over the
             pairs a < b < K and one division, per cutoff

The tool asserts that a repeat of each kernel call gives equal bits, and records
how many of the torch restatement's lists (it rounds differently; no assertion)
differ and how far its ILS is from the kernel's.  Device times are events around
`reps` back-to-back calls (reps sized from a warm-up so that a window is at least
~50 ms, at most 20 calls), per call; the variants alternate within a round and
the median over the rounds is reported with min and max, with the peak device
memory of one torch call beside it.  Needs a HIP device; writes one JSON document
(default profiles/diverse_bench.json).

    python tools/diverse_bench.py [--out FILE] [--rounds N] [--shapes ml-1m,pinterest-20]
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
POOL, K, LAM, CUTS = 128, 100, 0.7, (10, 100)


def timed(fn, reps, torch):
    """ms per call: events around `reps` back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def unit_rows(Q, ids, torch):
    R = Q[ids.long().clamp(min=0)]
    return R / R.norm(dim=2, keepdim=True).clamp_min(1e-30)


def mmr_torch(Q, pool, rel, k, lam, torch):
    n, m = pool.shape
    R = unit_rows(Q, pool, torch)
    S = torch.bmm(R, R.transpose(1, 2))
    open_ = (pool >= 0) & torch.isfinite(rel)
    a = lam * rel
    ninf = torch.full_like(a, float("-inf"))
    items = torch.full((n, k), -1, dtype=torch.int32, device=pool.device)
    pen = None
    for j in range(k):
        o = torch.where(open_, a if pen is None else a - (1.0 - lam) * pen, ninf)
        best = o.argmax(dim=1, keepdim=True)
        took = open_.gather(1, best)
        items[:, j:j + 1] = torch.where(took, pool.gather(1, best), items[:, j:j + 1])
        open_ = open_.scatter(1, best, False)
        s = S.gather(2, best[:, :, None].expand(n, m, 1)).squeeze(2)
        pen = s if pen is None else torch.maximum(pen, s)
    return items


def ils_torch(Q, lists, cutoffs, torch):
    n, k = lists.shape
    R = unit_rows(Q, lists, torch)
    S = torch.bmm(R, R.transpose(1, 2)).double()
    valid = lists >= 0
    upper = torch.ones(k, k, dtype=torch.bool, device=lists.device).triu(1)
    out = []
    for c in cutoffs:
        v = valid.clone()
        v[:, c:] = False
        pairs = v[:, :, None] & v[:, None, :] & upper
        L = v.sum(1).double()
        cnt = L * (L - 1) / 2
        out.append(torch.where(cnt > 0, (S * pairs).sum((1, 2)) / cnt.clamp_min(1), torch.zeros_like(cnt)))
    return torch.stack(out, dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "diverse_bench.json"))
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="ml-1m,pinterest-20")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("diverse_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    dev = torch.device("cuda:0")
    doc = {"tool": "tools/diverse_bench.py", "device": torch.cuda.get_device_name(0), "dim": args.dim,
           "rounds": args.rounds, "pool": POOL, "k": K, "lam": LAM, "cutoffs": list(CUTS), "metric": "cosine",
           "cases": []}
    for shape in args.shapes.split(","):
        ds = {"ml-1m": data.ml1m_like, "pinterest-20": data.pinterest_like}[shape]()
        rng = np.random.default_rng(64)
        P = torch.as_tensor(0.1 * rng.standard_normal((ds.num_users, args.dim)), dtype=torch.float32, device=dev)
        Q = torch.as_tensor(0.1 * rng.standard_normal((ds.num_items, args.dim)), dtype=torch.float32, device=dev)
        users = np.arange(ds.num_users, dtype=np.int32)
        off, ex = ev.train_exclusions(ds, users)
        pool, scores = ops.recommend_topk(P, Q, users, POOL, ds.num_items, off, ex)
        rel = ev.normalise_relevance(pool, scores, "minmax")
        lists = pool[:, :K].contiguous()
        n = int(pool.shape[0])
        keep = {}
        variants = {
            "mmr": lambda: keep.__setitem__("mmr", ops.rerank_mmr(Q, pool, rel, K, LAM, "cosine", check=False)),
            "mmr_torch": lambda: keep.__setitem__("mmr_torch", mmr_torch(Q, pool, rel, K, LAM, torch)),
            "ils": lambda: keep.__setitem__("ils", ops.list_similarity(Q, lists, CUTS, "cosine", check=False)),
            "ils_torch": lambda: keep.__setitem__("ils_torch", ils_torch(Q, lists, CUTS, torch)),
        }
        reps, peak = {}, {}
        for v, fn in variants.items():  # warm-up, the size of a window, the peak memory of one call
            fn()
            torch.cuda.synchronize()
            reps[v] = max(1, min(20, int(50.0 / max(timed(fn, 1, torch), 1e-3))))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            fn()
            torch.cuda.synchronize()
            peak[v] = int(torch.cuda.max_memory_allocated(dev) - before)
        first = [t.clone() for t in (*keep["mmr"], *keep["ils"])]
        variants["mmr"]()
        variants["ils"]()
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                   for a, b in zip(first, (*keep["mmr"], *keep["ils"]))), f"{shape}: a repeat gave other bits"
        lists_differ = int((keep["mmr"][0] != keep["mmr_torch"]).any(dim=1).sum())
        ils_gap = float((keep["ils"][0] - keep["ils_torch"]).abs().max())
        ms = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v, fn in variants.items():
                ms[v].append(timed(fn, reps[v], torch))
        med = {v: statistics.median(x) for v, x in ms.items()}
        case = {"shape": shape, "users": n, "items": int(ds.num_items), "calls_per_window": reps, "ms_median": med,
                "ms_min": {v: min(x) for v, x in ms.items()}, "ms_max": {v: max(x) for v, x in ms.items()},
                "torch_over_mmr": med["mmr_torch"] / med["mmr"], "torch_over_ils": med["ils_torch"] / med["ils"],
                "peak_bytes": peak, "mmr_lists_that_differ_from_torch": lists_differ,
                "ils_max_abs_gap_to_torch": ils_gap, "ils_means": keep["ils"][1].cpu().tolist()}
        doc["cases"].append(case)
        print(json.dumps(case), flush=True)
        del keep, variants, first
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
