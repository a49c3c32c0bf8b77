#!/usr/bin/env python3
"""Time NeuMF's all-items ranking (NeuMFContext.rank_all: positions + the 100
best items per user, no pair list, no score array) at the yelp shape, d = 64,
Keras-initialised parameters, in one process:

  full     every user of yelp_like() against all 25,816 item rows
  chunk    the first 2,048 users
  baseline the same chunk the way it had to be done before: int32 pair index
           arrays built on the GPU outside the timed region, ctx.predict over
           them (timed), then the exclusion mask, torch.topk(., 100) and a >=
           count on the [2048, 25816] score matrix (timed)

Exclusions are each user's train items, item 0 and the test item.  Times are
device events around one call each after a warm-up; the median of `rounds`
alternating repeats is reported with pairs/s and MFMA FLOP/s against the
algorithmic 2 (4 d^2 + 2 d^2) per pair.  Also the workspace against the score
array, whether a repeat is bit-identical, whether the chunk equals the baseline
(score bits, positions; items wherever the list's scores are distinct), and
the wall time of evaluation.evaluate_model_all over every user of the run.py
dataset (what `run.py --model neumf --eval all` pays per evaluation).  Needs a
HIP device; writes one JSON document (default profiles/neumf_rank_all_yelp.json).

    python tools/neumf_rank_all_bench.py [--out FILE] [--rounds N] [--no-eval-wall]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "adversarial-collaborative-filtering_amd"
sys.path.insert(0, REPO)


def timed(fn, torch):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "neumf_rank_all_yelp.json"))
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-eval-wall", action="store_true")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("neumf_rank_all_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    nm = importlib.import_module(PKG + ".neumf")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    dev = torch.device("cuda:0")
    ds = data.yelp_like()
    n, nc, d, k, C = ds.num_users, ds.num_items + 1, args.dim, args.k, args.chunk
    st = nm.NeuMFState(n, nc, d, dev)
    st.keras_init(0)
    ctx = nm.NeuMFContext(st, 1024)
    users = np.arange(n, dtype=np.int64)
    tests = np.zeros(n, np.int64)
    for u, t in ds.testRatings:
        tests[int(u)] = int(t)
    off, ex = ev.train_exclusions(ds, users)
    off, ex = nm._append_columns(off, ex, np.stack([np.zeros(n, np.int32), tests.astype(np.int32)], 1))
    g = lambda a, dt: torch.as_tensor(a, dtype=dt, device=dev)  # noqa: E731
    t_users, t_tests, t_off, t_ex = g(users, torch.int32), g(tests, torch.int32), g(off, torch.int64), g(ex, torch.int32)
    c_off = (t_off[:C + 1] - t_off[0]).contiguous()
    c_ex = t_ex[: int(off[C])].contiguous()
    full = lambda: ctx.rank_all(t_users, k, nc, t_off, t_ex, t_tests)  # noqa: E731
    chunk = lambda: ctx.rank_all(t_users[:C], k, nc, c_off, c_ex, t_tests[:C])  # noqa: E731
    # the baseline's inputs, outside the timed region
    pu = t_users[:C].repeat_interleave(nc).contiguous()
    pi = torch.arange(nc, dtype=torch.int32, device=dev).repeat(C).contiguous()
    mask = torch.zeros((C, nc), dtype=torch.bool, device=dev)
    owner = torch.repeat_interleave(torch.arange(C, device=dev), c_off[1:] - c_off[:-1])
    mask[owner, c_ex.long()] = True
    rows = torch.arange(C, device=dev)
    keep = {}

    def base_predict():
        keep["s"] = ctx.predict(pu, pi).view(C, nc)

    def base_select():
        s = keep["s"]
        ts = s[rows, t_tests[:C].long()]
        s = s.masked_fill(mask, float("-inf"))
        keep["top"] = torch.topk(s, k, dim=1)
        keep["pos"] = (s >= ts[:, None]).sum(1)

    variants = {"full": full, "chunk": chunk, "baseline_predict": base_predict, "baseline_select": base_select}
    first, again = chunk(), chunk()
    same = all(bool(torch.equal(x, y)) for x, y in zip(first, again))
    base_predict()
    base_select()
    torch.cuda.synchronize()
    pos, items, scores = first
    bs, bi = keep["top"]
    scores_equal = bool(torch.equal(scores.view(torch.int32), bs.view(torch.int32)))
    pos_equal = bool(torch.equal(pos.long(), keep["pos"]))
    distinct = torch.ones_like(scores, dtype=torch.bool)  # a score no neighbour in the list shares
    distinct[:, 1:] &= scores[:, 1:] != scores[:, :-1]
    distinct[:, :-1] &= scores[:, :-1] != scores[:, 1:]
    items_equal = bool(torch.equal(items[distinct].long(), bi[distinct]))
    full()
    torch.cuda.synchronize()
    ms = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v, fn in variants.items():
            ms[v].append(timed(fn, torch))
    med = {v: statistics.median(x) for v, x in ms.items()}
    med["baseline"] = statistics.median(a + b for a, b in zip(ms["baseline_predict"], ms["baseline_select"]))
    pairs = {"full": n * nc, "chunk": C * nc, "baseline": C * nc}
    flop = 2 * (4 * d * d + 2 * d * d)
    ws = nm.rank_all_workspace(n, nc, k)
    doc = {"tool": "tools/neumf_rank_all_bench.py", "device": torch.cuda.get_device_name(0),
           "dataset": "yelp_like", "users": int(n), "item_rows": int(nc), "dim": d, "k": k, "chunk_users": C,
           "excluded_entries": int(off[-1]), "rounds": args.rounds,
           "ms_median": med, "ms_min": {v: min(x) for v, x in ms.items()}, "ms_max": {v: max(x) for v, x in ms.items()},
           "pairs": pairs, "pairs_per_s": {v: pairs[v] / (med[v] * 1e-3) for v in pairs},
           "mfma_flop_per_pair": flop,
           "mfma_TFLOPs_vs_algorithmic": {v: pairs[v] * flop / (med[v] * 1e-3) / 1e12 for v in pairs},
           "chunk_over_baseline": med["chunk"] / med["baseline"],
           "workspace_bytes": ws, "score_array_bytes": n * nc * 4, "workspace_over_score_array": ws / (n * nc * 4),
           "chunk_workspace_bytes": nm.rank_all_workspace(C, nc, k),
           "baseline_chunk_bytes": {"pair_indices": 2 * C * nc * 4, "scores": C * nc * 4},
           "repeat_is_bit_identical": same,
           "equals_baseline": scores_equal and pos_equal and items_equal,
           "equals_baseline_parts": {"score_bits": scores_equal, "positions": pos_equal,
                                     "items_where_scores_distinct": items_equal,
                                     "list_entries_with_a_tied_neighbour": int((~distinct).sum())}}
    del pu, pi, mask, keep
    if not args.no_eval_wall:
        rc = importlib.import_module(PKG + ".run_cli")
        evn = importlib.import_module(PKG + ".evaluation")
        t0 = time.perf_counter()
        rds = rc.RunDataset(ds, "all")
        t_ds = time.perf_counter() - t0
        model = nm.NeuMF(rds.num_users, rds.num_items, d, seed=0, device=dev)
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hits, ndcgs = evn.evaluate_model_all(model, rds.testRatings, rds.trainMatrix, 100)
            walls.append(time.perf_counter() - t0)
        doc["evaluate_model_all"] = {"users": len(hits), "dataset_build_s": t_ds,
                                     "wall_s_first_call_with_exclusion_csr": walls[0], "wall_s": min(walls[1:]),
                                     "hr_at_100_untrained": float(np.mean(hits))}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
