#!/usr/bin/env python3
"""Time the certified worst-case positions (ops.eval_positions_worst) at the
ml-1m and pinterest-20 shapes, d = 64, random sigma = 0.1 tables, 1 and 4 eps,
both sides, in one process.

Every user is one entry: its held-out item against all items minus its train
items (evaluate.init_eval_model's all-items plan).

  worst   ops.eval_positions_worst(check=False) on the plan
  floor   ops.eval_positions_all(kernel="valu") on the same inputs: the VALU
          sweep with one chain per candidate instead of two (user side: plus a
          square root), no eps
  torch   the same counts restated in torch: P[u] @ Q.T, torch.cdist (user
          side) or the row norms (item side), compare, mask, sum.  The dense
          candidate mask is built once outside the timed region; the peak
          device memory of one call is recorded

The tool asserts that the eps = 0 row of `worst` equals `floor`'s positions and
that a repeat gives equal bits, and records how many counts of the torch
restatement differ (it rounds differently; no assertion).  Device times are
events around `reps` back-to-back calls (reps sized from a warm-up so that a
window is at least ~50 ms, at most 20 calls), per call; the variants alternate
within a round and the median over the rounds is reported with min and max.
ACF_ALT_LIB=path times that build of libacf_apr.so in place of the package's.
Needs a HIP device; writes one JSON document (default
profiles/certify_bench.json).

    python tools/certify_bench.py [--out FILE] [--rounds N] [--shapes ml-1m,pinterest-20]
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
from tools.alt_lib import use_alt_lib  # noqa: E402
EPS = {1: (0.05,), 4: (0.0, 0.02, 0.05, 0.1)}


def timed(fn, reps, torch):
    """ms per call: events around `reps` back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "certify_bench.json"))
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="ml-1m,pinterest-20")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("certify_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    alt = use_alt_lib(PKG)  # $ACF_ALT_LIB: that build in place of the package's
    dev = torch.device("cuda:0")
    g = lambda a, dt: torch.as_tensor(a, dtype=dt, device=dev)  # noqa: E731
    doc = {"tool": "tools/certify_bench.py", "lib": alt or "package", "device": torch.cuda.get_device_name(0),
           "dim": args.dim, "rounds": args.rounds, "eps": {str(k): list(v) for k, v in EPS.items()}, "cases": []}
    for shape in args.shapes.split(","):
        ds = data.get_dataset(shape + "-synthetic")
        plan = ev.init_eval_model(ds, argparse.Namespace(eval_mode="all"))
        rng = np.random.default_rng(64)
        P = g(0.1 * rng.standard_normal((ds.num_users, args.dim)), torch.float32)
        Q = g(0.1 * rng.standard_normal((ds.num_items, args.dim)), torch.float32)
        u, t, eo, ex = plan.device_arrays(dev)
        n, nc = int(u.numel()), int(plan.num_candidates)
        ul, tl = u.long(), t.long()
        cand = torch.ones((n, nc), dtype=torch.bool, device=dev)  # the plan's lists hold the test item
        rows = torch.repeat_interleave(torch.arange(n, device=dev), eo[1:] - eo[:-1])
        cand[rows, ex[:int(eo[-1])].long()] = False
        for side in ("user", "item"):
            for ne, eps in EPS.items():
                keep = {}
                teps = g(eps, torch.float32)

                def worst():
                    keep["worst"] = ops.eval_positions_worst(P, Q, u, t, nc, eo, ex, eps=eps, side=side, check=False)

                def floor():
                    keep["floor"] = ops.eval_positions_all(P, Q, u, t, nc, eo, ex, kernel="valu", unique_lists=True)

                def restated():
                    p = P[ul]
                    m = (p * Q[tl]).sum(1, keepdim=True) - p @ Q[:nc].T
                    base = torch.cdist(Q[tl], Q[:nc]) if side == "user" else 2.0 * p.norm(dim=1, keepdim=True)
                    keep["torch"] = torch.stack([((m <= e * base) & cand).sum(1) for e in teps]).int()

                variants = {"worst": worst, "floor": floor, "torch": restated}
                reps = {}
                for v, fn in variants.items():  # warm-up, and the size of a window
                    fn()
                    torch.cuda.synchronize()
                    reps[v] = max(1, min(20, int(50.0 / max(timed(fn, 1, torch), 1e-3))))
                if eps[0] == 0.0:
                    assert torch.equal(keep["worst"][0], keep["floor"]), f"{shape} {side}: eps = 0 is not the floor"
                first = keep["worst"].clone()
                worst()
                assert torch.equal(first, keep["worst"]), f"{shape} {side}: a repeat gave other counts"
                differ = int((keep["torch"] != keep["worst"]).sum())
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                restated()
                torch.cuda.synchronize()
                torch_peak = torch.cuda.max_memory_allocated(dev) - before
                ms = {v: [] for v in variants}
                for _ in range(args.rounds):
                    for v, fn in variants.items():
                        ms[v].append(timed(fn, reps[v], torch))
                med = {v: statistics.median(x) for v, x in ms.items()}
                case = {"shape": shape, "users": n, "items": nc, "side": side, "n_eps": ne,
                        "excluded_entries": int(eo[-1]), "calls_per_window": reps, "ms_median": med,
                        "ms_min": {v: min(x) for v, x in ms.items()}, "ms_max": {v: max(x) for v, x in ms.items()},
                        "worst_over_floor": med["worst"] / med["floor"], "torch_over_worst": med["torch"] / med["worst"],
                        "workspace_bytes": ops.eval_positions_worst_workspace(n, nc, ne),
                        "torch_peak_bytes": int(torch_peak), "torch_counts_that_differ": differ,
                        "counts": int(keep["worst"].numel()), "eps0_equals_floor": eps[0] == 0.0 or None}
                doc["cases"].append(case)
                print(json.dumps(case), flush=True)
                del keep
        del cand
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
