#!/usr/bin/env python3
"""Time the certified radius (ops.eval_radius) at the ml-1m and pinterest-20
shapes, d = 64, random sigma = 0.1 tables, K = 10 and 100, both sides, in one
process: tools/certify_bench.py's shapes and protocol.

Every user is one entry: its held-out item against all items minus its train
items (evaluate.init_eval_model's all-items plan).

  radius  ops.eval_radius(check=False) on the plan, the workspace kept
  worst   ops.eval_positions_worst(check=False) at 1 eps on the same inputs: the
          same chains without a selection, the floor of `radius`
  bisect  24 such calls, one eps each: a bisection of the radius at one K to 24
          bits, what a caller without eval_radius does (and its counts are at one
          eps for every user, although every user has an own radius)

The tool asserts, per case, that a repeat gives equal bits and that at eps =
the median finite radius at K the worst-case positions are < K exactly for the
users whose radius at K exceeds it.  Device times are events around `reps`
back-to-back calls (reps sized from a warm-up so that a window is at least ~50
ms, at most 20 calls), per call; the variants alternate within a round and the
median over the rounds is reported with min and max.  Expectation on record,
not a pass bar: radius within 1.5x of worst at K = 10.  ACF_ALT_LIB=path times
that build of libacf_apr.so in place of the package's.  Needs a HIP device;
writes one JSON document (default profiles/radius_bench.json).

    python tools/radius_bench.py [--out FILE] [--rounds N] [--shapes ml-1m,pinterest-20]
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
KS = (10, 100)
BISECT_STEPS = 24


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "radius_bench.json"))
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="ml-1m,pinterest-20")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("radius_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    alt = use_alt_lib(PKG)  # $ACF_ALT_LIB: that build in place of the package's
    dev = torch.device("cuda:0")
    g = lambda a, dt: torch.as_tensor(a, dtype=dt, device=dev)  # noqa: E731
    doc = {"tool": "tools/radius_bench.py", "lib": alt or "package", "device": torch.cuda.get_device_name(0),
           "dim": args.dim, "rounds": args.rounds, "bisect_steps": BISECT_STEPS, "cases": []}
    for shape in args.shapes.split(","):
        ds = data.get_dataset(shape + "-synthetic")
        plan = ev.init_eval_model(ds, argparse.Namespace(eval_mode="all"))
        rng = np.random.default_rng(64)
        P = g(0.1 * rng.standard_normal((ds.num_users, args.dim)), torch.float32)
        Q = g(0.1 * rng.standard_normal((ds.num_items, args.dim)), torch.float32)
        u, t, eo, ex = plan.device_arrays(dev)
        n, nc = int(u.numel()), int(plan.num_candidates)
        for side in ("user", "item"):
            for K in KS:
                keep = {}
                nbytes = ops.eval_radius_workspace(n, nc, K)
                work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)

                def radius():
                    keep["radius"] = ops.eval_radius(P, Q, u, t, nc, eo, ex, k=K, side=side, check=False,
                                                     workspace=work)

                radius()
                col = keep["radius"][0][:, K - 1]
                finite = col[torch.isfinite(col)]
                mid = float(finite.median()) if finite.numel() else 0.0
                hi = float(finite.max()) if finite.numel() else 1.0
                grid = [mid] + [hi * (s + 1) / BISECT_STEPS for s in range(BISECT_STEPS - 1)]

                def worst():
                    keep["worst"] = ops.eval_positions_worst(P, Q, u, t, nc, eo, ex, eps=(mid,), side=side,
                                                             check=False)

                def bisect():
                    for e in grid:
                        keep["bisect"] = ops.eval_positions_worst(P, Q, u, t, nc, eo, ex, eps=(e,), side=side,
                                                                  check=False)

                variants = {"radius": radius, "worst": worst, "bisect": bisect}
                reps = {}
                for v, fn in variants.items():  # warm-up, and the size of a window
                    fn()
                    torch.cuda.synchronize()
                    reps[v] = max(1, min(20, int(50.0 / max(timed(fn, 1, torch), 1e-3))))
                first = [x.clone() for x in keep["radius"]]
                radius()
                assert all(torch.equal(a, b) for a, b in zip(first, keep["radius"])), \
                    f"{shape} {side} K={K}: a repeat gave other bits"
                mid32 = float(torch.tensor(mid, dtype=torch.float32))
                assert torch.equal(keep["worst"][0] < K, col > mid32), f"{shape} {side} K={K}: radius and worst disagree"
                ms = {v: [] for v in variants}
                for _ in range(args.rounds):
                    for v, fn in variants.items():
                        ms[v].append(timed(fn, reps[v], torch))
                med = {v: statistics.median(x) for v, x in ms.items()}
                case = {"shape": shape, "users": n, "items": nc, "side": side, "K": K,
                        "excluded_entries": int(eo[-1]), "calls_per_window": reps, "ms_median": med,
                        "ms_min": {v: min(x) for v, x in ms.items()}, "ms_max": {v: max(x) for v, x in ms.items()},
                        "radius_over_worst": med["radius"] / med["worst"],
                        "bisect_over_radius": med["bisect"] / med["radius"], "workspace_bytes": nbytes,
                        "median_finite_radius": mid, "share_radius_zero": float((col == 0).float().mean()),
                        "share_unbounded": float(torch.isinf(col).float().mean())}
                doc["cases"].append(case)
                print(json.dumps(case), flush=True)
                del keep, work
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
