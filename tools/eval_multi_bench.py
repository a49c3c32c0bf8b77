#!/usr/bin/env python3
"""Time the evaluation against several held-out items per user
(ops.eval_positions_multi + ops.rank_metrics) at the ml-1m and pinterest-20
shapes, d = 64, random sigma = 0.1 tables, in one process.

Every user gets T = 1, 10 and 50 test items taken from the tail of its sorted
train list (a user with fewer than T + 1 train items keeps one train item); the
rest of the list is the user's exclusion list.

  multi      ops.eval_positions_multi(check=False): one candidate sweep per user
  multi_chk  the same with check=True (its default: one synchronise per call)
  repeated   the only way to get these numbers before: ops.eval_positions_all
             with every user repeated once per test item and the exclusions set
             to the rest of the list plus that item (unique_lists=True: no
             dedup pass; its range check is cached after the first call)
  metrics    ops.rank_metrics on the positions, cutoffs (10, 50, 100)
  host       evaluate.metrics_from_positions_multi on the same positions
             (numpy on the host; wall clock, positions already on the host)

The tool asserts that `multi` and `repeated` give equal positions and that the
device metrics match the host's within rtol 1e-9.  Device times are events
around `reps` back-to-back calls (reps sized from a warm-up so that a window is
at least ~50 ms, at most 20 calls), per call; the variants alternate within a
round and the median over the rounds is reported with min and max.  Needs a HIP
device; writes one JSON document (default profiles/eval_multi_bench.json).

    python tools/eval_multi_bench.py [--out FILE] [--rounds N] [--shapes ml-1m,pinterest-20]
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
CUTS = (10, 50, 100)


def timed(fn, reps, torch):
    """ms per call: events around `reps` back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def split(ds, T, np):
    """(users, test CSR, exclusion CSR, n_neg) for `multi`, and (users, tests, exclusion CSR) for `repeated`."""
    soff, sitems = ds.sorted_lists()
    soff = np.asarray(soff, np.int64)
    n = len(soff) - 1
    lens = np.diff(soff)
    m = np.minimum(T, np.maximum(lens - 1, 0))
    kept = lens - m
    users = np.arange(n, dtype=np.int32)
    to = np.zeros(n + 1, np.int64)
    np.cumsum(m, out=to[1:])
    eo = np.zeros(n + 1, np.int64)
    np.cumsum(kept, out=eo[1:])
    ramp = lambda off, cnt: np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], cnt)  # noqa: E731
    tests = sitems[np.repeat(soff[1:] - m, m) + ramp(to, m)].astype(np.int32)
    excl = sitems[np.repeat(soff[:-1], kept) + ramp(eo, kept)].astype(np.int32)
    n_neg = (ds.num_items - lens).astype(np.int32)
    # repeated: entry e = (user, test item x); its list = the user's kept items, then the item
    r_users = np.repeat(users, m)
    r_len = np.repeat(kept, m) + 1
    ro = np.zeros(len(r_users) + 1, np.int64)
    np.cumsum(r_len, out=ro[1:])
    within = ramp(ro, r_len)
    src = np.repeat(soff[:-1][r_users], r_len) + within
    r_excl = sitems[np.minimum(src, len(sitems) - 1)].astype(np.int32)
    r_excl[ro[1:] - 1] = tests
    return (users, to, tests, eo, excl, n_neg), (r_users, tests, ro, r_excl)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_multi_bench.json"))
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="ml-1m,pinterest-20")
    ap.add_argument("--tests", default="1,10,50")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("eval_multi_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    dev = torch.device("cuda:0")
    g = lambda a, dt: torch.as_tensor(a, dtype=dt, device=dev)  # noqa: E731
    doc = {"tool": "tools/eval_multi_bench.py", "device": torch.cuda.get_device_name(0), "dim": args.dim,
           "cutoffs": list(CUTS), "rounds": args.rounds, "cases": []}
    for shape in args.shapes.split(","):
        ds = data.get_dataset(shape + "-synthetic")
        rng = np.random.default_rng(64)
        P = g(0.1 * rng.standard_normal((ds.num_users, args.dim)), torch.float32)
        Q = g(0.1 * rng.standard_normal((ds.num_items, args.dim)), torch.float32)
        for T in [int(t) for t in args.tests.split(",")]:
            (users, to, tests, eo, excl, n_neg), (r_users, r_tests, ro, r_excl) = split(ds, T, np)
            u, tto, tt, teo, tex, tnn = (g(users, torch.int32), g(to, torch.int64), g(tests, torch.int32),
                                         g(eo, torch.int64), g(excl, torch.int32), g(n_neg, torch.int32))
            ru, rt, rro, rex = g(r_users, torch.int32), g(r_tests, torch.int32), g(ro, torch.int64), g(r_excl, torch.int32)
            nc = int(ds.num_items)
            keep = {}

            def multi(check=False):
                keep["pos"] = ops.eval_positions_multi(P, Q, u, tto, tt, nc, teo, tex, check=check)

            def repeated():
                keep["rep"] = ops.eval_positions_all(P, Q, ru, rt, nc, rro, rex, unique_lists=True)

            def metrics():
                keep["rm"] = ops.rank_metrics(keep["pos"], tto, tnn, CUTS)

            variants = {"multi": multi, "multi_chk": lambda: multi(True), "repeated": repeated, "metrics": metrics}
            reps = {}
            for v, fn in variants.items():  # warm-up, and the size of a window
                fn()
                torch.cuda.synchronize()
                reps[v] = max(1, min(20, int(50.0 / max(timed(fn, 1, torch), 1e-3))))
            assert torch.equal(keep["pos"], keep["rep"]), f"{shape} T={T}: positions differ from the repeated call"
            again = ops.eval_positions_multi(P, Q, u, tto, tt, nc, teo, tex, check=False)
            assert torch.equal(again, keep["pos"]), f"{shape} T={T}: a repeat gave other positions"
            ms = {v: [] for v in variants}
            for _ in range(args.rounds):
                for v, fn in variants.items():
                    ms[v].append(timed(fn, reps[v], torch))
            pos_h = keep["pos"].cpu().numpy()
            t0 = time.perf_counter()
            want = ev.metrics_from_positions_multi(pos_h, to, n_neg, CUTS)
            host_ms = (time.perf_counter() - t0) * 1e3
            rm = keep["rm"]
            np.testing.assert_allclose(rm.per_user.cpu().numpy(), want["per_user"], rtol=1e-9, atol=0)
            np.testing.assert_allclose(rm.mean_cut.cpu().numpy(), want["mean_cut"], rtol=1e-9, atol=0)
            np.testing.assert_allclose(rm.mean_free.cpu().numpy(), want["mean_free"], rtol=1e-9, atol=0)
            assert int(rm.n_scored.item()) == want["n_scored"]
            med = {v: statistics.median(x) for v, x in ms.items()}
            case = {"shape": shape, "users": int(ds.num_users), "items": nc, "T": T, "n_tests": int(len(tests)),
                    "excluded_entries": int(len(excl)), "repeated_entries": int(len(r_users)),
                    "repeated_excluded_entries": int(len(r_excl)), "calls_per_window": reps,
                    "ms_median": med, "ms_min": {v: min(x) for v, x in ms.items()},
                    "ms_max": {v: max(x) for v, x in ms.items()},
                    "multi_over_repeated": med["multi"] / med["repeated"],
                    "multi_chk_over_repeated": med["multi_chk"] / med["repeated"],
                    "host_metrics_ms_one_call": host_ms, "metrics_over_host": med["metrics"] / host_ms,
                    "workspace_bytes": ops.eval_positions_multi_workspace(len(users), len(tests), nc),
                    "positions_equal_repeated": True, "metrics_match_host_rtol_1e-9": True}
            doc["cases"].append(case)
            print(json.dumps(case), flush=True)
            del ru, rt, rro, rex, keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
