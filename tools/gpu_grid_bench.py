#!/usr/bin/env python3
"""Time grid training against the existing trainer at the ml-1m shape (6,041 x 3,707
rows, one sampled epoch of 1,941 batches of 512, d = 64, adver = 1), for M members:

  grid      (a) ONE ops.grid_train call over the epoch for all M members
  serial    (b) M back-to-back epochs of the existing trainer (training_batch's
            pipeline: ops.PlanPipeline.run with check, then the step error word), one
            model after the other in the same process: what a sweep costs without (a)

Every figure is wall time from the first call to the end of a device synchronise,
the median of `reps` repetitions after a warm-up, with min and max.  For (a) the
JSON also holds the device time between two events around the call, the host time
the call itself takes to return (a launch-rate bound shows as host ~ device), and
the plan kernel's share of the device time (from torch.profiler's kernel records;
null where the profiler gives none).

Each M runs in a child process of its own under `timeout`; the first failure stops
the run.  Needs a HIP device; writes one JSON document (default
profiles/grid_bench.json) and prints it.

    python tools/gpu_grid_bench.py [--out FILE] [--members 1,4,16,64] [--reps N]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "adversarial-collaborative-filtering_amd"
sys.path.insert(0, REPO)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def plan_share(torch, fn):
    """Device time of k_grid_plan over the device time of all kernels of one call."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        plan = total = 0.0
        for e in prof.key_averages():
            t = float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)))
            if "k_grid_" in e.key:
                total += t
                if "k_grid_plan" in e.key:
                    plan += t
        return plan / total if total > 0 else None
    except Exception as exc:  # the profiler is optional: the figure is for information
        print(f"gpu_grid_bench: no plan share ({type(exc).__name__}: {exc})", file=sys.stderr)
        return None


def child(M, d, B, reps, warmup):
    import torch
    ops = importlib.import_module(PKG + ".ops")
    data = importlib.import_module(PKG + ".data")
    sampler_mod = importlib.import_module(PKG + ".sampler")
    train = importlib.import_module(PKG + ".train")
    dev = torch.device("cuda:0")
    ds = data.ml1m_like(seed=2019)
    ep = sampler_mod.DeviceSampler(ds, B, dev, seed=0).epoch(0)
    u, i, j = ep.user, ep.item_pos, ep.item_neg
    nb = ep.n_batches
    U1, I1 = ds.num_users + 1, ds.num_items + 1
    g = torch.Generator().manual_seed(1)

    def fresh():
        P = (torch.randn(M, U1, d, generator=g) * 0.01).to(dev)
        Q = (torch.randn(M, I1, d, generator=g) * 0.01).to(dev)
        return [P, Q, torch.full_like(P, 0.1), torch.full_like(Q, 0.1)]

    hps = [ops.StepHParams(adver=1, eps=0.1 + 0.9 * m / max(1, M - 1), reg_adv=1.0) for m in range(M)]

    # (a) one grid_train call
    tabs = fresh()
    wall, devms, host = [], [], []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        ops.grid_train(*tabs, hps, u, i, j, B, check=True)
        stop.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r >= warmup:
            wall.append((t2 - t0) * 1e3)
            host.append((t1 - t0) * 1e3)
            devms.append(start.elapsed_time(stop))
    share = plan_share(torch, lambda: ops.grid_train(*tabs, hps, u, i, j, B, check=True))
    finite = bool(all(torch.isfinite(t).all() for t in tabs))

    # (b) M epochs of the existing trainer, one model after the other
    tabs = fresh()
    pipe = ops.PlanPipeline(U1, I1, d, B, min(nb, train.plan_chunk(B)), dev, overlap=None)
    serial = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for m in range(M):
            pipe.run([t[m] for t in tabs], hps[m], u, i, j, graph=True, check=True)
            errs = pipe.step_errors()
            if errs:
                raise ops.StepWaitError(errs)
        torch.cuda.synchronize()
        if r >= warmup:
            serial.append((time.perf_counter() - t0) * 1e3)
    a, b = stats(wall), stats(serial)
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    out = {"members": M, "dim": d, "batch_size": B, "n_batches": nb, "user_rows": U1, "item_rows": I1, "reps": reps,
           "warmup": warmup, "grid_ms": a, "grid_device_ms": stats(devms), "grid_host_ms": stats(host),
           "grid_plan_share": share, "grid_workspace_bytes": ops.grid_workspace(M, B, nb, U1, I1, d),
           "serial_ms": b, "serial_over_grid": b["median"] / a["median"],
           "grid_below_serial_by_more_than_the_spread": b["median"] - a["median"] > spread,
           "grid_tables_finite": finite}
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grid_bench.json"))
    ap.add_argument("--members", default="1,4,16,64")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--batch_size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step_timeout", type=int, default=240, help="seconds per member count")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:
        return child(args.child, args.dim, args.batch_size, args.reps, args.warmup)
    import torch
    if not torch.cuda.is_available():
        print("gpu_grid_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    name = torch.cuda.get_device_name(0)
    results = []
    for M in [int(x) for x in args.members.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child",
               str(M), "--dim", str(args.dim), "--batch_size", str(args.batch_size), "--reps", str(args.reps),
               "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"gpu_grid_bench: M = {M} failed with status {p.returncode}; stopping", file=sys.stderr)
            sys.stderr.write(p.stdout[-2000:])
            return 1
        results.append(json.loads(line[-1][len("RESULT "):]))
    doc = {"tool": "tools/gpu_grid_bench.py", "device": name, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
