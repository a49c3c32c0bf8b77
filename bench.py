#!/usr/bin/env python
"""Benchmark of the APR (adversarial BPR-MF) training hot path on MI355X.

Workload (BASELINE.json configs[1]): APR on ml-1m-shaped synthetic data
(6,040 users x 3,706 items, ~994k training pairs, heavy-tailed user degree,
Zipf items), d = 64, eps = 0.5, reg_adv = 1, lr = 0.05 Adagrad, batch 512 —
the reference's run_adv_ori.py APR phase.  One "step" = one mini-batch of 512
(u, i, j) triplets through delta_update + optimizer_step (utils.py:117-119).

Timed region: dedup plan + hipGraph replay of the K steps, inputs (triplets,
tables) already resident in HBM.  value = triplets/s over all ranks.

--gpus N (torchrun, one rank per GPU): N independent APR jobs (replicas, weak
scaling) — the reference's experiments are independent single-process runs and a
B = 512 step has no data-parallel split worth an exchange.
An unaided `bench.py --gpus N` (no WORLD_SIZE in the environment) starts torchrun
with N ranks itself as a child process; a WORLD_SIZE that differs from --gpus is
an error.

A plain run (`--gpus 1 --steps K --warmup W`) does only what `value` needs: it
sets up, warms up, times the K steps, writes the tables the last timed step left
if --dump-outputs DIR is given (DIR/P.npy, Q.npy, accP.npy, accQ.npy, float32),
and prints the result line.  Everything below runs only with --full.

Extra fields (--full): "roofline" (dominant kernel, HIP-event kernel times),
"cpu_baseline" (the reference's CPU hot loop restated in torch-CPU on every
host thread, one ml-1m epoch, APR and BPR phases), "roofline_large_batch" /
"roofline_large_batch_d64" (BASELINE configs[4]: batch 65,536 on 10M x 5M tables,
d = 128 / 64, alias-table negatives from the device sampler; --no-large skips).
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
PKG = "adversarial-collaborative-filtering_amd"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
REF_CPU_TRIPLETS_PER_S = 993792 / 11.4  # ml-1m APR phase, best epoch 11.4 s


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3882, help="timed mini-batches (3882 = 2 ml-1m epochs)")
    p.add_argument("--warmup", type=int, default=1941)
    p.add_argument("--full", action="store_true",
                   help="also measure everything beside the headline line: the kernel-timing pass (roofline, "
                        "step_bandwidth, batch_stats), the CPU baseline, the split-step, NeuMF, evaluation and "
                        "synthetic-large lines (each with its --no-* switch)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the tables they left (P, Q and their Adagrad slots accP, "
                        "accQ) as DIR/<name>.npy, float32")
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--chunk", type=int, default=647,
                   help="batches per plan / graph (the next chunk's plan overlaps this chunk's training)")
    p.add_argument("--eager", action="store_true", help="eager launches instead of hipGraph replay")
    p.add_argument("--no-plan-overlap", action="store_true",
                   help="plan each chunk on the timed stream instead of beside the previous chunk's training (A/B)")
    p.add_argument("--cpu-batches", type=int, default=1941, help="CPU baseline sample (batches; 1,941 = one "
                   "ml-1m epoch)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--time-batches", type=int, default=400, help="batches in the kernel-timing pass")
    p.add_argument("--no-large", action="store_true",
                   help="skip the synthetic-large lines (batch 65,536 on 10M x 5M, d = 128 and 64)")
    p.add_argument("--no-neumf", action="store_true", help="skip the adversarial-NeuMF line (configs[3])")
    p.add_argument("--no-eval", action="store_true", help="skip the all-items evaluation line (SURVEY 8(f)2)")
    p.add_argument("--no-sharded", action="store_true",
                   help="skip the split-step lines (SURVEY 8(e): users/items sharded over the ranks)")
    p.add_argument("--sharded-steps", type=int, default=24, help="timed steps of the config-5 split-step line")
    p.add_argument("--rehearse-one-gpu", action="store_true",
                   help="N > 1 code path on a one-GPU box: every rank on cuda:0, gloo (host-staged) "
                        "instead of RCCL; a rehearsal of the launch, not a measurement")
    p.add_argument("--no-stream", action="store_true",
                   help="per-batch launches (two kernels per step) instead of the streamed step k_stream (A/B)")
    p.add_argument("--mapping", default="auto", choices=["auto", "wave", "group"],
                   help="slot mapping of the step kernels (auto: by batch size)")
    a = p.parse_args()
    if not a.full:  # a plain run measures the headline line alone
        a.no_cpu_baseline = a.no_sharded = a.no_neumf = a.no_eval = a.no_large = True
    return a


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def launch_command(argv, gpus: int, port: int) -> list:
    """The child command `--gpus N` (N > 1) runs when no launcher started this
    process: torchrun with one rank per GPU, every flag passed through unchanged
    (the ranks see WORLD_SIZE = N and run the multi-rank path)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
            "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__), *argv]


def check_world(gpus: int, env) -> str:
    """What `--gpus` asks of this process, decided before anything touches the GPU:
      "run"    -- this process is a rank (or the whole job at N = 1);
      "launch" -- N > 1 and no WORLD_SIZE: start N ranks as a child (launch_command);
    a WORLD_SIZE that disagrees with --gpus is an error (SystemExit 2), so a job can
    never report an n_gpus other than the one it was asked for."""
    if gpus < 1:
        raise SystemExit(f"bench.py: --gpus {gpus}: must be >= 1")
    ws = env.get("WORLD_SIZE")
    if ws is None:
        return "launch" if gpus > 1 else "run"
    if int(ws) != gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={ws} from the launcher but --gpus {gpus}")
    return "run"


def launch_ranks(a) -> int:
    """The parent of an unaided `bench.py --gpus N`: it never initialises the GPU
    (a process that has must not start another program in its place), checks that
    N devices exist (or --rehearse-one-gpu: every rank on cuda:0), runs torchrun as
    a child process whose rank 0 prints the one JSON line on the inherited stdout,
    and returns the child's exit status."""
    import subprocess
    if not a.rehearse_one_gpu:
        n = torch.cuda.device_count()  # counts devices without initialising HIP
        if n < a.gpus:
            raise SystemExit(f"bench.py: --gpus {a.gpus} but {n} GPU(s) visible "
                             f"(--rehearse-one-gpu puts every rank on cuda:0 over gloo)")
    port = 29500 + os.getpid() % 2000
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(launch_command(sys.argv[1:], a.gpus, port), env=env)


def batch_stats(u, i, j, B, nb, U1, I1):
    """Per-batch averages of the plan's shapes: unique user rows, unique item
    rows, fused triplets (user, positive and negative each occurring once)."""
    n = nb * B
    t = torch.arange(n, device=u.device, dtype=torch.int64) // B
    _, inv_u, cnt_u = torch.unique(t * U1 + u[:n].long(), return_inverse=True, return_counts=True)
    it = torch.cat([t * I1 + i[:n].long(), t * I1 + j[:n].long()])
    _, inv_i, cnt_i = torch.unique(it, return_inverse=True, return_counts=True)
    fused = (cnt_u[inv_u] == 1) & (cnt_i[inv_i[:n]] == 1) & (cnt_i[inv_i[n:]] == 1)
    return {"unique_user_rows": cnt_u.numel() / nb, "unique_item_rows": cnt_i.numel() / nb,
            "fused_triplets": float(fused.sum()) / nb}


def bytes_per_launch(kind: int, d: int, B: int, st: dict, nb: int = 1) -> float:
    """Algorithmic HBM bytes of one launch, fp32 rows of 4d bytes.
    adv (phase 2 + fused triplets + Adagrad) uses SURVEY.md §8(d)'s official figure:
      per triplet, reads of P[u], Q[i], Q[j] and their 3 Adagrad rows + 12 B of indices;
    clean (phase 1): P[u], Q[i], Q[j] + indices per triplet that is not fused;
    flush: read the scratch row + write the table row, per unique row (upper bound:
      rows a fused triplet wrote in place are not flushed);
    stream (k_stream = the whole APR step of all nb batches of a call in one launch):
      the official figure per triplet x every triplet of the launch."""
    rows = st["unique_user_rows"] + st["unique_item_rows"]
    clean, adv = (3 * d * 4 + 12) * (B - st["fused_triplets"]), (6 * d * 4 + 12) * B
    return {0: clean, 1: adv, 2: 2 * d * 4 * rows, 4: adv * nb}[kind]


def unique_rw_bytes(d: int, B: int, st: dict) -> float:
    """Compulsory traffic of a whole step with duplicates deflated: every unique
    row's weights and Adagrad slot read once and written once + the indices."""
    return 4 * d * 4 * (st["unique_user_rows"] + st["unique_item_rows"]) + 12 * B


def make_triplets(acf, ds, B, n_batches, dev, seed):
    sampler = acf.DeviceSampler(ds, B, dev, seed=seed)
    us, is_, js = [], [], []
    got, e = 0, 0
    while got < n_batches:
        ep = sampler.epoch(e)
        us.append(ep.user); is_.append(ep.item_pos); js.append(ep.item_neg)
        got += ep.n_batches
        e += 1
    n = n_batches * B
    return torch.cat(us)[:n].contiguous(), torch.cat(is_)[:n].contiguous(), torch.cat(js)[:n].contiguous()


DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs writes at most this much in all


def dump_outputs(path, tabs, rank=0):
    """--dump-outputs: the tables as the last timed step left them (what a caller
    of PlanPipeline.run holds afterwards), float32, as <path>/<name>.npy (rank r > 0
    of a replica run: <name>_rank<r>.npy).  Tables beyond DUMP_LIMIT_BYTES in all
    are written as a fixed, seeded sample of their rows (ascending row order)."""
    os.makedirs(path, exist_ok=True)
    total = sum(t.numel() * 4 for t in tabs)
    for name, t in zip(("P", "Q", "accP", "accQ"), tabs):
        x = t.detach().to(torch.float32).cpu().numpy()
        if total > DUMP_LIMIT_BYTES:
            keep = max(1, int(x.shape[0] * DUMP_LIMIT_BYTES / total))
            x = x[np.sort(np.random.default_rng(2019).choice(x.shape[0], keep, replace=False))]
        np.save(os.path.join(path, name + (f"_rank{rank}" if rank else "") + ".npy"), np.ascontiguousarray(x))


def init_tables(U1, I1, d, dev, seed):
    g = torch.Generator().manual_seed(seed)
    P = torch.nn.init.trunc_normal_(torch.empty(U1, d), 0, 0.01, -0.02, 0.02, generator=g).to(dev)
    Q = torch.nn.init.trunc_normal_(torch.empty(I1, d), 0, 0.01, -0.02, 0.02, generator=g).to(dev)
    return [P, Q, torch.full((U1, d), 0.1, device=dev), torch.full((I1, d), 0.1, device=dev)]


def step_kernel_name(kind: str, d: int, B: int) -> str:
    """Template instance of the step kernel the library launches for (d, B) with
    fusion on (csrc/acf_apr.hip: geometry(), get_kernels())."""
    d4 = d // 4
    lpr = 1
    while lpr < d4 and lpr < 64:
        lpr <<= 1
    nv = (d4 + lpr - 1) // lpr
    if B >= 4096:  # packed mapping with fusion: the triplet-centric list step
        if kind == "adv":  # (r06) hash plans: the clean combine rides in the adversarial launch
            return f"k_tri_cadv<{lpr}, {nv}>"
        if kind == "clean":
            return f"k_tri_clean<{lpr}, {nv}, false>"
        return "k_flush"
    team = 1 if lpr == 64 else 64 // lpr
    if kind == "stream":
        return f"k_stream<{lpr}, {nv}, {team}>"
    if kind == "stream_flush":
        return "k_stream_flush"
    if kind == "adv":
        return f"k_adv<{lpr}, {nv}, {team}, true>"
    if kind == "clean":
        return f"k_clean<{lpr}, {nv}, false, {team}, false>"
    return "k_flush"


def pmc_traffic(kernel: str, batches: int = 1):
    """HBM bytes per launch from the newest profiles/rNN/pmc_traffic.json (rocprofv3
    FETCH_SIZE / WRITE_SIZE passes of this bench, tools/profile_bench.sh), or None.
    A k_stream record is per batch (its profiled launches span 647 batches):
    scaled to this launch's `batches`."""
    root = os.path.join(REPO, "profiles")
    for r in sorted(os.listdir(root) if os.path.isdir(root) else [], reverse=True):
        f = os.path.join(root, r, "pmc_traffic.json")
        if os.path.isfile(f):
            with open(f) as fh:
                rec = json.load(fh).get(kernel)
            if rec and "traffic_bytes_per_batch" in rec:
                return int(rec["traffic_bytes_per_batch"] * batches), f"{r}/pmc_traffic.json (per batch x {batches})"
            if rec:
                return rec["traffic_bytes_per_launch"], f"{r}/pmc_traffic.json"
    return None


def kernel_roofline(ops, ctx, tabs, hp, u, i, j, B, d, nb, st, beside=None):
    """beside: another context whose plan of the NEXT nb batches runs on a side
    stream while this pass is timed -- the large-batch throughput pass's
    configuration (PlanPipeline plans chunk c + 1 beside chunk c), so the kernel
    times describe the run that produces `value`."""
    s = slice(0, nb * B)
    ctx.plan(u[s], i[s], j[s], B, check=False)
    if beside is not None:
        main = torch.cuda.current_stream()
        side = torch.cuda.Stream(main.device)
        side.wait_stream(main)
        s1 = slice(nb * B, 2 * nb * B)
        with torch.cuda.stream(side):
            beside.plan(u[s1], i[s1], j[s1], B, check=False)
    t = ctx.time_kernels(tabs, hp, 0, nb)
    if beside is not None:
        torch.cuda.synchronize()
    kinds = ["clean", "adv", "flush", "stream", "hot"]
    tot = {k: t[k][0] for k in kinds}
    dom = max(kinds[:4], key=lambda k: tot[k])  # the step kernels (hot = their hot-slot combine)
    kid = {"clean": 0, "adv": 1, "flush": 2, "stream": 4}[dom]  # bytes_per_launch's kinds
    avg_ms = t[dom][0] / max(t[dom][1], 1)
    alg_bytes = bytes_per_launch(kid, d, B, st, nb)
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
    rw = None
    if kid == 1:
        rw = unique_rw_bytes(d, B, st) / (avg_ms * 1e-3) / 1e9
    elif kid == 4:
        rw = unique_rw_bytes(d, B, st) * nb / (avg_ms * 1e-3) / 1e9
    per_kernel_us = {k: round(1e3 * t[k][0] / max(t[k][1], 1), 3) for k in kinds if t[k][1]}
    name = step_kernel_name(dom, d, B)
    if t["stream"][1]:
        per_kernel_us["stream_per_batch"] = round(1e3 * t["stream"][0] / t["stream"][1] / nb, 3)
    tr = pmc_traffic(name, nb if kid == 4 else 1)
    return {"bound": "hbm", "kernel": name, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
            "traffic": None if tr is None else tr[0],
            "traffic_source": None if tr is None else tr[1],
            "bytes_per_launch": int(alg_bytes), "avg_launch_us": round(avg_ms * 1e3, 3),
            "batches_per_launch": nb if kid == 4 else 1,
            "per_kernel_avg_us": per_kernel_us,
            "achieved_unique_rw_GBs": None if rw is None else round(rw, 2),
            # the dominant kernel's measured HBM traffic (PMC, reads + writes) per
            # second: how close the kernel runs to the memory system, which the
            # read-only algorithmic frac above does not show for write-heavy steps
            "traffic_GBs": None if tr is None else round(tr[0] / (avg_ms * 1e-3) / 1e9, 2),
            "traffic_frac_of_copy_ceiling": None if tr is None else round(tr[0] / (avg_ms * 1e-3) / 1e9 / 6290.0, 4)}


def step_bandwidth(d, B, st, triplets_per_s):
    """Whole-step rates per GPU: SURVEY §8(d)'s HBM-read roofline (official) and the
    duplicate-deflated unique-row read+write traffic."""
    official = (6 * d * 4 + 12) * triplets_per_s / 1e9
    rw = unique_rw_bytes(d, B, st) * triplets_per_s / B / 1e9
    return {"bytes_per_triplet": 6 * d * 4 + 12, "achieved_GBs": round(official, 2),
            "frac": round(official / HBM_PEAK_GBS, 5),
            "unique_rw_bytes_per_batch": int(unique_rw_bytes(d, B, st)),
            "unique_rw_GBs": round(rw, 2)}


def cpu_baseline(u, i, j, P0, Q0, B, nb):
    """BASELINE.md §2 / SURVEY §8(d): the reference's CPU hot loop restated, timed
    on this box's host over ONE full ml-1m-shaped epoch (nb batches of B) of the
    APR phase with the reference's dense delta work (APR.py:183-191).  `value` is
    the STRONGEST faithful restatement measured: the C
    oracle (oracle/apr_oracle.c, dense mode) on one thread and on every host
    thread this job may use (OMP_NUM_THREADS: 16 on the GPU box).  Beside it: the TF graph
    op for op in torch-CPU fp32 on every host thread (TF's CPU kernels run on its
    intra-op pool) for the APR phase, the BPR phase and a touched-rows-only APR
    variant.  Sampling and evaluation are excluded (APR.py:261-263)."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    from apr_oracle import COracle, HParams
    from apr_torch_cpu import apr_step, cpu_model, threads
    torch.set_num_threads(threads())
    U, I, J = (x[: nb * B].cpu().long() for x in (u, i, j))

    def run(adver, dense):
        tabs = [P0.cpu().clone(), Q0.cpu().clone(), torch.full(P0.shape, 0.1), torch.full(Q0.shape, 0.1)]
        t0 = time.perf_counter()
        for t in range(nb):
            s = slice(t * B, (t + 1) * B)
            apr_step(*tabs, U[s], I[s], J[s], adver=adver, dense=dense)
        return nb * B / (time.perf_counter() - t0)

    apr_dense, bpr, apr_sparse = run(True, True), run(False, True), run(True, False)
    o = COracle()
    Pn, Qn = P0.cpu().numpy().copy(), Q0.cpu().numpy().copy()
    Un, In, Jn = U.int().numpy(), I.int().numpy(), J.int().numpy()
    t0 = time.perf_counter()
    o.apr_train(Pn, Qn, np.full_like(Pn, 0.1), np.full_like(Qn, 0.1), Un, In, Jn, B, HParams(adver=1), dense=True)
    c1 = nb * B / (time.perf_counter() - t0)
    # the same restatement on every host thread this job may use (rows partitioned
    # by thread, sums in the one-thread order: the same bits)
    nthr = threads()
    Pm, Qm = P0.cpu().numpy().copy(), Q0.cpu().numpy().copy()
    t0 = time.perf_counter()
    o.apr_train_mt(Pm, Qm, np.full_like(Pm, 0.1), np.full_like(Qm, 0.1), Un, In, Jn, B, HParams(adver=1),
                   dense=True, threads=nthr)
    cm = nb * B / (time.perf_counter() - t0)
    same = bool(np.array_equal(Pm, Pn) and np.array_equal(Qm, Qn))
    variants = {"c_oracle_dense": (c1, 1, "oracle/apr_oracle.c (dense mode), the TF graph's arithmetic in C, "
                                          "one thread"),
                "c_oracle_dense_threads": (cm, nthr, f"oracle/apr_oracle.c (dense mode, oracle_apr_train_mt), the "
                                                     f"TF graph's arithmetic in C on {nthr} OpenMP threads, the "
                                                     f"one-thread result bit for bit"),
                "torch_cpu_dense": (apr_dense, nthr, f"oracle/apr_torch_cpu.py, the TF graph op for op in "
                                                     f"torch-CPU fp32 on {nthr} threads")}
    best = max(variants, key=lambda k: variants[k][0])
    v, cores, what = variants[best]
    return {"value": round(v, 1), "unit": "triplets/s", "cores": cores, "kind": "port",
            "cpu_model": cpu_model(), "variant": best,
            "sample": f"one ml-1m-shaped epoch ({nb} batches x {B}) of the APR phase with the reference's dense "
                      f"delta densify/normalise/assign per batch (APR.py:183-191): {what}; the strongest of "
                      f"the CPU restatements measured here",
            "c_oracle_1thread_apr_dense": round(c1, 1),
            "c_oracle_threads_apr_dense": {"value": round(cm, 1), "cores": nthr, "bits_equal_1thread": same},
            "torch_cpu_apr_dense": {"value": round(apr_dense, 1), "cores": nthr},
            "torch_cpu_bpr_phase": round(bpr, 1),
            "torch_cpu_apr_touched_rows_only": round(apr_sparse, 1),
            "reference_published": {"value": round(REF_CPU_TRIPLETS_PER_S, 1),
                                    "source": "out/janEval/ml-1m-sort_apr_..._11_56_42.out:54-55 (UCL CPU, TF1)"}}


def large_batch_roofline(acf, ops, dev, ds, d=128, nb=256, chunk=32, graph=True):
    """BASELINE configs[4] / SURVEY §8(d) "synthetic large" on one GPU: 10M users
    x 5M items (~200M interactions, Zipf items), batch 65,536, triplets from the
    device sampler with its alias-table negatives (equal weights: the reference's
    uniform rule, APR.py:76-78).  Tables (d = 128: 15.4 GB with the Adagrad slots)
    are far beyond the 256 MB Infinity Cache, so rows come from HBM.  256 batches
    in chunks of 32: the first chunk's plan runs in line, the others beside the
    previous chunk's step, as in an epoch (3,052 batches) where the in-line plan
    is amortised."""
    U1, I1, B = ds.num_users + 1, ds.num_items + 1, 65536
    sampler = acf.DeviceSampler(ds, B, dev, seed=7, weights=np.ones(ds.num_items, np.float32))
    ep = sampler.epoch(0)
    n = nb * B
    u, i, j = (x[:n].contiguous() for x in (ep.user, ep.item_pos, ep.item_neg))
    del ep
    g = torch.Generator(device=dev).manual_seed(5)
    tabs = [torch.randn(U1, d, device=dev, generator=g) * 0.01, torch.randn(I1, d, device=dev, generator=g) * 0.01,
            torch.full((U1, d), 0.1, device=dev), torch.full((I1, d), 0.1, device=dev)]
    pipe = ops.PlanPipeline(U1, I1, d, B, chunk, dev)
    hp = ops.StepHParams(adver=1)
    pipe.run(tabs, hp, u, i, j, 0, nb, graph=graph)  # warm (graph capture)
    torch.cuda.synchronize(dev)
    # three timed passes over the same nb batches: the line is their median, with
    # min / max beside it, so box-to-box noise can be told from a change
    dts = []
    for _ in range(3):
        t0 = time.perf_counter()
        pipe.run(tabs, hp, u, i, j, 0, nb, graph=graph)
        torch.cuda.synchronize(dev)
        dts.append(time.perf_counter() - t0)
    dt = sorted(dts)[1]
    errors = pipe.step_errors()
    st = batch_stats(u, i, j, B, nb, U1, I1)
    # the dominant kernel timed alone, then with the next chunk's plan beside it
    # (the throughput pass's configuration): `frac` is the latter, VERDICT r04 #10
    alone = kernel_roofline(ops, pipe.ctx[0], tabs, hp, u, i, j, B, d, chunk, st)
    rl = kernel_roofline(ops, pipe.ctx[0], tabs, hp, u, i, j, B, d, chunk, st, beside=pipe.ctx[1])
    rl["timing"] = "events on every launch of one chunk, the next chunk's plan running beside it (as in the throughput pass)"
    rl["alone"] = {"avg_launch_us": alone["avg_launch_us"], "frac": alone["frac"],
                   "per_kernel_avg_us": alone["per_kernel_avg_us"]}
    rl["triplets_per_s"] = round(nb * B / dt, 1)
    rl["triplets_per_s_passes"] = {"median": round(nb * B / dt, 1), "min": round(nb * B / max(dts), 1),
                                   "max": round(nb * B / min(dts), 1), "passes": len(dts)}
    rl["step_bandwidth"] = step_bandwidth(d, B, st, nb * B / dt)
    rl["batch_stats"] = {k: round(v, 1) for k, v in st.items()}
    rl["step_errors"] = errors
    rl["config"] = {"workload": "APR, synthetic large (BASELINE configs[4], one GPU)", "users": U1 - 1,
                    "items": I1 - 1, "interactions": len(ds), "dim": d, "batch": B, "batches": nb, "chunk": chunk,
                    "negatives": "device sampler, alias table of equal weights (uniform, APR.py:76-78)"}
    del tabs, pipe
    torch.cuda.empty_cache()
    return rl


def sharded_lines(acf, ops, dev, dist, world, rank, big, steps):
    """one APR step split over the ranks (distributed.ShardedAPR):
    users and items row-sharded (row r on rank r % N), each triplet on its
    user's rank, the batch-global item sums completed by the item owners over
    four all_to_alls per step (RCCL over xGMI).  Two lines:
      large: BASELINE configs[4] (10M x 5M, d = 128, Zipf items, alias-table
             negatives), 65,536 triplets per GPU per step (weak scaling), routed at
             sampling time (each rank samples its own users);
      pinterest: BASELINE configs[2] (pinterest-20-shaped, d = 64), the
             reference's global batch of 512 split over the ranks (strong scaling).
    value = triplets of all ranks / max-over-ranks time of the timed steps."""
    import torch.distributed as tdist
    D_ = importlib.import_module(PKG + ".distributed")
    own_group = False
    if dist is None:  # one process: a world-1 group over RCCL for the collectives
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29000 + os.getpid() % 1000))
        tdist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        own_group = True
    out = {}
    try:
        def timed(sh, run, n_trip):
            torch.cuda.synchronize(dev)
            tdist.barrier()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(dev)
            tdist.barrier()
            el = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
            tdist.all_reduce(el, op=tdist.ReduceOp.MAX)
            tot = torch.tensor([float(n_trip)], device=dev, dtype=torch.float64)
            tdist.all_reduce(tot)
            return float(el.item()), float(tot.item())

        # configs[4], weak scaling, routed at sampling time
        b, d = 65536, 128
        sel = big.pos_user % world == rank
        sub = type(big)(big.num_users, big.num_items, big.pos_user[sel].contiguous(), big.pos_item[sel].contiguous(),
                        big.list_off, big.list_items, name="synthetic-large-rank")
        sampler = acf.DeviceSampler(sub, b, dev, seed=11 + rank, weights=np.ones(big.num_items, np.float32))
        ep = sampler.epoch(0)
        warm = steps  # one untimed chunk of the timed size: routing buffers come from the cache
        n = (warm + steps) * b
        u, i, j = (x[:n].contiguous() for x in (ep.user, ep.item_pos, ep.item_neg))
        del ep, sampler, sub
        g = torch.Generator(device=dev).manual_seed(5)
        sh = D_.ShardedAPR(big.num_users + 1, big.num_items + 1, d, b * world, device=dev, local_batch=b)
        sh.P.normal_(0, 0.01, generator=g)
        sh.Q.normal_(0, 0.01, generator=g)
        hp = ops.StepHParams(adver=1)
        ck = steps  # one chunk: its routing (a fixed cost per chunk) is paid once
        sh.train_routed(u[: warm * b], i[: warm * b], j[: warm * b], hp, chunk=ck)
        s = slice(warm * b, n)
        st0 = dict(sh.stats)
        el, tot = timed(sh, lambda: sh.train_routed(u[s], i[s], j[s], hp, chunk=ck), steps * b)
        req = (sh.stats["items_requested"] - st0["items_requested"]) / steps
        out["large"] = {
            "metric": "APR triplets/sec, split step (users/items sharded over the ranks)",
            "value": round(tot / el, 1), "unit": "triplets/s", "n_gpus": world, "steps": steps,
            "ms_per_step": round(1e3 * el / steps, 4), "scaling": "weak", "dtype": "f32",
            "data": "synthetic 10M x 5M, 200M Zipf interactions, alias-table negatives (device sampler per rank)",
            "config": {"workload": "APR, BASELINE configs[4] split over the ranks", "users": big.num_users,
                       "items": big.num_items, "dim": d, "per_gpu_batch": b, "global_batch": b * world,
                       "parallelism": f"user/item row shards x{world}, all_to_all x4 per step"},
            "exchange_bytes_per_step_rank0": int(4 * req * d * 4),
            # the share that leaves the rank (its own items stay local), averaged over
            # the whole step: the xGMI egress rate beside the per-GPU HBM fraction (§8(e))
            "xgmi_egress_GBs_rank0": round(4 * req * d * 4 * (world - 1) / world / (el / steps) / 1e9, 2),
            "items_per_rank_step": round(req, 1),
            "route_ms_rank0": round(1e3 * (sh.stats["route_s"] - st0["route_s"]), 3),
            "launch": "hipGraph" if sh.stats["graph_replays"] > st0["graph_replays"] else "eager",
            "step_errors": sh.step_errors()}
        sh.close()
        del sh, u, i, j
        torch.cuda.empty_cache()

        # configs[2], strong scaling: the reference's global batch of 512, B / N triplets
        # of it per rank, routed at sampling time (each rank samples its own users), so
        # every step has the same shape and the chunk replays as captured hipGraphs
        B, d = 512, 64
        bl = B // world
        ds = acf.pinterest_like(seed=2019)
        pu = ds.pair_user % world == rank
        sub = type(ds)(ds.num_users, ds.num_items, ds.pair_user[pu], ds.pair_item[pu], ds.test_items,
                       name="pinterest-20-synthetic-rank")
        psamp = acf.DeviceSampler(sub, bl, dev, seed=3 + rank)
        ep = psamp.epoch(0)
        steps_p = 200
        warm = steps_p  # as above: untimed chunks of the timed size (graphs captured after them)
        n = (warm + steps_p) * bl
        u, i, j = (x[:n].contiguous() for x in (ep.user, ep.item_pos, ep.item_neg))
        for key, exchange in (("pinterest", "all_to_all"), ("pinterest_allgather", "allgather")):
            sh = D_.ShardedAPR(ds.num_users + 1, ds.num_items + 1, d, B, device=dev, item_exchange=exchange,
                               local_batch=bl)
            sh.P.normal_(0, 0.01, generator=g)
            sh.Q.normal_(0, 0.01, generator=g)
            ck = steps_p  # one chunk: its routing (a fixed cost per chunk) is paid once
            sh.train_routed(u[: warm * bl], i[: warm * bl], j[: warm * bl], hp, chunk=ck)
            s = slice(warm * bl, n)
            r0 = sh.stats["graph_replays"]
            el, tot = timed(sh, lambda: sh.train_routed(u[s], i[s], j[s], hp, chunk=ck), steps_p * bl)
            out[key] = {
                "metric": "APR triplets/sec, split step (users/items sharded over the ranks)",
                "value": round(tot / el, 1), "unit": "triplets/s", "n_gpus": world, "steps": steps_p,
                "ms_per_step": round(1e3 * el / steps_p, 4), "scaling": "strong", "dtype": "f32",
                "data": "synthetic pinterest-20-shaped (55,187 x 9,916), device sampler per rank",
                "config": {"workload": "APR, BASELINE configs[2] split over the ranks", "users": ds.num_users,
                           "items": ds.num_items, "dim": d, "global_batch": B, "per_gpu_batch": bl,
                           "parallelism": f"user/item row shards x{world}, E1 by {exchange}, all_to_all x3"},
                "launch": "hipGraph" if sh.stats["graph_replays"] > r0 else "eager",
                "step_errors": sh.step_errors()}
            sh.close()
            del sh
            torch.cuda.empty_cache()
    finally:
        if own_group:
            tdist.destroy_process_group()
    return out


def neumf_bench(acf, dev):
    """BASELINE configs[3]: adversarial NeuMF (GMF + MLP towers perturbed) on
    yelp-sort-shaped synthetic data, d = 64, batch 512 (run.py --bs default), one
    epoch of Keras-style training (libacf_neumf.so).  The epoch (acf_neumf_train)
    runs Keras's dense Adam lazily (bit-identical) and is a
    latency-bound chain of small launches; the roofline is its dominant kernel,
    k_nmf_step, and the dense Adam of the stepwise API is
    reported beside it."""
    import scipy.sparse as sp
    nm = importlib.import_module(PKG + ".neumf")
    ds = acf.yelp_like()
    train = sp.coo_matrix((np.ones(len(ds.pair_user), np.float32), (ds.pair_user, ds.pair_item)),
                          shape=(ds.num_users, ds.num_items))
    B, d = 512, 64
    r = nm.AdversarialNeuMF(ds.num_users, ds.num_items, d, weight=1.0, pop_percent=0.2, seed=0,
                            device=dev)
    x, y = r.get_train_instances(train)
    n = len(y)
    perm = np.random.default_rng(0).permutation(n)
    U = torch.as_tensor(x[0][perm], dtype=torch.int32, device=dev)
    I = torch.as_tensor(x[1][perm], dtype=torch.int32, device=dev)
    Y = torch.as_tensor(y[perm], dtype=torch.float32, device=dev)
    ctx = r._context(B)
    hp = r.hparams()
    ctx.train(U[: 64 * B], I[: 64 * B], Y[: 64 * B], B, hp)  # warm
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    losses = ctx.train(U, I, Y, B, hp)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    nb = losses.shape[0]
    st = r.state

    def adam_time(c, reps=50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c.adam(hp)
        e0.record()
        for _ in range(reps):
            c.adam(hp)
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / reps

    # the timed path's dominant kernel: k_nmf_step (both passes of a step in one
    # launch), timed through unchecked acf_neumf_grad calls on the
    # same batches (each call = k_nmf_step + the small k_nmf_wsum launch, so the
    # figure is an upper bound for the kernel); grad is restored afterwards
    reps = 200
    gsave = st.grad.clone()
    lb = torch.zeros(2, device=dev)
    for k in range(8):
        s_ = slice(k * B, (k + 1) * B)
        ctx.grad(U[s_], I[s_], Y[s_], hp, lb, check=False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        s_ = slice((k % 64) * B, (k % 64 + 1) * B)
        ctx.grad(U[s_], I[s_], Y[s_], hp, lb, check=False)
    e1.record()
    torch.cuda.synchronize(dev)
    step_us = e0.elapsed_time(e1) * 1e3 / reps
    ctx.predict(U[:8], I[:8])  # verifies the unchecked calls (a give-up would raise here)
    st.grad.copy_(gsave)
    del gsave
    d4 = 4 * d
    # algorithmic bytes of one step: the 4 embedding rows of every instance gathered
    # by the clean and by the adversarial pass, the adversarial pass's 4 delta rows,
    # and the MLP/head weights read once per instance workgroup (B / 16 of them per pass)
    nwg = -(-B // 16)
    wbytes = 4 * (2 * d * 2 * d + 2 * d + 2 * d * d + d + 2 * d + 1)
    step_bytes = 2 * B * 4 * d4 + B * 4 * d4 + 2 * nwg * wbytes
    step_gbs = step_bytes / (step_us * 1e-6) / 1e9

    # the yelp-shaped buffer (212 MB of p, g, m, v) stays in the 256 MB Infinity
    # Cache between steps: its Adam rate is not an HBM rate.  The dense Adam's
    # rate is taken on the same kernel over a 1.2 GB buffer (262,144 user rows),
    # which streams from HBM; the yelp-shaped rate is reported beside it.
    adam_us_mall = adam_time(ctx)
    nparam = st.params.numel()
    big = nm.NeuMFState(262_144, ds.num_items + 1, d, dev)
    bctx = nm.NeuMFContext(big, B)
    adam_us = adam_time(bctx)
    nbig = big.params.numel()
    achieved = 8 * 4 * nbig / (adam_us * 1e-6) / 1e9
    del bctx, big
    return {"metric": "adversarial NeuMF training instances/sec (yelp-sort-shaped, d=64)",
            "value": round(n / dt, 1), "unit": "instances/s", "ms_per_step": round(1e3 * dt / nb, 4),
            "dtype": "f32", "data": "synthetic yelp-sort-shaped (25,677 users x 25,815 items, 705k "
                                    "pairs) + 1 rejected negative each (MF.py:42-56)",
            "config": {"workload": "AdversarialNeuMF, FGSM on the 4 embedding tables, eps 0.5, "
                                   "weight 1, Keras Adam lr 0.001, batch 512", "dim": d, "batch": B,
                       "instances": n, "params": nparam},
            "final_loss": round(float(losses[-1, 0]), 5),
            "recoveries": ctx.recoveries(),
            "roofline": {"bound": "latency", "kernel": "k_nmf_step", "achieved": round(step_gbs, 2),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(step_gbs / HBM_PEAK_GBS, 5),
                         "bytes_per_launch": int(step_bytes), "avg_launch_us": round(step_us, 3),
                         "bytes_formula": "2 passes x B x 4 embedding rows x 4d B + B x 4 delta rows x 4d B "
                                          "+ 2 x (B/16 workgroups) x MLP/head weights",
                         "timing": f"HIP events over {reps} unchecked acf_neumf_grad calls on the bench's "
                                   "batches (k_nmf_step + k_nmf_wsum each): an upper bound for the kernel",
                         "note": "one step is a dependent chain (gather -> 4 MFMA layers -> weight "
                                 "gradients -> row sums -> adversarial pass) on 64 workgroups at B = 512: "
                                 "latency-bound, far from any bandwidth or MFMA limit",
                         "traffic": None},
            "adam_dense": {"kernel": "k_nmf_adam", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                           "bytes_per_launch": 8 * 4 * nbig, "avg_launch_us": round(adam_us, 3),
                           "buffer": "1.2 GB (262,144 user rows: beyond the 256 MB Infinity Cache)",
                           "note": "the stepwise API's dense Adam; acf_neumf_train runs it lazily "
                                   "(k_nmf_adam_next + catch-up)"},
            "adam_yelp_shape": {"bytes_per_launch": 8 * 4 * nparam, "avg_launch_us": round(adam_us_mall, 3),
                                "achieved_GBs": round(8 * 4 * nparam / (adam_us_mall * 1e-6) / 1e9, 2),
                                "note": "212 MB buffer resident in the Infinity Cache between steps",
                                "traffic": (pmc_traffic("k_nmf_adam") or (None,))[0]}}


def eval_bench(acf, dev, reps=5):
    """the all-items ranking of utils.py:178-267 ("all" mode, K =
    100: every item but the user's trainList and test item) at the ml-1m and
    pinterest-20 shapes, d = 64, on random tables of the trained magnitude.  The
    U x I score sweep runs on v_mfma_f32_16x16x4_f32 (k_eval_mfma, with exact
    rescoring inside the f32 error band), timed per whole positions call (prep +
    sweep + exclusion correction) with HIP events; the VALU sweep (k_eval_all)
    beside it, and both must give the same positions.  Roofline: the sweep's
    2 U I d flops against the f32 MFMA peak (157.3 TFLOP/s)."""
    from argparse import Namespace
    ev = importlib.import_module(PKG + ".evaluate")
    out = {}
    for name, ds, ref_s in (("ml-1m", acf.ml1m_like(seed=2019), 5.3), ("pinterest-20", acf.pinterest_like(seed=2019),
                                                                        None)):
        d = 64
        g = torch.Generator(device=dev).manual_seed(3)
        P = torch.randn(ds.num_users + 1, d, device=dev, generator=g) * 0.3
        Q = torch.randn(ds.num_items + 1, d, device=dev, generator=g) * 0.3
        plan = ev.init_eval_model(ds, Namespace(eval_mode="all"))
        nu, nc = len(plan.users), plan.num_candidates

        for kernel in ("auto", "mfma", "valu"):  # warm (and the one-off index range checks)
            ev.positions(P, Q, plan, kernel)

        def timed(kernel):
            pos = ev.positions(P, Q, plan, kernel)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(reps):
                pos = ev.positions(P, Q, plan, kernel)
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1) / reps, pos.cpu().numpy()

        ms, pos = timed("auto")
        ms_mfma, pos_mfma = timed("mfma")
        ms_valu, pos_valu = timed("valu")
        tf = 2.0 * nu * nc * d / (ms * 1e-3) / 1e12
        tf_mfma = 2.0 * nu * nc * d / (ms_mfma * 1e-3) / 1e12
        out[name] = {"users": nu, "candidates": nc, "dim": d, "ms_per_eval": round(ms, 3),
                     "users_per_s": round(nu / (ms * 1e-3), 1), "mfma_ms_per_eval": round(ms_mfma, 3),
                     "valu_ms_per_eval": round(ms_valu, 3),
                     "positions_equal_valu": bool((pos == pos_valu).all() and (pos_mfma == pos_valu).all()),
                     "roofline": {"bound": "mfma", "kernel": "k_eval_fused", "achieved": round(tf_mfma, 2),
                                  "peak": 157.3, "unit": "TFLOP/s", "frac": round(tf_mfma / 157.3, 4),
                                  "auto_achieved": round(tf, 2)},
                     "reference_published_s": ref_s}
        del P, Q, plan
    return out


def main():
    a = parse()
    if check_world(a.gpus, os.environ) == "launch":
        sys.exit(launch_ranks(a))
    # RCCL prints its version banner on stdout at init: keep fd 1 for the one JSON line
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if a.rehearse_one_gpu:
        local = 0
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        if a.rehearse_one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    acf = importlib.import_module(PKG)
    ops = importlib.import_module(PKG + ".ops")
    B, d = a.batch, a.dim
    ds = acf.ml1m_like(seed=2019 + rank)
    U1, I1 = ds.num_users + 1, ds.num_items + 1
    total = a.warmup + a.steps
    chunk = min(a.chunk, a.steps)
    # the batches the warm-up calls below read; --full's timing pass and CPU baseline
    # read a prefix of the same stream (its first batches do not depend on its length)
    need = max(total, 2 * chunk + a.steps % chunk)
    u, i, j = make_triplets(acf, ds, B, max(need, a.time_batches, a.cpu_batches) if a.full else need, dev,
                            seed=rank)
    tabs = init_tables(U1, I1, d, dev, seed=rank)
    P0, Q0 = (tabs[0].clone(), tabs[1].clone()) if a.full else (None, None)
    # chunk c+1 is planned on a side stream beside chunk c's streamed step
    pipe = ops.PlanPipeline(U1, I1, d, B, chunk, dev, overlap=False if a.no_plan_overlap else None)
    pipe.set_slot_mapping(a.mapping)
    pipe.set_stream(not a.no_stream)
    hp = ops.StepHParams(lr=0.05, eps=0.5, reg=0.0, reg_adv=1.0, adver=1)
    graph = not a.eager
    # warmup: W steps plus every chunk size the timed region uses on both contexts
    # (graph capture happens here)
    pipe.run(tabs, hp, u, i, j, 0, max(a.warmup, 2 * chunk), graph=graph)
    if a.steps % chunk:
        pipe.run(tabs, hp, u, i, j, 0, 2 * chunk + a.steps % chunk, graph=graph)
    # and the exact call the timed region makes, a few times: its first issue pays
    # one-off host costs (≈25 us of enqueue on a 20-batch call), and the next few
    # are still ~5 us slower than the steady state of a training loop that issues
    # it over and over (tools/short_call.py --same: 133, 130, 128, ... 126 us)
    # (a call of more than 100,000 batches runs for the better part of a second:
    # those costs vanish in it, and one issue is enough)
    for _ in range(3 if a.steps <= 100_000 else 1):
        pipe.run(tabs, hp, u, i, j, a.warmup, a.steps, graph=graph)
        torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    if dist:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    pipe.run(tabs, hp, u, i, j, a.warmup, a.steps, graph=graph)
    torch.cuda.synchronize(dev)
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    value = world * a.steps * B / elapsed
    finite = bool(torch.isfinite(tabs[0]).all() and torch.isfinite(tabs[1]).all())
    step_errors = pipe.step_errors()
    recoveries = pipe.stream_recoveries()  # streamed calls replayed (a hand-off wait gave up)
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, tabs, rank)

    out = {
        "metric": "BPR triplets/sec (APR ml-1m d=64)",
        "value": round(value, 1),
        "unit": "triplets/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(1e3 * elapsed / a.steps, 5),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": round(value / REF_CPU_TRIPLETS_PER_S, 2),
        "dtype": "f32",
        "data": "synthetic ml-1m-shaped (seeded; users>=20 interactions, Zipf items), device sampler",
        "config": {"workload": "APR phase, ml-1m-shaped, d=64, batch 512, eps 0.5, reg_adv 1, "
                               "lr 0.05 Adagrad (run_adv_ori.py --model apr)",
                   "users": ds.num_users, "items": ds.num_items, "dim": d, "global_batch": B * world,
                   "per_gpu_batch": B, "parallelism": f"replicas x{world}",
                   "launch": "eager" if a.eager else "hipGraph"},
        "tables_finite": finite,
        "step_errors": step_errors,
        "stream_recoveries": recoveries,
        # the process group this line was measured in: ranks, backend, and how many
        # of them talk over RCCL (0 for the one-GPU gloo rehearsal)
        "world": {"ranks": world, "backend": None if dist is None else dist.get_backend(),
                  "rccl_ranks": world if dist is not None and dist.get_backend() == "nccl" else 0,
                  "gpus_flag": a.gpus, "rehearsal": bool(a.rehearse_one_gpu)},
    }
    tctx = None
    if a.full:
        # roofline of the dominant kernel (separate eager pass with per-launch events)
        tctx = ops.APRContext(U1, I1, d, B, a.time_batches, dev)
        tctx.set_slot_mapping(a.mapping)
        tctx.set_stream(not a.no_stream)
        st = batch_stats(u, i, j, B, a.time_batches, U1, I1)
        out["roofline"] = roof = kernel_roofline(ops, tctx, tabs, hp, u, i, j, B, d, a.time_batches, st)
        out["step_bandwidth"] = step_bandwidth(d, B, st, value / world)
        out["batch_stats"] = {k: round(v, 1) for k, v in st.items()}
        out["step_stream"] = roof["kernel"].startswith("k_stream")
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        out["cpu_baseline"] = cb = cpu_baseline(u, i, j, P0, Q0, B, a.cpu_batches)
        out["vs_cpu_baseline"] = round(value / cb["value"], 2)  # vs_baseline: the published 87k
    big = None
    if not a.no_sharded or (rank == 0 and not a.no_large):
        del pipe, tctx
        torch.cuda.empty_cache()
        big = acf.synthetic_large(device=dev)
    def side_line(fn, *args, collective=False):
        """A side line that raises is recorded, not fatal: the headline line above
        is measured and must still be printed.  Except a line whose collectives
        run on every rank (sharded_lines) at world > 1: a rank that failed alone
        would leave its peers blocked in their next collective until the
        watchdog fires, so the exception propagates and the launcher ends the
        job at once."""
        if collective and world > 1:
            return fn(*args)
        try:
            return fn(*args)
        except Exception as e:  # noqa: BLE001
            print(f"bench: {fn.__name__} failed: {e!r}", file=sys.stderr, flush=True)
            return {"error": repr(e)[:300]}

    if not a.no_sharded:  # every rank takes part
        out["sharded"] = side_line(sharded_lines, acf, ops, dev, dist, world, rank, big, a.sharded_steps,
                                   collective=True)
    if rank == 0 and not a.no_neumf:
        out["neumf"] = side_line(neumf_bench, acf, dev)
    if rank == 0 and not a.no_eval:
        out["eval_all_items"] = side_line(eval_bench, acf, dev)
    if rank == 0 and not a.no_large:
        out["roofline_large_batch"] = side_line(large_batch_roofline, acf, ops, dev, big, 128)
        out["roofline_large_batch_d64"] = side_line(large_batch_roofline, acf, ops, dev, big, 64)
        del big
        torch.cuda.empty_cache()
    if rank == 0:
        print(json.dumps(out), file=json_out, flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
