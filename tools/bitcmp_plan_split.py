"""Bit-compare two builds of libacf_apr.so across the plan / step seam and the
leaf entry points of acf_sample.hip, at the smallest shapes that reach each
plan builder and each step schedule (tables of 3,000 x 2,000 rows, Zipf items:
rows repeat within and across batches; 2 calls of 4 batches per case):

  batch plan + k_stream    B = 512, d = 64 and d = 20 (the odd geometry)
  sort plan                the same with set_plan_mode("sort")
  two-kernel schedule      B = 512, d = 320 (NV = 2: no streamed step)
  hash plan, k_tri_*       B = 4,096, d = 64
  packed sort plan         the same with set_plan_mode("sort"): k_tri_*, and the list
                           kernels (k_clean_list, k_adv_list) with fusion off
  small shard plan         ShardedAPR (one rank), B = 512, one-batch plans
  shard passes, hash plan  ShardedAPR, B = 2,048, a 4-step chunk plan
  sample_epoch (uniform and alias), dns_select, bpr_forward

One JSON line per case: sha256 of P, Q, accP, accQ, the per-triplet losses
(not in shard mode: the passes keep none), the plan kinds and, for the second
call, the launch counts per kernel kind.  ACF_ALT_LIB=path loads that build in
place of the package's (as tools/bitcmp_lib.py).  Run it once per build, then
  python3 tools/bitcmp_plan_split.py --compare a.jsonl b.jsonl out.json
writes the per-case equality."""
import ctypes
import hashlib
import importlib
import json
import os
import socket
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(a, b, out):
    ra, rb = ([json.loads(x) for x in open(p) if x.startswith("{")] for p in (a, b))
    cases = []
    for x, y in zip(ra, rb):
        keys = [k for k in x if k != "lib"]
        cases.append({"case": x["case"], "d": x.get("d"), "equal": all(x[k] == y.get(k) for k in keys) and x["case"] == y["case"],
                      "differs": [k for k in keys if x[k] != y.get(k)], "plan_kinds": x.get("plan_kinds"),
                      "launches": x.get("launches")})
    res = {"parent": ra[0]["lib"], "change": rb[0]["lib"], "n_cases": [len(ra), len(rb)],
           "all_equal": len(ra) == len(rb) and all(c["equal"] for c in cases), "cases": cases}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({"all_equal": res["all_equal"], "cases": len(cases)}))
    return 0 if res["all_equal"] else 1


if len(sys.argv) > 1 and sys.argv[1] == "--compare":
    sys.exit(compare(*sys.argv[2:5]))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import bench  # noqa: E402

ops = importlib.import_module(bench.PKG + ".ops")
alt = os.environ.get("ACF_ALT_LIB")
if alt:
    nat = importlib.import_module(bench.PKG + "._native")
    lib = ctypes.CDLL(alt)
    for fname, (res, args) in nat.SIGNATURES.items():
        if hasattr(lib, fname):
            fn = getattr(lib, fname)
            fn.restype, fn.argtypes = res, args
    nat._lib = lib
dev = torch.device("cuda", 0)
U1, I1, NB, CALLS = 3000, 2000, 4, 2


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def report(case, **fields):
    print(json.dumps({"case": case, "lib": alt or "package", **fields}), flush=True)


def problem(seed, d, n):
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((U1, d)) * 0.1).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.1).astype(np.float32)
    u = rng.integers(0, U1, n).astype(np.int32)
    i = ((rng.zipf(1.2, n) - 1) % I1).astype(np.int32)  # hot items: many occurrences per batch
    j = rng.integers(0, I1, n).astype(np.int32)
    j[::29] = i[::29]
    return P, Q, u, i, j


def step_case(case, d, B, mode, fusion=True):
    P, Q, u, i, j = problem(1000 * d + B, d, CALLS * NB * B)
    tabs = [torch.tensor(P, device=dev), torch.tensor(Q, device=dev),
            torch.full((U1, d), 0.1, device=dev), torch.full((I1, d), 0.1, device=dev)]
    ctx = ops.APRContext(U1, I1, d, B, NB, dev)
    ctx.set_plan_mode(mode)
    ctx.set_fusion(fusion)  # off: a packed plan is the slot plan of the list kernels (k_clean_list, k_adv_list)
    hp = ops.StepHParams(adver=1)
    kinds, losses, launches = [], [], None
    for c in range(CALLS):
        s = slice(c * NB * B, (c + 1) * NB * B)
        ctx.plan(*(torch.tensor(x[s], device=dev) for x in (u, i, j)), B)
        kinds.append(ctx.plan_kind())
        if c == 0:
            ctx.train_planned(tabs, hp)
        else:
            launches = {k: v[1] for k, v in ctx.time_kernels(tabs, hp).items()}
        losses += list(ctx.losses())
    torch.cuda.synchronize()
    report(case, d=d, B=B, plan_kinds=kinds, launches=launches, step_errors=ctx.step_errors(),
           recoveries=ctx.stream_recoveries(), P=sha(tabs[0]), Q=sha(tabs[1]), accP=sha(tabs[2]), accQ=sha(tabs[3]),
           losses=sha(*losses))


def shard_case(case, d, B, chunk):
    D_ = importlib.import_module(bench.PKG + ".distributed")
    P, Q, u, i, j = problem(77 + B, d, CALLS * NB * B)
    with D_.ShardedAPR(U1, I1, d, B, device=dev, init_P=P, init_Q=Q) as sh:
        sh.train(*(torch.tensor(x, device=dev) for x in (u, i, j)), ops.StepHParams(adver=1), chunk=chunk)
        torch.cuda.synchronize(dev)
        got = sh.full_tables()
        report(case, d=d, B=B, plan_kinds=[sh.local.ctx.plan_kind()], step_errors=sh.step_errors(),
               **{n: sha(torch.as_tensor(g)) for n, g in zip(("P", "Q", "accP", "accQ"), got)})


def leaf_cases():
    d, n, B = 64, 4000, 512
    P, Q, u, i, _ = problem(5, d, n)
    order = np.lexsort((i, u))
    u, i = u[order], i[order]
    keep = np.r_[True, (u[1:] != u[:-1]) | (i[1:] != i[:-1])]  # sorted trainLists without repeats
    u, i = u[keep], i[keep]
    off = np.searchsorted(u, np.arange(U1 + 1)).astype(np.int64)
    pu, pi = torch.tensor(u, device=dev), torch.tensor(i, device=dev)
    ou, op, on = ops.sample_epoch(pu, pi, B, I1, off, pi, seed=11)
    report("sample_epoch", n_pos=int(u.size), u=sha(ou), pos=sha(op), neg=sha(on))
    prob, al = ops.alias_table(np.bincount(i, minlength=I1) + 1.0)
    au, ap, an = ops.sample_epoch(pu, pi, B, I1, off, pi, seed=12,
                                  alias=(torch.tensor(prob, device=dev), torch.tensor(al, device=dev)))
    report("sample_epoch_alias", prob=sha(torch.tensor(prob)), alias=sha(torch.tensor(al)), u=sha(au), pos=sha(ap),
           neg=sha(an))
    for dd in (64, 20):
        Pd, Qd, _, _, _ = problem(6 + dd, dd, 8)
        Pt, Qt = torch.tensor(Pd, device=dev), torch.tensor(Qd, device=dev)
        cand = torch.randint(0, I1, (ou.numel() * 4,), dtype=torch.int32, device=dev,
                             generator=torch.Generator(device=dev).manual_seed(3))
        report("dns_select", d=dd, out=sha(ops.dns_select(Pt, Qt, ou, cand, 4)))
        report("bpr_forward", d=dd, out=sha(*[t for t in ops.bpr_forward(Pt, Qt, ou, op, on, B) if t is not None]))


for d in (64, 20):
    step_case("batch_plan_stream", d, 512, "auto")
    step_case("sort_plan_stream", d, 512, "sort")
step_case("two_kernel", 320, 512, "auto")
step_case("hash_plan_tri", 64, 4096, "auto")
step_case("packed_sort_plan_tri", 64, 4096, "sort")
step_case("packed_sort_plan_lists", 64, 4096, "sort", fusion=False)
s = socket.socket()
s.bind(("127.0.0.1", 0))
port = s.getsockname()[1]
s.close()
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
try:
    shard_case("shard_plan_small", 64, 512, 1)
    shard_case("shard_pass_hash_plan", 64, 2048, 4)
finally:
    dist.destroy_process_group()
leaf_cases()
