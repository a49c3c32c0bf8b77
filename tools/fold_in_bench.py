#!/usr/bin/env python3
"""Time the fold-in of new users in one process: the 6,040 users of ml1m_like()
from their train lists against a random item table, d = 64, 20 epochs, slices of
512 (ops.fold_in_users, one launch), and in the same run on the same GPU a torch
restatement of the same steps on padded batched tensors ([users, 512] index
blocks, [users, 512, d] gathers, dozens of kernels per step): what one would
write without the kernel.

Times are device events around one call each after a warm-up; the median of
`rounds` alternating repeats is reported, with milliseconds, triplet-steps per
second and the gather bandwidth against the algorithmic bytes (per epoch T
triplets x 2 rows of Q x d x 4 B, each row counted once: the adversarial half
re-reads it from cache).  Needs a HIP device; writes one JSON document (default
profiles/fold_in_ml1m.json).

    python tools/fold_in_bench.py [--out FILE] [--epochs E] [--rounds N]
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


def timed(fn, torch):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


class TorchFold:
    """The same steps with torch ops: users padded to [n, slices, batch] blocks."""

    def __init__(self, Q, off, items, neg, batch, hp, torch):
        import numpy as np
        self.torch, self.Q, self.hp, self.B = torch, Q, hp, batch
        dev = Q.device
        lens = np.diff(off)
        n, E = len(lens), neg.shape[0]
        S = int(max(1, -(-lens.max() // batch)))
        pos = np.zeros((n, S * batch), np.int64)
        ng = np.zeros((E, n, S * batch), np.int64)
        mask = np.zeros((n, S * batch), bool)
        owner = np.repeat(np.arange(n), lens)
        within = np.arange(off[-1]) - np.repeat(off[:-1], lens)
        pos[owner, within] = items
        ng[:, owner, within] = neg
        mask[owner, within] = True
        self.slices = []
        for s in range(S):
            act = np.flatnonzero(lens > s * batch)
            sl = slice(s * batch, (s + 1) * batch)
            self.slices.append((torch.as_tensor(act, device=dev), torch.as_tensor(pos[act, sl], device=dev),
                                torch.as_tensor(ng[:, act, sl], device=dev),
                                torch.as_tensor(mask[act, sl], device=dev)))
        self.n, self.E = n, E

    def run(self):
        torch, Q, hp = self.torch, self.Q, self.hp
        F = torch.nn.functional
        d, I1 = Q.shape[1], Q.shape[0]
        p = torch.zeros(self.n, d, device=Q.device)
        a = torch.full_like(p, 0.1)
        loss = torch.zeros(self.E, self.n, device=Q.device)

        def grad_scale(x, m):
            xc = x.clamp(hp.clip_lo, hp.clip_hi)
            return -torch.sigmoid(-xc) * ((x >= hp.clip_lo) & (x <= hp.clip_hi)) * m, F.softplus(-xc) * m

        for e in range(self.E):
            for act, i, jn, m in self.slices:
                j = jn[e]
                pr = p[act]
                qi, qj = Q[i], Q[j]                                   # [na, B, d]
                x = (pr[:, None, :] * qi).sum(-1) - (pr[:, None, :] * qj).sum(-1)
                g, ls = grad_scale(x, m)
                loss[e, act] += ls.sum(1)
                grad = (g[..., None] * qi).sum(1) - (g[..., None] * qj).sum(1)
                if hp.adver:
                    dp = hp.eps * F.normalize(grad, dim=1, eps=1e-6)
                    # item rows of a slice: coefficients summed per (user of the block, item)
                    row = torch.arange(act.numel(), device=Q.device)[:, None] * I1
                    keys = torch.cat([row + i, row + j], 1)
                    uniq, inv = torch.unique(keys.reshape(-1), return_inverse=True)
                    c = torch.zeros(uniq.numel(), device=Q.device).index_add_(0, inv, torch.cat([g, -g], 1).reshape(-1))
                    c = c[inv].reshape(keys.shape)
                    B = i.shape[1]
                    di = hp.eps * F.normalize(c[:, :B, None] * pr[:, None, :], dim=2, eps=1e-6)
                    dj = hp.eps * F.normalize(c[:, B:, None] * pr[:, None, :], dim=2, eps=1e-6)
                    pp, qia, qja = pr + dp, qi + di, qj + dj
                    xa = (pp[:, None, :] * qia).sum(-1) - (pp[:, None, :] * qja).sum(-1)
                    ga, _ = grad_scale(xa, m)
                    ga = hp.reg_adv * ga
                    grad = grad + (ga[..., None] * qia).sum(1) - (ga[..., None] * qja).sum(1)
                if hp.reg:
                    grad = grad + (2.0 * hp.reg / d) * (2.0 if hp.adver else 1.0) * pr
                an = a[act] + grad * grad
                a[act] = an
                p[act] = pr - hp.lr * grad * torch.rsqrt(an)
        return p, a, loss


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fold_in_ml1m.json"))
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("fold_in_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    dev = torch.device("cuda:0")
    ds = data.ml1m_like()
    soff, sitems = ds.sorted_lists()
    n = ds.num_users
    off = np.asarray(soff[:n + 1], dtype=np.int64)
    items = np.asarray(sitems[:off[-1]], dtype=np.int32)
    T, E, d = int(off[-1]), args.epochs, args.dim
    neg = ev.fold_negatives(off, items, ds.num_items, E, seed=0)
    g = torch.Generator().manual_seed(1)
    Q = (torch.randn(ds.num_items + 1, d, generator=g) * 0.1).to(dev)
    hp = ops.StepHParams(adver=1)
    t_off, t_items, t_neg = (torch.as_tensor(x, device=dev) for x in (off, items, neg))
    kernel = lambda: ops.fold_in_users(Q, t_off, t_items, t_neg, hp, E, args.batch, check=False)  # noqa: E731
    restated = TorchFold(Q, off, items, neg, args.batch, hp, torch)
    variants = {"fold_in_users": kernel, "torch_padded": restated.run}
    first = kernel()
    again = kernel()
    same = all(bool(torch.equal(x, y)) for x, y in zip(first, again))
    ref = restated.run()
    diff = float((first[0] - ref[0]).abs().max())
    loss_diff = float(((first[2] - ref[2]).abs() / ref[2].abs().clamp_min(1.0)).max())
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, torch))
    med = {k: statistics.median(v) for k, v in ms.items()}
    steps = T * E
    alg_bytes = steps * 2 * d * 4
    lens = np.diff(off)
    doc = {"tool": "tools/fold_in_bench.py", "device": torch.cuda.get_device_name(0), "dataset": "ml1m_like",
           "users": int(n), "item_rows": int(Q.shape[0]), "dim": d, "epochs": E, "batch": args.batch,
           "triplets_per_epoch": T, "list_len_min_median_max": [int(lens.min()), int(np.median(lens)), int(lens.max())],
           "slices_per_epoch": int((-(-lens // args.batch)).sum()), "rounds": args.rounds,
           "repeat_is_bit_identical": same, "max_abs_diff_P_vs_torch": diff, "max_rel_diff_loss_vs_torch": loss_diff,
           "ms_median": med, "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
           "triplet_steps_per_s": {k: steps / (v * 1e-3) for k, v in med.items()},
           "algorithmic_gather_bytes": alg_bytes,
           "gather_GBps_vs_algorithmic_bytes": {k: alg_bytes / (v * 1e-3) / 1e9 for k, v in med.items()},
           "kernel_over_torch": med["fold_in_users"] / med["torch_padded"]}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
