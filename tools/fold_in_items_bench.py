#!/usr/bin/env python3
"""Time the fold-in of new items in one process: ml1m_like() transposed -- every
item's user list as a "new item" against random tables of the trained size,
d = 64, 20 epochs, slices of 512, APR step (ops.fold_in_items, one launch) -- and
in the same run on the same GPU
  (a) ops.fold_in_users on the untransposed lists (the same number of
      triplet-steps through the user kernel), and
  (b) a torch restatement of the same item steps on padded batched tensors
      ([items, 512] index blocks, [items, 512, d] gathers, dozens of kernels per
      step): what one would write without the kernel.
The longest list of each side is also timed alone (one workgroup): a launch
cannot end before its longest list has run its dependent slices.

Times are device events around one call each after a warm-up; the median of
`rounds` alternating repeats is reported, with milliseconds, triplet-steps per
second and the gather bandwidth against the algorithmic bytes (per epoch T
triplets x (one row of P + one row of Q) x d x 4 B, each row counted once: the
adversarial half re-reads it from cache).  Needs a HIP device; writes one JSON
document (default profiles/fold_in_items_ml1m.json).

    python tools/fold_in_items_bench.py [--out FILE] [--epochs E] [--rounds N]
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


class TorchFoldItems:
    """The same steps with torch ops: items padded to [n, slices, batch] blocks.
    The lists hold no user twice, so a user row has one reference per slice; a
    negative may repeat inside a slice, so its gradient is a segment sum."""

    def __init__(self, P, Q, off, users, neg, batch, hp, torch):
        import numpy as np
        self.torch, self.P, self.Q, self.hp, self.B = torch, P, Q, hp, batch
        dev = Q.device
        lens = np.diff(off)
        n, E = len(lens), neg.shape[0]
        S = int(max(1, -(-lens.max() // batch)))
        pos = np.zeros((n, S * batch), np.int64)
        mask = np.zeros((n, S * batch), bool)
        owner = np.repeat(np.arange(n), lens)
        within = np.arange(off[-1]) - np.repeat(off[:-1], lens)
        pos[owner, within] = users
        mask[owner, within] = True
        self.slices = []
        for s in range(S):
            act = np.flatnonzero(lens > s * batch)
            sl = slice(s * batch, (s + 1) * batch)
            ng = np.zeros((E, len(act), batch), np.int64)
            inside = (within >= s * batch) & (within < (s + 1) * batch)
            row = np.searchsorted(act, owner[inside])
            ng[:, row, within[inside] - s * batch] = neg[:, inside]
            self.slices.append((torch.as_tensor(act, device=dev), torch.as_tensor(pos[act, sl], device=dev),
                                torch.as_tensor(ng, device=dev), torch.as_tensor(mask[act, sl], device=dev)))
        self.n, self.E = n, E

    def run(self):
        torch, P, Q, hp = self.torch, self.P, self.Q, self.hp
        F = torch.nn.functional
        d, I1 = Q.shape[1], Q.shape[0]
        q = torch.zeros(self.n, d, device=Q.device)
        a = torch.full_like(q, 0.1)
        loss = torch.zeros(self.E, self.n, device=Q.device)

        def grad_scale(x, m):
            xc = x.clamp(hp.clip_lo, hp.clip_hi)
            return -torch.sigmoid(-xc) * ((x >= hp.clip_lo) & (x <= hp.clip_hi)) * m, F.softplus(-xc) * m

        for e in range(self.E):
            for act, u, jn, m in self.slices:
                j = jn[e]
                qr = q[act]
                pu, qj = P[u], Q[j]                                   # [na, B, d]
                x = (pu * qr[:, None, :]).sum(-1) - (pu * qj).sum(-1)
                g, ls = grad_scale(x, m)
                loss[e, act] += ls.sum(1)
                grad = (g[..., None] * pu).sum(1)
                if hp.adver:
                    dq = hp.eps * F.normalize(grad, dim=1, eps=1e-6)
                    du = hp.eps * F.normalize(g[..., None] * qr[:, None, :] - g[..., None] * qj, dim=2, eps=1e-6)
                    # negative rows of a slice: gradients summed per (item of the block, negative)
                    keys = torch.arange(act.numel(), device=Q.device)[:, None] * I1 + j
                    uniq, inv = torch.unique(keys.reshape(-1), return_inverse=True)
                    gj = torch.zeros(uniq.numel(), d, device=Q.device).index_add_(0, inv, (-g[..., None] * pu).reshape(-1, d))
                    dj = hp.eps * F.normalize(gj[inv].reshape(pu.shape), dim=2, eps=1e-6)
                    pp, qq, qja = pu + du, qr + dq, qj + dj
                    xa = (pp * qq[:, None, :]).sum(-1) - (pp * qja).sum(-1)
                    ga, _ = grad_scale(xa, m)
                    grad = grad + ((hp.reg_adv * ga)[..., None] * pp).sum(1)
                if hp.reg:
                    grad = grad + (2.0 * hp.reg / d) * (2.0 if hp.adver else 1.0) * qr
                an = a[act] + grad * grad
                a[act] = an
                q[act] = qr - hp.lr * grad * torch.rsqrt(an)
        return q, a, loss


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fold_in_items_ml1m.json"))
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("fold_in_items_bench: no HIP device; nothing is measured without one", file=sys.stderr)
        return 2
    ops = importlib.import_module(PKG + ".ops")
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    dev = torch.device("cuda:0")
    ds = data.ml1m_like()
    soff, sitems = ds.sorted_lists()
    nu, ni = ds.num_users, ds.num_items
    uoff = np.asarray(soff[:nu + 1], dtype=np.int64)
    uitems = np.asarray(sitems[:uoff[-1]], dtype=np.int32)
    T, E, d = int(uoff[-1]), args.epochs, args.dim
    # transposed: the users of every item, ascending (a stable sort by item keeps the user order)
    owner = np.repeat(np.arange(nu, dtype=np.int32), np.diff(uoff))
    order = np.argsort(uitems, kind="stable")
    users = owner[order]
    ioff = np.zeros(ni + 1, dtype=np.int64)
    np.cumsum(np.bincount(uitems, minlength=ni)[:ni], out=ioff[1:])
    ineg = ev.fold_item_negatives(ioff, users, ni, E, seed=0)
    uneg = ev.fold_negatives(uoff, uitems, ni, E, seed=0)
    g = torch.Generator().manual_seed(1)
    P = (torch.randn(nu + 1, d, generator=g) * 0.1).to(dev)
    Q = (torch.randn(ni + 1, d, generator=g) * 0.1).to(dev)
    hp = ops.StepHParams(adver=1)
    t_ioff, t_users, t_ineg = (torch.as_tensor(x, device=dev) for x in (ioff, users, ineg))
    t_uoff, t_uitems, t_uneg = (torch.as_tensor(x, device=dev) for x in (uoff, uitems, uneg))
    kernel = lambda: ops.fold_in_items(P, Q, t_ioff, t_users, t_ineg, hp, E, args.batch, check=False)  # noqa: E731
    user_kernel = lambda: ops.fold_in_users(Q, t_uoff, t_uitems, t_uneg, hp, E, args.batch, check=False)  # noqa: E731
    restated = TorchFoldItems(P, Q, ioff, users, ineg, args.batch, hp, torch)
    variants = {"fold_in_items": kernel, "fold_in_users": user_kernel, "torch_padded": restated.run}
    # the longest list of each side alone: one workgroup, the launch's critical path
    ilens, ulens = np.diff(ioff), np.diff(uoff)
    ri, ru = int(np.argmax(ilens)), int(np.argmax(ulens))
    li = [torch.as_tensor(x, device=dev) for x in (np.array([0, ilens[ri]], np.int64), users[ioff[ri]:ioff[ri + 1]],
                                                   np.ascontiguousarray(ineg[:, ioff[ri]:ioff[ri + 1]]))]
    lu = [torch.as_tensor(x, device=dev) for x in (np.array([0, ulens[ru]], np.int64), uitems[uoff[ru]:uoff[ru + 1]],
                                                   np.ascontiguousarray(uneg[:, uoff[ru]:uoff[ru + 1]]))]
    alone = {"fold_in_items": lambda: ops.fold_in_items(P, Q, li[0], li[1], li[2], hp, E, args.batch, check=False),
             "fold_in_users": lambda: ops.fold_in_users(Q, lu[0], lu[1], lu[2], hp, E, args.batch, check=False)}
    first = kernel()
    again = kernel()
    same = all(bool(torch.equal(x, y)) for x, y in zip(first, again))
    ref = restated.run()
    diff = float((first[0] - ref[0]).abs().max())
    loss_diff = float(((first[2] - ref[2]).abs() / ref[2].abs().clamp_min(1.0)).max())
    del ref
    for fn in [*variants.values(), *alone.values()]:
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    ms_alone = {k: [] for k in alone}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, torch))
        for k, fn in alone.items():
            ms_alone[k].append(timed(fn, torch))
    med = {k: statistics.median(v) for k, v in ms.items()}
    steps = T * E
    alg_bytes = steps * 2 * d * 4
    doc = {"tool": "tools/fold_in_items_bench.py", "device": torch.cuda.get_device_name(0), "dataset": "ml1m_like",
           "new_items": int(ni), "user_rows": int(P.shape[0]), "item_rows": int(Q.shape[0]), "dim": d, "epochs": E,
           "batch": args.batch, "triplets_per_epoch": T,
           "item_list_len_min_median_max": [int(ilens.min()), int(np.median(ilens)), int(ilens.max())],
           "user_list_len_min_median_max": [int(ulens.min()), int(np.median(ulens)), int(ulens.max())],
           "item_slices_per_epoch": int((-(-ilens // args.batch)).sum()),
           "user_slices_per_epoch": int((-(-ulens // args.batch)).sum()), "rounds": args.rounds,
           "repeat_is_bit_identical": same, "max_abs_diff_Q_vs_torch": diff, "max_rel_diff_loss_vs_torch": loss_diff,
           "ms_median_longest_list_alone": {k: statistics.median(v) for k, v in ms_alone.items()},
           "ms_median": med, "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
           "triplet_steps_per_s": {k: steps / (v * 1e-3) for k, v in med.items()},
           "algorithmic_gather_bytes": alg_bytes,
           "gather_GBps_vs_algorithmic_bytes": {k: alg_bytes / (v * 1e-3) / 1e9 for k, v in med.items()},
           "items_over_users_per_triplet": med["fold_in_items"] / med["fold_in_users"],
           "kernel_over_torch": med["fold_in_items"] / med["torch_padded"]}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
