"""``MF`` — drop-in for the reference's APR/BPR-MF graph (``APR.py:85-202``).

The reference builds a TF1 graph and drives it with ``sess.run``.  This class keeps
that surface: the same constructor and attributes, ``build_graph()``, placeholder
handles (``user_input``, ``item_input_pos``, ``item_input_neg``) and fetch handles
(``update_P``, ``update_Q``, ``optimizer``, ``loss``, ``output``, ``output_neg``,
``embedding_P``, ``embedding_Q`` …), and :class:`Session` runs those fetches.
Under it, the tables are fp32 tensors on a HIP device and every fetch is a call
into ``libacf_apr.so``:

  ``sess.run([update_P, update_Q], fd)``  -> ``acf_apr_delta_update``
  ``sess.run(optimizer, fd)``             -> ``acf_apr_optimizer_step``
  ``sess.run([loss, output, output_neg])``-> ``acf_bpr_forward``
  ``sess.run(output, {user, item_pos})``  -> scores P[u]·Q[i]

For whole epochs ``train.training_batch`` bypasses the per-call plan and runs the
entire epoch from one plan through a cached hipGraph.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class _Handle:
    __slots__ = ("name",)

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return f"<acf handle {self.name}>"


def default_device():
    import os
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: the APR path runs only on MI355X (gfx950); "
                           "there is no CPU fallback")
    return torch.device("cuda", int(os.environ.get("LOCAL_RANK", torch.cuda.current_device())))


class MF:
    """MF(num_users, num_items, args) — APR.py:86-97.  Tables have num_users + 1 /
    num_items + 1 rows like APR.py:108,111 (twin=True: evaluation_adv.py:120,123
    sizes them num_users / num_items)."""

    def __init__(self, num_users, num_items, args, twin: bool = False):
        self.num_items = num_items
        self.num_users = num_users
        self.embedding_size = args.embed_size
        self.learning_rate = args.lr
        self.reg = args.reg
        self.dns = args.dns
        self.adv = args.adv
        self.eps = args.eps
        self.adver = args.adver
        self.reg_adv = args.reg_adv
        self.epochs = args.epochs
        self.twin = twin
        self.seed = getattr(args, "seed", None)
        # the K-step inner attack: trained by MFGrid only (ops.grid_train); an MF carries the
        # fields so that a grid member reports them, and its own trainers refuse K > 1
        self.adv_iters = getattr(args, "adv_iters", 1)
        self.adv_step = getattr(args, "adv_step", None)
        self.built = False

    # -- graph ----------------------------------------------------------------
    def _create_placeholders(self):
        self.user_input = _Handle("user_input")
        self.item_input_pos = _Handle("item_input_pos")
        self.item_input_neg = _Handle("item_input_neg")

    def _create_variables(self, device=None, generator=None):
        self.device = torch.device(device) if device is not None else default_device()
        extra = 0 if self.twin else 1
        self.num_user_rows = self.num_users + extra
        self.num_item_rows = self.num_items + extra
        d = self.embedding_size
        g = generator
        if g is None and self.seed is not None:
            g = torch.Generator().manual_seed(int(self.seed))
        # tf.truncated_normal(stddev=0.01): normal redrawn beyond 2 sigma (APR.py:107-112)
        P = torch.empty(self.num_user_rows, d, dtype=torch.float32)
        Q = torch.empty(self.num_item_rows, d, dtype=torch.float32)
        torch.nn.init.trunc_normal_(P, 0.0, 0.01, -0.02, 0.02, generator=g)
        torch.nn.init.trunc_normal_(Q, 0.0, 0.01, -0.02, 0.02, generator=g)
        self.embedding_P = P.to(self.device)
        self.embedding_Q = Q.to(self.device)
        # AdagradOptimizer slots, initial_accumulator_value = 0.1 (APR.py:195)
        self.accumulator_P = torch.full_like(self.embedding_P, 0.1)
        self.accumulator_Q = torch.full_like(self.embedding_Q, 0.1)
        self.h = None  # the ones-vector of APR.py:119 is the row reduction in the kernels

    def _create_fetches(self):
        for name in ("update_P", "update_Q", "optimizer", "loss", "loss_adv", "output", "output_neg",
                     "output_adv", "output_neg_adv", "opt_loss", "result"):
            setattr(self, name, _Handle(name))

    def build_graph(self, device=None, generator=None):
        """APR.py:197-202."""
        self._create_placeholders()
        self._create_variables(device, generator)
        self._create_fetches()
        # delta_P / delta_Q (APR.py:111-116): zeros until train.adv_update assigns them
        self.delta_P = torch.zeros_like(self.embedding_P)
        self.delta_Q = torch.zeros_like(self.embedding_Q)
        self._adv_calls = 0
        self._ctx = None
        self._pipe = None
        self._delta_feed = None
        self.built = True
        return self

    # -- state ----------------------------------------------------------------
    @property
    def tables(self):
        """The four tables for a READER: every queued streamed call is settled
        first (its lazy verification, ops.settle_tables)."""
        ops.settle_tables()
        return self.launch_tables

    @property
    def launch_tables(self):
        """The four tables for a training LAUNCH, without settling: a launch on
        them is ordered after the queued calls on the stream, and the native
        failure-safe gate covers the rest (settling here blocked the
        host on every queued call at each epoch)."""
        return (self.embedding_P, self.embedding_Q, self.accumulator_P, self.accumulator_Q)

    def hparams(self, adver=None) -> ops.StepHParams:
        adver = int(self.adver if adver is None else adver)
        return ops.StepHParams(lr=self.learning_rate, eps=self.eps, reg=self.reg,
                               reg_adv=self.reg_adv, adver=adver, adv=self.adv, seed=int(self.seed or 0),
                               adv_iters=self.adv_iters if adver else 1,  # a BPR step has no attack
                               adv_step=self.adv_step if adver else None)

    def context(self, batch_size: int, n_batches: int) -> ops.APRContext:
        self.hparams().require_one_step("MF.context")
        ctx = self._ctx
        if ctx is None or not ctx.fits(batch_size, n_batches):
            cap_b = max(batch_size, ctx.max_batch_size if ctx else 0)
            cap_n = max(n_batches, ctx.max_batches if ctx else 0)
            self._ctx = ctx = ops.APRContext(self.num_user_rows, self.num_item_rows,
                                             self.embedding_size, cap_b, cap_n, self.device)
        return ctx

    def pipeline(self, batch_size: int, chunk: int = 512) -> ops.PlanPipeline:
        """Epoch trainer: chunks of `chunk` batches, next chunk planned while one trains."""
        self.hparams().require_one_step("MF.pipeline")
        p = self._pipe
        if p is None or p.batch_size != batch_size or p.chunk != chunk:
            # concurrent planning for large batches only (device-wide sort plan); small
            # batches plan in line (batch-local plan, two launches per chunk)
            self._pipe = p = ops.PlanPipeline(self.num_user_rows, self.num_item_rows,
                                              self.embedding_size, batch_size, chunk, self.device,
                                              overlap=None)
        return p

    def reset_optimizer(self):
        """A fresh MF in the reference means fresh Adagrad slots (run_adv_ori.py:108)."""
        self.accumulator_P.fill_(0.1)
        self.accumulator_Q.fill_(0.1)

    def load_embeddings(self, P, Q):
        self.embedding_P.copy_(torch.as_tensor(np.asarray(P), dtype=torch.float32))
        self.embedding_Q.copy_(torch.as_tensor(np.asarray(Q), dtype=torch.float32))

    # -- single-batch entry points (one sess.run each) -------------------------
    def _plan_feed(self, u, i, j):
        u = ops._idx(u, "user_input", self.device)
        B = u.numel()
        ctx = self.context(B, 1)
        ctx.plan(u, i, j, B)
        return ctx

    def delta_update(self, u, i, j):
        """sess.run([update_P, update_Q], feed) — utils.py:117-118."""
        ctx = self._plan_feed(u, i, j)
        ctx.delta_update(self.launch_tables, self.hparams(adver=1), 0)
        self._delta_feed = (u, i, j)

    def optimizer_step(self, u, i, j):
        """sess.run(optimizer, feed) — utils.py:119."""
        ctx = self._ctx
        same = (self._delta_feed is not None and ctx is not None and ctx.n_batches == 1
                and all(a is b for a, b in zip(self._delta_feed, (u, i, j))))
        if self.adver and not same:
            self.delta_update(u, i, j)
            ctx = self._ctx
        elif not self.adver:
            ctx = self._plan_feed(u, i, j)
        ctx.optimizer_step(self.launch_tables, self.hparams(), 0)
        self._delta_feed = None

    def scores(self, users, items):
        """model.output for arbitrary (user, item) pairs: P[u]·Q[i] ([n,1])."""
        u = ops._idx(users, "user_input", self.device)
        i = ops._idx(items, "item_input_pos", self.device)
        n = u.numel()
        if n == 0:
            return np.zeros((0, 1), np.float32)
        _, _, op, _ = ops.bpr_forward(self.embedding_P, self.embedding_Q, u, i, i, n, want_scores=True)
        return op.cpu().numpy().reshape(-1, 1)

    def recommend(self, users, k, dataset=None):
        """The k best items of each user: (items [n, k] int32, scores [n, k]
        float32) numpy arrays, best first, -1 / -inf past a user's candidates.
        With a dataset the candidates are its items minus the user's train items
        (evaluate.recommend); without one, every item row."""
        from .evaluate import recommend
        return recommend(self, dataset, users=users, k=k)

    def fold_in(self, lists, **fold_args):
        """evaluate.fold_in: rows for new users fitted against this model's frozen
        item table (a FoldIn)."""
        from .evaluate import fold_in
        return fold_in(self, lists, **fold_args)

    def recommend_new(self, lists, k, **fold_args):
        """evaluate.recommend_new: the k best items of new users, their own lists
        excluded: (items [n, k], scores [n, k]) numpy arrays."""
        from .evaluate import recommend_new
        return recommend_new(self, lists, k, **fold_args)

    def fold_in_items(self, lists, **fold_args):
        """evaluate.fold_in_items: rows for new items fitted to their user lists
        against this model's frozen tables (a FoldInItems)."""
        from .evaluate import fold_in_items
        return fold_in_items(self, lists, **fold_args)

    def audience_new(self, lists, k, **fold_args):
        """evaluate.audience_new: the k best existing users of new items, their own
        users excluded: (users [n, k], scores [n, k]) numpy arrays."""
        from .evaluate import audience_new
        return audience_new(self, lists, k, **fold_args)

    def similar_items(self, items, k=10, metric="cosine", rows=None):
        """evaluate.similar_items: the k items nearest to each of `items` in the
        item table ('cosine', 'dot' or 'euclid'): (ids [n, k], scores [n, k])
        numpy arrays; never the item itself, never the padding row.  With rows (a
        FoldInItems or a [m, d] tensor) the queries are those rows instead."""
        from .evaluate import similar_items
        return similar_items(self, items, k=k, metric=metric, rows=rows)

    def similar_users(self, users, k=10, metric="cosine", rows=None):
        """evaluate.similar_users: the k users nearest to each of `users`; with
        rows (a FoldIn or a [m, d] tensor) the queries are those rows instead."""
        from .evaluate import similar_users
        return similar_users(self, users, k=k, metric=metric, rows=rows)

    def evaluate(self, dataset, plan, output_adv=0, args=None):
        """evaluate.evaluate: ((hr, ndcg, auc) per K, raw [users, 3, K]) of the
        leave-one-out protocol (plan: evaluate.init_eval_model)."""
        from .evaluate import evaluate
        return evaluate(self, None, dataset, plan, output_adv, args)

    def evaluate_multi(self, plan, cutoffs=(10, 50, 100), raw=False):
        """evaluate.evaluate_multi: recall / ndcg / map / ... @K, mrr and auc against
        several held-out items per user (plan: evaluate.init_eval_multi)."""
        from .evaluate import evaluate_multi
        return evaluate_multi(self, plan, cutoffs=cutoffs, raw=raw)

    def adv_update(self, train_batches, adv=None):
        """train.adv_update: delta_P / delta_Q over all the triplets as one batch."""
        from .train import adv_update
        return adv_update(self, None, train_batches, adv=adv)

    def robustness(self, dataset, plan, triplets, eps_list, modes=("grad", "random"), seed=0, iters=10, step=None,
                   side="both"):
        """evaluate.robustness: rows (mode, eps, hr@K, ndcg@K, auc) under a
        perturbation of both tables; iters, step and side are the "pgd" mode's."""
        from .evaluate import robustness
        return robustness(self, dataset, plan, triplets, eps_list, modes=modes, seed=seed, iters=iters, step=step,
                          side=side)

    def exposure(self, dataset, users=None, k=100, cutoffs=(10, 100), exclude_train=True):
        """evaluate.exposure: rows (cutoff, total, coverage, gini, entropy, arp,
        aplt) of this model's own top-k lists."""
        from .evaluate import exposure
        return exposure(self, dataset, users=users, k=k, cutoffs=cutoffs, exclude_train=exclude_train)

    def recommend_diverse(self, dataset=None, users=None, k=10, pool=128, lam=0.7, metric="cosine",
                          rel_norm="minmax", exclude_train=True):
        """evaluate.recommend_diverse: this model's `pool` best items per user
        re-ranked to k by maximal marginal relevance: (items [n, k], scores [n, k])
        numpy arrays."""
        from .evaluate import recommend_diverse
        return recommend_diverse(self, dataset, users=users, k=k, pool=pool, lam=lam, metric=metric,
                                 rel_norm=rel_norm, exclude_train=exclude_train)

    def diversity(self, dataset, users=None, k=100, cutoffs=(10, 100), metric="cosine"):
        """evaluate.diversity: rows (cutoff, ils), the mean intra-list similarity of
        this model's own top-k lists."""
        from .evaluate import diversity
        return diversity(self, dataset, users=users, k=k, cutoffs=cutoffs, metric=metric)

    def diversity_tradeoff(self, dataset, lams=(1.0, 0.7, 0.5), k=10, pool=128, cutoffs=(10,), metric="cosine"):
        """evaluate.diversity_tradeoff: rows (lam, cutoff, hr, ndcg, ils, total,
        coverage, gini, entropy, arp, aplt) of the MMR re-ranked lists."""
        from .evaluate import diversity_tradeoff
        return diversity_tradeoff(self, dataset, lams=lams, k=k, pool=pool, cutoffs=cutoffs, metric=metric)

    def list_robustness(self, dataset, triplets, eps_list, k=100, cutoffs=(1, 10, 100), modes=("grad", "random"),
                        p=0.9, seed=0, iters=10, step=None, side="both", users=None):
        """evaluate.list_robustness: rows (mode, eps, cutoff, jaccard, rbo, overlap,
        coverage, gini, entropy, arp, aplt), how far each attack of robustness moves
        the top-k lists and what the attacked lists do to the items."""
        from .evaluate import list_robustness
        return list_robustness(self, dataset, triplets, eps_list, k=k, cutoffs=cutoffs, modes=modes, p=p, seed=seed,
                               iters=iters, step=step, side=side, users=users)

    def certified(self, plan, eps_list, side="user", cutoffs=None):
        """evaluate.certified: rows (side, eps, K, hr_lb, ndcg_lb, auc_lb), lower
        bounds under EVERY perturbation of that side within eps per row."""
        from .evaluate import certified
        return certified(self, plan, eps_list, side=side, cutoffs=cutoffs)

    def certified_radius(self, plan, k=None, side="user"):
        """evaluate.certified_radius: (eps [n, k], items [n, k]), per user the
        largest eps up to which the held-out item provably stays in the top 1..k
        and the items that break the certificate first."""
        from .evaluate import certified_radius
        return certified_radius(self, plan, k=k, side=side)


class MFGrid:
    """M MF models over one triplet stream: the sweep the reference runs as one
    job per (eps, reg_adv) point, trained by ops.grid_train in one call per epoch.

    grid: a list of dicts over GRID_KEYS (eps, reg_adv, lr, reg, adver, seed,
    adv_iters, adv_step); a key a dict leaves out takes the value of `args`
    (adv_iters 1, adv_step None where args has none).  adv_iters = K > 1 trains the
    member against a K-step projected-gradient attack (ops.grid_train).  The tables are
    [M, rows, d], member-major: slice m is an ordinary dense table, and
    member(m) is an MF whose tables are views of it, so evaluation, top-K,
    robustness, certificates, neighbours and checkpoints work on a member as on
    any MF.  Members are initialised as MF._create_variables does with that
    member's seed (equal seeds: equal tables)."""

    GRID_KEYS = ("eps", "reg_adv", "lr", "reg", "adver", "seed", "adv_iters", "adv_step")

    def __init__(self, num_users, num_items, args, grid, device=None, _init=True):
        import copy
        grid = [dict(g) for g in grid]
        if not 1 <= len(grid) <= ops.GRID_MAX_MODELS:
            raise ValueError(f"a grid has 1 to {ops.GRID_MAX_MODELS} members, got {len(grid)}")
        for g in grid:
            bad = set(g) - set(self.GRID_KEYS)
            if bad:
                raise ValueError(f"unknown grid keys {sorted(bad)}: a member varies {self.GRID_KEYS}")
        d = args.embed_size
        if d % 4 or not 4 <= d <= ops.GRID_MAX_DIM:
            raise ValueError(f"grid dim must be a multiple of 4 in [4, {ops.GRID_MAX_DIM}], got {d}")
        if getattr(args, "adv", "grad") != "grad" or getattr(args, "dns", 1) != 1:
            raise ValueError("a grid trains adv='grad' with dns=1 only")
        self.num_users, self.num_items, self.args = num_users, num_items, args
        self.grid = grid
        self.member_args = []
        for g in grid:
            a = copy.copy(args)
            if not hasattr(a, "adver"):
                a.adver = 1
            if not hasattr(a, "adv_iters"):
                a.adv_iters = 1
            if not hasattr(a, "adv_step"):
                a.adv_step = None
            for k, v in g.items():
                setattr(a, k, v)
            self.member_args.append(a)
        self.embedding_size = d
        self.num_user_rows, self.num_item_rows = num_users + 1, num_items + 1
        self._members = [None] * len(grid)
        self.built = False
        if _init:
            self.build_graph(device)

    def __len__(self):
        return len(self.grid)

    @staticmethod
    def product(eps=None, reg_adv=None, lr=None, seeds=None, adv_iters=None, adv_step=None):
        """The product of the given lists as grid dicts, in itertools.product order
        over (adv_iters, eps, reg_adv, lr, seed): adv_iters, when given, varies
        slowest, then eps, the seed fastest.  A list left out (None) is not a key of
        the dicts.  seeds: a list of seeds, or an int N for seeds 0..N-1.  adv_step:
        one step size for every member (not an axis; None: each member's default)."""
        import itertools
        if isinstance(seeds, int):
            seeds = list(range(seeds))
        axes = [(k, list(v)) for k, v in (("adv_iters", adv_iters), ("eps", eps), ("reg_adv", reg_adv), ("lr", lr),
                                          ("seed", seeds)) if v is not None]
        if any(not v for _, v in axes):
            raise ValueError("a grid axis is empty")
        grid = [dict(zip([k for k, _ in axes], vals)) for vals in itertools.product(*[v for _, v in axes])]
        if adv_step is not None:
            for g in grid:
                g["adv_step"] = adv_step
        return grid

    def _allocate(self, device):
        self.device = torch.device(device) if device is not None else default_device()
        M, d = len(self.grid), self.embedding_size
        self.embedding_P = torch.empty(M, self.num_user_rows, d, dtype=torch.float32, device=self.device)
        self.embedding_Q = torch.empty(M, self.num_item_rows, d, dtype=torch.float32, device=self.device)
        self.accumulator_P = torch.full_like(self.embedding_P, 0.1)
        self.accumulator_Q = torch.full_like(self.embedding_Q, 0.1)
        self.built = True

    def build_graph(self, device=None):
        self._allocate(device)
        drawn = {}
        for m, a in enumerate(self.member_args):
            seed = getattr(a, "seed", None)
            if seed is None or seed not in drawn:
                tmp = MF(self.num_users, self.num_items, a)
                tmp._create_variables(self.device)
                src = (tmp.embedding_P, tmp.embedding_Q)
                if seed is not None:
                    drawn[seed] = src
            else:
                src = drawn[seed]
            self.embedding_P[m].copy_(src[0])
            self.embedding_Q[m].copy_(src[1])
        return self

    @classmethod
    def from_model(cls, mf, grid, args=None):
        """Every member starts from one trained model's P and Q, with fresh Adagrad
        slots at 0.1: the reference's BPR -> APR switch, pre-train once, branch M ways.
        args: what a grid dict leaves out (default: the model's own values, with
        adver = 1)."""
        import copy
        if mf.twin:
            raise ValueError("a grid branches from an MF with num_users + 1 / num_items + 1 rows (twin=False)")
        ops.settle_tables()
        args = copy.copy(args) if args is not None else argparse_like(mf)
        if args.embed_size != mf.embedding_size:
            raise ValueError(f"args.embed_size {args.embed_size} is not the model's {mf.embedding_size}")
        args.adver = 1  # the branch is the APR phase unless a member says adver = 0
        g = cls(mf.num_users, mf.num_items, args, grid, _init=False)
        g._allocate(mf.device)
        g.embedding_P.copy_(mf.embedding_P.unsqueeze(0).expand_as(g.embedding_P))
        g.embedding_Q.copy_(mf.embedding_Q.unsqueeze(0).expand_as(g.embedding_Q))
        return g

    def hparams(self):
        """The members' StepHParams, in member order."""
        return [ops.StepHParams(lr=a.lr, eps=a.eps, reg=a.reg, reg_adv=a.reg_adv, adver=int(bool(a.adver)),
                                adv_iters=a.adv_iters, adv_step=a.adv_step)
                for a in self.member_args]

    def member(self, m):
        """Member m as an MF on views of slice m: it owns no table storage, and
        what the grid trains it sees (and the other way round)."""
        if self._members[m] is None:
            mf = MF(self.num_users, self.num_items, self.member_args[m])
            mf._create_placeholders()
            mf.device = self.device
            mf.num_user_rows, mf.num_item_rows = self.num_user_rows, self.num_item_rows
            mf.embedding_P, mf.embedding_Q = self.embedding_P[m], self.embedding_Q[m]
            mf.accumulator_P, mf.accumulator_Q = self.accumulator_P[m], self.accumulator_Q[m]
            mf.h = None
            mf._create_fetches()
            mf.delta_P = torch.zeros_like(mf.embedding_P)
            mf.delta_Q = torch.zeros_like(mf.embedding_Q)
            mf._adv_calls, mf._ctx, mf._pipe, mf._delta_feed = 0, None, None, None
            mf.built = True
            self._members[m] = mf
        return self._members[m]

    def train_epoch(self, user, item_pos, item_neg, batch_size, losses=False, check=True):
        """One ops.grid_train call over the triplets, on every member."""
        return ops.grid_train(self.embedding_P, self.embedding_Q, self.accumulator_P, self.accumulator_Q,
                              self.hparams(), user, item_pos, item_neg, batch_size, losses=losses, check=check)


def argparse_like(mf):
    """The constructor arguments of an MF, read back from it (MFGrid.from_model)."""
    import argparse
    return argparse.Namespace(embed_size=mf.embedding_size, lr=mf.learning_rate, reg=mf.reg, dns=mf.dns, adv=mf.adv,
                              eps=mf.eps, adver=mf.adver, reg_adv=mf.reg_adv, epochs=mf.epochs, seed=mf.seed,
                              adv_iters=mf.adv_iters, adv_step=mf.adv_step)


class Session:
    """Minimal ``tf.Session`` stand-in for the fetches the APR path uses."""

    def __init__(self, model: MF):
        self.model = model

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def run(self, fetches, feed_dict=None):
        m = self.model
        single = not isinstance(fetches, (list, tuple))
        fl = [fetches] if single else list(fetches)
        # variables are fetched by value, like TF returns their numpy arrays (utils.py:92)
        names = [f.name if isinstance(f, _Handle) else
                 ("embedding_P" if f is m.embedding_P else "embedding_Q" if f is m.embedding_Q else f)
                 if isinstance(f, torch.Tensor) else f for f in fl]
        fd = {k.name if isinstance(k, _Handle) else k: v for k, v in (feed_dict or {}).items()}
        u, i, j = fd.get("user_input"), fd.get("item_input_pos"), fd.get("item_input_neg")
        out = {}
        if any(isinstance(n, str) and n in ("update_P", "update_Q") for n in names):
            # build_graph always creates the adversarial ops (APR.py:197-202), so a BPR
            # graph runs them too: delta is computed, and its optimizer never reads it
            m.delta_update(u, i, j)
            out["update_P"] = out["update_Q"] = None
        if "optimizer" in names:
            m.optimizer_step(u, i, j)
            out["optimizer"] = None
        if any(isinstance(n, str) and n in ("loss", "output_neg") for n in names) or (
                "output" in names and j is not None):
            uu = ops._idx(u, "user_input", m.device)
            n = uu.numel()
            bl, bc, op, on = ops.bpr_forward(m.embedding_P, m.embedding_Q, uu, i, j, n, want_scores=True)
            out["loss"] = float(bl.cpu()[0])
            out["output"] = op.cpu().numpy().reshape(-1, 1)
            out["output_neg"] = on.cpu().numpy().reshape(-1, 1)
        elif "output" in names:
            out["output"] = m.scores(u, i)
        if "embedding_P" in names or "embedding_Q" in names:
            ops.settle_tables()
        if "embedding_P" in names:
            out["embedding_P"] = m.embedding_P.cpu().numpy()
        if "embedding_Q" in names:
            out["embedding_Q"] = m.embedding_Q.cpu().numpy()
        for k, n in enumerate(names):
            if isinstance(n, torch.Tensor):  # any other tensor: its value
                names[k] = "_t%d" % k
                out[names[k]] = n.detach().cpu().numpy()
        missing = [n for n in names if n not in out]
        if missing:
            raise NotImplementedError(f"fetch(es) {missing} not supported by the APR session")
        res = [out[n] for n in names]
        return res[0] if single else res
