"""All-items / sampled evaluation: ``init_eval_model``, ``evaluate``,
``_eval_by_user`` (``utils.py:178-267``).

Per user the reference builds a candidate list, scores it with one
``sess.run(model.output)`` and takes ``position = #(neg >= pos)``; HR@k, NDCG@k
and AUC for k = 1..K follow from the position alone.  Here the candidate sets are
kept implicit ("all": every item in ``[0, num_items)`` minus the user's
``trainList`` and test item) or explicit ("sample": the 100 draws of
``utils.py:201-209``, reproduced exactly with Python's ``random`` seeded 2019), one
kernel computes every user's position, and the metrics are vectorised on the host.
"""
from __future__ import annotations

import math
import random

import numpy as np

from . import ops


class EvalPlan:
    """What init_eval_model returns: device-ready candidate descriptions."""

    def __init__(self, mode, users, tests, n_neg, K, excl_off=None, excl=None, cand_off=None,
                 cand=None, num_candidates=0):
        self.mode, self.users, self.tests, self.n_neg, self.K = mode, users, tests, n_neg, K
        self.excl_off, self.excl, self.cand_off, self.cand = excl_off, excl, cand_off, cand
        self.num_candidates = num_candidates
        self._dev = {}

    def device_arrays(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            T = lambda a, dt: torch.as_tensor(a, dtype=dt, device=device)  # noqa: E731
            if self.mode == "all":
                self._dev[key] = (T(self.users, torch.int32), T(self.tests, torch.int32),
                                  T(self.excl_off, torch.int64),
                                  T(self.excl if len(self.excl) else np.zeros(1), torch.int32))
            else:
                self._dev[key] = (T(self.users, torch.int32), T(self.tests, torch.int32),
                                  T(self.cand_off, torch.int64),
                                  T(self.cand if len(self.cand) else np.zeros(1), torch.int32))
        return self._dev[key]


def _sample_candidates(dataset, user, test_item, candidates):
    """utils.py:201-209 verbatim: random.seed(2019) per user, 100 draws from the
    df.iid list, redrawn while in trainList[user] or equal to the test item."""
    random.seed(2019)
    tl = set(dataset.trainList[user])
    out = []
    for _ in range(100):
        r = random.choice(candidates)
        while r in tl or test_item == r:
            r = random.choice(candidates)
        out.append(r)
    return out


def init_eval_model(dataset, args, users=None, twin=False):
    """utils.py:178-195 (twin=True: evaluation_adv.py:406-437 — users 1..U-1,
    item 0 never a candidate, K = 100)."""
    mode = "all" if twin else getattr(args, "eval_mode", "sample")
    if users is None:
        users = np.arange(1 if twin else 0, dataset.num_users, dtype=np.int64)
    users = np.asarray(users, dtype=np.int64)
    tests = np.asarray([dataset.testRatings[u][1] for u in users], dtype=np.int64)
    K = 100 if mode == "all" else 10
    if mode == "all":
        off, items = dataset.sorted_lists()
        n = dataset.num_items
        excl_lists = []
        n_neg = np.empty(len(users), dtype=np.int64)
        for k, u in enumerate(users.tolist()):
            tl = items[off[u]:off[u + 1]] if u < len(off) - 1 else np.zeros(0, np.int32)
            ex = np.union1d(tl, [tests[k]])
            if twin:
                ex = np.union1d(ex, [0])
            ex = ex[(ex >= 0) & (ex < n)]
            excl_lists.append(ex.astype(np.int32))
            n_neg[k] = n - len(ex)
        eo = np.zeros(len(users) + 1, dtype=np.int64)
        np.cumsum([len(e) for e in excl_lists], out=eo[1:])
        ex = np.concatenate(excl_lists) if excl_lists else np.zeros(0, np.int32)
        return EvalPlan("all", users, tests, n_neg, K, excl_off=eo, excl=ex, num_candidates=n)
    candidates = dataset.df.iid.tolist()
    cl = [_sample_candidates(dataset, int(u), int(t), candidates) for u, t in zip(users, tests)]
    co = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cl], out=co[1:])
    cand = np.concatenate([np.asarray(c, np.int32) for c in cl]) if cl else np.zeros(0, np.int32)
    n_neg = np.diff(co)
    return EvalPlan("sample", users, tests, n_neg, K, cand_off=co, cand=cand)


def positions(P, Q, plan: EvalPlan, kernel: str = "auto"):
    """Per-user position (#candidates scoring >= the test item), on the GPU
    (kernel: the all-items sweep, ops.eval_positions_all)."""
    dev = P.device
    u, t, o, c = plan.device_arrays(dev)
    if plan.mode == "all":
        return ops.eval_positions_all(P, Q, u, t, plan.num_candidates, o, c, kernel=kernel, unique_lists=True)
    return ops.eval_positions_list(P, Q, u, t, o, c)


def train_exclusions(dataset, users):
    """Exclusion CSR (offsets int64 [n + 1], items int32) for recommendation
    lists: the sorted unique trainList[u] of every user in `users`, in that order
    (repeats allowed).  Train items only: the held-out test item stays
    recommendable.  A user without a train list gets an empty one.  Pure numpy."""
    soff, sitems = dataset.sorted_lists()
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    soff = np.append(np.asarray(soff, dtype=np.int64), soff[-1])  # one empty list past the end
    known = (users >= 0) & (users < len(soff) - 2)
    safe = np.where(known, users, len(soff) - 2)  # users without a trainList: the empty one
    lens = soff[safe + 1] - soff[safe]
    off = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    within = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], lens)
    items = np.asarray(sitems)[np.repeat(soff[safe], lens) + within].astype(np.int32)
    return off, items


def recommend(model_or_tables, dataset=None, users=None, k: int = 10, exclude_train: bool = True,
              kernel: str = "auto"):
    """The k best items per user from the model's tables, on the GPU
    (ops.recommend_topk): (items int32 [n, k], scores float32 [n, k]) as numpy
    arrays, -1 / -inf past a user's candidates.  model_or_tables: an MF (or
    anything with embedding_P / embedding_Q) or a (P, Q) pair of device tensors.
    users: default every user of the dataset.  Candidates are the dataset's items
    [0, num_items) (no dataset: every row of Q), minus the user's train items when
    exclude_train."""
    if hasattr(model_or_tables, "embedding_P"):
        P, Q = model_or_tables.embedding_P, model_or_tables.embedding_Q
    else:
        P, Q = model_or_tables[0], model_or_tables[1]
    if users is None:
        if dataset is None:
            raise ValueError("users=None needs a dataset")
        users = np.arange(dataset.num_users, dtype=np.int64)
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    num_candidates = min(int(dataset.num_items), Q.shape[0]) if dataset is not None else Q.shape[0]
    off = ex = None
    if exclude_train and dataset is not None:
        off, ex = train_exclusions(dataset, users)
    items, scores = ops.recommend_topk(P, Q, users.astype(np.int32), int(k), num_candidates, off, ex, kernel=kernel)
    return items.cpu().numpy(), scores.cpu().numpy()


def metrics_from_positions(pos, n_neg, K):
    """utils.py:256-261 for k = 1..K -> raw [U, 3, K] array of (hr, ndcg, auc)."""
    pos = np.asarray(pos, dtype=np.int64)
    ks = np.arange(1, K + 1)
    hit = pos[:, None] < ks[None, :]
    ndcg_val = np.array([math.log(2) / math.log(p + 2) for p in pos.tolist()], dtype=np.float64)
    ndcg = np.where(hit, ndcg_val[:, None], 0.0)
    auc = np.repeat((1 - (pos / np.asarray(n_neg, np.float64)))[:, None], K, axis=1)
    return np.stack([hit.astype(np.float64), ndcg, auc], axis=1)


def evaluate(model, sess, dataset, feed_dicts: EvalPlan, output_adv=0, args=None):
    """utils.py:221-241: returns ((hr, ndcg, auc) as per-K lists, raw [U,3,K]).
    output_adv=1 ranks with model.output_adv, (P + delta_P)[u] . (Q + delta_Q)[i]
    (APR.py:130-141): delta_P / delta_Q are what the last train.adv_update put
    there (zeros before any), not the last mini-batch's delta as in TF, because
    training here never materialises delta."""
    P, Q = model.embedding_P, model.embedding_Q
    if output_adv:
        P, Q = perturbed_tables(model)
    pos = positions(P, Q, feed_dicts).cpu().numpy()
    raw = metrics_from_positions(pos, feed_dicts.n_neg, feed_dicts.K)
    hr, ndcg, auc = raw.mean(axis=0).tolist()
    return (hr, ndcg, auc), raw


def perturbed_tables(model):
    """(P + delta_P, Q + delta_Q) of a model, each one rounded fp32 add
    (ops.adv_apply); the model's own tables are not written."""
    return (ops.adv_apply(model.embedding_P, model.delta_P, 1.0),
            ops.adv_apply(model.embedding_Q, model.delta_Q, 1.0))


def triplet_arrays(triplets):
    """(user, item_pos, item_neg) of what training_batch returns: an EpochTriplets
    (device tensors, passed through) or the lists (user_input, item_input_pos,
    [user_dns,] item_neg) of per-batch arrays, concatenated to int32 numpy."""
    if hasattr(triplets, "item_neg"):
        return triplets.user, triplets.item_pos, triplets.item_neg
    if len(triplets) not in (3, 4):
        raise ValueError("triplets must be an EpochTriplets or the lists training_batch returns")
    u, i, j = triplets[0], triplets[1], triplets[-1]
    cat = lambda xs: (np.concatenate([np.asarray(x).reshape(-1) for x in xs]).astype(np.int32)  # noqa: E731
                      if len(xs) else np.zeros(0, np.int32))
    return cat(u), cat(i), cat(j)


def _metrics_row(mode, eps, pos, plan):
    raw = metrics_from_positions(pos, plan.n_neg, plan.K)
    hr, ndcg, auc = raw.mean(axis=0)[:, -1].tolist() if len(pos) else (0.0, 0.0, 0.0)
    return (mode, eps, hr, ndcg, auc)


def robustness(model, dataset, plan: EvalPlan, triplets, eps_list, modes=("grad", "random"), seed=0, iters=10,
               step=None, side="both"):
    """HR@K, NDCG@K and AUC (K = plan.K) under a perturbation of both tables, per
    mode and eps: rows (mode, eps, hr, ndcg, auc).  "grad" / "random": one
    direction per mode over ALL the triplets as one batch (ops.adv_direction;
    "random": the draw of (seed, call 1, t 0)), then per eps one ops.adv_apply per
    table and one positions() on the perturbed tables.  "pgd": per eps > 0 one
    ops.adv_pgd from zeros (`iters` steps of size `step`, None: 2.5 * eps / iters,
    moving `side`), every eps on one shared ops.adv_plan, then positions() on
    (P + delta_P, Q + delta_Q); it needs at least one triplet.  eps = 0 reproduces
    evaluate(output_adv=0).  The model's tables and delta_P / delta_Q are left
    as they are."""
    return [_metrics_row(mode, eps, positions(Pa, Qa, plan).cpu().numpy(), plan)
            for mode, eps, Pa, Qa in attacked_tables(model, triplets, eps_list, modes, seed, iters, step, side)]


def attacked_tables(model, triplets, eps_list, modes=("grad", "random"), seed=0, iters=10, step=None, side="both"):
    """The attack loop robustness and list_robustness share: a generator of
    (mode, eps, P', Q') for every mode, then every eps, in that order; modes,
    directions and the "pgd" arguments as robustness describes them.  The
    arguments are checked when the generator is made, before anything runs; the
    model's tables are read, never written."""
    for mode in modes:
        if mode not in ops.ADV_MODES and mode != "pgd":
            raise ValueError(f"mode must be one of {sorted(ops.ADV_MODES) + ['pgd']}, got {mode!r}")
    eps_list = [float(e) for e in eps_list]
    if any(e < 0 for e in eps_list):
        raise ValueError("eps must be >= 0")
    pgd = "pgd" in modes
    if pgd:
        for e in eps_list:
            ops.pgd_arguments(e, iters, step, side)
    u, i, j = triplet_arrays(triplets)
    if pgd:
        if not len(u) == len(i) == len(j):
            raise ValueError("user, item_pos and item_neg must have equal lengths")
        if len(u) == 0:
            raise ValueError("the 'pgd' mode must be given at least one triplet: without a stream there is no "
                             "gradient to iterate on")
    P, Q = model.embedding_P, model.embedding_Q

    def tables():
        adv_plan = None
        for mode in modes:
            if mode == "pgd":
                if adv_plan is None:
                    adv_plan = ops.adv_plan(u, i, j, P.shape[0], Q.shape[0], device=P.device)
                for eps in eps_list:
                    Pa, Qa = P, Q
                    if eps > 0:
                        dP, dQ, _ = ops.adv_pgd(P, Q, u, i, j, eps, iters=iters, alpha=step, side=side,
                                                plan=adv_plan)
                        Pa, Qa = ops.adv_apply(P, dP, 1.0), ops.adv_apply(Q, dQ, 1.0)
                    yield mode, eps, Pa, Qa
                continue
            nP, nQ = ops.adv_direction(P, Q, u, i, j, adv=mode, seed=int(seed or 0), call=1, t=0)
            for eps in eps_list:
                yield mode, eps, ops.adv_apply(P, nP, eps), ops.adv_apply(Q, nQ, eps)
    return tables()


def item_popularity(dataset, head_share=0.2):
    """(pop int32 [num_items], tail bool [num_items]) from the train lists: pop[i]
    is the number of train interactions of item i; the head is the
    ceil(head_share * num_items) most popular items, ties going to the lower id,
    and tail marks the rest.  Pure numpy."""
    if not 0.0 <= float(head_share) <= 1.0:
        raise ValueError(f"head_share must lie in [0, 1], got {head_share!r}")
    n = int(dataset.num_items)
    _, items = dataset.sorted_lists()
    items = np.asarray(items, dtype=np.int64).reshape(-1)
    items = items[(items >= 0) & (items < n)]
    pop = np.bincount(items, minlength=n).astype(np.int32)
    head = int(math.ceil(float(head_share) * n))
    order = np.lexsort((np.arange(n), -pop.astype(np.int64)))  # popularity descending, then id ascending
    tail = np.ones(n, dtype=bool)
    tail[order[:head]] = False
    return pop, tail


def _tables_of(model_or_tables):
    if hasattr(model_or_tables, "embedding_P"):
        return model_or_tables.embedding_P, model_or_tables.embedding_Q
    return model_or_tables[0], model_or_tables[1]


def _list_cutoffs(cutoffs, k):
    cutoffs = [int(c) for c in cutoffs]
    if any(c > int(k) for c in cutoffs):
        raise ValueError(f"every cutoff must be <= k = {k}, got {cutoffs}")
    return cutoffs


class _ListSweep:
    """recommend_topk for a fixed set of users and exclusions, and the exposure
    metrics of such lists against a dataset's popularity, all on the device."""

    def __init__(self, P, dataset, users, k, cutoffs, exclude_train):
        import torch
        dev = P.device
        if users is None:
            users = np.arange(dataset.num_users, dtype=np.int64)
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        self.k, self.cutoffs, self.num_items = int(k), cutoffs, int(dataset.num_items)
        self.users = torch.as_tensor(users.astype(np.int32), device=dev)
        self.off = self.ex = None
        if exclude_train:
            off, ex = train_exclusions(dataset, users)
            self.off = torch.as_tensor(off, device=dev)
            self.ex = torch.as_tensor(ex if len(ex) else np.zeros(1, np.int32), device=dev)
        pop, tail = item_popularity(dataset)
        self.pop = torch.as_tensor(pop, device=dev)
        self.tail = torch.as_tensor(tail.astype(np.uint8), device=dev)

    def lists(self, P, Q):
        return ops.recommend_topk(P, Q, self.users, self.k, min(self.num_items, Q.shape[0]), self.off, self.ex)[0]

    def exposure(self, lists):
        """rows [n_cut][6] in ops.EXPOSURE_METRICS order, as Python floats"""
        counts = ops.list_exposure(lists, self.num_items, self.cutoffs)
        return ops.exposure_metrics(counts, self.pop, self.tail).cpu().tolist()


def exposure(model_or_tables, dataset, users=None, k=100, cutoffs=(10, 100), exclude_train=True):
    """What the model's own top-k lists do to the items: rows (cutoff, total,
    coverage, gini, entropy, arp, aplt), one per cutoff (ops.EXPOSURE_METRICS;
    arp and aplt against item_popularity(dataset)).  The lists stay on the device
    between ops.recommend_topk and the metrics.  users: default every user of
    the dataset; cutoffs above k are an error."""
    cutoffs = _list_cutoffs(cutoffs, k)
    P, Q = _tables_of(model_or_tables)
    sweep = _ListSweep(P, dataset, users, k, cutoffs, exclude_train)
    return [(c, *row) for c, row in zip(cutoffs, sweep.exposure(sweep.lists(P, Q)))]


def list_robustness(model, dataset, triplets, eps_list, k=100, cutoffs=(1, 10, 100), modes=("grad", "random"),
                    p=0.9, seed=0, iters=10, step=None, side="both", users=None):
    """How far an attack moves the top-k lists: rows (mode, eps, cutoff, jaccard,
    rbo, overlap, coverage, gini, entropy, arp, aplt).  One clean
    ops.recommend_topk (train items excluded) gives the rows ("clean", 0.0,
    cutoff, 1.0, 1.0, overlap, exposure...) first, overlap being the mean list
    length up to the cutoff; then, for every (mode, eps) of robustness' own attack
    loop (attacked_tables), one recommend_topk on the perturbed tables, one
    ops.list_compare against the clean lists (jaccard, rbo with persistence p and
    overlap are means over the users) and one ops.list_exposure +
    ops.exposure_metrics.  Cutoffs above k are an error.  The model's tables and
    delta_P / delta_Q are left as they are."""
    cutoffs = _list_cutoffs(cutoffs, k)
    attacks = attacked_tables(model, triplets, eps_list, modes, seed, iters, step, side)
    P, Q = model.embedding_P, model.embedding_Q
    sweep = _ListSweep(P, dataset, users, k, cutoffs, True)
    clean = sweep.lists(P, Q)

    def rows_of(mode, eps, lists):
        cmp = ops.list_compare(clean, lists, cutoffs, p).mean.cpu().tolist()  # [n_cut][overlap, jaccard, rbo]
        return [(mode, eps, c, m[1], m[2], m[0], *e[1:]) for c, m, e in zip(cutoffs, cmp, sweep.exposure(lists))]

    # a list against itself: jaccard and rbo are 1 by definition (the fp64 rbo sum is 1 to a few ulps)
    rows = [(*r[:3], 1.0, 1.0, *r[5:]) for r in rows_of("clean", 0.0, clean)]
    for mode, eps, Pa, Qa in attacks:
        rows += rows_of(mode, eps, sweep.lists(Pa, Qa))
    return rows


REL_NORMS = ("minmax", "none")


def normalise_relevance(items, scores, rel_norm="minmax"):
    """The relevances ops.rerank_mmr gets for a pool (items int32 [n, m], scores
    float32 [n, m] tensors, as ops.recommend_topk writes them), in torch on the
    pool's device.  'minmax': per row (s - min) / (max - min) over the valid
    entries (id >= 0), so that relevance and similarity share a scale; 0 where
    max = min (a constant row, a single valid entry) and at the entries that are
    not valid.  'none': the scores as they are."""
    import torch
    if rel_norm not in REL_NORMS:
        raise ValueError(f"rel_norm must be one of {REL_NORMS}, got {rel_norm!r}")
    if rel_norm == "none":
        return scores.contiguous()
    valid = items >= 0
    inf = torch.full_like(scores, float("inf"))
    lo = torch.where(valid, scores, inf).min(dim=1, keepdim=True).values
    hi = torch.where(valid, scores, -inf).max(dim=1, keepdim=True).values
    span = hi - lo
    ok = valid & (span > 0)
    rel = (scores - lo) / torch.where(span > 0, span, torch.ones_like(span))
    return torch.where(ok, rel, torch.zeros_like(rel)).contiguous()


def _pool_scores(pool_items, pool_scores, items):
    """The pool's scores of the re-ranked ids (a pool holds an id once): sort each
    pool row by id, search, gather; -inf at the -1 tail."""
    import torch
    sid, perm = pool_items.sort(dim=1)
    at = torch.searchsorted(sid, items.clamp(min=0).contiguous()).clamp(max=pool_items.shape[1] - 1)
    out = pool_scores.gather(1, perm.gather(1, at))
    return torch.where(items >= 0, out, torch.full_like(out, float("-inf")))


def _rerank(Q, pool_items, pool_scores, k, lam, metric, rel_norm):
    rel = normalise_relevance(pool_items, pool_scores, rel_norm)
    return ops.rerank_mmr(Q, pool_items, rel, int(k), float(lam), metric)[0]


def _check_pool(k, pool):
    if not 1 <= int(k) <= int(pool) <= ops.TOPK_MAX_K:
        raise ValueError(f"need 1 <= k <= pool <= {ops.TOPK_MAX_K}, got k = {k}, pool = {pool}")


def recommend_diverse(model_or_tables, dataset=None, users=None, k: int = 10, pool: int = 128, lam: float = 0.7,
                      metric: str = "cosine", rel_norm: str = "minmax", exclude_train: bool = True):
    """k diverse items per user: recommend's `pool` best items, re-ranked greedily
    by maximal marginal relevance on the GPU (ops.rerank_mmr): each pick maximises
    lam * relevance - (1 - lam) * the largest similarity to what is already picked,
    similarity being `metric` between rows of the item table.  rel_norm: 'minmax'
    scales a user's pool scores to [0, 1] first, 'none' uses them as they are.
    Returns (items int32 [n, k], scores float32 [n, k]) numpy arrays in the order
    picked, the scores the model's own; -1 / -inf past a user's candidates.
    lam = 1 is recommend(k)."""
    _check_pool(k, pool)
    if rel_norm not in REL_NORMS:
        raise ValueError(f"rel_norm must be one of {REL_NORMS}, got {rel_norm!r}")
    P, Q = _tables_of(model_or_tables)
    if users is None:
        if dataset is None:
            raise ValueError("users=None needs a dataset")
        users = np.arange(dataset.num_users, dtype=np.int64)
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    num_candidates = min(int(dataset.num_items), Q.shape[0]) if dataset is not None else Q.shape[0]
    off = ex = None
    if exclude_train and dataset is not None:
        off, ex = train_exclusions(dataset, users)
    pool_items, pool_scores = ops.recommend_topk(P, Q, users.astype(np.int32), int(pool), num_candidates, off, ex)
    items = _rerank(Q, pool_items, pool_scores, k, lam, metric, rel_norm)
    return items.cpu().numpy(), _pool_scores(pool_items, pool_scores, items).cpu().numpy()


def diversity(model_or_tables, dataset, users=None, k=100, cutoffs=(10, 100), metric="cosine", exclude_train=True):
    """How alike the items of the model's own top-k lists are: rows (cutoff, ils),
    ils the mean over the users of the intra-list similarity at that cutoff
    (ops.list_similarity: the mean `metric` over the pairs of a list's items).
    The lists stay on the device.  Cutoffs above k are an error."""
    cutoffs = _list_cutoffs(cutoffs, k)
    P, Q = _tables_of(model_or_tables)
    sweep = _ListSweep(P, dataset, users, k, cutoffs, exclude_train)
    _, means = ops.list_similarity(Q, sweep.lists(P, Q), cutoffs, metric)
    return list(zip(cutoffs, means.cpu().tolist()))


def _held_out_metrics(lists, tests, cutoffs):
    """[(hr, ndcg)] per cutoff of each row's held-out item in its list, on the
    device: the item's index p in the list gives 1 / log2(p + 2) when p < K."""
    import torch
    hit = lists == tests[:, None]
    found = hit.any(dim=1)
    p = torch.where(found, hit.to(torch.int32).argmax(dim=1), torch.full_like(tests, lists.shape[1])).to(torch.float64)
    gain = math.log(2) / torch.log(p + 2.0)
    n = max(1, lists.shape[0])
    return [(float((p < K).sum()) / n, float(torch.where(p < K, gain, torch.zeros_like(gain)).sum()) / n)
            for K in cutoffs]


def diversity_tradeoff(model_or_tables, dataset, lams=(1.0, 0.7, 0.5), k=10, pool=128, cutoffs=(10,),
                       metric="cosine", rel_norm="minmax", users=None):
    """What diversifying costs and buys: rows (lam, cutoff, hr, ndcg, ils, total,
    coverage, gini, entropy, arp, aplt), one per (lam, cutoff).  The pool (every
    user's `pool` best items, train items excluded) is computed once; per lam it is
    re-ranked to k items (ops.rerank_mmr) and the lists are held against the
    dataset's held-out item (hr, ndcg at the cutoff), against themselves
    (ops.list_similarity) and against the catalogue (ops.list_exposure +
    ops.exposure_metrics), all on the device.  lam = 1 is the plain top-k row."""
    import torch
    _check_pool(k, pool)
    cutoffs = _list_cutoffs(cutoffs, k)
    P, Q = _tables_of(model_or_tables)
    sweep = _ListSweep(P, dataset, users, pool, cutoffs, True)
    tests = torch.as_tensor(np.asarray([dataset.testRatings[int(u)][1] for u in sweep.users.cpu().tolist()],
                                       dtype=np.int32), device=P.device)
    pool_items, pool_scores = ops.recommend_topk(P, Q, sweep.users, sweep.k, min(sweep.num_items, Q.shape[0]),
                                                 sweep.off, sweep.ex)
    rows = []
    for lam in lams:
        lists = _rerank(Q, pool_items, pool_scores, k, lam, metric, rel_norm)
        ils = ops.list_similarity(Q, lists, cutoffs, metric)[1].cpu().tolist()
        rows += [(float(lam), c, hr, ndcg, s, *e) for c, (hr, ndcg), s, e in
                 zip(cutoffs, _held_out_metrics(lists, tests, cutoffs), ils, sweep.exposure(lists))]
    return rows


def pgd_host(P, Q, u, i, j, eps, iters=10, alpha=None, side="both", start=None, lo=-80.0, hi=1e8):
    """ops.adv_pgd restated in float64 numpy, the tests' yardstick: (delta_P,
    delta_Q, losses [iters + 1]).  Per iteration the clean BPR gradient of all the
    triplets at (P + delta_P, Q + delta_Q), summed per row and l2-normalised with the
    1e-12 floor; on every moving side v = delta + alpha * n, rows with |v| > eps
    scaled by eps / |v|.  start: None (zeros) or (delta_P0, delta_Q0), taken as given.
    alpha None: 2.5 * eps / iters."""
    eps, iters, alpha, _ = ops.pgd_arguments(eps, iters, alpha, side)
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    u, i, j = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (u, i, j))
    if not len(u) == len(i) == len(j):
        raise ValueError("user, item_pos and item_neg must have equal lengths")
    if start is None:
        dP, dQ = np.zeros_like(P), np.zeros_like(Q)
    else:
        dP, dQ = np.array(start[0], dtype=np.float64), np.array(start[1], dtype=np.float64)
        if dP.shape != P.shape or dQ.shape != Q.shape:
            raise ValueError("start must be (delta_P0, delta_Q0) with the tables' shapes")

    def grad(Pa, Qa):
        p, qi, qj = Pa[u], Qa[i], Qa[j]
        x = (p * qi).sum(1) - (p * qj).sum(1)
        g = -1.0 / (np.exp(np.clip(x, lo, hi)) + 1.0) * ((x >= lo) & (x <= hi))
        gP, gQ = np.zeros_like(Pa), np.zeros_like(Qa)
        np.add.at(gP, u, g[:, None] * qi)
        np.add.at(gP, u, -g[:, None] * qj)
        np.add.at(gQ, i, g[:, None] * p)
        np.add.at(gQ, j, -g[:, None] * p)
        unit = lambda t: t / np.sqrt(np.maximum((t * t).sum(1, keepdims=True), 1e-12))  # noqa: E731
        return unit(gP), unit(gQ), float(np.logaddexp(0.0, -np.clip(x, lo, hi)).sum())

    def step(delta, n):
        v = delta + alpha * n
        s = np.sqrt((v * v).sum(1, keepdims=True))
        return np.where(s <= eps, v, v * (eps / np.where(s > 0, s, 1.0)))

    losses = np.zeros(iters + 1)
    for k in range(iters):
        nP, nQ, losses[k] = grad(P + dP, Q + dQ)
        if side != "item":
            dP = step(dP, nP)
        if side != "user":
            dQ = step(dQ, nQ)
    losses[iters] = grad(P + dP, Q + dQ)[2]
    return dP, dQ, losses


# ---- certified robustness: worst-case positions under an eps attack -----------
CERT_SIDES = ("user", "item")


def worst_margins_host(P, Q, users, test_items, num_candidates, excl_lists, side="user"):
    """The pieces of the worst-case predicate in float64 numpy, [n, num_candidates]
    each: m (score(u,t) - score(u,c)), base (the threshold is eps * base: |q_t -
    q_c| for side "user", 2 |p| for "item") and cand (c is a candidate of the
    entry: not in its exclusion set, not t).  excl_lists: None or one iterable
    per entry; entries outside [0, num_candidates) are ignored."""
    if side not in CERT_SIDES:
        raise ValueError(f"side must be one of {CERT_SIDES}, got {side!r}")
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    tests = np.asarray(test_items, dtype=np.int64).reshape(-1)
    C = int(num_candidates)
    p, qt, qc = P[users], Q[tests], Q[:C]
    m = np.einsum("nd,nd->n", p, qt)[:, None] - p @ qc.T
    if side == "user":
        base = np.empty((len(users), C), dtype=np.float64)
        for r in range(len(users)):  # the difference form: identical rows give exactly 0
            base[r] = np.sqrt(((qt[r][None, :] - qc) ** 2).sum(axis=1))
    else:
        base = np.repeat(2.0 * np.sqrt((p * p).sum(1))[:, None], C, axis=1)
    cand = np.ones((len(users), C), dtype=bool)
    for r in range(len(users)):
        if excl_lists is not None:
            ex = np.asarray(list(excl_lists[r]), dtype=np.int64).reshape(-1)
            cand[r, ex[(ex >= 0) & (ex < C)]] = False
        if 0 <= tests[r] < C:
            cand[r, tests[r]] = False
    return m, base, cand


def worst_positions_host(P, Q, users, test_items, num_candidates, excl_lists, eps, side="user"):
    """ops.eval_positions_worst restated in float64 numpy, the tests' yardstick:
    int64 [len(eps), n], worst[e][r] = #{c in C_r, c != t : m_c <= eps_e *
    base_c} (worst_margins_host).  Candidate c can be brought to score >= t by a
    perturbation within the budget iff its inequality holds (Cauchy-Schwarz, with
    equality for delta along q_c - q_t; for the item side q_t and q_c move
    against each other along p), so no admissible perturbation puts more than
    worst candidates at or above t."""
    eps = [float(e) for e in eps]
    if any(not (math.isfinite(e) and e >= 0) for e in eps):
        raise ValueError("eps must be finite and >= 0")
    m, base, cand = worst_margins_host(P, Q, users, test_items, num_candidates, excl_lists, side)
    return np.stack([((m <= e * base) & cand).sum(axis=1) for e in eps]).astype(np.int64).reshape(len(eps), -1)


def certified(model_or_tables, plan: EvalPlan, eps_list, side="user", cutoffs=None):
    """Certified lower bounds of HR@K, NDCG@K and AUC under EVERY perturbation of
    one side within eps per row in L2 (side "user": the user rows; "item": every
    item row its own delta): rows (side, eps, K, hr_lb, ndcg_lb, auc_lb), for
    every eps in eps_list's order and every K of cutoffs (default plan.K).  The
    worst-case positions come from ops.eval_positions_worst on the plan's
    exclusions (all-items plans only; up to 8 eps share one candidate sweep), the
    metrics from ops.rank_metrics with one test item per user, both on the GPU.
    The metrics do not increase with the position, so at the worst-case position
    they bound every attack from below; evaluate.robustness, one particular
    attack, bounds from above.  eps = 0 reproduces evaluate()'s means."""
    import torch
    if plan.mode != "all":
        raise ValueError("certified needs an all-items plan (init_eval_model with eval_mode='all')")
    if side not in CERT_SIDES:
        raise ValueError(f"side must be one of {CERT_SIDES}, got {side!r}")
    eps_list = [float(e) for e in eps_list]
    if any(not (math.isfinite(e) and e >= 0) for e in eps_list):
        raise ValueError("eps must be finite and >= 0")
    cutoffs = (int(plan.K),) if cutoffs is None else tuple(int(k) for k in cutoffs)
    if hasattr(model_or_tables, "embedding_P"):
        P, Q = model_or_tables.embedding_P, model_or_tables.embedding_Q
    else:
        P, Q = model_or_tables[0], model_or_tables[1]
    u, t, eo, ex = plan.device_arrays(P.device)
    n = int(u.numel())
    one_each = torch.arange(n + 1, dtype=torch.int64, device=P.device)
    nn = torch.as_tensor(np.asarray(plan.n_neg), dtype=torch.int32, device=P.device)
    rows = []
    for a in range(0, len(eps_list), ops.WORST_MAX_EPS):
        chunk = eps_list[a:a + ops.WORST_MAX_EPS]
        worst = ops.eval_positions_worst(P, Q, u, t, int(plan.num_candidates), eo, ex, eps=chunk, side=side)
        for e, eps in enumerate(chunk):
            rm = ops.rank_metrics(worst[e], one_each, nn, cutoffs)
            mean_cut, mean_free = rm.mean_cut.cpu().numpy(), rm.mean_free.cpu().numpy()
            for c, K in enumerate(cutoffs):
                rows.append((side, eps, K, float(mean_cut[c, CUT_METRICS.index("hit")]),
                             float(mean_cut[c, CUT_METRICS.index("ndcg")]), float(mean_free[FREE_METRICS.index("auc")])))
    return rows


# ---- certified radius: the largest eps each user's top-K hit survives -----------
_F32_MAX = np.float32(np.finfo(np.float32).max)


def min_eps_f32(m, base, side="user", return_fallback=False):
    """Per element the smallest finite float32 e >= 0 with the fp32 predicate of
    ops.eval_positions_worst, m <= fl(e * base) (side "user") or m <= fl(fl(2 e) *
    base) ("item"), +inf where no finite e satisfies it: ops.eval_radius's
    per-candidate value restated in numpy float32 with the kernel's operations
    (the quotient, up to 4 steps over neighbouring floats, then a bisection on
    the bit pattern).  m and base broadcast; float32 out.  return_fallback: also
    the mask of the elements the 4 steps did not settle."""
    if side not in CERT_SIDES:
        raise ValueError(f"side must be one of {CERT_SIDES}, got {side!r}")
    m, base = np.broadcast_arrays(np.asarray(m, dtype=np.float32), np.asarray(base, dtype=np.float32))
    shape = m.shape
    m, base = np.ascontiguousarray(m).reshape(-1), np.ascontiguousarray(base).reshape(-1)
    two, half = np.float32(2.0), np.float32(0.5)

    def pred(e):
        return m <= (e * base if side == "user" else (two * e) * base)

    def nudge(e, by):  # the float whose bit pattern is by away
        return (e.view(np.int32) + np.int32(by)).view(np.float32)

    with np.errstate(all="ignore"):
        out = np.full(m.shape, np.inf, dtype=np.float32)
        zero = pred(np.zeros_like(m))
        out[zero] = 0.0
        todo = ~zero & pred(np.full_like(m, _F32_MAX))
        e = m / base if side == "user" else (m / base) * half
        e = np.where(e <= _F32_MAX, e, _F32_MAX).astype(np.float32)
        e = np.where(e > 0, e, np.uint32(1).view(np.float32)).astype(np.float32)  # the smallest denormal
        for _ in range(4):
            lo = nudge(e, -1)
            p = pred(e)
            hit = todo & p & ~pred(lo)
            out[hit] = e[hit]
            todo &= ~hit
            e = np.where(p, lo, nudge(e, 1))
        fallback = todo.copy()
        if todo.any():
            idx = np.flatnonzero(todo)
            lo = np.zeros(len(idx), dtype=np.uint32)
            hi = np.full(len(idx), _F32_MAX.view(np.uint32), dtype=np.uint32)
            m, base = m[idx], base[idx]  # pred is over these from here on
            while ((hi - lo) > 1).any():  # !pred(lo), pred(hi): at most 31 rounds
                wide = (hi - lo) > 1
                mid = lo + ((hi - lo) >> np.uint32(1))
                ok = pred(mid.view(np.float32))
                hi = np.where(wide & ok, mid, hi)
                lo = np.where(wide & ~ok, mid, lo)
            out[idx] = hi.view(np.float32)
    out = out.reshape(shape)
    return (out, fallback.reshape(shape)) if return_fallback else out


def _k_smallest(val, cand, k):
    """Per row the k smallest val over cand, ascending, ties to the lower column:
    (values [n, k] padded with +inf, columns int64 [n, k] padded with -1)."""
    n = val.shape[0]
    eps = np.full((n, k), np.inf, dtype=val.dtype)
    items = np.full((n, k), -1, dtype=np.int64)
    for r in range(n):
        cols = np.flatnonzero(cand[r])
        order = cols[np.argsort(val[r, cols], kind="stable")][:k]
        eps[r, :len(order)], items[r, :len(order)] = val[r, order], order
    return eps, items


def radius_host(P, Q, users, test_items, num_candidates, excl_lists, k, side="user"):
    """ops.eval_radius restated in float64 numpy from worst_margins_host: per
    candidate m / base clipped at 0 (+inf for m > 0 with base 0), per entry the k
    smallest ascending, ties to the lower id: (eps float64 [n, k] padded with
    +inf, items int64 [n, k] padded with -1)."""
    m, base, cand = worst_margins_host(P, Q, users, test_items, num_candidates, excl_lists, side)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(m <= 0, 0.0, m / base)
    return _k_smallest(e, cand, int(k))


def certified_radius(model_or_tables, plan: EvalPlan, k=None, side="user"):
    """The certified radius of every user of an all-items plan
    (ops.eval_radius on the plan's exclusions): (eps float32 [n, k], items int32
    [n, k]), device tensors, k = plan.K by default.  eps[r, j] is the largest
    budget up to which user r's held-out item provably stays in the top j + 1
    under every perturbation of the side's rows (strictly below it the item is
    certified; at it, it no longer is), items[r] the candidates that break the
    certificate first.  One sweep of the catalogue serves every cutoff <= k;
    radius_summary and radius_curve reduce eps."""
    if plan.mode != "all":
        raise ValueError("certified_radius needs an all-items plan (init_eval_model with eval_mode='all')")
    if side not in CERT_SIDES:
        raise ValueError(f"side must be one of {CERT_SIDES}, got {side!r}")
    k = int(plan.K) if k is None else k
    if hasattr(model_or_tables, "embedding_P"):
        P, Q = model_or_tables.embedding_P, model_or_tables.embedding_Q
    else:
        P, Q = model_or_tables[0], model_or_tables[1]
    u, t, eo, ex = plan.device_arrays(P.device)
    return ops.eval_radius(P, Q, u, t, int(plan.num_candidates), eo, ex, k=k, side=side)


RADIUS_QUANTILES = (0.10, 0.25, 0.50, 0.75, 0.90)


def _radius_column(eps, K):
    eps = np.asarray(eps)
    if eps.ndim != 2 or not 1 <= int(K) <= eps.shape[1]:
        raise ValueError(f"K must lie in [1, {eps.shape[1] if eps.ndim == 2 else 0}] of eps [n, k], got {K!r}")
    return eps[:, int(K) - 1].astype(np.float64)


def radius_summary(eps, cutoffs):
    """The distribution over users of the radius at every K of cutoffs: rows (K,
    the share of users already missed (radius 0), the share unbounded (+inf: no
    finite budget pushes the item out), the 10 / 25 / 50 / 75 / 90 % quantiles of
    the finite radii (nan without one)).  eps: certified_radius's [n, k] array."""
    rows = []
    for K in cutoffs:
        col = _radius_column(eps, K)
        n = max(len(col), 1)
        finite = col[np.isfinite(col)]
        qs = np.quantile(finite, RADIUS_QUANTILES) if len(finite) else np.full(len(RADIUS_QUANTILES), np.nan)
        rows.append((int(K), float((col == 0).sum() / n), float(np.isposinf(col).sum() / n), *[float(q) for q in qs]))
    return rows


def radius_curve(eps, K, eps_list):
    """hr_lb(e) = the share of users whose radius at K exceeds e, for every e of
    eps_list: certified(..., eps_list, cutoffs=(K,))'s hr_lb, since worst < K iff
    e < eps[:, K - 1]."""
    col = _radius_column(eps, K)
    return [float((col > float(e)).sum() / max(len(col), 1)) for e in eps_list]


# ---- fold-in: rows for users who were not in the training set -----------------
class _Folded:
    """A fold-in's result: keys, the CSR (offsets, list) of the sorted unique
    lists, the fitted rows, their Adagrad accumulators and the losses, in that
    order; a side names the CSR and the rows (_names)."""
    _names = ()

    def __init__(self, keys, off, first, rows, acc, loss):
        self.keys, self.acc, self.loss = keys, acc, loss
        for name, value in zip(self._names, (off, first, rows)):
            setattr(self, name, value)

    def __len__(self):
        return len(self.keys)


class FoldIn(_Folded):
    """What fold_in returns: keys (the dict's keys ascending, or 0..n-1 for a
    list of lists), the CSR (user_off int64 [n + 1], item_pos int32 [T], numpy)
    of the sorted unique lists, and the device tensors P [n, d], acc [n, d] (the
    fitted rows and their Adagrad accumulators) and loss [epochs, n]."""
    _names = ("user_off", "item_pos", "P")


def fold_lists(lists):
    """(keys, user_off int64 [n + 1], item_pos int32 [T]) of `lists`: a sequence
    of item lists (keys 0..n-1, in order) or a dict key -> items (keys
    ascending).  Each list is sorted and de-duplicated; an empty list stays an
    empty row.  Items must be integers >= 0.  Pure numpy."""
    if isinstance(lists, dict):
        keys = sorted(lists)
        rows = [lists[k] for k in keys]
    else:
        rows = list(lists)
        keys = list(range(len(rows)))
    out = []
    for k, row in zip(keys, rows):
        a = np.asarray(list(row) if not isinstance(row, np.ndarray) else row)
        if a.size == 0:
            out.append(np.zeros(0, np.int32))
            continue
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise ValueError(f"list of {k!r}: items must be a flat sequence of integers")
        if a.min() < 0 or a.max() >= 2 ** 31:
            raise ValueError(f"list of {k!r}: item outside [0, 2^31)")
        out.append(np.unique(a).astype(np.int32))
    off = np.zeros(len(out) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in out], out=off[1:])
    items = np.concatenate(out) if out else np.zeros(0, np.int32)
    return keys, off, items.astype(np.int32)


def _redraw(rng, neg, own, keys, num_items: int):
    """Redraw neg[k], uniform on [0, num_items), while own[k] * num_items + neg[k]
    is one of `keys` (sorted, not empty unless neg is): in place, one rng.randint
    per round over what is still refused (APR.py:76-77)."""
    todo = np.arange(len(neg))
    while len(todo):
        k = own[todo] * num_items + neg[todo]
        at = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        todo = todo[keys[at] == k]
        neg[todo] = rng.randint(num_items, size=len(todo))


def fold_negatives(user_off, item_pos, num_items: int, epochs: int, seed: int = 0):
    """item_neg int32 [epochs, T]: per positive and epoch one item uniform on
    [0, num_items), redrawn while it is in that user's own list (APR.py:76-77).
    Reproducible from `seed` (numpy RandomState).  A user whose list holds every
    item has no admissible negative: ValueError."""
    off = np.asarray(user_off, dtype=np.int64)
    items = np.asarray(item_pos, dtype=np.int64)
    num_items, epochs, T = int(num_items), int(epochs), len(items)
    if num_items <= 0:
        raise ValueError("num_items must be positive")
    if T and (items.min() < 0 or items.max() >= num_items):
        raise ValueError(f"a list holds an item outside [0, {num_items})")
    lens = np.diff(off)
    if (lens >= num_items).any():
        raise ValueError("a list holds every item: no admissible negative")
    owner = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    keys = owner * num_items + items  # ascending: owners ascend, lists are sorted
    rng = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    neg = rng.randint(num_items, size=epochs * T).astype(np.int64)
    _redraw(rng, neg, np.tile(owner, epochs), keys, num_items)
    return neg.astype(np.int32).reshape(epochs, T)


def _fold_hparams(m):
    """The default hparams of a fold-in.  A model's (anything with hparams())
    takes its lr, eps, reg, reg_adv and adver as they are: a plain BPR model
    (adver=0) folds in WITHOUT the adversarial term.  The rest is not carried
    over: the delta is always the gradient one (a model trained with adv="random"
    folds in with adv="grad", the only delta fold-in takes) and the clip bounds
    are the graph's constants (-80, 1e8).  Bare tables: StepHParams(adver=1)."""
    if not hasattr(m, "hparams"):
        return ops.StepHParams(adver=1)
    hp = m.hparams()
    return ops.StepHParams(lr=hp.lr, eps=hp.eps, reg=hp.reg, reg_adv=hp.reg_adv, adver=hp.adver)


def _fold_target(model_or_tables):
    """(Q, num_items, default hparams: _fold_hparams) of an MF-like model, a
    (P, Q) pair or Q."""
    m = model_or_tables
    if hasattr(m, "embedding_Q"):
        return m.embedding_Q, min(int(m.num_items), m.embedding_Q.shape[0]), _fold_hparams(m)
    Q = m[1] if isinstance(m, (tuple, list)) else m
    return Q, Q.shape[0], _fold_hparams(m)


def fold_in(model_or_tables, lists, epochs: int = 20, batch: int = 512, seed: int = 0, hp=None, init=None,
            num_items=None) -> FoldIn:
    """Fit a row to every NEW user's item list while the item table stays fixed
    (ops.fold_in_users): APR's own step, adversarial term included, so a
    folded-in user is regularised like a trained one.  model_or_tables: an MF (or
    anything with embedding_Q / num_items / hparams()), a (P, Q) pair or Q.
    lists: a sequence of item lists or a dict key -> items (see fold_lists).
    Negatives: fold_negatives(seed) over [0, num_items) (default: the model's
    num_items, or every row of Q).  hp: default the model's own lr, eps, reg,
    reg_adv and adver with the gradient delta -- so a BPR model (adver=0) folds
    in without the adversarial term; pass hp=StepHParams(adver=1, ...) to force
    it (tables: StepHParams(adver=1)).  init: None, a
    FoldIn, or (P [n, d], acc [n, d]) device tensors of an earlier fit of the
    same users, to continue when lists have grown."""
    Q, n_items, hp0 = _fold_target(model_or_tables)
    hp = hp0 if hp is None else hp
    n_items = int(n_items if num_items is None else num_items)
    if n_items > Q.shape[0]:
        raise ValueError("num_items exceeds item rows")
    keys, off, items = fold_lists(lists)
    neg = fold_negatives(off, items, n_items, epochs, seed)
    P0 = A0 = None
    if init is not None:
        P0, A0 = (init.P, init.acc) if isinstance(init, FoldIn) else init
    P, acc, loss = ops.fold_in_users(Q, off, items, neg, hp, int(epochs), int(batch), init=P0, acc_init=A0)
    return FoldIn(keys, off, items, P, acc, loss)


def recommend_new(model_or_tables, lists, k: int, **fold_args):
    """The k best items for every NEW user: fold_in(lists, **fold_args), then
    ops.recommend_topk on the folded rows with the user's own list excluded.
    (items int32 [n, k], scores float32 [n, k]) numpy arrays, rows in fold_lists'
    key order (a dict's keys ascending)."""
    import torch
    Q, n_items, _ = _fold_target(model_or_tables)
    n_items = int(fold_args.get("num_items") or n_items)
    f = fold_in(model_or_tables, lists, **fold_args)
    users = torch.arange(len(f), dtype=torch.int32, device=Q.device)
    items, scores = ops.recommend_topk(f.P, Q, users, int(k), n_items, excl_off=f.user_off, excl_items=f.item_pos)
    return items.cpu().numpy(), scores.cpu().numpy()


# ---- fold-in: rows for items that were not in the training set ----------------
class FoldInItems(_Folded):
    """What fold_in_items returns: keys (the dict's keys ascending, or 0..n-1 for
    a list of lists), the CSR (item_off int64 [n + 1], user_pos int32 [T], numpy)
    of the sorted unique user lists, and the device tensors Q [n, d], acc [n, d]
    (the fitted rows and their Adagrad accumulators) and loss [epochs, n]."""
    _names = ("item_off", "user_pos", "Q")


def fold_item_negatives(item_off, user_pos, num_items: int, epochs: int, seed: int = 0, excl_off=None, excl=None):
    """item_neg int32 [epochs, T] for ops.fold_in_items: per position and epoch one
    item uniform on [0, num_items).  With a train CSR of the existing users
    (excl_off int64 [U + 1] / excl: the items of user u are
    excl[excl_off[u]:excl_off[u+1]], what train_exclusions(dataset, arange(U))
    returns) a draw that is a train item of that position's user is redrawn
    (APR.py:76-77); without it the draws are plain uniform.  Reproducible from
    `seed` (numpy RandomState).  ValueError: a user outside the CSR (or negative),
    or a user whose train list holds every item."""
    off = np.asarray(item_off, dtype=np.int64)
    users = np.asarray(user_pos, dtype=np.int64).reshape(-1)
    num_items, epochs, T = int(num_items), int(epochs), len(users)
    if num_items <= 0:
        raise ValueError("num_items must be positive")
    if off.ndim != 1 or off.size < 1 or off[0] != 0 or off[-1] != T or (np.diff(off) < 0).any():
        raise ValueError("item_off must be a CSR offset array over user_pos")
    if T and users.min() < 0:
        raise ValueError("a list holds a user outside the user table (negative)")
    if (excl_off is None) != (excl is None):
        raise ValueError("excl_off and excl go together")
    rng = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    neg = rng.randint(num_items, size=epochs * T).astype(np.int64)
    if excl_off is None or T == 0:
        return neg.astype(np.int32).reshape(epochs, T)
    eo = np.asarray(excl_off, dtype=np.int64).reshape(-1)
    ex = np.asarray(excl, dtype=np.int64).reshape(-1)
    n_users = len(eo) - 1
    if users.max() >= n_users:
        raise ValueError(f"a list holds a user outside [0, {n_users}), the users of the train CSR")
    owner = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(eo))
    inside = (ex >= 0) & (ex < num_items)  # other entries can never be drawn
    keys = np.unique(owner[inside] * num_items + ex[inside])
    full = np.bincount(keys // num_items, minlength=n_users) >= num_items
    if full[users].any():
        raise ValueError("a user's train list holds every item: no admissible negative")
    if len(keys) == 0:
        return neg.astype(np.int32).reshape(epochs, T)
    _redraw(rng, neg, np.tile(users, epochs), keys, num_items)
    return neg.astype(np.int32).reshape(epochs, T)


def _fold_items_target(model_or_tables):
    """(P, Q, num_users, num_items, default hparams) of an MF-like model or a
    (P, Q) pair; the defaults are _fold_hparams'."""
    return (*_neighbor_tables(model_or_tables), _fold_hparams(model_or_tables))


def fold_in_items(model_or_tables, lists, epochs: int = 20, batch: int = 512, seed: int = 0, hp=None, init=None,
                  dataset=None) -> FoldInItems:
    """Fit a row to every NEW item's list of users while both tables stay fixed
    (ops.fold_in_items): APR's own step with the new item as the positive of
    every triplet.  model_or_tables: an MF (or anything with embedding_P /
    embedding_Q / num_users / num_items) or a (P, Q) pair.  lists: a sequence of
    user lists or a dict key -> users (sorted and de-duplicated by fold_lists);
    users must lie in [0, num_users).  Negatives: fold_item_negatives(seed) over
    [0, num_items); with a dataset, a draw among the train items of that
    position's user is rejected.  hp and init as in fold_in (init: a FoldInItems
    or (Q [n, d], acc [n, d]) of an earlier fit of the same items)."""
    P, Q, n_users, n_items, hp0 = _fold_items_target(model_or_tables)
    hp = hp0 if hp is None else hp
    keys, off, users = fold_lists(lists)
    if len(users) and users.max() >= n_users:
        raise ValueError(f"a list holds a user outside [0, {n_users})")
    eo = ex = None
    if dataset is not None:
        eo, ex = train_exclusions(dataset, np.arange(n_users, dtype=np.int64))
    neg = fold_item_negatives(off, users, n_items, epochs, seed, eo, ex)
    Q0 = A0 = None
    if init is not None:
        Q0, A0 = (init.Q, init.acc) if isinstance(init, FoldInItems) else init
    Qn, acc, loss = ops.fold_in_items(P, Q, off, users, neg, hp, int(epochs), int(batch), init=Q0, acc_init=A0)
    return FoldInItems(keys, off, users, Qn, acc, loss)


def audience_new(model_or_tables, lists, k: int, **fold_args):
    """The k best EXISTING users for every new item ("whom do I show it to?"):
    fold_in_items(lists, **fold_args), then ops.recommend_topk with the folded
    rows as queries over the user table, the item's own users excluded.
    (users int32 [n, k], scores float32 [n, k]) numpy arrays, rows in fold_lists'
    key order."""
    import torch
    P, _, n_users, _, _ = _fold_items_target(model_or_tables)
    f = fold_in_items(model_or_tables, lists, **fold_args)
    rows = torch.arange(len(f), dtype=torch.int32, device=P.device)
    users, scores = ops.recommend_topk(f.Q, P, rows, int(k), n_users, excl_off=f.item_off, excl_items=f.user_pos)
    return users.cpu().numpy(), scores.cpu().numpy()


def extend_items(model_or_tables, fold):
    """A tables namespace that holds the folded items as well: embedding_P,
    embedding_Q = the num_items real rows of Q followed by the folded rows
    (fold: a FoldInItems or a [n, d] tensor), num_users, num_items + n.  New item
    r has id num_items + r for evaluate.recommend, similar_items and
    evaluate_multi.  The model itself is not modified."""
    import types

    import torch
    P, Q, n_users, n_items, _ = _fold_items_target(model_or_tables)
    rows = fold.Q if isinstance(fold, FoldInItems) else fold
    return types.SimpleNamespace(embedding_P=P, embedding_Q=torch.cat([Q[:n_items], rows]).contiguous(),
                                 num_users=n_users, num_items=n_items + int(rows.shape[0]))


# ---- nearest neighbours: similar items, similar users -----------------------
def _neighbor_tables(model_or_tables):
    """(P, Q, num_users, num_items) of an MF-like model or a (P, Q) pair.  A
    model's tables carry one padding row past its users / items (APR.py:108,111:
    [U + 1, d] / [I + 1, d]), which the counts keep out of the candidates; a bare
    pair has no counts, so every row is a candidate unless the caller says
    otherwise."""
    m = model_or_tables
    if hasattr(m, "embedding_P"):
        P, Q = m.embedding_P, m.embedding_Q
        return P, Q, min(int(m.num_users), P.shape[0]), min(int(m.num_items), Q.shape[0])
    return m[0], m[1], m[0].shape[0], m[1].shape[0]


def similar_items(model_or_tables, items, k: int = 10, metric: str = "cosine", num_candidates=None, rows=None):
    """The k items most like each item of `items` (rows of the item table), on
    the GPU (ops.neighbors_topk): (ids int32 [n, k], scores float32 [n, k]) numpy
    arrays, best first, -1 / -inf past the candidates.  metric: 'cosine', 'dot'
    or 'euclid' (minus the squared distance).  An item is never its own
    neighbour, and the table's padding row (a model's row num_items) is never a
    candidate: the candidates are [0, num_candidates), default the model's
    num_items (a (P, Q) pair: every row of Q).  rows: a [m, d] device tensor of
    other rows, for example a FoldInItems' Q (or the FoldInItems itself); `items`
    then index `rows`, the candidates are still the model's items, and nothing is
    self-excluded (row j of `rows` is not item j)."""
    _, Q, _, n_items = _neighbor_tables(model_or_tables)
    n_items = int(n_items if num_candidates is None else num_candidates)
    items = np.asarray(items, dtype=np.int64).reshape(-1)
    X = rows.Q if isinstance(rows, FoldInItems) else rows
    ids, scores = ops.neighbors_topk(Q, items.astype(np.int32), int(k), metric, X=X, num_candidates=n_items,
                                     exclude_self=X is None)
    return ids.cpu().numpy(), scores.cpu().numpy()


def similar_users(model_or_tables, users, k: int = 10, metric: str = "cosine", rows=None):
    """The k users most like each user of `users` (rows of the user table), as
    similar_items: a user is never its own neighbour and the padding row (a
    model's row num_users) is never a candidate.  rows: a [m, d] device tensor
    of other rows, for example a FoldIn's P (or the FoldIn itself); `users` then
    index `rows`, the candidates are still the model's users, and nothing is
    self-excluded (row j of `rows` is not user j)."""
    P, _, n_users, _ = _neighbor_tables(model_or_tables)
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    X = rows.P if isinstance(rows, FoldIn) else rows
    ids, scores = ops.neighbors_topk(P, users.astype(np.int32), int(k), metric, X=X, num_candidates=int(n_users),
                                     exclude_self=X is None)
    return ids.cpu().numpy(), scores.cpu().numpy()


# ---- several held-out items per user ----------------------------------------
CUT_METRICS = ("hit", "recall", "precision", "ndcg", "map")  # ops.RANK_CUT_METRICS
FREE_METRICS = ("mrr", "auc")                                # ops.RANK_FREE_METRICS


def metrics_from_positions_multi(pos, test_off, n_neg, cutoffs):
    """Ranking metrics of the positions of several test items per user, in fp64
    on the host: the yardstick of ops.rank_metrics.  User u owns
    pos[test_off[u]:test_off[u+1]]; sorted ascending they are r_0 <= ... <=
    r_{m-1} (ties: the smaller index first).  Per cutoff K
      hit = [r_0 < K]      recall = #{r_j < K} / m      precision = #{r_j < K} / K
      ndcg = sum_{r_j<K} 1/log2(r_j + 2) / sum_{i<min(m,K)} 1/log2(i + 2)
      map = sum_{r_j<K} (j + 1)/(r_j + 1) / min(m, K)
    and mrr = 1/(r_0 + 1), auc = (1/m) sum_j (1 - (r_j - j)/n_neg[u]).  They
    assume that every test item is a candidate and that a list holds no item
    twice: then r_j - j is the number of non-test candidates ahead of item j and
    n_neg[u] the number of non-test candidates.  Returns a dict: per_user
    [n, n_cut, 5] (CUT_METRICS order), per_user_free [n, 2] (FREE_METRICS order),
    mean_cut [n_cut, 5] and mean_free [2] over the users with m > 0 (zeros when
    there is none), n_scored."""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1)
    off = np.asarray(test_off, dtype=np.int64).reshape(-1)
    nn = np.asarray(n_neg, dtype=np.float64).reshape(-1)
    ks = [int(k) for k in cutoffs]
    n = len(off) - 1
    per_user = np.zeros((n, len(ks), 5), dtype=np.float64)
    free = np.zeros((n, 2), dtype=np.float64)
    scored = np.zeros(n, dtype=bool)
    for u in range(n):
        r = np.sort(pos[off[u]:off[u + 1]], kind="stable").astype(np.float64)
        m = len(r)
        if m == 0:
            continue
        scored[u] = True
        j = np.arange(m, dtype=np.float64)
        free[u, 0] = 1.0 / (r[0] + 1.0)
        free[u, 1] = float(np.sum(1.0 - (r - j) / nn[u])) / m
        disc = 1.0 / np.log2(r + 2.0)
        prec = (j + 1.0) / (r + 1.0)
        for c, K in enumerate(ks):
            inside = r < K
            top = min(m, K)
            idcg = float(np.sum(1.0 / np.log2(np.arange(top, dtype=np.float64) + 2.0)))
            cnt = float(inside.sum())
            per_user[u, c] = (float(r[0] < K), cnt / m, cnt / K, float(disc[inside].sum()) / idcg,
                              float(prec[inside].sum()) / top)
    ns = int(scored.sum())
    mean_cut = per_user[scored].sum(axis=0) / ns if ns else np.zeros((len(ks), 5))
    mean_free = free[scored].sum(axis=0) / ns if ns else np.zeros(2)
    return {"per_user": per_user, "per_user_free": free, "mean_cut": mean_cut, "mean_free": mean_free,
            "n_scored": ns}


class MultiEvalPlan:
    """What init_eval_multi returns (numpy): users int64 [n]; the test lists as a
    CSR test_off int64 [n + 1] / test_items int32 (duplicates dropped, first
    occurrence kept); the exclusions excl_off / excl (sorted train items minus the
    user's test items); n_neg int32 [n], the candidates that are not test items;
    num_candidates."""

    def __init__(self, users, test_off, test_items, excl_off, excl, n_neg, num_candidates):
        self.users, self.test_off, self.test_items = users, test_off, test_items
        self.excl_off, self.excl, self.n_neg, self.num_candidates = excl_off, excl, n_neg, num_candidates
        self._dev = {}

    def device_arrays(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            T = lambda a, dt: torch.as_tensor(a, dtype=dt, device=device)  # noqa: E731
            self._dev[key] = (T(self.users, torch.int32), T(self.test_off, torch.int64),
                              T(self.test_items, torch.int32), T(self.excl_off, torch.int64),
                              T(self.excl, torch.int32), T(self.n_neg, torch.int32))
        return self._dev[key]


def init_eval_multi(dataset, test_lists, users=None) -> MultiEvalPlan:
    """The plan of an all-items evaluation against several held-out items per
    user.  test_lists: a dict user -> items (users: default its keys ascending) or
    a list of lists (users: default 0..n-1; with `users`, the list of users[k] is
    test_lists[k]).  A user missing from a dict has an empty list and is not
    scored.  Duplicates within a list are dropped, the first occurrence kept;
    items must lie in [0, dataset.num_items).  The candidates of a user are all
    items minus its sorted train items that are not test items, so every test
    item is a candidate; n_neg = the candidates that are not test items (>= 1:
    ValueError otherwise).  Pure numpy."""
    n_items = int(dataset.num_items)
    if isinstance(test_lists, dict):
        if users is None:
            users = sorted(test_lists)
        rows = [test_lists.get(int(u), ()) for u in users]
    else:
        rows = list(test_lists)
        if users is None:
            users = range(len(rows))
    users = np.asarray(list(users), dtype=np.int64).reshape(-1)
    if len(rows) != len(users):
        raise ValueError(f"{len(rows)} test lists for {len(users)} users")
    if len(users) and (users.min() < 0 or users.max() >= dataset.num_users):
        raise ValueError(f"a user is outside [0, {dataset.num_users})")
    soff, sitems = dataset.sorted_lists()
    tests, excls = [], []
    n_neg = np.zeros(len(users), dtype=np.int32)
    for k, (u, row) in enumerate(zip(users.tolist(), rows)):
        a = np.asarray(list(row) if not isinstance(row, np.ndarray) else row).reshape(-1)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"test list of user {u}: items must be integers")
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= n_items):
            raise ValueError(f"test list of user {u}: item outside [0, {n_items})")
        _, first = np.unique(a, return_index=True)
        t = a[np.sort(first)].astype(np.int32)
        tl = sitems[soff[u]:soff[u + 1]] if u < len(soff) - 1 else np.zeros(0, np.int32)
        ex = np.setdiff1d(tl[(tl >= 0) & (tl < n_items)], t).astype(np.int32)
        n_neg[k] = n_items - len(ex) - len(t)
        if n_neg[k] < 1:
            raise ValueError(f"user {u} has no candidate besides its test items")
        tests.append(t)
        excls.append(ex)
    to = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in tests], out=to[1:])
    eo = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in excls], out=eo[1:])
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)  # noqa: E731
    return MultiEvalPlan(users, to, cat(tests), eo, cat(excls), n_neg, n_items)


def metric_names(cutoffs):
    """The keys of evaluate_multi's dict, in the order of the .multi file."""
    return [f"{m}@{int(k)}" for k in cutoffs for m in CUT_METRICS] + list(FREE_METRICS) + ["n_users"]


def evaluate_multi(model_or_tables, plan: MultiEvalPlan, cutoffs=(10, 50, 100), raw: bool = False):
    """Recall / NDCG / MAP / precision / hit @K, MRR and AUC against the plan's
    test lists, positions and metrics both on the GPU (ops.eval_positions_multi:
    one candidate sweep per user; ops.rank_metrics): {"hit@10": ..., "recall@10":
    ..., ..., "mrr": ..., "auc": ..., "n_users": the users scored}, means over the
    users with a non-empty list.  raw=True: (that dict, {"positions",
    "per_user", "per_user_free"} as numpy arrays).  model_or_tables: an MF (or
    anything with embedding_P / embedding_Q) or a (P, Q) pair of device tensors."""
    if hasattr(model_or_tables, "embedding_P"):
        P, Q = model_or_tables.embedding_P, model_or_tables.embedding_Q
    else:
        P, Q = model_or_tables[0], model_or_tables[1]
    cutoffs = tuple(int(k) for k in cutoffs)
    u, to, t, eo, ex, nn = plan.device_arrays(P.device)
    pos = ops.eval_positions_multi(P, Q, u, to, t, int(plan.num_candidates), eo, ex)
    rm = ops.rank_metrics(pos, to, nn, cutoffs)
    mean_cut, mean_free = rm.mean_cut.cpu().numpy(), rm.mean_free.cpu().numpy()
    out = {}
    for c, k in enumerate(cutoffs):
        for q, name in enumerate(CUT_METRICS):
            out[f"{name}@{k}"] = float(mean_cut[c, q])
    for q, name in enumerate(FREE_METRICS):
        out[name] = float(mean_free[q])
    out["n_users"] = int(rm.n_scored.item())
    if raw:
        return out, {"positions": pos.cpu().numpy(), "per_user": rm.per_user.cpu().numpy(),
                     "per_user_free": rm.per_user_free.cpu().numpy()}
    return out
