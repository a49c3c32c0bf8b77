"""The score sweep shared by the ranking kernels (csrc/acf_sweep.h) at the edges
the feature tests miss: d = 4 (one partial K chunk), 36 (a full chunk plus 4) and
1024 (the maximum); 70 users (ragged against tiles of 8 and of 64); 300 of 320
item rows as candidates (ragged against windows of 128 and 256, rows past the
candidates present); exclusion lists that are unsorted, repeated, partly past the
candidates and empty for some users.

Table entries are integers in [-3, 3], so every score is an integer below 2^24:
exact in float whatever the order of the sum, and a numpy integer matmul is the
oracle with no tolerance."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U1, I1, NUM_CAND, N_USERS, K = 90, 320, 300, 70, 10
KERNELS = ("mfma", "valu")


@functools.lru_cache(maxsize=None)
def case(d):
    rng = np.random.default_rng(7000 + d)
    P = rng.integers(-3, 4, (U1, d))
    Q = rng.integers(-3, 4, (I1, d))
    users = rng.permutation(U1)[:N_USERS].astype(np.int32)
    scores = P[users] @ Q.T  # int64 [70, 320]
    cand = np.arange(NUM_CAND)

    def unique_top(s, keep):
        return (s[cand][keep] == s[cand][keep].max()).sum() == 1

    # users whose best candidate is unique with nothing excluded keep an empty list
    empty = [j for j in range(N_USERS) if unique_top(scores[j], np.ones(NUM_CAND, bool))][:6]
    assert len(empty) >= 3
    lists, keep = [], np.ones((N_USERS, NUM_CAND), bool)
    for j in range(N_USERS):
        if j in empty:
            lists.append(np.zeros(0, np.int32))
            continue
        ex = rng.integers(0, I1, 25)  # unsorted, some >= NUM_CAND
        ex = np.concatenate([ex, ex[:7]])  # repeated
        keep[j, ex[ex < NUM_CAND]] = False
        # a unique best candidate: the others that tie with it are excluded too
        tied = cand[keep[j] & (scores[j, :NUM_CAND] == scores[j, :NUM_CAND][keep[j]].max())]
        keep[j, tied[1:]] = False
        lists.append(rng.permutation(np.concatenate([ex, tied[1:]])).astype(np.int32))
    off = np.zeros(N_USERS + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate(lists).astype(np.int32)
    # the oracle's lists: (score desc, id asc) over the kept candidates
    top = np.stack([cand[keep[j]][np.lexsort((cand[keep[j]], -scores[j, :NUM_CAND][keep[j]]))][:K]
                    for j in range(N_USERS)]).astype(np.int32)
    tests = rng.integers(0, I1, N_USERS).astype(np.int32)  # any row: excluded ones and rows past the candidates too
    for a in (scores, keep, top):
        a.setflags(write=False)
    return P.astype(np.float32), Q.astype(np.float32), users, off, flat, scores, keep, top, tests


def positions(scores, keep, tests, count_self):
    """#(kept candidates scoring >= the test item), the item itself counted or not."""
    j = np.arange(len(tests))
    pos = (keep & (scores[:, :NUM_CAND] >= scores[j, tests][:, None])).sum(axis=1)
    if not count_self:
        own = tests < NUM_CAND
        pos[own] -= keep[j[own], tests[own]]
    return pos.astype(np.int32)


@pytest.mark.parametrize("d", [4, 36, 1024])
def test_shared_sweep_at_its_edges(ops, dev, d):
    P, Q, users, off, flat, scores, keep, top, tests = case(d)
    tP, tQ, tu = torch.tensor(P, device=dev), torch.tensor(Q, device=dev), torch.tensor(users, device=dev)
    one_each = np.arange(N_USERS + 1, dtype=np.int64)
    top1 = np.ascontiguousarray(top[:, 0])
    assert (positions(scores, keep, top1, count_self=False) == 0).all()  # the case is what it claims

    def multi(items):
        return ops.eval_positions_multi(tP, tQ, tu, one_each, items, NUM_CAND, off, flat).cpu().numpy()

    np.testing.assert_array_equal(multi(tests), positions(scores, keep, tests, count_self=False))
    np.testing.assert_array_equal(multi(top1), np.zeros(N_USERS, np.int32))
    for kernel in KERNELS:
        pos = ops.eval_positions_all(tP, tQ, tu, tests, NUM_CAND, off, flat, kernel=kernel).cpu().numpy()
        np.testing.assert_array_equal(pos, positions(scores, keep, tests, count_self=True), err_msg=kernel)
        items, sc = ops.recommend_topk(tP, tQ, tu, K, NUM_CAND, off, flat, kernel=kernel)
        np.testing.assert_array_equal(items.cpu().numpy(), top, err_msg=kernel)
        np.testing.assert_array_equal(sc.cpu().numpy(), np.take_along_axis(scores, top.astype(np.int64), axis=1),
                                      err_msg=kernel)
        # the top-1 item counts itself once and nothing else reaches it
        pos = ops.eval_positions_all(tP, tQ, tu, top1, NUM_CAND, off, flat, kernel=kernel).cpu().numpy()
        np.testing.assert_array_equal(pos - 1, np.zeros(N_USERS, np.int32), err_msg=kernel)
