"""Grid training (ops.grid_train / acf_apr_grid_train, csrc/acf_grid.hip) at the
shapes test_gpu_grid.py does not run, with that file's helpers and its bar
(rtol 1e-5 / atol 1e-6, rtol widened to the Higham bound 2 n u of the longest
row sum), fixtures from tests/ops_ref.py (checked without a GPU in
test_ops_ref_host.py):

  plan widths   B = 64 | 65, 100, 256 | 257 | 513, 1000, 1024: k_grid_plan<1>,
                <4>, <8>, <16> (test_gpu_grid.py launches <1> and <8> only),
                batch sizes that are no power of two (padding keys share a
                thread's items with real ones), and B = 1024, where term
                indices reach 4,095 and slots 3,071
  hot item      an item row of 600 terms in three partial sums of GRID_CHUNK =
                256 (+g terms, +g and -g mixed, -g terms), one of exactly 256
                and one of 257
  chunk length  GRID_CHUNK itself, bit for bit: a row whose 512 terms are two
                identical runs of 256 sums to exactly twice the row of one run
  last term     terms 1,023 / 2,047 / 3,071 / 4,095 on rows of their own
  many members  M = 64 = ACF_GRID_MAX_MODELS (k_grid_hp's 64-way copy); M = 65
  wide tables   70,000 x 70,000 rows: row keys beyond 2^16 and 2^17 (end_bit)
"""
import numpy as np
import pytest
import torch

import ops_ref as R
from apr_oracle import HParams
from test_gpu_grid import ATOL, HPS3, NAMES, _check_against_oracle, _gpu, _oracle_member, _rtol, _tables, _triplets

pytestmark = pytest.mark.gpu
ALL = NAMES + ("loss_clean", "loss_adv")
HPS2 = (HPS3[1], HPS3[2])  # an APR member with reg, a BPR member


def _t(x, dev):
    return torch.tensor(x, device=dev)


@pytest.mark.parametrize("B", R.GRID_B)
def test_every_plan_width(ops, oracle, dev, B):
    """Two batches of B at d = 16, M = 2, per member against the oracle, losses
    included; for B = 65, 256 and 1024 one call of two batches == two calls of
    one, bit for bit."""
    u, i, j = R.grid_width_triplets(B)
    P, Q = _tables(200 + B, 2, 16)
    one = _check_against_oracle(ops, oracle, dev, P, Q, u, i, j, B, HPS2)
    if B not in (65, 256, 1024):
        return
    hps = [ops.StepHParams(**h) for h in HPS2]
    two = _gpu(P, Q, dev)
    for t in range(2):
        s = slice(t * B, (t + 1) * B)
        ops.grid_train(*two, hps, _t(u[s], dev), _t(i[s], dev), _t(j[s], dev), B)
    torch.cuda.synchronize()
    for x, y, n in zip(one, two, NAMES):
        assert torch.equal(x, y), n


def test_hot_item_row_in_three_partial_sums(ops, oracle, dev):
    u, i, j = R.grid_hot_item_triplets()
    assert np.bincount(np.concatenate([i, j]))[3] == 600
    P, Q = _tables(41, 3, 16)
    _check_against_oracle(ops, oracle, dev, P, Q, u, i, j, 1024, HPS3)


def test_partial_sums_are_of_256_terms(ops, dev):
    """GRID_CHUNK is part of the bit contract.  R.grid_chunk_triplets: in batch A
    item 3's 512 terms are two identical runs of 256 (triplet 256 + t copies
    triplet t; every term reads the tables as they were before the batch), so
    partial sums of 256 give acc + acc = 2 G exactly; in batch B the second run
    goes to item 4 and the row's gradient is G.  One BPR member, reg 0,
    accumulators at 0: the item's Adagrad slot is fl((2 G)^2) in A and fl(G^2)
    in B, and A == 4 B bit for bit.  With partial sums of another length A's
    sum is no exact doubling (test_ops_ref_host.py shows it for 64, 128, 512
    and 1,024 on this fixture).  No kernel output serves as the reference."""
    P, Q = R.grid_chunk_tables()
    slots = []
    for u, i, j in R.grid_chunk_triplets():
        tabs = [_t(P, dev), _t(Q, dev), torch.zeros(P.shape, device=dev), torch.zeros(Q.shape, device=dev)]
        ops.grid_train(*tabs, [ops.StepHParams(adver=0, reg=0.0)], _t(u, dev), _t(i, dev), _t(j, dev), 1024)
        torch.cuda.synchronize()
        slots.append(tabs[3][0, R.CHUNK_ITEM].cpu().numpy())
    a, b = slots
    assert np.isfinite(a).all() and (b > 1e-30).all()
    assert np.array_equal(a.view(np.int32), (np.float32(4) * b).view(np.int32))


def test_last_term_index_on_rows_of_its_own(ops, oracle, dev):
    u, i, j = R.grid_last_term_triplets()
    P, Q = _tables(42, 3, 16)
    tabs = _check_against_oracle(ops, oracle, dev, P, Q, u, i, j, 1024, HPS3)
    # the three rows moved: their terms were not lost
    assert not torch.equal(tabs[0][:, int(u[-1])], _t(P[:, int(u[-1])], dev))
    for r in (int(i[-1]), int(j[-1])):
        assert not torch.equal(tabs[1][:, r], _t(Q[:, r], dev))


def test_sixty_four_members(ops, oracle, dev):
    """M = 64 distinct hyper-parameter sets at d = 8, B = 32, three batches:
    members 0, 31 and 63 against the oracle, member 63 == a call with M = 1 bit
    for bit; M = 65 is rejected with the tables untouched."""
    B, d = 32, 8
    hd = R.grid_hps64()
    hps = [ops.StepHParams(**h) for h in hd]
    P, Q = _tables(43, 64, d)
    u, i, j = _triplets(44, 3 * B)
    tu, ti, tj = (_t(x, dev) for x in (u, i, j))
    tabs = _gpu(P, Q, dev)
    lc, la = ops.grid_train(*tabs, hps, tu, ti, tj, B, losses=True)
    torch.cuda.synchronize()
    rtol = _rtol(u, i, j, B)
    for m in (0, 31, 63):
        want, lc_w, la_w = _oracle_member(oracle, P[m], Q[m], u, i, j, B, HParams(**hd[m]))
        for g, w, n in zip(tabs, want, NAMES):
            np.testing.assert_allclose(g[m].cpu().numpy(), w, rtol=rtol, atol=ATOL, err_msg=f"member {m} {n}")
        np.testing.assert_allclose(lc[m].cpu().numpy(), lc_w, rtol=rtol, atol=ATOL, err_msg=f"member {m} loss_clean")
        assert hd[m]["adver"] == 1
        np.testing.assert_allclose(la[m].cpu().numpy(), la_w, rtol=rtol, atol=ATOL, err_msg=f"member {m} loss_adv")
    single = _gpu(P[63:], Q[63:], dev)
    lc1, la1 = ops.grid_train(*single, hps[63:], tu, ti, tj, B, losses=True)
    for x, y, n in zip(single + [lc1, la1], tabs + [lc, la], ALL):
        assert torch.equal(x[0], y[63]), n
    P65, Q65 = _tables(45, 65, d)
    tabs = _gpu(P65, Q65, dev)
    before = [t.clone() for t in tabs]
    with pytest.raises(ValueError):
        ops.grid_train(*tabs, hps + [hps[0]], tu, ti, tj, B)
    torch.cuda.synchronize()
    for x, y in zip(tabs, before):
        assert torch.equal(x, y)


def test_tables_wider_than_two_to_the_sixteen(ops, oracle, dev):
    """70,000 x 70,000 rows at d = 4, one batch of 64 with rows 0, 65,535,
    65,536 and 69,999 on both sides: against the oracle (which touches the
    batch's rows only), and the rows outside the batch keep their bits."""
    u, i, j = R.grid_wide_triplets()
    P, Q = _tables(46, 1, 4, u1=R.WIDE_ROWS, i1=R.WIDE_ROWS)
    tabs = _check_against_oracle(ops, oracle, dev, P, Q, u, i, j, 64, [HPS3[1]])
    for rows, (W, A), start in ((np.unique(u), (tabs[0], tabs[2]), P), (np.unique(np.concatenate([i, j])),
                                                                      (tabs[1], tabs[3]), Q)):
        idle = np.setdiff1d(np.arange(R.WIDE_ROWS), rows)
        assert np.array_equal(W[0].cpu().numpy()[idle].view(np.int32), start[0][idle].view(np.int32))
        assert bool((A[0].cpu()[torch.tensor(idle)] == 0.1).all())
        moved = W[0].cpu().numpy()[rows] != start[0][rows]
        assert moved.any(axis=1).all()  # every row of the batch moved, the edge rows among them
