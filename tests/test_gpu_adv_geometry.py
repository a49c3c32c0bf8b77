"""ops.adv_direction at every row geometry, sort depth, chunk edge and tile edge.

The whole-stream adversarial direction (csrc/acf_adv.h, acf_adv_direction in
csrc/acf_rank.hip) is a coefficient kernel, a hand-written stable LSD radix sort
on 8-bit digits, an offsets / records pass, a chunk-sum kernel and a combine
kernel; the last two and k_adv_random are instantiated per (LPR, NV).
test_gpu_adv.py compares it with the oracle where d/4 is a power of two, with
at most 90 table rows (one radix pass), and with two long rows that are not
neighbours.  This file runs it on tiny problems at

  1. every dispatched geometry, padded ones included (D below);
  2. the same for random mode;
  3. R = U1 + I1 = 256 / 257 / 65,536 / 65,537: one, two and three radix passes;
  4. a stream and the same stream with its rows renumbered inside much larger
     tables: identical bits, whatever the sort depth and the neighbours;
  5. rows of exactly 255 .. 514 terms (0/1/2/3-chunk boundaries), neighbours in
     key order, at the start and at the very end of the item range;
  6. N = 4n a multiple of the sort tile, a partial tile whose real keys carry
     digit 255, and one stream above 2,097,152 triplets (k_adv_scan2 with two
     tile sums per thread);
  7. the error word for a bad user index.

The bar is the single-step bar of test_gpu_adv.py, rtol 1e-5 / atol 1e-6 on
delta = direction * 0.5 against the C oracle's apr_batch with the whole stream
as one batch, scaled by _few_step_scale's k: 1 where the fp32 oracle itself
holds that bar against the float64 restatement _delta64, else 4x its own
distance.  k is computed from the oracle and float64 alone and pinned in a CPU
test at the end of this file, beside a restatement of geometry() and
adv_layout() that proves the cases reach the branches they are here for.
"""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_adv as adv
from test_gpu_adv import ATOL, EPS, RTOL, _close, _delta64, _gpu_delta, _oracle_delta, _problem, _zero_bits
from test_gpu_step_geometry import DISPATCHED, _few_step_scale, _geometry

gpu = pytest.mark.gpu

D = [4, 12, 20, 48, 100, 132, 252, 260, 516, 768, 772, 1024]
D_RANDOM = [8] + D  # test_gpu_adv.py draws at d = 16 and 64 only: <2,1> (d = 8 alone) is added here
NS = (1, 63, 1000)
SORT_ROWS = ((128, 128), (128, 129), (40000, 25536), (40000, 25537))  # R = 256, 257, 65,536, 65,537
ITEM_TERMS = (255, 256, 257, 511, 512, 513)  # terms per planted item row: 1, 1, 2, 2, 2, 3 chunks
USER_TRIPLETS = (128, 129, 256, 257)         # triplets per planted user row: 256, 258, 512, 514 terms
BIG_N = 2_097_200

ADV_CHUNK, ADV_TILE, ADV_SCAN_TILE = 256, 2048, 1024  # csrc/acf_adv.h


def _layout(n, U1, I1):
    """adv_layout() of csrc/acf_adv.h and the `per` of k_adv_scan2."""
    N, R = 4 * n, U1 + I1
    ntiles = (N + ADV_TILE - 1) // ADV_TILE
    M = 256 * ntiles
    T = (M + ADV_SCAN_TILE - 1) // ADV_SCAN_TILE
    bits = 1
    while bits < 32 and (1 << bits) < R:
        bits += 1
    return dict(N=N, R=R, ntiles=ntiles, M=M, T=T, passes=(bits + 7) // 8, per=(T + 1023) // 1024)


def _terms(u, i, j, U1, I1):
    """Terms per user row and per item row."""
    return 2 * np.bincount(u, minlength=U1), np.bincount(i, minlength=I1) + np.bincount(j, minlength=I1)


# ---- the input families ----------------------------------------------------------
def _geometry_case(d, n):
    return _problem(d + n, 33, 29, d, n)


def _sort_case(U1, I1, d):
    P, Q, u, i, j = _problem(U1 + I1 + d, U1, I1, d, 5000)
    u[7], i[1234], j[4321] = U1 - 1, I1 - 1, I1 - 1  # the last key of either table, as both item branches
    return P, Q, u, i, j


def _planted_stream(rng, n_random, users, items, user_rows, item_rows):
    """n_random triplets over `users` x `items` (index arrays to draw from), then
    for every (row, t) of user_rows t triplets of that user, and for every
    (row, c) of item_rows c triplets holding that item once, alternately as the
    positive and as the negative; shuffled."""
    draw = lambda pool, k: pool[rng.integers(0, len(pool), k)]  # noqa: E731
    us, ps, ns = [draw(users, n_random)], [draw(items, n_random)], [draw(items, n_random)]
    for row, t in user_rows:
        us.append(np.full(t, row))
        ps.append(draw(items, t))
        ns.append(draw(items, t))
    for row, c in item_rows:
        pos = np.arange(c) % 2 == 0
        other = draw(items, c)
        us.append(draw(users, c))
        ps.append(np.where(pos, row, other))
        ns.append(np.where(pos, other, row))
    order = rng.permutation(sum(len(x) for x in us))
    return tuple(np.concatenate(x)[order].astype(np.int32) for x in (us, ps, ns))


CHUNK_VARIANTS = ("after", "front", "last")


def _chunk_case(d, variant):
    """600 x 700 rows, 6,000 random triplets over 500 users and 600 items.
    "after": item rows 600..605 with ITEM_TERMS terms, user rows 500..503 with
    USER_TRIPLETS triplets.  "front": the six item rows are 0..5 (the random
    items are 6..605) and the user rows 596..599, the last of P: ten long rows
    side by side in key order, the item ones from term offset 0 of the item
    range.  "last": one item row of 513 terms, the last of Q, behind 99 rows no
    triplet touches."""
    U1, I1 = 600, 700
    rng = np.random.default_rng(500 + d + CHUNK_VARIANTS.index(variant))
    P = (rng.standard_normal((U1, d)) * 0.3).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.3).astype(np.float32)
    items, u0, i0 = np.arange(600), 500, 600
    if variant == "front":
        items, u0, i0 = np.arange(6, 606), 596, 0
    item_rows = [(i0 + k, c) for k, c in enumerate(ITEM_TERMS)] if variant != "last" else [(I1 - 1, 513)]
    user_rows = [(u0 + k, t) for k, t in enumerate(USER_TRIPLETS)]
    u, i, j = _planted_stream(rng, 6000, np.arange(500), items, user_rows, item_rows)
    return P, Q, u, i, j, user_rows, item_rows


def _tile_case(n):
    P, Q, u, i, j = _problem(6 + n, 128, 128, 12, n)
    # key 255 = item 127: in the pos branch, and among the last four terms of the stream
    i[5], j[-3], j[-1] = 127, 127, 127
    return P, Q, u, i, j


def _big_case():
    return _problem(2097, 3000, 3000, 4, BIG_N)


_refs = {}


def _reference(oracle, key, make):
    """(inputs, the oracle's delta tables, the float64 ones, k) of a case, once."""
    if key not in _refs:
        P, Q, u, i, j = make()[:5]
        orc = _oracle_delta(oracle, P, Q, u, i, j)
        ref = _delta64(P, Q, u, i, j, EPS)
        k = _few_step_scale(orc, ref)
        for x in (P, Q, u, i, j) + tuple(orc) + tuple(ref):
            x.setflags(write=False)
        _refs[key] = ((P, Q, u, i, j), orc, ref, k)
    return _refs[key]


def _held(got, want, k, name):
    """|got - want| <= k (ATOL + RTOL |want|)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    dist = float((np.abs(got.astype(np.float64) - want) / (ATOL + RTOL * np.abs(want))).max())
    print(f"{name}: {dist:.3f} bars from the oracle (k = {k:.1f})")
    np.testing.assert_allclose(got, want, rtol=k * RTOL, atol=k * ATOL, err_msg=name)


def _rows(idx, dev):
    return torch.as_tensor(np.asarray(idx, dtype=np.int64), device=dev)


def _check_grad(ops, dev, case, tag):
    """Both delta tables within the bar, rows no triplet touches +0.0, every row
    with a gradient of unit norm.  Returns the direction tables."""
    (P, Q, u, i, j), orc, ref, k = case
    nP, nQ, dP, dQ = _gpu_delta(ops, dev, P, Q, u, i, j)
    _held(dP, orc[0], k, f"{tag} delta_P")
    _held(dQ, orc[1], k, f"{tag} delta_Q")
    for name, t, touched, w in (("P", nP, np.unique(u), ref[0]), ("Q", nQ, np.unique(np.concatenate([i, j])), ref[1])):
        free = np.setdiff1d(np.arange(t.shape[0]), touched)
        if free.size:
            assert _zero_bits(t[_rows(free, dev)]), f"untouched rows of n{name} must be +0.0"
        # a touched row whose terms cancel exactly (i == j) has no direction; every other one is a unit vector
        unit = touched[np.abs(np.linalg.norm(w[touched], axis=1) - EPS) < 1e-9]
        assert unit.size or len(u) == 1
        norms = np.linalg.norm(t[_rows(unit, dev)].cpu().numpy().astype(np.float64), axis=1)
        np.testing.assert_allclose(norms, 1.0, rtol=0, atol=1e-5, err_msg=f"norms of n{name}")
    return nP, nQ


# ---------------------------------------------------------------------------
# 1. every geometry
@gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", D)
def test_grad_direction_at_every_geometry(ops, oracle, dev, d, n):
    """test_grad_direction_matches_oracle at D: k_adv_chunks<LPR,NV> with idle
    lanes, whose zeros enter adv_normalize's dot_row."""
    _check_grad(ops, dev, _reference(oracle, ("geom", d, n), lambda: _geometry_case(d, n)), f"d={d} n={n}")


@gpu
@pytest.mark.parametrize("d", [12, 100, 772, 1024])
def test_torch_op_gives_the_same_bits_at_padded_geometries(ops, dev, d):
    acf_ops = importlib.import_module("adversarial-collaborative-filtering_amd.torch_ops").load()
    P, Q, u, i, j = _geometry_case(d, 1000)
    Pt, Qt, ut, it, jt = (adv._T(x, dev) for x in (P, Q, u, i, j))
    for kw in (dict(adv="grad"), dict(adv="random", seed=5, call=3, t=2)):
        a = ops.adv_direction(Pt, Qt, ut, it, jt, **kw)
        b = acf_ops.adv_direction(Pt, Qt, ut, it, jt, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), kw


# ---------------------------------------------------------------------------
# 2. random mode at every geometry
@gpu
@pytest.mark.parametrize("d", D_RANDOM)
def test_random_direction_at_every_geometry(ops, oracle, dev, d):
    """test_random_direction_matches_the_steps_draw at D: a padded lane that drew
    noise would change the row's norm."""
    U1, I1, B = 50, 40, 64
    P, Q, u, i, j = _problem(8 + d, U1, I1, d, B)
    j[::7] = i[::7]
    dP_w, dQ_w = _oracle_delta(oracle, P, Q, u, i, j, adv="random", seed=77, call=1, t=0)
    kw = dict(adv="random", seed=77, call=1, t=0)
    nP, nQ, dP, dQ = _gpu_delta(ops, dev, P, Q, u, i, j, **kw)
    ru, ri = np.unique(u), np.unique(np.concatenate([i, j]))
    _close(dP.cpu().numpy()[ru], dP_w[ru], "delta_P (touched rows)")
    _close(dQ.cpu().numpy()[ri], dQ_w[ri], "delta_Q (touched rows)")
    for name, t in (("P", dP), ("Q", dQ)):
        norms = np.linalg.norm(t.cpu().numpy().astype(np.float64), axis=1)
        np.testing.assert_allclose(norms, EPS, rtol=1e-5, err_msg=f"every row of delta_{name} has norm eps")
    again = _gpu_delta(ops, dev, P, Q, u, i, j, **kw)
    assert torch.equal(nP, again[0]) and torch.equal(nQ, again[1])
    other = _gpu_delta(ops, dev, P, Q, u, i, j, adv="random", seed=77, call=2, t=0)
    assert not torch.equal(nP, other[0]) and not torch.equal(nQ, other[1])


# ---------------------------------------------------------------------------
# 3. sort depth and the R boundaries
@gpu
@pytest.mark.parametrize("d", [4, 12])
@pytest.mark.parametrize("U1,I1", SORT_ROWS)
def test_sort_depth_matches_oracle(ops, oracle, dev, U1, I1, d):
    """One, two and three radix passes over ten tiles and three scan tiles, the
    last key of either table present.  From the second pass on "a row's terms lie
    together in ascending e" holds only while every pass is stable."""
    case = _reference(oracle, ("sort", U1, I1, d), lambda: _sort_case(U1, I1, d))
    (P, Q, u, i, j) = case[0]
    assert u.max() == U1 - 1 and i.max() == I1 - 1 and j.max() == I1 - 1
    _check_grad(ops, dev, case, f"R={U1 + I1} d={d}")


# ---------------------------------------------------------------------------
# 4. relabelling invariance, bit for bit
def _relabel_case():
    """128 x 128 rows, d = 20, n = 5,000: 1,926 random triplets over users 0..123
    and items 0..121, item rows 122..127 with ITEM_TERMS terms and user rows
    124..127 with USER_TRIPLETS triplets."""
    rng = np.random.default_rng(44)
    P = (rng.standard_normal((128, 20)) * 0.3).astype(np.float32)
    Q = (rng.standard_normal((128, 20)) * 0.3).astype(np.float32)
    u, i, j = _planted_stream(rng, 5000 - sum(ITEM_TERMS) - sum(USER_TRIPLETS), np.arange(124), np.arange(122),
                              [(124 + k, t) for k, t in enumerate(USER_TRIPLETS)],
                              [(122 + k, c) for k, c in enumerate(ITEM_TERMS)])
    return P, Q, u, i, j


# (rows of the large P, of the large Q, user map (a, b): u -> (a u + b) mod rows, item map)
RELABEL = {"three_passes": (40000, 30000, (7919, 97), (7907, 41)), "two_passes": (128, 129, (37, 5), (37, 11))}


def _relabel_maps(name):
    U1b, I1b, (au, bu), (ai, bi) = RELABEL[name]
    mu = ((np.arange(128, dtype=np.int64) * au + bu) % U1b).astype(np.int32)
    mi = ((np.arange(128, dtype=np.int64) * ai + bi) % I1b).astype(np.int32)
    return U1b, I1b, mu, mi


@gpu
@pytest.mark.parametrize("name", list(RELABEL))
def test_relabelled_rows_give_identical_bits(ops, dev, name):
    """A row's sum depends only on its own terms in ascending e, and chunks are
    cut relative to the row's first term, so renumbering the rows (here through
    a multiplicative map mod the table size, which changes every digit of every
    key and the order of the rows) cannot change one bit of a touched row.  Pins
    the stability of every radix pass, the offsets, the unit map and the
    workspace slots of long rows at once: no tolerance."""
    P, Q, u, i, j = _relabel_case()
    ut, it = _terms(u, i, j, 128, 128)
    assert ut.min() > 0 and it.min() > 0 and ut.max() == 514 and it.max() == 513
    U1b, I1b, mu, mi = _relabel_maps(name)
    assert len(np.unique(mu)) == 128 and len(np.unique(mi)) == 128 and mu.max() < U1b and mi.max() < I1b
    assert list(mu) != sorted(mu) and list(mi) != sorted(mi)  # the rows change their order too
    rng = np.random.default_rng(45)
    Pb = (rng.standard_normal((U1b, 20)) * 0.3).astype(np.float32)
    Qb = (rng.standard_normal((I1b, 20)) * 0.3).astype(np.float32)
    Pb[mu], Qb[mi] = P, Q
    nP, nQ, _, _ = _gpu_delta(ops, dev, P, Q, u, i, j)
    bP, bQ, _, _ = _gpu_delta(ops, dev, Pb, Qb, mu[u], mi[i], mi[j])
    for t in (nP, nQ):  # every row of the small tables is touched and has a direction
        assert bool(torch.isfinite(t).all()) and float(torch.linalg.vector_norm(t, dim=1).min()) > 0.99
    for tag, small, big, m, rows in (("P", nP, bP, mu, U1b), ("Q", nQ, bQ, mi, I1b)):
        same = (small.view(torch.int32) == big[_rows(m, dev)].view(torch.int32)).all(dim=1).cpu().numpy()
        assert same.all(), f"n{tag}: rows {np.flatnonzero(~same).tolist()} differ after relabelling"
        free = np.setdiff1d(np.arange(rows), m)
        if free.size:
            assert _zero_bits(big[_rows(free, dev)]), f"untouched rows of the large n{tag} must be +0.0"


# ---------------------------------------------------------------------------
# 5. chunk boundaries, long rows side by side
@gpu
@pytest.mark.parametrize("variant", CHUNK_VARIANTS)
@pytest.mark.parametrize("d", [20, 64])
def test_chunk_boundaries_match_oracle(ops, oracle, dev, d, variant):
    """Rows of exactly 255, 256, 257, 511, 512, 513 (item) and 256, 258, 512, 514
    (user) terms: the nch = 1 / 2 / 3 boundaries between "normalise now" and
    "write the chunk sum to the workspace", in rows that are neighbours in key
    order, so that the slot formula and the unit map are what keeps their chunk
    sums apart."""
    case = _reference(oracle, ("chunk", d, variant), lambda: _chunk_case(d, variant))
    P, Q, u, i, j = case[0]
    _, _, _, _, _, user_rows, item_rows = _chunk_case(d, variant)
    ut, it = _terms(u, i, j, 600, 700)
    assert [int(ut[r]) for r, _ in user_rows] == [256, 258, 512, 514]
    assert [int(it[r]) for r, _ in item_rows] == ([513] if variant == "last" else list(ITEM_TERMS))
    if variant == "last":
        assert item_rows[0][0] == 699 and it[600:699].max() == 0 and it[:600].min() > 0
    if variant == "front":  # ten long rows and nothing between them
        assert [r for r, _ in user_rows] == [596, 597, 598, 599] and [r for r, _ in item_rows] == [0, 1, 2, 3, 4, 5]
    _check_grad(ops, dev, case, f"d={d} {variant}")


# ---------------------------------------------------------------------------
# 6. tile and scan edges
@gpu
@pytest.mark.parametrize("n", [512, 513, 1024])
def test_tile_edges_match_oracle(ops, oracle, dev, n):
    """N = 4n = 2,048 (one full tile), 2,052 (a tile and four terms) and 4,096.
    Key 255 (item 127) is among the last four terms, so at n = 513 the padded
    tile holds real keys of digit 255, the digit of k_adv_reorder's padding."""
    case = _reference(oracle, ("tile", n), lambda: _tile_case(n))
    j = case[0][4]
    assert 127 in j[-4:] and 127 in case[0][3]
    _check_grad(ops, dev, case, f"n={n}")


def _row_errors(got, orc, ref):
    e_got = np.linalg.norm(got.astype(np.float64) - ref, axis=1)
    e_orc = np.linalg.norm(orc.astype(np.float64) - ref, axis=1)
    return e_got, e_orc


@gpu
def test_two_tile_sums_per_scan_thread(ops, oracle, dev):
    """n = 2,097,200 triplets on 3,000 x 3,000 rows, d = 4: 4,097 sort tiles,
    1,025 scan tiles, so k_adv_scan2 adds two tile sums per thread (below
    2,097,153 triplets that loop runs once); two radix passes; rows of 1,120
    to 1,576 terms, five to seven chunks.  The fp32 oracle is 0.6 bars from float64 here, so
    the per-row convention of test_hot_rows_within_the_oracles_own_error holds:
    GPU L2 error against float64 <= 4x the oracle's + 1e-6, every row."""
    (P, Q, u, i, j), orc, ref, _ = _reference(oracle, ("big",), _big_case)
    assert _layout(BIG_N, 3000, 3000)["per"] == 2
    bars = max(float((np.abs(o.astype(np.float64) - w) / (ATOL + RTOL * np.abs(w))).max()) for o, w in zip(orc, ref))
    print(f"n = {BIG_N}: the oracle is {bars:.3f} bars from float64")
    nP, nQ, dP, dQ = _gpu_delta(ops, dev, P, Q, u, i, j)
    for name, got, o, w in (("P", dP, orc[0], ref[0]), ("Q", dQ, orc[1], ref[1])):
        e_gpu, e_orc = _row_errors(got.cpu().numpy(), o, w)
        assert len(e_gpu) == 3000
        print(f"n = {BIG_N}, delta_{name}: worst GPU error {e_gpu.max():.3e}, worst oracle error {e_orc.max():.3e}")
        bad = np.flatnonzero(e_gpu > 4 * e_orc + 1e-6)
        assert bad.size == 0, f"delta_{name} rows {bad.tolist()}: GPU {e_gpu[bad]} vs oracle {e_orc[bad]}"


# ---------------------------------------------------------------------------
# 7. the error word
@gpu
def test_bad_user_index_is_named_and_the_next_call_is_clean(ops, dev):
    native = importlib.import_module("adversarial-collaborative-filtering_amd._native")
    P, Q, u, i, j = _problem(1, 33, 29, 16, 100)
    Pt, Qt = adv._T(P, dev), adv._T(Q, dev)

    def run(*triplets):
        return ops.adv_direction(Pt, Qt, *(adv._T(x, dev) for x in triplets), check=True)
    before = run(u, i, j)
    for bad in (-1, 33):
        ub = u.copy()
        ub[40] = bad
        with pytest.raises(native.NativeIndexError, match="user >=") as e:
            run(ub, i, j)
        assert "item >=" not in str(e.value)
    ub, jb = u.copy(), j.copy()
    ub[3], jb[77] = 33, -1
    with pytest.raises(native.NativeIndexError, match="user >=.*item >="):
        run(ub, i, jb)
    after = run(u, i, j)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


# ---------------------------------------------------------------------------
# CPU guards
def test_dims_cover_the_dispatch_table():
    """geometry() restated: D and test_gpu_adv.py's dims reach all ten
    instantiations of DISPATCH_GEOM, in both modes; every lane width from 4 on
    and every NV appears with idle lanes."""
    def dims(test):
        return next(list(m.args[1]) for m in test.pytestmark if m.name == "parametrize" and m.args[0] == "d")
    assert {_geometry(d) for d in range(4, 1025, 4)} == DISPATCHED
    assert dims(test_grad_direction_at_every_geometry) == D
    assert {_geometry(d) for d in D + dims(adv.test_grad_direction_matches_oracle)} == DISPATCHED
    assert {_geometry(d) for d in D} == DISPATCHED - {(2, 1)}  # d = 8 alone, test_gpu_adv.py's
    assert dims(test_random_direction_at_every_geometry) == D_RANDOM
    assert {_geometry(d) for d in D_RANDOM} == DISPATCHED
    padded = [d for d in D if d // 4 < _geometry(d)[0] * _geometry(d)[1]]
    assert padded == [12, 20, 48, 100, 132, 252, 260, 516, 772]
    assert {_geometry(d) for d in padded} == {(4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4)}
    assert {_geometry(d) for d in D if d not in padded} == {(1, 1), (64, 3), (64, 4)}


def test_cases_reach_every_sort_and_scan_branch():
    """adv_layout() restated.  The cases of this file give one, two and three
    radix passes on either side of both boundaries, more than one scan tile, two
    tile sums per k_adv_scan2 thread, a full last tile and a partial one."""
    assert _layout(1000, 6041, 3707) == dict(N=4000, R=9748, ntiles=2, M=512, T=1, passes=2, per=1)
    assert [_layout(5000, U1, I1)["passes"] for U1, I1 in SORT_ROWS] == [1, 2, 2, 3]
    assert [U1 + I1 for U1, I1 in SORT_ROWS] == [256, 257, 65536, 65537]
    L = _layout(5000, 128, 128)
    assert (L["N"], L["ntiles"], L["T"], L["per"]) == (20000, 10, 3, 1)
    assert all(_layout(n, 33, 29)["passes"] == 1 for n in NS) and _layout(9074, 600, 700)["passes"] == 2
    assert [_layout(5000, *RELABEL[k][:2])["passes"] for k in ("three_passes", "two_passes")] == [3, 2]
    assert _layout(5000, 128, 128)["passes"] == 1  # the relabelled stream's own tables
    full = [_layout(n, 128, 128)["N"] % ADV_TILE for n in (512, 513, 1024)]
    assert full == [0, 4, 0] and [_layout(n, 128, 128)["ntiles"] for n in (512, 513, 1024)] == [1, 2, 2]
    B = _layout(BIG_N, 3000, 3000)
    assert (B["ntiles"], B["T"], B["per"], B["passes"]) == (4097, 1025, 2, 2)
    assert _layout(BIG_N - 48, 3000, 3000)["per"] == 1 and _layout(BIG_N - 47, 3000, 3000)["per"] == 2
    assert 4 * BIG_N // 6000 // ADV_CHUNK + 1 == 6  # chunks of an average row
    # the planted rows sit on the chunk-count boundaries
    chunks = lambda t: -(-t // ADV_CHUNK)  # noqa: E731
    assert [chunks(t) for t in ITEM_TERMS] == [1, 1, 2, 2, 2, 3]
    assert [chunks(2 * t) for t in USER_TRIPLETS] == [1, 2, 2, 3]
    for d in (20, 64):
        for v in CHUNK_VARIANTS:
            P, Q, u, i, j, user_rows, item_rows = _chunk_case(d, v)
            ut, it = _terms(u, i, j, 600, 700)
            assert all(ut[r] == 2 * t for r, t in user_rows) and all(it[r] == c for r, c in item_rows)
            assert len(u) == 6000 + sum(t for _, t in user_rows) + sum(c for _, c in item_rows)


def test_bars_come_from_the_oracle_alone(oracle):
    """k of every oracle-compared family, from the fp32 oracle and float64 alone:
    the oracle holds the project's bar in each, so k = 1 throughout.  The largest
    distance per family is printed (run with -s)."""
    families = {
        "geometry": [(("geom", d, n), lambda d=d, n=n: _geometry_case(d, n)) for d in D for n in NS],
        "sort": [(("sort", U1, I1, d), lambda U1=U1, I1=I1, d=d: _sort_case(U1, I1, d))
                 for U1, I1 in SORT_ROWS for d in (4, 12)],
        "chunk": [(("chunk", d, v), lambda d=d, v=v: _chunk_case(d, v)) for d in (20, 64) for v in CHUNK_VARIANTS],
        "tile": [(("tile", n), lambda n=n: _tile_case(n)) for n in (512, 513, 1024)],
    }
    for name, cases in families.items():
        worst = 0.0
        for key, make in cases:
            _, orc, ref, k = _reference(oracle, key, make)
            worst = max(worst, max(float((np.abs(o.astype(np.float64) - w) / (ATOL + RTOL * np.abs(w))).max())
                                   for o, w in zip(orc, ref)))
            assert k == 1.0, (key, k)
        print(f"{name}: the oracle is at most {worst:.3f} bars from float64")
        assert worst <= 1.0


def test_a_zeroed_row_fails_the_bar(oracle):
    """The checks of this file notice a row that was never written."""
    for key, make, table, row in ((("geom", 12, 63), lambda: _geometry_case(12, 63), 0, None),
                                  (("chunk", 20, "after"), lambda: _chunk_case(20, "after"), 1, 605)):
        (P, Q, u, i, j), orc, ref, k = _reference(oracle, key, make)
        got = orc[table].copy()
        _held(got, orc[table], k, "the oracle against itself")
        row = int(u[0]) if row is None else row
        assert np.linalg.norm(got[row]) > 0.4
        got[row] = 0.0
        with pytest.raises(AssertionError):
            _held(got, orc[table], k, "one row zeroed")
    # the per-row convention of the large case
    e_got, e_orc = _row_errors(np.zeros((1, 4), np.float32), np.full((1, 4), 0.25, np.float32) * (1 + 1e-6),
                               np.full((1, 4), 0.25))
    assert e_got[0] > 4 * e_orc[0] + 1e-6
