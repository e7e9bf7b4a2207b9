"""CPU checks of the radix-sort case builders (sort_cases.py): the sizes sit on
the seams of the sort's two tilings as radix_sort.h states them, every order
and wave pattern has the shape it claims, every key map is injective, stays
off KEY_RESERVED and varies in the bits it claims, the engines' Python replays
decide a mapped batch as the unmapped one, and the large engine cases lie above
the tile threshold with a partial last tile and yield every outcome the GPU
test (test_gpu_sort_paths.py) claims to cover."""
import numpy as np
import pytest

import _oracle as orc
import locktab_ref
import mvcc_ref
import nowait_ref
import sort_cases as sc
import tso_ref
import waitdie_ref
from deneva_amd import KEY_RESERVED, RC_ABORT, RC_RCOK, RC_WAIT
from waitdie_cases import new_state

MAPS = list(sc.KEY_MAPS)


# ------------------------------------------------------- sizes and patterns
def test_sizes_sit_on_the_seams():
    assert sc.T4 == sc.RS_THREADS * sc.RS_ITEMS_SMALL and sc.T16 == sc.RS_THREADS * sc.RS_ITEMS
    assert sc.RS_SMALL % sc.T16 == 0 and sc.RS_SMALL % sc.T4 == 0
    assert max(sc.SMALL_SIZES) <= sc.RS_SMALL == min(sc.LARGE_SIZES)
    # one size on the small tile's side of the threshold, the rest on the large tile's
    assert [n > sc.RS_SMALL for n in sc.LARGE_SIZES] == [False, True, True, True, True]
    assert {n % sc.T16 for n in sc.LARGE_SIZES} == {0, 1, sc.T16 - 1}
    assert {n % sc.T4 for n in sc.SMALL_SIZES} >= {0, 1, sc.T4 - 1}
    assert sc.above_threshold(sc.LARGE_ALL) and sc.LARGE_ALL % 2 == 1 and sc.SMALL_ALL % 2 == 1
    # an odd count: the second u32 buffer at byte 20 n and the second u64 buffer
    # at byte 8 n of the workspace are not 16-byte aligned
    for n in (sc.SMALL_ALL, sc.LARGE_ALL, sc.RS_SMALL + 1, sc.RS_SMALL + sc.T16 - 1):
        assert (20 * n) % 16 != 0 and (8 * n) % 16 != 0


def test_dispatch_cases_cover_what_they_claim():
    cases = sc.DISPATCH_CASES
    assert len(set(cases)) == len(cases)
    for n in sc.SMALL_SIZES + sc.LARGE_SIZES:
        assert any(c[0] == n and c[1] == "random" for c in cases), n
    for at in (sc.SMALL_ALL, sc.LARGE_ALL):
        here = [c for c in cases if c[0] == at]
        assert {c[1] for c in here} == set(sc.ORDER_PATTERNS)
        assert {c[2] for c in [c for c in cases if (c[0] > sc.T4 * 3) == (at > sc.T4 * 3)]} == set(sc.WAVE_MAX)
    assert len([c for c in cases if c[0] >= sc.RS_SMALL]) <= 13
    assert max(sc.WAVE_MAX) < 1 << 20
    # bit counts of the wave sort: none, one, one byte, one byte + 1 bit, two bytes, two bytes + 1 bit, 20
    assert [int(w).bit_length() for w in sc.WAVE_MAX] == [0, 1, 8, 9, 16, 17, 20]


@pytest.mark.parametrize("n", [sc.SMALL_ALL, sc.RS_SMALL + 1])
def test_order_patterns(n):
    rng = np.random.default_rng(n)
    o = sc.make_order("random", n, rng)
    assert o.dtype == np.uint64 and (o >= np.uint64(1 << 63)).any() and (o < np.uint64(1 << 63)).any()
    assert sc.varying_bits(o) == 64
    assert np.unique(sc.make_order("equal", n, rng)).size == 1
    assert np.unique(sc.make_order("eight", n, rng)).size == 8
    o = sc.make_order("descending", n, rng)
    assert (o[1:] < o[:-1]).all() and int(o[0]) == (1 << 64) - 1 and int(o[0] - o[-1]) == n - 1
    for j in (0, 3, 7):
        o = sc.make_order(f"byte{j}", n, rng)
        assert (int(np.bitwise_or.reduce(o)) ^ int(np.bitwise_and.reduce(o))) == 0xFF << (8 * j)
        assert np.unique(o).size == 256
    o = sc.make_order("digits_0_255", n, rng)
    digits = np.unique(o.view(np.uint8))
    assert digits.tolist() == [0, 255] and np.unique(o).size == 256
    for wmax in sc.WAVE_MAX:
        w = sc.make_wave(wmax, n, rng)
        assert w.dtype == np.uint32 and int(w.max()) == wmax


def test_dispatch_expected_by_hand():
    wave = np.asarray([1, 0, 1, 0, 2, 1], np.uint32)
    order = np.asarray([5, 5, 1, 9, 0, 1], np.uint64)
    # sequence order (ties by index): 4, 2, 5, 0, 1, 3
    off, txn = sc.dispatch_expected(wave, order)
    assert off.tolist() == [0, 2, 5, 6] and txn.tolist() == [1, 3, 2, 5, 0, 4]
    off, txn = sc.dispatch_expected(wave, None)
    assert off.tolist() == [0, 2, 5, 6] and txn.tolist() == [1, 3, 0, 2, 5, 4]
    w, o = sc.dispatch_arrays(*sc.DISPATCH_CASES[0])
    w2, o2 = sc.dispatch_arrays(*sc.DISPATCH_CASES[0])
    assert np.array_equal(w, w2) and np.array_equal(o, o2)


# ----------------------------------------------------------------- key maps
@pytest.mark.parametrize("name", MAPS)
def test_map_is_injective_and_varies_as_claimed(name):
    b, _ = sc.hot_base()
    raw = np.unique(b.keys)
    assert int(raw.max()) < 0xFFF and sc.varying_bits(raw) == 12
    k = sc.KEY_MAPS[name](raw)
    assert k.dtype == np.uint64 and np.unique(k).size == raw.size
    assert not (k == np.uint64(KEY_RESERVED)).any()
    if sc.MAP_BITS[name] is not None:
        assert sc.varying_bits(k) == sc.MAP_BITS[name]
    if name == "spread_odd":
        assert (k >> np.uint64(63)).any() and not (k >> np.uint64(63)).all()
    if name == "top":
        assert int(k.max()) >= KEY_RESERVED - 1 - int(raw.min()) and int(k.min()) > KEY_RESERVED - 0x1000
    m = sc.mapped(b, name)
    assert np.array_equal(m.keys, sc.KEY_MAPS[name](b.keys)) and m.offsets is b.offsets


def test_spreads_have_32_one_bit_runs():
    raw = np.unique(sc.hot_base()[0].keys)
    for name, first in (("spread_even", 0), ("spread_odd", 1)):
        k = sc.KEY_MAPS[name](raw)
        v = int(np.bitwise_or.reduce(k)) ^ int(np.bitwise_and.reduce(k))
        assert v == sum(1 << (2 * i + first) for i in range(32))


def test_varying64_refuses_the_reserved_row():
    f = sc.KEY_MAPS["varying64"]
    assert int(f(np.asarray([0xFFD], np.uint64))[0]) == KEY_RESERVED - 2
    assert int(f(np.asarray([0xFFE], np.uint64))[0]) == 0xFFE
    with pytest.raises(AssertionError):
        f(np.asarray([0xFFF], np.uint64))


def remap(dct, f):
    ks = np.fromiter(dct.keys(), np.uint64, len(dct))
    return dict(zip(f(ks).tolist(), dct.values()))


@pytest.mark.parametrize("name", MAPS[1:])
def test_replays_decide_a_mapped_batch_as_the_unmapped_one(name):
    """The replays compare keys for equality only.  This guards the builders,
    not the engine."""
    b, ts = sc.hot_base()
    f = sc.KEY_MAPS[name]
    m = sc.mapped(b, name)
    # NO_WAIT
    for x, y in zip(nowait_ref.replay(b), nowait_ref.replay(m)):
        assert np.array_equal(x, y)
    # TIMESTAMP: decisions and rows
    r0, r1 = {}, {}
    for x, y in zip(tso_ref.replay(b, ts, r0), tso_ref.replay(m, ts, r1)):
        assert np.array_equal(x, y)
    assert remap(r0, f) == r1
    # MVCC: decisions, versions read, rows and store
    s0, s1 = {}, {}
    for x, y in zip(mvcc_ref.replay(b, ts, s0), mvcc_ref.replay(m, ts, s1)):
        assert np.array_equal(x, y)
    assert remap(s0, f) == s1
    # WAIT_DIE: epoch, release, epoch
    rc, pos = new_state(b.n_txn)
    e0, e1 = waitdie_ref.replay_epoch(b, ts, rc, pos), waitdie_ref.replay_epoch(m, ts, rc, pos)
    assert all(np.array_equal(x, y) for x, y in zip(e0[:3], e1[:3])) and e0[3] == e1[3]
    leave = np.isin(e0[0], [RC_RCOK, RC_ABORT]).astype(np.uint8)
    q0 = waitdie_ref.replay_release(b, ts, e0[0], e0[1], leave)
    q1 = waitdie_ref.replay_release(m, ts, e0[0], e0[1], leave)
    assert all(np.array_equal(x, y) for x, y in zip(q0[:2], q1[:2])) and q0[2:] == q1[2:]
    f0, f1 = waitdie_ref.replay_epoch(b, ts, q0[0], q0[1]), waitdie_ref.replay_epoch(m, ts, q0[0], q0[1])
    assert all(np.array_equal(x, y) for x, y in zip(f0[:3], f1[:3])) and f0[3] == f1[3]
    # the lock table: epoch, release of the committed, export
    t0, t1 = locktab_ref.LockTable(), locktab_ref.LockTable()
    l0, l1 = t0.lock_epoch(b), t1.lock_epoch(m)
    assert np.array_equal(l0[0], l1[0]) and np.array_equal(l0[1], l1[1])
    assert remap(t0.export(), f) == t1.export() and len(t1.export()) > 0
    half = np.where(np.arange(b.n_txn) % 2 == 0, l0[0], RC_ABORT).astype(np.uint8)
    assert t0.release(b, half) == t1.release(m, half)
    assert remap(t0.export(), f) == t1.export() and len(t1.export()) > 0
    # Calvin
    for x, y in zip(orc.calvin(b), orc.calvin(m)):
        assert np.array_equal(x, y)


def test_hot_base_yields_every_outcome():
    b, ts = sc.hot_base()
    rc, pos = new_state(b.n_txn)
    e1 = waitdie_ref.replay_epoch(b, ts, rc, pos)
    assert min(e1[3]["n_commit"], e1[3]["n_abort"], e1[3]["n_survivors"]) > 0
    leave = np.isin(e1[0], [RC_RCOK, RC_ABORT]).astype(np.uint8)
    r1 = waitdie_ref.replay_release(b, ts, e1[0], e1[1], leave)
    assert r1[3] > 0, "the release promotes nobody"
    e2 = waitdie_ref.replay_epoch(b, ts, r1[0], r1[1])
    assert e2[3]["n_commit"] > 0
    for erc in (nowait_ref.replay(b)[0], tso_ref.replay(b, ts, {})[0], locktab_ref.LockTable().lock_epoch(b)[0]):
        assert 0 < int((erc == RC_RCOK).sum()) < erc.size
    g, crc, _ = orc.calvin(b)
    assert 0 < int((crc == 0).sum()) < crc.size and int(g.max()) > 3


# ------------------------------------------------------ large engine cases
def test_large_ycsb_cases_lie_above_the_threshold():
    b, ts = sc.big_ycsb()
    assert b.n_txn == sc.BIG_TXN and b.nnz == sc.RS_SMALL + 16 and sc.above_threshold(b.nnz)
    assert -(-b.nnz // sc.T16) == 257 and b.nnz % sc.T16 == 16
    assert np.unique(ts).size == b.n_txn


def test_large_tso_yields_both_outcomes():
    _, _, rc, cf, k, wts, rts = sc.big_tso()
    assert 0 < int((rc == RC_ABORT).sum()) < rc.size and int((cf[rc == RC_ABORT] > 0).sum()) > 0
    assert (wts > 0).any() and (rts > 0).any() and k.size > 100000


def test_large_mvcc_yields_both_outcomes():
    _, _, rc, cf, vts, k, latest, rts, vk, vt = sc.big_mvcc()
    assert 0 < int((rc == RC_ABORT).sum()) < rc.size
    assert vk.size > 1000 and np.unique(vk).size < vk.size, "no row has two versions"
    late = int(((vts != np.uint64(mvcc_ref.VTS_BASE)) & (vts != np.uint64(mvcc_ref.VTS_NONE))).sum())
    assert late > 0 and int((vts == np.uint64(mvcc_ref.VTS_BASE)).sum()) > 0


def test_large_waitdie_yields_every_outcome_and_promotions():
    b, ts, e1, leave, r1, e2 = sc.big_waitdie()
    st = e1[3]
    print(f"WAIT_DIE at {b.nnz} accesses: {st['n_commit']} RCOK, {st['n_abort']} ABORT, {st['n_survivors']} WAIT, "
          f"{r1[3]} promotions")
    assert min(st["n_commit"], st["n_abort"], st["n_survivors"]) > 1000
    assert st["n_commit"] + st["n_abort"] + st["n_survivors"] == b.n_txn
    assert int((e1[0] == RC_WAIT).sum()) == st["n_survivors"]
    assert r1[2] == int(leave.sum()) == st["n_commit"] + st["n_abort"] and r1[3] > 1000
    assert e2[3]["n_commit"] > 0 and e2[3]["n_abort"] + e2[3]["n_survivors"] > 0


def test_large_calvin_cases():
    b, (g, rc, _) = sc.big_calvin_keys()
    assert sc.above_threshold(b.nnz) and 32 < sc.varying_bits(b.keys) <= sc.CALVIN_WIDE_BITS
    assert not (b.keys == np.uint64(KEY_RESERVED)).any()
    assert np.array_equal(rc, orc.calvin(sc.big_ycsb()[0])[1]) and 0 < int((rc == 0).sum()) < rc.size
    b, (g, rc, _) = sc.big_calvin_order()
    assert b.n_txn == b.nnz == sc.RS_SMALL + 1 and sc.above_threshold(b.n_txn)
    assert 32 < sc.varying_bits(b.order) <= 63 and (np.diff(b.order.astype(np.int64)) < 0).any()
    assert 0 < int((rc == 0).sum()) < rc.size


@pytest.mark.parametrize("two_sorts", [False, True])
def test_large_history_case(two_sorts):
    appends, b, (erc, etn, etnc), (hk, ht) = sc.big_history(two_sorts)
    assert appends[-1][0].size == sc.HIST_PAIRS and sc.above_threshold(hk.size)
    assert int(hk.max()) == KEY_RESERVED - 1 and not (hk == np.uint64(KEY_RESERVED)).any()
    assert sc.varying_bits(hk) == 64
    # several tns per key, not in append order
    k, t = appends[-1]
    o = np.argsort(k, kind="stable")
    same = k[o][1:] == k[o][:-1]
    assert int(same.sum()) > sc.HIST_PAIRS // 2 and (t[o][1:][same] < t[o][:-1][same]).any()
    if two_sorts:  # the later append reaches below the first one's tns
        assert len(appends) == 2 and int(appends[1][1].min()) < int(appends[0][1].min())
    # the history decides: without it other txns abort
    plain = orc.occ(b, tnc=sc.HIST_TNC)[0]
    assert int((plain != erc).sum()) > 100 and 0 < int((erc == 0).sum()) < erc.size
