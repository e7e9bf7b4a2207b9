"""GPU: the persistent row table MaaT and TIMESTAMP share (csrc/rowtab.h),
through each engine's public *_rows_set / _get / _clear / _size calls only: the
empty table, the growth seams of the minimum table (2^12 slots, at most half
full), overwriting, clearing and a rejected set.  Every value is read back
exactly."""
import numpy as np
import pytest

import deneva_amd as d
import rowtab_cases as rtc
from deneva_amd import _abi

pytestmark = pytest.mark.gpu

MIN_ROWS = 2048  # half of the minimum table's 2^12 slots


class Rows:
    """One engine's row-table calls on a fresh context."""

    def __init__(self, eng, alg):
        self.eng, self.alg = eng, alg
        self.set = getattr(eng, alg + "_rows_set")
        self.get = getattr(eng, alg + "_rows_get")
        self.clear = getattr(eng, alg + "_rows_clear")

    @property
    def size(self):
        return getattr(self.eng, self.alg + "_rows_size")

    def check(self, k, a, b):
        ga, gb = self.get(k)
        assert np.array_equal(ga, a) and np.array_equal(gb, b)
        assert self.size == np.unique(k).size


@pytest.fixture(params=["maat", "tso"])
def rows(request):
    with d.Engine(0) as eng:
        yield Rows(eng, request.param)


def keys_values(n, seed=11):
    """n distinct random 40-bit keys (test_row_table_growth's kind) and two values each."""
    rng = np.random.default_rng(seed)
    k = rng.choice(1 << 40, size=n, replace=False).astype(np.uint64)
    a = rng.integers(1, 1 << 62, size=n).astype(np.uint64)
    b = rng.integers(1, 1 << 62, size=n).astype(np.uint64)
    return k, a, b


def test_before_any_table(rows):
    assert rows.size == 0
    k, _, _ = keys_values(100)
    a, b = rows.get(k)
    assert not a.any() and not b.any()
    assert rows.size == 0
    rows.clear()  # nothing to clear
    assert rows.size == 0


def test_growth_seams(rows):
    """Exactly half of the minimum table (no growth), one more row (the first
    rehash), and on to 8,193 rows (the third): after every step every row set
    so far reads back and size is the number of distinct keys."""
    k, a, b = keys_values(4 * MIN_ROWS + 1)
    done = 0
    for upto in (MIN_ROWS, MIN_ROWS + 1, 2 * MIN_ROWS, 2 * MIN_ROWS + 1, 4 * MIN_ROWS, 4 * MIN_ROWS + 1):
        rows.set(k[done:upto], a[done:upto], b[done:upto])
        done = upto
        rows.check(k[:done], a[:done], b[:done])
    # keys the table does not have, next to ones it has
    other = np.setdiff1d(keys_values(500, seed=12)[0], k)
    ga, gb = rows.get(np.concatenate([other, k[:3]]))
    assert not ga[:other.size].any() and not gb[:other.size].any()
    assert np.array_equal(ga[other.size:], a[:3]) and np.array_equal(gb[other.size:], b[:3])


def test_set_overwrites(rows):
    k, a, b = keys_values(3500)
    rows.set(k[:3000], a[:3000], b[:3000])
    rows.check(k[:3000], a[:3000], b[:3000])
    # 1,000 present keys with other values: size stays
    a[:1000] += np.uint64(1)
    b[:1000] += np.uint64(2)
    rows.set(k[:1000], a[:1000], b[:1000])
    rows.check(k[:3000], a[:3000], b[:3000])
    # present keys and new ones in one call, a key twice with one value
    a[2000:3000] += np.uint64(3)
    sel = np.concatenate([np.arange(2000, 3500), np.arange(3400, 3450)])
    rows.set(k[sel], a[sel], b[sel])
    rows.check(k, a, b)


def test_clear(rows):
    k, a, b = keys_values(MIN_ROWS + 5)
    rows.set(k, a, b)
    rows.check(k, a, b)
    rows.clear()
    assert rows.size == 0
    ga, gb = rows.get(k)
    assert not ga.any() and not gb.any()
    rows.set(k[:7], a[:7], b[:7])  # the cleared table takes rows again
    rows.check(k[:7], a[:7], b[:7])


def test_reserved_key_rejects_the_set(rows):
    k, a, b = keys_values(MIN_ROWS)
    rows.set(k, a, b)
    # a batch of new and present keys with the reserved key in it; one that would grow the table
    k2, a2, b2 = keys_values(MIN_ROWS, seed=14)
    for n in (10, MIN_ROWS):
        bad = np.concatenate([k2[:n], k[:5]])
        bad[n // 2] = d.KEY_RESERVED
        with pytest.raises(d.DccError) as e:
            rows.set(bad, np.concatenate([a2[:n], a2[:5]]), np.concatenate([b2[:n], b2[:5]]))
        assert e.value.code == _abi.DCC_EINVAL
        rows.check(k, a, b)
        ga, gb = rows.get(k2[:n][~np.isin(k2[:n], k)])
        assert not ga.any() and not gb.any()
    rows.set(k2[:10], a2[:10], b2[:10])  # the context still works
    ga, gb = rows.get(k2[:10])
    assert np.array_equal(ga, a2[:10]) and np.array_equal(gb, b2[:10])


# ------------------------------------------------------------ clustered keys
# Keys placed by rowtab_cases.py (their homes are proved by
# test_rowtab_cases.py).  Every case has a fresh context: clear() keeps the
# table's size.
def values(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 1 << 62, size=n).astype(np.uint64),
            rng.integers(1, 1 << 62, size=n).astype(np.uint64))


def policy_of(rows):
    return {"maat": "fib", "tso": "mix"}[rows.alg]


def test_walk_wraps_at_the_last_slot(rows):
    """10 keys whose home is the last slot of the 2^12 table: all but one lie
    past the wrap.  The same after growth to 2^13 slots, with keys that share
    the last slot there too."""
    pol = policy_of(rows)
    last = (1 << rtc.RT_MIN_BITS) - 1
    k = rtc.keys_with_home(pol, last, rtc.RT_MIN_BITS, 20, rtc.RT_MIN_BITS + 1, 1)
    k, absent = k[:10], k[10:]
    a, b = values(10, 21)
    rows.set(k, a, b)
    rows.check(k, a, b)
    ga, gb = rows.get(absent)  # the same home: the walk wraps and ends at an empty slot
    assert not ga.any() and not gb.any()
    a[:5] += np.uint64(7)
    b[5:] += np.uint64(9)
    rows.set(k[::-1], a[::-1], b[::-1])  # overwrite
    rows.check(k, a, b)
    # grow: 2,048 rows more than half of 2^12 slots
    fk, fa, fb = keys_values(MIN_ROWS, seed=22)
    rows.set(fk, fa, fb)
    allk, alla, allb = np.concatenate([k, fk]), np.concatenate([a, fa]), np.concatenate([b, fb])
    rows.check(allk, alla, allb)
    ga, gb = rows.get(absent)
    assert not ga.any() and not gb.any()
    a += np.uint64(1)
    rows.set(k, a, b)
    rows.set(absent[:3], a[:3], b[:3])  # three more behind the wrap
    rows.check(np.concatenate([k, fk, absent[:3]]), np.concatenate([a, fa, a[:3]]),
               np.concatenate([b, fb, b[:3]]))


CLUSTER_HOMES = [100, (1 << rtc.RT_MIN_BITS) - 100]  # inside the table; the walk crosses its end


def cluster_batch(k, seed, n_txn=300):
    """Txns of 1 .. 4 accesses over the keys k."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 5, size=n_txn)
    off = np.zeros(n_txn + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    keys = k[rng.integers(0, k.size, size=int(off[-1]))]
    at = np.where(rng.random(keys.size) < 0.4, d.WR, d.RD).astype(np.uint8)
    return d.EpochBatch(off, keys, at)


@pytest.mark.parametrize("h", CLUSTER_HOMES)
def test_maat_walk_bound_at_its_limit(h):
    """MT_WALK keys sharing one home at every table size up to 2^24, set in
    one call: all are stored (the last one MT_WALK - 1 slots from its home),
    and an epoch over exactly those rows finds every one."""
    from test_gpu_maat import run
    k = rtc.keys_with_home("fib", h, rtc.RT_MIN_BITS, rtc.MT_WALK, 24, 0x5A5)
    a, b = values(k.size, 31)
    with d.Engine(0) as eng:
        r = Rows(eng, "maat")
        r.set(k, a, b)
        r.check(k, a, b)
        run(eng, cluster_batch(k, 32), rows=(k, a % np.uint64(1000), b % np.uint64(1000)))
        assert r.size == rtc.MT_WALK
        run(eng, cluster_batch(k, 33), rows=(k, a, b))
        assert r.size == rtc.MT_WALK


@pytest.mark.parametrize("h", CLUSTER_HOMES)
def test_maat_walk_bound_passed_by_one(h):
    """A 257th key of that home: the set and an epoch that accesses it fail
    with DCC_EIO (the epoch after the driver's second attempt), the 256 rows
    stay as they were, and the context goes on working."""
    import _oracle as orc
    k = rtc.keys_with_home("fib", h, rtc.RT_MIN_BITS, rtc.MT_WALK + 1, 24, 0x5A5)
    k, extra = k[:rtc.MT_WALK], k[rtc.MT_WALK:]
    a, b = values(k.size, 41)
    a, b = a % np.uint64(1000), b % np.uint64(1000)
    with d.Engine(0) as eng:
        r = Rows(eng, "maat")
        r.set(k, a, b)
        r.check(k, a, b)

        def unchanged():
            r.check(k, a, b)
            ga, gb = r.get(extra)
            assert not ga.any() and not gb.any()

        with pytest.raises(d.DccError) as e:
            r.set(extra, a[:1], b[:1])
        assert e.value.code == _abi.DCC_EIO
        unchanged()
        one = d.EpochBatch(np.array([0, 1], np.uint32), extra, np.array([d.WR], np.uint8))
        with pytest.raises(d.DccError) as e:
            eng.maat_validate_epoch(one)
        assert e.value.code == _abi.DCC_EIO
        unchanged()
        # the cluster's rows next to the failing one: nothing of the epoch lands
        mixed = cluster_batch(np.concatenate([k[:50], extra]), 42)
        assert (mixed.keys == extra[0]).any()
        with pytest.raises(d.DccError) as e:
            eng.maat_validate_epoch(mixed)
        assert e.value.code == _abi.DCC_EIO
        unchanged()
        # an ordinary epoch on the same context: the cluster and other rows
        # (rows whose walk would run into the cluster's 256 slots are one past the bound too)
        fk, _, _ = keys_values(300, seed=43)
        dist = (np.array([rtc.home("fib", x, rtc.RT_MIN_BITS) for x in fk]) - h) % (1 << rtc.RT_MIN_BITS)
        fk = fk[(dist > 2 * rtc.MT_WALK) & (dist < (1 << rtc.RT_MIN_BITS) - 2 * rtc.MT_WALK)]
        assert fk.size > 150
        ok = cluster_batch(np.concatenate([k, fk]), 44, n_txn=600)
        rc, cts, st = eng.maat_validate_epoch(ok)
        erc, ects, (ek, elr, elw) = orc.maat(ok, k, a, b)
        assert np.array_equal(np.asarray(rc), erc) and np.array_equal(np.asarray(cts, np.uint64), ects)
        assert 0 < st["n_commit"] == int((erc == 0).sum()) < ok.n_txn
        glr, glw = r.get(ek)
        assert np.array_equal(glr, elr) and np.array_equal(glw, elw)
        assert r.size == np.union1d(k, ok.keys).size


def test_tso_cluster_beyond_the_maat_bound():
    """ProbeMix walks the whole table: 300 keys of one home (more than
    MT_WALK) are all stored, and a TIMESTAMP epoch over them equals the replay."""
    from test_gpu_tso import both_outcomes, check, reference
    last = (1 << rtc.RT_MIN_BITS) - 1
    k = rtc.keys_with_home("mix", last - 150, rtc.RT_MIN_BITS, 300, 24, 0x777)
    assert k.size > rtc.MT_WALK
    a, b = values(k.size, 51)
    with d.Engine(0) as eng:
        r = Rows(eng, "tso")
        r.set(k, a, b)
        r.check(k, a, b)
        bt = cluster_batch(k, 52, n_txn=400)
        rng = np.random.default_rng(53)
        ts = (np.uint64(1000) + rng.permutation(bt.n_txn).astype(np.uint64))
        seed = {int(x): (int(w), int(q)) for x, w, q in zip(k, rng.integers(0, 1400, size=k.size),
                                                           rng.integers(0, 1400, size=k.size))}
        ref = reference(bt, ts, seed)
        both_outcomes(ref)
        check(eng, bt, ts, seed, ref=ref)
        assert r.size == k.size
