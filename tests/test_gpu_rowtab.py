"""GPU: the persistent row table MaaT and TIMESTAMP share (csrc/rowtab.h),
through each engine's public *_rows_set / _get / _clear / _size calls only: the
empty table, the growth seams of the minimum table (2^12 slots, at most half
full), overwriting, clearing and a rejected set.  Every value is read back
exactly."""
import numpy as np
import pytest

import deneva_amd as d
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
