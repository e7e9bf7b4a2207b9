"""Directed cases of the GPU index (csrc/index.hip) and the range check of
dcc_calvin_dispatch, against the dict oracle (index_ref.py).

The table: open addressing, unit step, home = the top `bits` bits of
key * 0x9E3779B97F4A7C15 (ProbeFib's rule, so rowtab_cases.keys_with_home
places keys in it).  dcc_ctx::index_reserve(want = distinct keys so far + keys
of the call, duplicates counted) keeps the table while 2 * want <= capacity,
else rehashes into the smallest table of at least 2^12 slots with 2 * want <=
capacity: 2,048 keys fit the first table, the 2,049th insert rehashes to 2^13.
The cases keep clusters on one home across those rehashes, put them on the
table's last slot (the walk wraps with (s + 1) & mask) and make one call's
lanes race for one slot (k_ix_insert's CAS, the ordinals' atomicMax)."""
import ctypes as C
import re
import os

import numpy as np
import pytest

import deneva_amd as d
import rowtab_cases as rt
from deneva_amd import _abi
from deneva_amd._abi import ROW_NONE
from index_ref import IX_MIN_BITS, bits_after_insert, index_oracle

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva_amd", "csrc")
RES = np.uint64(d.KEY_RESERVED)


class Model:
    """The engine's index next to the oracle's inserts and the table size."""

    def __init__(self, eng):
        self.eng = eng
        self.inserts = []
        self.bits = 0
        self.nrow = 0

    @property
    def nkeys(self):
        return len({k for ks, _ in self.inserts for k in ks.tolist()})

    def insert(self, keys, rows=None):
        keys = np.asarray(keys, np.uint64)
        if rows is None:  # a row id no other insert has: the call and the position
            rows = (np.uint64(len(self.inserts) + 1) << np.uint64(32)) | np.arange(keys.size, dtype=np.uint64)
        self.bits = bits_after_insert(self.bits, self.nkeys, keys.size)
        self.eng.index_insert(keys, rows)
        self.inserts.append((keys, np.asarray(rows, np.uint64)))
        assert self.eng.index_size == self.nkeys

    def clear(self):
        self.eng.index_clear()
        self.inserts = []
        self.bits = 0
        assert self.eng.index_size == 0

    def check(self, probe, dev=False):
        probe = np.asarray(probe, np.uint64)
        want = index_oracle(self.inserts, probe)
        if dev:
            import torch
            out, miss = self.eng.index_probe(torch.from_numpy(probe.view(np.int64)).cuda())
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint64)
        else:
            got, miss = self.eng.index_probe(probe)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"{bad.size} of {probe.size} rows differ, first at {bad[:5]}: "
                               f"got {got[bad[:5]]}, want {want[bad[:5]]}")
        assert miss == int((want == np.uint64(ROW_NONE)).sum())
        return want


def all_keys(m):
    return np.unique(np.concatenate([k for k, _ in m.inserts]))


def test_the_restated_rules_are_index_hip_s():
    src = open(os.path.join(CSRC, "index.hip")).read()
    assert "return (key * 0x%Xull) >> (64 - bits);" % rt.FIB in src
    assert "if (ix_bits && 2 * want <= (1ull << ix_bits)) return DCC_OK;" in src
    assert int(re.search(r"std::max<uint32_t>\(ix_bits, (\d+)\)", src).group(1)) == IX_MIN_BITS
    assert "while ((1ull << bits) < 2 * want) bits++;" in src
    assert "CR(ctx->index_reserve(ctx->ix_nkeys + n));" in src
    assert bits_after_insert(0, 0, 2048) == 12 and bits_after_insert(12, 2048, 1) == 13
    assert bits_after_insert(12, 10, 5) == 12 and bits_after_insert(13, 0, 1) == 13


@pytest.mark.parametrize("dev", [False, True])
def test_empty_and_trivial(dev):
    rng = np.random.default_rng(1)
    with d.Engine(0) as eng:
        m = Model(eng)
        some = rng.integers(0, 1 << 63, size=257).astype(np.uint64)
        m.check(some, dev)                      # never filled: every key misses
        m.check(some[:1], dev)
        eng.index_insert(np.zeros(0, np.uint64), np.zeros(0, np.uint64))
        got, miss = eng.index_probe(np.zeros(0, np.uint64))
        assert got.size == 0 and miss == 0 and eng.index_size == 0
        m.check(some, dev)
        m.insert(some[:1], np.array([7], np.uint64))
        assert m.check(some[:1], dev)[0] == 7
        m.check(some, dev)                      # 256 misses beside the one hit
        m.insert(np.array([0], np.uint64))      # key 0 is a key like any other
        m.check(np.array([0, 1], np.uint64), dev)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_miss_counts_of_partial_waves(n, dev):
    """The misses are summed per wave (wave_reduce) and per call: the probe
    sizes around one wave and one workgroup, with a known number of misses at
    known places -- none, all, the first and last lane, every third."""
    rng = np.random.default_rng(n)
    with d.Engine(0) as eng:
        m = Model(eng)
        have = rng.permutation(1 << 20)[:n].astype(np.uint64) + np.uint64(1)
        m.insert(have)
        absent = have + np.uint64(1 << 32)
        for sel in (np.zeros(n, bool), np.ones(n, bool), np.arange(n) % 3 == 0,
                    (np.arange(n) == 0) | (np.arange(n) == n - 1), np.arange(n) >= 64):
            probe = np.where(sel, absent, have)
            want = m.check(probe, dev)
            assert int((want == np.uint64(ROW_NONE)).sum()) == int(sel.sum())


def test_duplicates_last_ordinal_wins():
    rng = np.random.default_rng(2)
    with d.Engine(0) as eng:
        m = Model(eng)
        k = np.uint64(0xDEADBEEF12345)
        m.insert(np.full(64, k))                 # one key in every lane of a wave
        assert m.check(np.array([k]))[0] == m.inserts[-1][1][63]
        m.insert(np.full(1024, k))               # ... and in every key of four workgroups
        assert m.check(np.array([k]))[0] == m.inserts[-1][1][1023] and eng.index_size == 1
        m.insert(np.array([k, k + np.uint64(1), k]))  # across calls
        assert m.check(np.array([k]))[0] == m.inserts[-1][1][2]
        # a few keys, each many times, shuffled: the last position of each wins
        few = rng.integers(0, 1 << 62, size=7).astype(np.uint64)
        m.insert(few[rng.integers(0, 7, size=1500)])
        m.check(np.concatenate([few, [k, k + np.uint64(1), k + np.uint64(2)]]))
        # the table grows twice, then the key again
        assert m.bits == 12
        m.insert(rng.integers(0, 1 << 62, size=5000).astype(np.uint64))
        b = m.bits
        assert b > 12
        m.insert(rng.integers(0, 1 << 62, size=9000).astype(np.uint64))
        assert m.bits > b
        m.check(np.concatenate([few, [k]]))
        m.insert(np.array([k, few[0]]))
        assert m.check(np.array([k]))[0] == m.inserts[-1][1][0]
        m.check(all_keys(m))


@pytest.mark.parametrize("count", [64, 300])
@pytest.mark.parametrize("dups", [False, True])
def test_one_home_in_one_call(count, dups):
    """`count` distinct keys of one home inserted by one call: every lane
    starts its walk on the same slot, one wins the CAS and the others -- who
    lost it to ANOTHER key -- must move on; with duplicates mixed in, the
    lanes that lose to their OWN key must stay and raise its ordinal."""
    rng = np.random.default_rng(count + dups)
    with d.Engine(0) as eng:
        m = Model(eng)
        k = rt.keys_with_home("fib", 1234, 12, count, 16, 5)
        call = np.concatenate([k, k[rng.integers(0, count, size=2 * count)]]) if dups else k
        call = call[rng.permutation(call.size)]
        m.insert(call)
        assert m.bits == 12 and eng.index_size == count
        absent = rt.keys_with_home("fib", 1234, 12, 20, 16, 5, seed=9)
        absent = np.setdiff1d(absent, k)
        m.check(np.concatenate([k, absent]))
        m.check(np.concatenate([k, absent]), dev=True)
        # a second call on the cluster: every key found again, not inserted twice
        m.insert(k[::-1].copy())
        assert eng.index_size == count
        m.check(np.concatenate([k, absent]))


def test_cluster_on_the_last_slot_at_every_size():
    """40 keys homed on the last slot at 2^12 .. 2^16 slots: the walk wraps to
    slot 0 in k_ix_insert, k_ix_rehash and k_ix_probe, for members and for an
    absent key of that home (whose walk ends on the first empty slot after the
    wrap)."""
    rng = np.random.default_rng(4)
    with d.Engine(0) as eng:
        m = Model(eng)
        k = rt.keys_with_home("fib", 4095, 12, 40, 16, 15)
        other = np.setdiff1d(rt.keys_with_home("fib", 4095, 12, 30, 16, 15, seed=5), k)
        for b in range(12, 17):
            assert {rt.home("fib", x, b) for x in np.concatenate([k, other])} == {(1 << b) - 1}
        m.insert(k[:25])
        seen = {m.bits}
        m.check(np.concatenate([k, other]))
        m.insert(k[20:])                         # the rest, some again, on the wrapped cluster
        m.check(np.concatenate([k, other]))
        for total in (2100, 4200, 8300, 16500):  # one rehash each: 2^13 .. 2^16
            fill = rng.integers(0, 1 << 62, size=total - m.nkeys).astype(np.uint64)
            m.insert(fill)
            seen.add(m.bits)
            m.check(np.concatenate([k, other, fill[:50]]))
            m.insert(k[:3])                      # newest rows on the wrapped cluster after the rehash
            m.check(np.concatenate([k, other]), dev=True)
        assert seen == {12, 13, 14, 15, 16}
        m.check(all_keys(m))


def test_growth_keeps_the_newest_rows():
    rng = np.random.default_rng(5)
    with d.Engine(0) as eng:
        m = Model(eng)
        cl = rt.keys_with_home("fib", 77, 12, 100, 16, 3)   # one home through 2^16 slots
        first = np.concatenate([cl, rng.integers(0, 1 << 62, size=1948).astype(np.uint64)])
        m.insert(first)                          # 2,048 keys: 2 * 2,048 <= 4,096, no growth
        assert m.bits == 12 and eng.index_size == 2048
        m.insert(first[:10])                     # older rows replaced before the rehash
        # (the call counted its 10 duplicates: 2,058 wanted, so this one already rehashed)
        assert m.bits == 13
        m.check(first)
        m.insert(np.array([1 << 50], np.uint64))
        m.check(np.concatenate([first, [1 << 50, 1 << 51]]))
        for add in (3000, 6000):                 # twice more
            b = m.bits
            m.insert(rng.integers(0, 1 << 62, size=add).astype(np.uint64))
            assert m.bits == b + 1
            m.insert(cl[::7].copy())
            m.check(np.concatenate([first, cl]))
        m.check(all_keys(m))
        m.check(all_keys(m), dev=True)


def test_exactly_2048_then_one_more():
    rng = np.random.default_rng(6)
    with d.Engine(0) as eng:
        m = Model(eng)
        first = rng.permutation(1 << 22)[:2048].astype(np.uint64)
        m.insert(first)
        assert m.bits == 12
        m.check(first)
        m.insert(np.array([1 << 40], np.uint64))  # the 2,049th key: rehash to 2^13
        assert m.bits == 13 and eng.index_size == 2049
        m.check(np.concatenate([first, [1 << 40, 1 << 41]]))


def test_clear_restarts():
    rng = np.random.default_rng(7)
    with d.Engine(0) as eng:
        m = Model(eng)
        k = rng.integers(0, 1 << 62, size=3000).astype(np.uint64)
        m.insert(k, k ^ np.uint64(0x55))
        m.check(k)
        m.clear()
        m.check(k[:300])                         # every old key misses
        m.insert(k[:5], np.arange(5, dtype=np.uint64) + np.uint64(100))   # ordinals restart at 0
        assert m.bits == 12
        want = m.check(k[:10])
        assert list(want[:5]) == [100, 101, 102, 103, 104] and (want[5:] == np.uint64(ROW_NONE)).all()
        m.insert(k[3:8], np.arange(5, dtype=np.uint64) + np.uint64(200))
        m.check(k[:10], dev=True)
        m.clear()
        m.clear()
        m.check(k[:10])


def test_multi_context_is_not_supported():
    k = np.arange(1, 9, dtype=np.uint64)
    with d.Engine(devices=[0, 0]) as m:
        with pytest.raises(d.DccError) as e:
            m.index_insert(k, k)
        assert e.value.code == _abi.DCC_ENOTSUP
        with pytest.raises(d.DccError) as e:
            m.index_probe(k)
        assert e.value.code == _abi.DCC_ENOTSUP


@pytest.mark.parametrize("dev", [False, True])
def test_probe_of_the_reserved_key(dev):
    """DCC_KEY_RESERVED marks an empty slot, so a probe that compares the slot
    with its key first 'finds' the reserved key in the first empty slot of its
    walk and returns rows[0] -- the first row ever inserted, or whatever the
    rows buffer holds on an empty index.  It is never in the index: ROW_NONE,
    counted as missing."""
    rng = np.random.default_rng(8)
    with d.Engine(0) as eng:
        m = Model(eng)
        probe = np.array([5, d.KEY_RESERVED, 6, d.KEY_RESERVED], np.uint64)
        want = m.check(probe, dev)               # empty index
        assert (want == np.uint64(ROW_NONE)).all()
        k = rng.integers(0, 1 << 62, size=500).astype(np.uint64)
        m.insert(k, k + np.uint64(1))
        probe = np.concatenate([k[:100], [RES], k[100:130], [RES, RES]])
        want = m.check(probe, dev)
        assert int((want == np.uint64(ROW_NONE)).sum()) == 3
        # the reserved key's own home (the top bits of -FIB) filled, so its walk is not empty at once
        near = rt.keys_with_home("fib", rt.home("fib", d.KEY_RESERVED, 12), 12, 30, 16,
                                 rt.home("fib", d.KEY_RESERVED, 16) & 15)
        m.insert(near)
        m.check(np.concatenate([[RES], near, [RES]]), dev)


def test_insert_with_the_reserved_key_changes_nothing():
    """A call with DCC_KEY_RESERVED among its keys is DCC_EINVAL and leaves
    the index as it was: not its other keys inserted, not the rows of keys it
    repeats replaced, not the size moved -- even where the call would have made
    the table grow."""
    rng = np.random.default_rng(9)
    with d.Engine(0) as eng:
        m = Model(eng)
        bad0 = np.array([1, 2, d.KEY_RESERVED, 3], np.uint64)
        with pytest.raises(d.DccError) as e:     # on an index that has no table yet
            eng.index_insert(bad0, bad0)
        assert e.value.code == _abi.DCC_EINVAL and eng.index_size == 0
        m.check(bad0)
        k = rng.integers(0, 1 << 62, size=1500).astype(np.uint64)
        m.insert(k)
        before = m.check(np.concatenate([k, bad0]))
        new = rng.integers(0, 1 << 62, size=1000).astype(np.uint64)   # 2,500 keys would not fit 2^12
        for pos in (0, 650, 1299):
            bad = np.concatenate([k[:300], new])
            bad[pos] = RES
            with pytest.raises(d.DccError) as e:
                eng.index_insert(bad, np.full(bad.size, 0xBAD, np.uint64))
            assert e.value.code == _abi.DCC_EINVAL
            assert eng.index_size == 1500
            assert np.array_equal(m.check(np.concatenate([k, bad0])), before)
            m.check(np.concatenate([new, k[:300]]))
            m.check(np.concatenate([new, k[:300]]), dev=True)
        assert m.bits == 12
        m.insert(np.concatenate([k[:300], new]))  # the same call without it works
        assert m.bits == 13
        m.check(np.concatenate([k, new, bad0]))


def test_dispatch_rejects_a_wave_level_of_all_ones():
    """max wave + 1 is the wave count: a level of 0xFFFFFFFF wraps it to 0.
    Only the count query (out_wave_off NULL) is made here, on purpose: that
    form never launches the offsets kernel, whose fill loop would run to
    2^32 - 1 over a buffer sized for a wrapped count of waves -- with offsets
    asked for (or through Engine.calvin_dispatch, which asks for them in its
    second call) unfixed code does not return.  The query answered DCC_OK with
    0 waves before the check; it is DCC_ERANGE.  One level below is still a
    count that fits."""
    with d.Engine(0) as eng:
        txn = np.zeros(8, np.uint32)
        for top, code, nwaves in ((0xFFFFFFFE, _abi.DCC_OK, 0xFFFFFFFF), (0xFFFFFFFF, _abi.DCC_ERANGE, None)):
            wave = np.array([0, 3, top, 1, 3, 0], np.uint32)
            nw = C.c_uint32(12345)
            r = _abi.lib.dcc_calvin_dispatch(eng.handle, wave.ctypes.data, None, wave.size, 0, None, 0,
                                             txn.ctypes.data, C.byref(nw))
            assert r == code
            if nwaves is not None:
                assert nw.value == nwaves
                assert list(txn[:6]) == [0, 5, 3, 1, 4, 2]
        # the context still works
        off, t = eng.calvin_dispatch(np.array([1, 0, 1], np.uint32))
        assert list(off) == [0, 1, 3] and list(t) == [1, 0, 2]
