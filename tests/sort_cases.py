"""Cases for the shared stable LSD radix sort (csrc/radix_sort.hip) and for the
key packing in front of it (make_keypack / keypack_apply), shared by the CPU
check of the builders (test_sort_cases.py) and the GPU parity test
(test_gpu_sort_paths.py).  Pure numpy; every expectation comes from numpy's
stable argsort or from an engine's Python replay.

The sort takes 2,048-pair tiles (RS_ITEMS_SMALL items per thread) up to
RS_SMALL pairs and 8,192-pair tiles (RS_ITEMS) above: the sizes below sit on
the tile seams of both and on the threshold between them.  An odd pair count
also leaves the second ping-pong buffer of the dispatch workspace (u32 keys at
byte 20 n, u64 keys at byte 8 n of a 16-byte aligned block) short of 16-byte
alignment, which takes k_rs_hist's scalar loads.

dcc_calvin_dispatch(wave, order) is a stable 64-bit sort of `order` followed by
a stable u32 sort of `wave` over bit_length(max wave) bits: dispatch_expected
states it as two numpy argsorts.

Key maps are injective u64 -> u64 functions applied to a batch's keys.  The
engines' replays compare keys for equality only, so a mapped batch decides as
the unmapped one while the packing in front of the sort sees 32 one-bit runs,
bit 63, keys next to KEY_RESERVED, or exactly B varying bits.
"""
import functools
import os
import re

import numpy as np

from deneva_amd import KEY_RESERVED, RC_ABORT, RC_RCOK, EpochBatch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva_amd", "csrc")


def sort_constant(name):
    """A constexpr of radix_sort.h: a literal, or `a << b`."""
    with open(os.path.join(CSRC, "radix_sort.h")) as f:
        src = f.read()
    m = re.search(r"constexpr uint(?:32|64)_t %s = (\d+)(?:ull)?(?:\s*<<\s*(\d+))?;" % name, src)
    assert m, f"{name} not found in radix_sort.h"
    return int(m.group(1)) << int(m.group(2) or 0)


RS_THREADS = sort_constant("RS_THREADS")
RS_ITEMS = sort_constant("RS_ITEMS")
RS_ITEMS_SMALL = sort_constant("RS_ITEMS_SMALL")
RS_SMALL = sort_constant("RS_SMALL")
T4 = RS_THREADS * RS_ITEMS_SMALL  # pairs per tile up to RS_SMALL pairs
T16 = RS_THREADS * RS_ITEMS       # pairs per tile above
# the seams below are built on these: a retune of the sort has to move them
assert (T4, T16, RS_SMALL) == (2048, 8192, 2097152), (T4, T16, RS_SMALL)

SMALL_SIZES = (1, 2, 63, 64, 65, T4 - 1, T4, T4 + 1, 2 * T4 + 1)
LARGE_SIZES = (RS_SMALL, RS_SMALL + 1, RS_SMALL + T16 - 1, RS_SMALL + T16, RS_SMALL + T16 + 1)
SMALL_ALL = 2 * T4 + 1            # every pattern runs at these two sizes
LARGE_ALL = RS_SMALL + T16 + 1

ORDER_PATTERNS = ("random", "equal", "eight", "descending", "byte0", "byte3", "byte7", "digits_0_255")
WAVE_MAX = (0, 1, 255, 256, 65535, 65536, (1 << 20) - 1)

M64 = (1 << 64) - 1


def make_order(pattern, n, rng):
    """u64[n] sequencer orders."""
    if pattern == "random":       # the whole range, values >= 2^63 included
        return rng.integers(0, M64, size=n, dtype=np.uint64, endpoint=True)
    if pattern == "equal":        # the result is index order
        return np.full(n, 0x0123456789ABCDEF, np.uint64)
    if pattern == "eight":        # long runs, ties across tiles and waves
        vals = rng.integers(0, M64, size=8, dtype=np.uint64, endpoint=True)
        return vals[rng.integers(0, 8, size=n)]
    if pattern == "descending":   # strictly, one apart: keys that share a digit share every higher one,
        return np.uint64(M64) - np.arange(n, dtype=np.uint64)  # so each pass rests on the order of the last
    if pattern.startswith("byte"):  # one byte varies: every other pass sees one digit
        j = int(pattern[4:])
        base = np.uint64(0xA5A5A5A5A5A5A5A5 & ~(0xFF << (8 * j)))
        return base | (rng.integers(0, 256, size=n).astype(np.uint64) << np.uint64(8 * j))
    if pattern == "digits_0_255":  # every digit of every key is 0 or 255
        out = np.zeros(n, np.uint64)
        for j in range(8):
            out |= (rng.integers(0, 2, size=n).astype(np.uint64) * np.uint64(0xFF)) << np.uint64(8 * j)
        return out
    raise ValueError(pattern)


def make_wave(wmax, n, rng):
    """u32[n] wave levels in [0, wmax], the maximum among them."""
    w = rng.integers(0, wmax + 1, size=n).astype(np.uint32)
    w[int(rng.integers(0, n))] = wmax
    return w


def dispatch_cases():
    """(n, order pattern, wave maximum): every size with the random pattern,
    every pattern at SMALL_ALL and LARGE_ALL, every wave maximum at both."""
    cases = []
    for sizes, all_at in ((SMALL_SIZES, SMALL_ALL), (LARGE_SIZES, LARGE_ALL)):
        q = 0
        for n in sizes:
            cases.append((n, "random", WAVE_MAX[q % len(WAVE_MAX)]))
            q += 1
        for p in ORDER_PATTERNS[1:]:
            cases.append((all_at, p, WAVE_MAX[q % len(WAVE_MAX)]))
            q += 1
    return cases


DISPATCH_CASES = dispatch_cases()


def dispatch_arrays(n, pattern, wmax):
    rng = np.random.default_rng([n, ORDER_PATTERNS.index(pattern), wmax])
    return make_wave(wmax, n, rng), make_order(pattern, n, rng)


def dispatch_expected(wave, order):
    """(wave_off u32[W + 1], txn u32[n]): the txns of each wave in sequence
    order, ties in index order."""
    n = wave.size
    seq = np.arange(n) if order is None else np.argsort(order, kind="stable")
    txn = seq[np.argsort(wave[seq], kind="stable")]
    counts = np.bincount(wave, minlength=int(wave.max()) + 1)
    off = np.concatenate([[0], np.cumsum(counts)])
    return off.astype(np.uint32), txn.astype(np.uint32)


# ------------------------------------------------------------------ key maps
def _deposit(h, odd):
    out = np.zeros(h.shape, np.uint64)
    for i in range(32):
        out |= ((h >> np.uint64(i)) & np.uint64(1)) << np.uint64(2 * i + odd)
    return out


def _hash32(k):
    k = np.asarray(k, np.uint64)
    assert k.size == 0 or int(k.max()) < 1 << 32, "the spreads are injective below 2^32"
    return (k * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)  # an odd multiplier: a bijection mod 2^32


def identity(k):
    return np.asarray(k, np.uint64).copy()


def spread_even(k):
    """Bit i of a 32-bit hash at bit 2 i: 32 runs of one bit."""
    return _deposit(_hash32(k), 0)


def spread_odd(k):
    """The same at bit 2 i + 1: bit 63 varies."""
    return _deposit(_hash32(k), 1)


def top(k):
    """Keys next to KEY_RESERVED."""
    return np.uint64(M64 - 1) - np.asarray(k, np.uint64)


def varying(B, low=12):
    """Row r < 2^low - 1 as r, with bits low .. B - 1 set when r is odd: over a
    batch whose rows vary in all `low` low bits, OR ^ AND has exactly B bits.
    The one row varying(64) would send to KEY_RESERVED, 2^low - 1, is refused."""
    assert low < B <= 64

    def f(k):
        k = np.asarray(k, np.uint64)
        assert k.size == 0 or int(k.max()) < (1 << low) - 1, f"varying: rows below {(1 << low) - 1}"
        hi = np.uint64(((1 << B) - 1) & ~((1 << low) - 1))
        return k | ((k & np.uint64(1)) * hi)

    f.__name__ = f"varying{B}"
    return f


VARYING_B = (31, 32, 33, 63, 64)
KEY_MAPS = {"identity": identity, "spread_even": spread_even, "spread_odd": spread_odd, "top": top}
KEY_MAPS.update({f"varying{B}": varying(B) for B in VARYING_B})
# popcount(OR ^ AND) a map claims over a batch (None: whatever the batch has)
MAP_BITS = {"identity": None, "spread_even": 32, "spread_odd": 32, "top": None}
MAP_BITS.update({f"varying{B}": B for B in VARYING_B})


def varying_bits(keys):
    keys = np.asarray(keys, np.uint64)
    return bin(int(np.bitwise_or.reduce(keys)) ^ int(np.bitwise_and.reduce(keys))).count("1")


def mapped(b, name_or_fn):
    """The batch with its keys sent through a map; everything else shared."""
    f = KEY_MAPS[name_or_fn] if isinstance(name_or_fn, str) else name_or_fn
    return EpochBatch(b.offsets, f(b.keys), b.acctype, b.start_tn, b.finish_tn, b.order, dict(b.meta))


# ------------------------------------------------- small base (key shapes)
HOT_N = 3000


@functools.lru_cache(maxsize=None)
def hot_base():
    """(batch, ts): 3,000 ragged txns over 500 hot rows, all four access types
    (the batch of test_gpu_waitdie.test_six_epoch_histories)."""
    from waitdie_cases import hot_batch, make_ts
    rng = np.random.default_rng(0x50A7)
    b = hot_batch(rng, HOT_N, 8, 500)
    return b, make_ts(rng, HOT_N, "permuted")


# ------------------------------------------- large engine cases (section B)
BIG_TXN = 131073  # x 16 accesses: 16 pairs past RS_SMALL, 257 large tiles, the last of 16 pairs


@functools.lru_cache(maxsize=None)
def big_ycsb():
    """(batch, ts): YCSB theta 0.9, permuted timestamps."""
    import deneva_amd as d
    from tso_cases import make_ts
    b = d.gen_ycsb(n_txn=BIG_TXN, zipf_theta=0.9)
    return b, make_ts(np.random.default_rng(BIG_TXN), BIG_TXN, "permuted")


def above_threshold(m):
    """The sort of m pairs takes the large tile and its last tile is partial."""
    return m > RS_SMALL and m % T16 != 0


@functools.lru_cache(maxsize=None)
def big_tso():
    """(batch, ts, rc, conflict, keys, wts, rts): the replay from an empty
    table, the rows as arrays over the batch's distinct keys."""
    import tso_ref
    b, ts = big_ycsb()
    rows = {}
    rc, cf = tso_ref.replay(b, ts, rows)
    k = np.unique(b.keys)
    wr = np.asarray([rows.get(x, (0, 0)) for x in k.tolist()], np.uint64).reshape(-1, 2)
    return b, ts, rc, cf, k, wr[:, 0].copy(), wr[:, 1].copy()


@functools.lru_cache(maxsize=None)
def big_mvcc():
    """(batch, ts, rc, conflict, vts, keys, latest, rts, version keys, version
    ts): the replay from an empty store; the versions sorted by (key, ts)."""
    import mvcc_ref
    b, ts = big_ycsb()
    state = {}
    rc, cf, vts = mvcc_ref.replay(b, ts, state)
    k = np.unique(b.keys)
    rows = mvcc_ref.rows_of(state)
    lr = np.asarray([rows.get(x, (0, 0)) for x in k.tolist()], np.uint64).reshape(-1, 2)
    v = np.asarray(mvcc_ref.versions_of(state), np.uint64).reshape(-1, 2)
    return b, ts, rc, cf, vts, k, lr[:, 0].copy(), lr[:, 1].copy(), v[:, 0].copy(), v[:, 1].copy()


@functools.lru_cache(maxsize=None)
def big_waitdie():
    """(batch, ts, epoch 1, leave, release, epoch 2): an epoch from (RUN, 0),
    the release of every RCOK and ABORT txn, a second epoch."""
    from waitdie_cases import new_state
    from waitdie_ref import replay_epoch, replay_release
    b, ts = big_ycsb()
    rc, pos = new_state(b.n_txn)
    e1 = replay_epoch(b, ts, rc, pos)
    leave = np.isin(e1[0], [RC_RCOK, RC_ABORT]).astype(np.uint8)
    r1 = replay_release(b, ts, e1[0], e1[1], leave)
    e2 = replay_epoch(b, ts, r1[0], r1[1])
    return b, ts, e1, leave, r1, e2


CALVIN_WIDE_BITS = 40


@functools.lru_cache(maxsize=None)
def big_calvin_keys():
    """(batch, (group, rc, wave)): the YCSB batch with its keys mapped to 40
    varying bits, more than the 32 a u32 key sort holds."""
    import _oracle as orc
    b, _ = big_ycsb()
    low = int(b.keys.max()).bit_length()
    if int(b.keys.max()) == (1 << low) - 1:
        low += 1
    wb = mapped(b, varying(CALVIN_WIDE_BITS, low))
    return wb, orc.calvin(wb)


@functools.lru_cache(maxsize=None)
def big_calvin_order():
    """(batch, (group, rc, wave)): RS_SMALL + 1 one-access txns on 4,096 rows
    under a random 63-bit order."""
    import _oracle as orc
    from deneva_amd import RD, WR
    n = RS_SMALL + 1
    rng = np.random.default_rng(n)
    b = EpochBatch(np.arange(n + 1, dtype=np.uint32), rng.integers(0, 4096, size=n).astype(np.uint64),
                   rng.choice(np.asarray([RD, WR], np.uint8), size=n, p=[0.7, 0.3]), None, None,
                   rng.integers(0, 1 << 63, size=n, dtype=np.uint64))
    return b, orc.calvin(b)


HIST_PAIRS = RS_SMALL + 16
HIST_FIRST = 16  # pairs appended first, above every later tn: the level is no longer tn-ordered
HIST_TNC = 1 << 20


@functools.lru_cache(maxsize=None)
def big_history(two_sorts):
    """(appends [(keys, tn)], epoch batch, (rc, tn, tnc) of the oracle, (keys,
    tn) of the whole history).  One append of HIST_PAIRS pairs over 2^18 random
    64-bit keys (KEY_RESERVED - 1 among them), several tns per key in no
    order.  An append is sorted by tn on the host, so a level of one append
    builds with one sort by key; with two_sorts, HIST_FIRST pairs of larger
    tns go in first, and the level needs the (tn, then key) build.  The
    epoch's windows are wide enough that the history decides many txns."""
    import _oracle as orc
    from deneva_amd import RD, WR
    rng = np.random.default_rng(HIST_PAIRS + two_sorts)
    pool = np.unique(rng.integers(0, M64 - 1, size=1 << 18, dtype=np.uint64, endpoint=True))
    pool[-1] = M64 - 1
    k = pool[rng.integers(0, pool.size, size=HIST_PAIRS)]
    t = rng.integers(1, HIST_TNC, size=HIST_PAIRS).astype(np.uint64)
    appends = [(k, t)]
    if two_sorts:
        appends.insert(0, (pool[rng.integers(0, pool.size, size=HIST_FIRST)],
                           np.full(HIST_FIRST, HIST_TNC, np.uint64) - np.arange(HIST_FIRST, dtype=np.uint64)))
    n = 4096
    lens = rng.integers(1, 9, size=n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    m = int(off[-1])
    b = EpochBatch(off, pool[rng.integers(0, pool.size, size=m)],
                   rng.choice(np.asarray([RD, WR], np.uint8), size=m, p=[0.7, 0.3]))
    b.start_tn = rng.integers(0, HIST_TNC, size=n).astype(np.uint64)
    b.finish_tn = b.start_tn + rng.integers(0, 1 << 14, size=n).astype(np.uint64)
    hk = np.concatenate([a[0] for a in appends])
    ht = np.concatenate([a[1] for a in appends])
    return appends, b, orc.occ(b, hist_keys=hk, hist_tn=ht, tnc=HIST_TNC), (hk, ht)
