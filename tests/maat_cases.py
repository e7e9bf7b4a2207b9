"""Directed cases for the MaaT epoch driver (csrc/maat.hip): each builder
returns (EpochBatch, seeded rows or None, facts) and names the branch of the
driver it forces -- long round sequences (the undecided ring, the batches of
rounds between host checks, the list and position compactions), both branches
of the prefix level and its filter, timestamps of 2^32 and more, and a row
group longer than one look-back window.

The expected results of a case always come from the oracle (_oracle.maat).
The Python model below restates only the driver's round rule; it supplies the
facts -- "this case needs r rounds", "this many txns survive the filter", "the
prefix has mp accesses" -- that test_maat_cases.py proves on the CPU, so a
case cannot silently stop forcing its branch.  Pure numpy: no GPU.
"""
from __future__ import annotations

import functools

import numpy as np

from deneva_amd import EpochBatch, RD, WR
from helpers import chain_batch, make_batch

# the engine's constants (test_maat_cases.py compares them with the sources)
MT_PREFIX = 1024   # txns of the prefix level; it runs for n > 4 * MT_PREFIX
MS_MAXPOS = 16384  # prefix accesses k_mt_small holds in LDS
MT_TILE = 4096     # sorted positions per scan tile
MT_RING = 64       # per-round undecided counters
MT_BATCH = 12      # rounds between host checks after the first
MAX_TXN_LEN = 64
MT_WALK = 256
RT_MIN_BITS = 12

UND, COM, ABO = 0, 1, 2
U64MAX = (1 << 64) - 1
_R, _W = 1, 2

WIDE_KINDS = ("lo32", "hi62", "full")


def seed_ts(rng, kind, size):
    """Row timestamps of the three wide ranges."""
    if kind == "lo32":
        return (np.uint64(1 << 32) + rng.integers(0, 50, size=size).astype(np.uint64))
    if kind == "hi62":
        return (np.uint64(1 << 62) + rng.integers(0, 50, size=size).astype(np.uint64))
    assert kind == "full"
    return rng.integers(0, 1 << 62, size=size).astype(np.uint64)


# ------------------------------------------------------------------ the model
def _prep(b, rows, rw_all):
    """base[t] and, per row, its (txn, R | W) groups in index order."""
    n = b.n_txn
    off = np.asarray(b.offsets).astype(np.int64)
    keys = np.asarray(b.keys, np.uint64)
    at = np.asarray(b.acctype)
    owner = np.repeat(np.arange(n), np.diff(off))
    bits = np.full(at.size, _R | _W) if rw_all else (at == RD) * _R + (at == WR) * _W
    uk, rid = np.unique(keys, return_inverse=True)
    lr = np.zeros(uk.size, np.uint64)
    lw = np.zeros(uk.size, np.uint64)
    if rows is not None and uk.size:
        rk = np.asarray(rows[0], np.uint64)
        pos = np.minimum(np.searchsorted(uk, rk), uk.size - 1)
        ok = uk[pos] == rk
        lr[pos[ok]] = np.asarray(rows[1], np.uint64)[ok]
        lw[pos[ok]] = np.asarray(rows[2], np.uint64)[ok]
    gw = np.zeros(n, np.uint64)
    gr = np.zeros(n, np.uint64)
    sel = bits > 0
    np.maximum.at(gw, owner[sel], lw[rid[sel]])
    wsel = (bits & _W) > 0
    np.maximum.at(gr, owner[wsel], lr[rid[wsel]])
    base = [int(x) + 1 for x in np.maximum(gw, gr).tolist()]
    rows_list = []
    gcount = [0] * n
    if sel.any():
        r_s, t_s, f_s = rid[sel], owner[sel], bits[sel]
        order = np.lexsort((t_s, r_s))
        r_s, t_s, f_s = r_s[order], t_s[order], f_s[order]
        starts = np.nonzero(np.r_[True, (r_s[1:] != r_s[:-1]) | (t_s[1:] != t_s[:-1])])[0]
        gf = np.bitwise_or.reduceat(f_s, starts)
        gt, grow = t_s[starts], r_s[starts]
        rb = np.nonzero(np.r_[True, grow[1:] != grow[:-1]])[0]
        for a, e in zip(rb.tolist(), np.r_[rb[1:], gt.size].tolist()):
            rows_list.append((gt[a:e].tolist(), gf[a:e].tolist()))
        gcount = np.bincount(gt, minlength=n).tolist()
    return base, rows_list, gcount


def _solve(rows_list, base, state, cts, txns, gcount=None, kept=0):
    """Rounds until every txn of `txns` is decided.  Per round and per row the
    groups in index order: rmax / wmin over committed readers / writers and
    the undecided bits, all from the state at the round's start.  Returns the
    undecided count and the kept-group count after each round."""
    und_list = [t for t in txns if state[t] == UND]
    active = rows_list
    und_hist, kept_hist = [], []
    while True:
        active = [r for r in active if any(state[t] == UND for t in r[0])]
        lacc, uacc, pend = {}, {}, set()
        for txs, fls in active:
            rmax, wmin, und = 0, U64MAX, 0
            for t, f in zip(txs, fls):
                s = state[t]
                if s == UND:
                    if (f & _W) and rmax and rmax + 1 > lacc.get(t, 0):
                        lacc[t] = rmax + 1
                    if wmin != U64MAX and wmin - 1 < uacc.get(t, U64MAX):
                        uacc[t] = wmin - 1
                    if (und & _W) or ((f & _W) and (und & _R)):
                        pend.add(t)
                    und |= f
                elif s == COM:
                    c = cts[t]
                    if (f & _R) and c > rmax:
                        rmax = c
                    if (f & _W) and c < wmin:
                        wmin = c
        left = []
        for t in und_list:
            L, U = max(base[t], lacc.get(t, 0)), uacc.get(t, U64MAX)
            if L >= U:
                state[t] = ABO
                if gcount is not None:
                    kept -= gcount[t]
            elif t not in pend:
                state[t] = COM
                cts[t] = L
            else:
                left.append(t)
        und_list = left
        und_hist.append(len(und_list))
        kept_hist.append(kept)
        if not und_list:
            return und_hist, kept_hist


def driver_checks(m, n, und_hist, kept_hist):
    """The host checks of the driver's one-level schedule (after round 1, then
    every MT_BATCH rounds) that do not end the epoch: (round, list compacted,
    positions compacted)."""
    out, mc, ulen, r, nb = [], m, n, 0, 1
    while True:
        r += nb
        nb = MT_BATCH
        if r >= len(und_hist):
            return out
        und, kept = und_hist[r - 1], kept_hist[r - 1]
        lc = und * 10 < ulen * 3
        if lc:
            ulen = und
        pc = mc > 0 and kept * 10 <= mc * 9
        if pc:
            mc = kept
        out.append((r, lc, pc))


def model(b, rows=None, rw_all=False):
    """The one-level schedule (n <= 4 * MT_PREFIX)."""
    base, rows_list, gcount = _prep(b, rows, rw_all)
    n = b.n_txn
    state, cts = [UND] * n, [0] * n
    und_hist, kept_hist = _solve(rows_list, base, state, cts, range(n), gcount, sum(gcount))
    return {"rounds": len(und_hist), "state": np.asarray(state, np.uint8), "cts": np.asarray(cts, np.uint64),
            "und": und_hist, "kept": kept_hist, "checks": driver_checks(b.nnz, n, und_hist, kept_hist)}


def model_prefix(b, rows=None, rw_all=False):
    """The prefix level: txns [0, MT_PREFIX) decided alone, the later txns
    filtered against the committed prefix with the same bounds, then rounds
    on the survivors."""
    base, rows_list, _ = _prep(b, rows, rw_all)
    n, P = b.n_txn, MT_PREFIX
    assert n > P
    state, cts = [UND] * n, [0] * n
    pre = []
    for txs, fls in rows_list:
        k = sum(1 for t in txs if t < P)
        if k:
            pre.append((txs[:k], fls[:k]))
    und1, _ = _solve(pre, base, state, cts, range(P))
    lacc, uacc = {}, {}
    for txs, fls in rows_list:
        rmax, wmin = 0, U64MAX
        for t, f in zip(txs, fls):
            if t < P:
                if state[t] == COM:
                    if f & _R:
                        rmax = max(rmax, cts[t])
                    if f & _W:
                        wmin = min(wmin, cts[t])
            else:
                if (f & _W) and rmax:
                    lacc[t] = max(lacc.get(t, 0), rmax + 1)
                if wmin != U64MAX:
                    uacc[t] = min(uacc.get(t, U64MAX), wmin - 1)
    for t in range(P, n):
        if max(base[t], lacc.get(t, 0)) >= uacc.get(t, U64MAX):
            state[t] = ABO
    surv = [t for t in range(P, n) if state[t] == UND]
    und2 = _solve(rows_list, base, state, cts, surv)[0] if surv else []
    return {"mp": int(np.asarray(b.offsets)[P]), "prefix_rounds": len(und1), "survivors": surv,
            "nsurv": len(surv), "surv_rounds": len(und2), "state": np.asarray(state, np.uint8),
            "cts": np.asarray(cts, np.uint64)}


def takes_prefix(b):
    return b.nnz != 0 and b.n_txn > 4 * MT_PREFIX


# ------------------------------------------------------------------ builders
def _ragged(rng, n, max_len, n_keys, p_write, key0=0, min_len=0):
    """n txns of min_len..max_len accesses, keys uniform in [key0, key0 + n_keys)
    (a txn may name a key twice), as three arrays."""
    lens = rng.integers(min_len, max_len + 1, size=n)
    tot = int(lens.sum())
    keys = (rng.integers(0, n_keys, size=tot) + key0).astype(np.uint64)
    at = np.where(rng.random(tot) < p_write, WR, RD).astype(np.uint8)
    return lens, keys, at


def _join(parts):
    """(lens, keys, acctype) parts, in order, into one batch."""
    lens = np.concatenate([np.asarray(p[0], np.int64) for p in parts])
    keys = np.concatenate([np.asarray(p[1], np.uint64) for p in parts])
    at = np.concatenate([np.asarray(p[2], np.uint8) for p in parts])
    off = np.zeros(lens.size + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    return EpochBatch(off, keys, at)


def _independents(count, key0):
    """Txns of private rows; half of them name a key several times (RD then
    WR, RD twice and more), so their groups have more than one position."""
    txns = []
    for i in range(count):
        k, k2 = key0 + 2 * i, key0 + 2 * i + 1
        txns.append(([(k, RD), (k, RD), (k, RD), (k, WR)], [(k, RD)] * 4, [(k, WR)],
                     [(k, RD), (k2, WR), (k, RD), (k, RD)])[i % 4])
    return txns


def _seed_all(b, kind, seed, skip=None):
    rk = np.unique(np.asarray(b.keys, np.uint64))
    if skip is not None:
        rk = rk[~skip(rk)]
    rng = np.random.default_rng(seed)
    return rk, seed_ts(rng, kind, rk.size), seed_ts(rng, kind, rk.size)


CHAIN_C = (64, 65, 73, 74, 129, 300)


@functools.lru_cache(maxsize=None)
def chain(c):
    """helpers.chain_batch alone: exactly c rounds.  The ring of MT_RING
    counters wraps once (64, 65, 73, 74), twice (129) and four times (300);
    c = 73 ends exactly at a host check (rounds 1 + 12 k) and c = 74 one round
    into a batch, so eleven rounds that find nothing to do follow."""
    return chain_batch(c), None, {"rounds": c}


COMPOSITE_C = (64, 65, 73, 74)
_H, _PRIV, _CH, _CPRIV, _IND = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20


@functools.lru_cache(maxsize=None)
def composite(c, k=1500, ind=500, wide=None):
    """Txn 0 writes hot row H; k txns read H and write a private row (they
    wait in round 1 and abort in round 2); a chain of c (each chain txn also
    writes 8 private rows); `ind` independents.  c rounds.  The independents'
    repeated keys drop the kept positions by more than 10 % at the first host
    check, the k aborts at the second and the chain's aborts later on: the
    position compaction runs into both buffer sets and back; the undecided
    count at the second check is a few dozen of n, which compacts the list.
    wide: every row but the readers' private ones seeded from that range,
    H's last write above its last read so the readers still abort."""
    txns = [[(_H, WR)]]
    txns += [[(_H, RD), (_PRIV + j, WR)] for j in range(k)]
    for i in range(c):
        t = [(_CH + i, WR)] if i == 0 else [(_CH + i - 1, RD), (_CH + i, WR)]
        txns.append(t + [(_CPRIV + 8 * i + q, WR) for q in range(8)])
    txns += _independents(ind, _IND)
    b = make_batch(txns)
    rows = None
    if wide:
        rk, lr, lw = _seed_all(b, wide, 0xC0 + c, skip=lambda x: (x >= _PRIV) & (x < _CH))
        h = int(np.searchsorted(rk, np.uint64(_H)))
        lr[h], lw[h] = min(lr[h], lw[h]), max(lr[h], lw[h])
        rows = (rk, lr, lw)
    return b, rows, {"rounds": c, "n": 1 + k + c + ind, "readers": (1, 1 + k), "chain": (1 + k, 1 + k + c)}


@functools.lru_cache(maxsize=None)
def wide_ts(kind):
    """A random batch of 1,500 txns over 300 rows whose seeded timestamps are
    all from one wide range: some commit timestamp is >= 2^32."""
    rng = np.random.default_rng(0x7300 + WIDE_KINDS.index(kind))
    b = _join([_ragged(rng, 1500, 8, 300, 0.3)])
    rk = np.arange(300, dtype=np.uint64)
    rows = (rk, seed_ts(rng, kind, 300), seed_ts(rng, kind, 300))
    return b, rows, {"rounds": model(b, rows)["rounds"], "min_max_cts": 1 << 32}


@functools.lru_cache(maxsize=None)
def prefix_gate(extra):
    """The same 4,096 txns (rows seeded at 2^32 and up) alone, n = 4 *
    MT_PREFIX, and with one more independent single write, n = 4 * MT_PREFIX +
    1: one input on both sides of the prefix level's gate."""
    rng = np.random.default_rng(0x6A7E)
    parts = [_ragged(rng, 4 * MT_PREFIX, 10, 6000, 0.3)]
    if extra:
        parts.append(([1], [1 << 30], [WR]))
    b = _join(parts)
    rk = np.arange(6000, dtype=np.uint64)
    rows = (rk, seed_ts(rng, "lo32", 6000), seed_ts(rng, "lo32", 6000))
    facts = {"prefix": bool(extra)}
    if not extra:
        facts["rounds"] = model(b, rows)["rounds"]
    return b, rows, facts


@functools.lru_cache(maxsize=None)
def prefix_small_cap(extra):
    """1,024 prefix txns of 16 accesses: mp = MS_MAXPOS, k_mt_small at its
    cap; with one access more on one prefix txn mp = MS_MAXPOS + 1, the
    k_mt_iota + solve branch.  3,200 later txns conflict with the prefix and
    among themselves in both."""
    rng = np.random.default_rng(0x5CA9)
    lens, keys, at = _ragged(rng, MT_PREFIX, 16, 30000, 0.25, min_len=16)
    later = _ragged(rng, 3200, 6, 60000, 0.3, min_len=1)
    parts = [(lens, keys, at), later]
    if extra:
        t = 500  # a 17th access (a cold read) on prefix txn 500
        lens = lens.copy()
        lens[t] += 1
        keys = np.insert(keys, 16 * t + 16, np.uint64(1 << 30))
        at = np.insert(at, 16 * t + 16, np.uint8(RD))
        parts = [(lens, keys, at), later]
    return _join(parts), None, {"mp": MS_MAXPOS + extra}


@functools.lru_cache(maxsize=None)
def prefix_chain(shift, wide=None):
    """A chain from txn `shift` (0 or 1) to txn 1,200, padded to n = 4,097
    with independents: k_mt_small runs about 1,024 rounds in one workgroup,
    the decision of txn 1,023 flips with the shift, so txn 1,024 is once
    killed by the filter and once a survivor, and the chain goes on among the
    survivors."""
    txns = [[(_IND - 1, WR)]] * shift
    for i in range(1201 - shift):
        txns.append([(_CH + i, WR)] if i == 0 else [(_CH + i - 1, RD), (_CH + i, WR)])
    txns += _independents(4 * MT_PREFIX + 1 - len(txns), _IND)
    b = make_batch(txns)
    rows = _seed_all(b, wide, 0xC4A1 + shift) if wide else None
    return b, rows, {"shift": shift}


@functools.lru_cache(maxsize=None)
def prefix_two_rows():
    """Later txn X writes row A and reads row B.  A is read by a committed
    prefix txn with cts 10 (L = 11), B is written by one with cts 11 (U = 10):
    X aborts only by combining both rows.  Its twin's prefix writer has cts 13
    (U = 12), so the twin commits at 11.  The prefix cts come from seeded rows."""
    A, B, A2, B2, PA, PA2 = 10, 11, 20, 21, 30, 31
    txns = _independents(4 * MT_PREFIX + 1, _IND)
    ra, wb, ra2, wb2, X, X2 = 17, 900, 1023, 3, 2000, 4096
    txns[ra] = [(A, RD), (PA, RD)]
    txns[wb] = [(B, WR)]
    txns[ra2] = [(PA2, RD), (A2, RD)]
    txns[wb2] = [(B2, WR)]
    txns[X] = [(A, WR), (B, RD)]
    txns[X2] = [(B2, RD), (A2, WR)]
    rk = np.array([PA, PA2, B, B2], np.uint64)
    lr = np.array([0, 0, 10, 12], np.uint64)
    lw = np.array([9, 9, 0, 0], np.uint64)
    return make_batch(txns), (rk, lr, lw), {"cts": {ra: 10, wb: 11, ra2: 10, wb2: 13, X2: 11}, "abort": X,
                                           "commit": X2}


@functools.lru_cache(maxsize=None)
def prefix_filter_boundary(gap):
    """The filter's bounds at their edge.  Every later txn writes row A (read
    by a committed prefix txn with cts 10: L = 11) and reads row B (written by
    one with cts 12 + gap: U = 11 + gap).  gap 0: L == U, the filter kills
    them all and the epoch ends with the prefix's rounds (a filter that folded
    the reader's cts and not cts + 1 would let them through to the survivor
    rounds: the same decisions one round later).  gap 1: all survive, the
    first commits at 11 and its write of A aborts the others."""
    A, B, PA = 10, 11, 30
    txns = _independents(MT_PREFIX, _IND)
    txns[5] = [(A, RD), (PA, RD)]
    txns[1000] = [(B, WR)]
    txns += [[(A, WR), (B, RD)] for _ in range(3 * MT_PREFIX + 1)]
    rows = (np.array([PA, B], np.uint64), np.array([0, 11 + gap], np.uint64), np.array([9, 0], np.uint64))
    return make_batch(txns), rows, {"nsurv": (3 * MT_PREFIX + 1) * gap, "cts": {5: 10, 1000: 12 + gap}}


@functools.lru_cache(maxsize=None)
def prefix_no_survivors():
    """Prefix txn 0 writes H and commits; every txn from 1,024 on reads H:
    all are killed by the filter, nsurv == 0, the survivor rounds are skipped."""
    txns = [[(_H, WR)]] + _independents(MT_PREFIX - 1, _IND)
    txns += [[(_PRIV + i, WR), (_H, RD)] for i in range(3 * MT_PREFIX + 1)]
    return make_batch(txns), None, {"nsurv": 0}


@functools.lru_cache(maxsize=None)
def prefix_empty():
    """The 1,024 prefix txns have no accesses (mp = 0); the 3,073 later ones
    have ordinary conflicts."""
    rng = np.random.default_rng(0xE)
    b = _join([(np.zeros(MT_PREFIX, np.int64), [], []), _ragged(rng, 3 * MT_PREFIX + 1, 8, 2000, 0.3)])
    return b, None, {"mp": 0}


@functools.lru_cache(maxsize=None)
def prefix_false_positives():
    """A prefix of 1,024 x 16 distinct rows, then 3,100 txns of 4 distinct
    cold rows each: the filter's 2^18-bit presence bitmap alone gives some 6 %
    false positives, and every such txn must survive and commit."""
    rng = np.random.default_rng(0xFA15E)
    npre, nl = MT_PREFIX * 16, 3100 * 4
    keys = rng.choice(1 << 40, size=npre + nl, replace=False).astype(np.uint64)
    at = np.where(rng.random(npre + nl) < 0.4, WR, RD).astype(np.uint8)
    lens = np.r_[np.full(MT_PREFIX, 16), np.full(3100, 4)]
    return _join([(lens, keys, at)]), None, {"nsurv": 3100}


LONG_N, LONG_W1 = 4400, 4300


@functools.lru_cache(maxsize=None)
def long_row(n=LONG_N, w1=LONG_W1):
    """Txn i reads hot row H 63 times and one private row seeded with lw =
    2^33 + i, so reader i commits at 2^33 + i + 1; W1 (index w1) and W2 (n - 1)
    blind-write H; the readers after W1 have private rows seeded low.  H's
    group is n x 63 positions with one row start (about 67 tiles at n =
    4,400): W1's cts is one more than reader w1 - 1's, 66 tiles behind the
    row's start flag, and the later readers' upper bound comes from W1."""
    lens = np.full(n, 64, np.int64)
    lens[[w1, n - 1]] = 1
    keys = np.full((n, 64), _H, np.uint64)
    keys[:, 63] = _PRIV + np.arange(n, dtype=np.uint64)
    at = np.full((n, 64), RD, np.uint8)
    sel = np.ones((n, 64), bool)
    for w in (w1, n - 1):
        at[w, 0] = WR
        sel[w, 1:] = False
    b = _join([(lens, keys[sel], at[sel])])
    idx = np.r_[np.arange(w1), np.arange(w1 + 1, n - 1)]
    rk = (_PRIV + idx).astype(np.uint64)
    lw = np.where(idx < w1, (1 << 33) + idx, 5).astype(np.uint64)
    return b, (rk, np.zeros(rk.size, np.uint64), lw), {"w1": w1, "w2": n - 1, "w1_cts": (1 << 33) + w1 + 1,
                                                       "h_positions": (n - 2) * 63 + 2}


# every case: id -> (builder, args).  DEV_CASES: one case per family that the
# GPU test also runs with device pointers; RW_ALL_CASES: those it also runs
# with DCC_MAAT_READ_AND_PREWRITE.
CASES = {}
for _c in CHAIN_C:
    CASES[f"chain-{_c}"] = (chain, (_c,))
for _c in COMPOSITE_C:
    CASES[f"composite-{_c}"] = (composite, (_c,))
CASES["composite-74-wide"] = (composite, (74, 1500, 500, "hi62"))
for _k in WIDE_KINDS:
    CASES[f"wide_ts-{_k}"] = (wide_ts, (_k,))
CASES["prefix_gate-4096"] = (prefix_gate, (0,))
CASES["prefix_gate-4097"] = (prefix_gate, (1,))
CASES["prefix_small_cap-16384"] = (prefix_small_cap, (0,))
CASES["prefix_small_cap-16385"] = (prefix_small_cap, (1,))
CASES["prefix_chain-0"] = (prefix_chain, (0,))
CASES["prefix_chain-1"] = (prefix_chain, (1,))
CASES["prefix_chain-1-wide"] = (prefix_chain, (1, "full"))
CASES["prefix_two_rows"] = (prefix_two_rows, ())
CASES["prefix_filter_boundary-0"] = (prefix_filter_boundary, (0,))
CASES["prefix_filter_boundary-1"] = (prefix_filter_boundary, (1,))
CASES["prefix_no_survivors"] = (prefix_no_survivors, ())
CASES["prefix_empty"] = (prefix_empty, ())
CASES["prefix_false_positives"] = (prefix_false_positives, ())
CASES["long_row"] = (long_row, ())

DEV_CASES = ("chain-74", "composite-73", "wide_ts-hi62", "prefix_gate-4097", "prefix_small_cap-16385",
             "prefix_chain-0", "prefix_two_rows", "prefix_filter_boundary-0", "prefix_no_survivors", "prefix_empty",
             "prefix_false_positives", "long_row")
RW_ALL_CASES = ("chain-73", "chain-129", "prefix_gate-4096", "prefix_gate-4097")


def build(name):
    fn, args = CASES[name]
    return fn(*args)


@functools.lru_cache(maxsize=None)
def expected_rounds(name, rw_all=False):
    """The driver's round count (dcc_stats.rounds): at the prefix level the
    prefix's rounds plus the survivors'."""
    b, rows, _ = build(name)
    if takes_prefix(b):
        m = model_prefix(b, rows, rw_all)
        return m["prefix_rounds"] + m["surv_rounds"]
    return model(b, rows, rw_all)["rounds"]
