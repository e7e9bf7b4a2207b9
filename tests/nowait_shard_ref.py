"""The key-sharded NO_WAIT lock epoch in plain Python, written
from the argument there and not from the kernels: R ranks, each with the lock
table of the rows `key_shard(key, R)` gives it, every rank holding the whole
batch and the whole held list.

Owner words are tag:6 | index:26 with the txn index shifted by one: tag 0 | 0
a held row, tag 0 | i + 1 a committed requester, round tag | i + 1 an
undecided one.  A table keeps two minima per row: over every requester (`own`,
read by an EX request) and over the EX requesters (`aux`, read by an SH one).

A round: every rank evaluates its own accesses of every undecided txn into a
status byte (0 none, 1 blocked, 2 killed); the bytes are reduced with
np.maximum; every rank applies the reduced byte.  After the fixed point the
ranks reduce 64 - ordinal of their first conflicting request the same way.

`selfc` chooses how a txn that names a row twice with EX on either side is
handled (only the row's rank can see it):
  "round1"  the design's choice: the row's rank marks the txn's status byte
            killed; the other ranks learn of it in round 1's exchange, their
            round-1 words of the txn block its readers for that round only
  "pre"     an exchange of its own before any round-1 word is published
  "silent"  the row's rank aborts the txn and tells nobody (no handling: the
            ranks' state bytes part, which the model reports)
"""
from __future__ import annotations

import numpy as np

from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RD, SCAN

IDX_BITS = 26
IDX_MASK = (1 << IDX_BITS) - 1
EMPTY = 0xFFFFFFFF
MAX_TAG_ROUND = 62
MAX_TXN_LEN = 64
UNDECIDED, COMMIT, ABORT = 0, 1, 2
NONE, BLOCKED, KILLED = 0, 1, 2


class RanksDisagree(AssertionError):
    pass


def round_tag(r):
    return 63 - r


def is_ex(t):
    return not (t == RD or t == SCAN)


class Rank:
    """One rank: its rows' words and its own accesses of every txn."""

    def __init__(self, n):
        self.own = {}
        self.aux = {}
        self.acc = [[] for _ in range(n)]  # per txn: (ordinal in the whole txn, key, ex)
        self.selfc = [False] * n
        self.state = [UNDECIDED] * n

    def publish(self, t, word):
        for _, k, ex in self.acc[t]:
            self.own[k] = min(self.own.get(k, EMPTY), word)
            if ex:
                self.aux[k] = min(self.aux.get(k, EMPTY), word)

    def word(self, k, ex):
        return (self.own if ex else self.aux).get(k, EMPTY)

    def status(self, t, tag):
        st = NONE
        for _, k, ex in self.acc[t]:
            w = self.word(k, ex)
            wt, idx = w >> IDX_BITS, w & IDX_MASK
            if wt == 0 and idx < t + 1:
                return KILLED
            if wt == tag and idx < t + 1:
                st = BLOCKED
        return st

    def retag(self):
        for tab in (self.own, self.aux):
            for k, w in tab.items():
                if w >> IDX_BITS:
                    tab[k] = EMPTY

    def first_conflict(self, t):
        """64 - the ordinal of the first of this rank's requests of txn t that
        names a row again with EX on either side, or meets a held row or a
        committed txn below t; 0: none here."""
        seen = []
        for o, k, ex in self.acc[t]:
            w = self.word(k, ex)
            if any(k == k2 and (ex or ex2) for k2, ex2 in seen) or \
                    ((w >> IDX_BITS) == 0 and (w & IDX_MASK) < t + 1):
                return MAX_TXN_LEN - o
            seen.append((k, ex))
        return 0


def sharded_epoch(batch, held, R, key_shard, selfc="round1"):
    """Returns (rc u8[n], conflict u32[n], info); info: rounds, collectives,
    bytes exchanged per rank, the ranks' own request and held-row counts."""
    off = np.asarray(batch.offsets).tolist()
    keys = np.asarray(batch.keys).tolist()
    at = np.asarray(batch.acctype).tolist()
    n = len(off) - 1
    info = {"rounds": 0, "collectives": 0, "bytes": 0, "own": [0] * R, "own_held": [0] * R}
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(0, np.uint32), info
    assert max(off[i + 1] - off[i] for i in range(n)) <= MAX_TXN_LEN
    ranks = [Rank(n) for _ in range(R)]
    shard = {}

    def owner(k):
        if k not in shard:
            shard[k] = key_shard(k, R) if R > 1 else 0
        return shard[k]

    def reduce(per_rank):
        info["collectives"] += 1
        info["bytes"] += n
        return np.maximum.reduce(np.asarray(per_rank, np.uint8), axis=0)

    # ---- build: held rows, then every rank's own requests; self-conflicts
    if held is not None:
        for k, t in zip(np.asarray(held[0]).tolist(), np.asarray(held[1]).tolist()):
            rk = ranks[owner(k)]
            info["own_held"][owner(k)] += 1
            rk.own[k] = 0
            if is_ex(t):
                rk.aux[k] = 0
    for t in range(n):
        for o, x in enumerate(range(off[t], off[t + 1])):
            r = owner(keys[x])
            rk = ranks[r]
            ex = is_ex(at[x])
            if any(k2 == keys[x] and (ex or ex2) for _, k2, ex2 in rk.acc[t]):
                rk.selfc[t] = True
            rk.acc[t].append((o, keys[x], ex))
            info["own"][r] += 1
    if selfc == "pre":  # every rank knows before a round-1 word exists
        known = reduce([[KILLED if rk.selfc[t] else NONE for t in range(n)] for rk in ranks])
        for rk in ranks:
            for t in range(n):
                if known[t]:
                    rk.state[t] = ABORT
    for rk in ranks:
        for t in range(n):
            if rk.selfc[t] and selfc == "silent":
                rk.state[t] = ABORT
            if rk.state[t] == UNDECIDED and not rk.selfc[t]:  # a txn aborted here publishes nothing here
                rk.publish(t, (round_tag(1) << IDX_BITS) | (t + 1))

    # ---- rounds
    und = list(range(n))
    r = 0
    while und:
        r += 1
        if r > n + 2:
            raise AssertionError("the fixed point did not converge")
        er = (r - 1) % MAX_TAG_ROUND + 1
        tag = round_tag(er)
        if r > 1:
            for rk in ranks:
                if er == 1:
                    rk.retag()
                for t in und:
                    rk.publish(t, (tag << IDX_BITS) | (t + 1))
        status = []
        for rk in ranks:
            row = [NONE] * n
            for t in und:
                if rk.state[t] != UNDECIDED:
                    continue
                if r == 1 and rk.selfc[t] and selfc == "round1":
                    row[t] = KILLED
                else:
                    row[t] = rk.status(t, tag)
            status.append(row)
        red = reduce(status)
        nxt = None
        for rk in ranks:
            mine = []
            for t in und:
                if rk.state[t] != UNDECIDED:
                    continue
                if red[t] == KILLED:
                    rk.state[t] = ABORT
                elif red[t] == NONE:
                    rk.state[t] = COMMIT
                    rk.publish(t, t + 1)
                else:
                    mine.append(t)
            if nxt is not None and mine != nxt:
                raise RanksDisagree(f"round {r}: the ranks' undecided lists differ")
            nxt = mine
        for rk in ranks[1:]:
            if rk.state != ranks[0].state:
                raise RanksDisagree(f"round {r}: the ranks' state bytes differ")
        und = nxt
    info["rounds"] = max(r, 1)

    # ---- the request each aborted txn aborted at
    state = ranks[0].state
    red = reduce([[rk.first_conflict(t) if state[t] == ABORT else 0 for t in range(n)] for rk in ranks])
    rc = np.where(np.asarray(state) == COMMIT, RC_RCOK, RC_ABORT).astype(np.uint8)
    conflict = np.full(n, ACCESS_NONE, np.uint32)
    for t in range(n):
        if state[t] == ABORT:
            if red[t] == 0:
                raise AssertionError(f"txn {t} aborted without a conflicting request on any rank")
            conflict[t] = MAX_TXN_LEN - int(red[t])
    return rc, conflict, info
