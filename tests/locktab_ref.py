"""Literal reference of the NO_WAIT lock table that lives across epochs
(dcc_locktab_*): Row_lock's `lock_type` / `owner_cnt` per row
(concurrency_control/row_lock.cpp) kept over calls.

lock_epoch is nowait_ref.replay's loop on the persistent state: the txns run
get_row in index order and list order, an aborted txn releases what it took, a
committed one keeps every grant.  release is lock_release (row_lock.cpp:240-256)
for every access of the selected txns; the reference's assert(owner_cnt > 0) is
an OverRelease here, raised before anything changes.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RD, SCAN
from nowait_ref import LOCK_EX, LOCK_NONE, LOCK_SH


class OverRelease(Exception):
    """The releases of one call name a row more often than it is held."""


def lock_of(t):
    return LOCK_SH if (t == RD or t == SCAN) else LOCK_EX  # row.cpp:228


class LockTable:
    def __init__(self):
        self.lock_type = {}  # row -> lock_t (absent: LOCK_NONE)
        self.owner_cnt = {}  # row -> owners

    def lock_epoch(self, batch):
        """Returns (rc u8[n], conflict u32[n]); the grants of the committed txns stay."""
        off = np.asarray(batch.offsets).tolist()
        keys = np.asarray(batch.keys).tolist()
        at = np.asarray(batch.acctype).tolist()
        n = len(off) - 1
        lock_type, owner_cnt = self.lock_type, self.owner_cnt
        rc = [RC_RCOK] * n
        conflict = [ACCESS_NONE] * n
        for i in range(n):
            a0 = off[i]
            taken = []
            for a in range(a0, off[i + 1]):
                k = keys[a]
                lt = lock_of(at[a])
                cur = lock_type.get(k, LOCK_NONE)
                # conflict_lock(lock_type, type), row_lock.cpp:69, 374-381
                if cur != LOCK_NONE and (cur == LOCK_EX or lt == LOCK_EX):
                    # NO_WAIT: rc = Abort (row_lock.cpp:86-90); cleanup releases
                    # what the txn took (system/txn.cpp:747-761), newest first
                    rc[i] = RC_ABORT
                    conflict[i] = a - a0
                    for r in reversed(taken):
                        self._release_one(r)
                    break
                # granted, row_lock.cpp:183-195: owner_cnt++, lock_type = type
                owner_cnt[k] = owner_cnt.get(k, 0) + 1
                lock_type[k] = lt
                taken.append(k)
        return np.asarray(rc, np.uint8), np.asarray(conflict, np.uint32)

    def _release_one(self, k):
        # lock_release, row_lock.cpp:240-256
        c = self.owner_cnt[k] - 1
        self.owner_cnt[k] = c
        if c == 0:
            self.lock_type[k] = LOCK_NONE

    def release_rows(self, keys):
        """lock_release once per entry; OverRelease, with the state unchanged, if
        the entries together name a row more often than it is held."""
        keys = np.asarray(keys).tolist()
        for k, c in Counter(keys).items():
            if c > self.owner_cnt.get(k, 0):
                raise OverRelease(f"row {k}: {c} releases of {self.owner_cnt.get(k, 0)} owners")
        for k in keys:
            self._release_one(k)

    def release(self, batch, rc=None, want=RC_RCOK):
        """Every access of the txns with rc[i] == want (rc None: of every txn).
        Returns (txns, accesses) released."""
        off = np.asarray(batch.offsets).astype(np.int64)
        if off.size < 1 or off[0] != 0 or off[-1] != np.asarray(batch.keys).size or np.any(np.diff(off) < 0):
            raise ValueError("malformed offsets")
        lens = np.diff(off)
        sel = np.ones(lens.size, bool) if rc is None else np.asarray(rc)[:lens.size] == want
        keys = np.asarray(batch.keys)[np.repeat(sel, lens)]
        self.release_rows(keys)
        return int(sel.sum()), int(keys.size)

    def acquire_rows(self, keys, acctype):
        """As the held prefix of nowait_ref.replay: EX if any entry of the row is
        EX, the count up by one per entry."""
        for k, t in zip(np.asarray(keys).tolist(), np.asarray(acctype).tolist()):
            self.owner_cnt[k] = self.owner_cnt.get(k, 0) + 1
            if self.lock_type.get(k, LOCK_NONE) != LOCK_EX:
                self.lock_type[k] = lock_of(t)

    def export(self):
        """{row: (lock_type, owner_cnt)} of the rows with owner_cnt > 0."""
        return {k: (self.lock_type[k], c) for k, c in self.owner_cnt.items() if c > 0}

    def clear(self):
        self.lock_type.clear()
        self.owner_cnt.clear()


def held_list(state):
    """An export as the held list of nowait_ref.replay / dcc_nowait_lock_epoch:
    a row with count c becomes c entries of its type."""
    ks, ts = [], []
    for k, (lt, c) in state.items():
        ks += [k] * c
        ts += [1 if lt == LOCK_EX else 0] * c  # WR / RD
    return np.asarray(ks, np.uint64), np.asarray(ts, np.uint8)
