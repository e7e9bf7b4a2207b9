"""Literal replay of Row_lock in NO_WAIT mode at the three isolation levels:
the parity reference of dcc_nowait_lock_epoch / dcc_locktab_* with DCC_ISO_*.

The txns run get_row txn by txn in index order and access by access in list
order against `lock_type` / `owner_cnt` per row (row_lock.cpp:52-256), as
nowait_ref.replay does.  The levels differ only in the releases:

  READ_COMMITTED    a granted RD/SCAN does lock_release at once
                    (ycsb_txn.cpp:233-236, txn.cpp:692-698); cleanup at abort
                    releases the EX rows only (txn.cpp:720-723); a committed
                    txn holds its EX rows.
  READ_UNCOMMITTED  every granted request does lock_release at once
                    (ycsb_txn.cpp:248-251); cleanup releases nothing
                    (txn.cpp:708); a committed txn holds nothing.

closed_form() is written from the closed forms of DESIGN.md §8q, not from the
replay.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from deneva_amd import (ACCESS_NONE, ISO_READ_COMMITTED, ISO_READ_UNCOMMITTED, ISO_SERIALIZABLE, RC_ABORT,
                        RC_RCOK, RD, SCAN)
from locktab_ref import OverRelease
from nowait_ref import LOCK_EX, LOCK_NONE, LOCK_SH

SER, RCL, RUL = ISO_SERIALIZABLE, ISO_READ_COMMITTED, ISO_READ_UNCOMMITTED
LEVELS = (SER, RCL, RUL)


def lock_of(t):
    return LOCK_SH if (t == RD or t == SCAN) else LOCK_EX  # row.cpp:228


class Table:
    """lock_type / owner_cnt per row, kept over calls (the lock-table handle)."""

    def __init__(self):
        self.lock_type = {}
        self.owner_cnt = {}

    def _get(self, k, lt):
        """lock_get in NO_WAIT mode: False is Abort (row_lock.cpp:69, 86-90)."""
        cur = self.lock_type.get(k, LOCK_NONE)
        if cur != LOCK_NONE and (cur == LOCK_EX or lt == LOCK_EX):
            return False
        self.owner_cnt[k] = self.owner_cnt.get(k, 0) + 1  # row_lock.cpp:183-195
        self.lock_type[k] = lt
        return True

    def _release_one(self, k):
        c = self.owner_cnt[k] - 1  # lock_release, row_lock.cpp:240-256
        self.owner_cnt[k] = c
        if c == 0:
            self.lock_type[k] = LOCK_NONE

    def acquire_rows(self, keys, acctype):
        for k, t in zip(np.asarray(keys).tolist(), np.asarray(acctype).tolist()):
            self.owner_cnt[k] = self.owner_cnt.get(k, 0) + 1
            if self.lock_type.get(k, LOCK_NONE) != LOCK_EX:
                self.lock_type[k] = lock_of(t)

    def lock_epoch(self, batch, level=SER):
        """Returns (rc u8[n], conflict u32[n]); what the committed txns still
        hold at `level` stays."""
        off = np.asarray(batch.offsets).tolist()
        keys = np.asarray(batch.keys).tolist()
        at = np.asarray(batch.acctype).tolist()
        n = len(off) - 1
        rc = [RC_RCOK] * n
        conflict = [ACCESS_NONE] * n
        for i in range(n):
            a0 = off[i]
            taken = []  # (row, lock type) still held by the txn
            for a in range(a0, off[i + 1]):
                k, lt = keys[a], lock_of(at[a])
                if not self._get(k, lt):
                    rc[i] = RC_ABORT
                    conflict[i] = a - a0
                    for r, rt in reversed(taken):  # cleanup
                        if level == SER or (level == RCL and rt == LOCK_EX):
                            self._release_one(r)
                    break
                if level == RUL or (level == RCL and lt == LOCK_SH):
                    self._release_one(k)  # release_last_row_lock
                else:
                    taken.append((k, lt))
        return np.asarray(rc, np.uint8), np.asarray(conflict, np.uint32)

    def release(self, batch, rc=None, want=RC_RCOK, level=SER):
        """The accesses of the txns with rc[i] == want that `level` still
        holds.  Returns (txns selected, accesses released); OverRelease with
        the state unchanged if they name a row more often than it is held."""
        off = np.asarray(batch.offsets).astype(np.int64)
        lens = np.diff(off)
        sel = np.ones(lens.size, bool) if rc is None else np.asarray(rc)[:lens.size] == want
        acc = np.repeat(sel, lens)
        at = np.asarray(batch.acctype)
        if level == RCL:
            acc &= (at != RD) & (at != SCAN)
        elif level == RUL:
            acc &= False
        keys = np.asarray(batch.keys)[acc].tolist()
        for k, c in Counter(keys).items():
            if c > self.owner_cnt.get(k, 0):
                raise OverRelease(f"row {k}: {c} releases of {self.owner_cnt.get(k, 0)} owners")
        for k in keys:
            self._release_one(k)
        return int(sel.sum()), len(keys)

    def export(self):
        return {k: (self.lock_type[k], c) for k, c in self.owner_cnt.items() if c > 0}


def replay(batch, held=None, level=SER):
    """Returns (rc u8[n], conflict u32[n]).  held = (keys, acctype): the state
    of the table before txn 0, never released."""
    t = Table()
    if held is not None:
        t.acquire_rows(held[0], held[1])
    return t.lock_epoch(batch, level)


def closed_form(batch, held=None, level=RCL):
    """The closed forms of READ_COMMITTED and READ_UNCOMMITTED."""
    assert level in (RCL, RUL)
    off = np.asarray(batch.offsets).tolist()
    keys = np.asarray(batch.keys).tolist()
    at = np.asarray(batch.acctype).tolist()
    n = len(off) - 1
    held_any, held_ex = set(), set()
    if held is not None:
        for k, t in zip(np.asarray(held[0]).tolist(), np.asarray(held[1]).tolist()):
            held_any.add(k)
            if t != RD and t != SCAN:
                held_ex.add(k)
    written = set()  # rows with an EX access of a committed txn below i
    rc = np.full(n, RC_RCOK, np.uint8)
    conflict = np.full(n, ACCESS_NONE, np.uint32)
    for i in range(n):
        own_ex = set()  # rows with an EX access of i at a lower ordinal
        first = None
        for a in range(off[i], off[i + 1]):
            k = keys[a]
            ex = at[a] != RD and at[a] != SCAN
            bad = k in held_ex or (ex and k in held_any)  # (2), (3)
            if level == RCL:
                bad = bad or k in own_ex or k in written  # (1), (4)
            if bad:
                first = a - off[i]
                break
            if ex:
                own_ex.add(k)
        if first is None:
            if level == RCL:
                written |= own_ex
        else:
            rc[i] = RC_ABORT
            conflict[i] = first
    return rc, conflict
