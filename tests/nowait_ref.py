"""Literal replay of Row_lock in NO_WAIT mode: the parity reference of
dcc_nowait_lock_epoch.

The txns of the batch run get_row for their accesses, txn by txn in index
order and access by access in list order (storage/row.cpp:226-238), against a
per-row `lock_type` / `owner_cnt` state (concurrency_control/row_lock.cpp).
NO_WAIT keeps no owner list (row_lock.cpp:176-182), so nothing here knows who
owns a row: a txn's own second request on a row meets the row's state like
anybody else's.
"""
from __future__ import annotations

import numpy as np

from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RD, SCAN

LOCK_EX, LOCK_SH, LOCK_NONE = 0, 1, 2  # lock_t, system/global.h:289


def replay(batch, held=None):
    """Returns (rc u8[n], conflict u32[n]).  held = (keys, acctype): rows still
    locked by txns of earlier epochs; they are taken first and never released."""
    off = np.asarray(batch.offsets).tolist()
    keys = np.asarray(batch.keys).tolist()
    at = np.asarray(batch.acctype).tolist()
    n = len(off) - 1
    lock_type = {}  # row -> lock_t (absent: LOCK_NONE)
    owner_cnt = {}  # row -> owners
    if held is not None:
        # owners of earlier epochs: a row is EX-held if any of its entries is EX
        for k, t in zip(np.asarray(held[0]).tolist(), np.asarray(held[1]).tolist()):
            lt = LOCK_SH if (t == RD or t == SCAN) else LOCK_EX
            owner_cnt[k] = owner_cnt.get(k, 0) + 1
            if lock_type.get(k, LOCK_NONE) != LOCK_EX:
                lock_type[k] = lt
    rc = [RC_RCOK] * n
    conflict = [ACCESS_NONE] * n
    get_type = lock_type.get
    get_cnt = owner_cnt.get
    for i in range(n):
        a0 = off[i]
        taken = []
        for a in range(a0, off[i + 1]):
            k = keys[a]
            t = at[a]
            lt = LOCK_SH if (t == RD or t == SCAN) else LOCK_EX  # row.cpp:228
            cur = get_type(k, LOCK_NONE)
            # conflict_lock(lock_type, type), row_lock.cpp:69, 374-381
            if cur != LOCK_NONE and (cur == LOCK_EX or lt == LOCK_EX):
                # NO_WAIT: rc = Abort (row_lock.cpp:86-90); the txn requests
                # nothing more and releases what it took (TxnManager::cleanup,
                # system/txn.cpp:747-761), newest first
                rc[i] = RC_ABORT
                conflict[i] = a - a0
                for r in reversed(taken):
                    # lock_release, row_lock.cpp:240-256
                    c = owner_cnt[r] - 1
                    owner_cnt[r] = c
                    if c == 0:
                        lock_type[r] = LOCK_NONE
                break
            # granted, row_lock.cpp:183-195: owner_cnt++, lock_type = type
            owner_cnt[k] = get_cnt(k, 0) + 1
            lock_type[k] = lt
            taken.append(k)
    return np.asarray(rc, np.uint8), np.asarray(conflict, np.uint32)
