"""Python restatement of the reference's abort queue (system/abort_queue.cpp:
26-82, abort_queue.h:37-42): the parity reference of the device queue
(abortq.hip, dcc_abortq_*, Engine.abort_queue).

The clock is an argument (the reference reads get_sys_clock(), lines 27 / 59).
A txn is parked with its accesses, its source identity and its abort count, not
only a txn id (lines 36-37): the device queue carries the batch itself.
"""
from __future__ import annotations

import heapq

import numpy as np

OK, EINVAL, ERANGE = 0, -22, -34
BACKOFF_REFERENCE, BACKOFF_NONE, BACKOFF_EXP = 0, 1, 2
U64, U32 = (1 << 64) - 1, (1 << 32) - 1


def penalty(policy, pen, pen_max, cnt):
    """abort_queue.cpp:28-31 in u64; cnt is abort_cnt after the increment of
    worker_thread.cpp:165."""
    p = pen & U64                                   # :28  penalty = g_abort_penalty
    if policy == BACKOFF_NONE:                      # :29  #if BACKOFF (false)
        return p
    if policy == BACKOFF_REFERENCE:
        # :30  penalty = max(penalty * 2^abort_cnt, g_abort_penalty_max): `^` is XOR
        # and binds looser than `*`, so this is max((penalty * 2) ^ abort_cnt, max)
        return max(((p * 2) & U64) ^ cnt, pen_max)
    # BACKOFF_EXP, the evident intent: min(penalty * 2**cnt, max); penalty_max when
    # cnt >= 64 or the shift loses bits
    if cnt >= 64 or (p << cnt) > U64:
        return pen_max
    return min(p << cnt, pen_max)


class AbortQueue:
    def __init__(self, cap_txn, cap_nnz, pen, pen_max, policy=BACKOFF_REFERENCE):
        self.cap_txn, self.cap_nnz = cap_txn, cap_nnz
        self.pen, self.pen_max, self.policy = pen, pen_max, policy
        self.heap = []   # (due, seq, src, cnt, keys, acctype): std::priority_queue on
        #                  penalty_end (abort_queue.h:37-42); seq settles the ties it leaves open
        self.seq = 0     # push ordinal over the queue's life
        self.nnz = 0

    def size(self):
        return len(self.heap), self.nnz

    def clear(self):
        self.heap, self.nnz = [], 0

    def push(self, batch, rc, want, src_in, cnt_in, now):
        """AbortQueue::enqueue (:26-50) for every txn with rc[i] == want, in index
        order.  Returns (code, n, nnz): what was parked, or what was needed."""
        off = np.asarray(batch.offsets).astype(np.int64)
        n = off.size - 1
        keys = np.asarray(batch.keys).astype(np.uint64)
        at = np.asarray(batch.acctype, np.uint8)
        if n and (off[0] != 0 or off[-1] != keys.size or np.any(np.diff(off) < 0)):
            return EINVAL, 0, 0
        sel = np.nonzero(np.asarray(rc, np.uint8)[:n] == np.uint8(want))[0]
        need_n, need_m = int(sel.size), int((off[sel + 1] - off[sel]).sum())
        if len(self.heap) + need_n > self.cap_txn or self.nnz + need_m > self.cap_nnz:
            return ERANGE, need_n, need_m
        for i in sel:
            i = int(i)
            cnt = min((0 if cnt_in is None else int(cnt_in[i])) + 1, U32)  # worker_thread.cpp:165
            src = i if src_in is None else int(src_in[i])
            due = min(now + penalty(self.policy, self.pen, self.pen_max, cnt), U64)  # :32
            a, b = int(off[i]), int(off[i + 1])
            heapq.heappush(self.heap, (due, self.seq, src, cnt, keys[a:b].copy(), at[a:b].copy()))  # :36-44
            self.seq += 1
        self.nnz += need_m
        return OK, need_n, need_m

    def pop(self, now, txn_base=0, nnz_base=0, cap_txn=None, cap_nnz=None):
        """AbortQueue::process (:52-82).  Returns (code, n, nnz, rows): rows as
        select_ref's (offsets at txn_base.., keys / acctype at nnz_base..) plus
        src, cnt, due at txn_base..; None unless code == OK."""
        due = sorted(e for e in self.heap if e[0] < now)   # :60-63, strict (:62), in heap order
        n, m = len(due), sum(int(e[4].size) for e in due)
        if (cap_txn is not None and n > cap_txn) or (cap_nnz is not None and m > cap_nnz) \
                or nnz_base + m > U32:
            return ERANGE, n, m, None
        for _ in range(n):
            heapq.heappop(self.heap)                       # :63
        self.nnz -= m
        lens = np.asarray([e[4].size for e in due], np.int64)
        rows = {
            "offsets": (nnz_base + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint32),
            "keys": np.concatenate([e[4] for e in due]).astype(np.uint64) if n else np.zeros(0, np.uint64),
            "acctype": np.concatenate([e[5] for e in due]).astype(np.uint8) if n else np.zeros(0, np.uint8),
            "src": np.asarray([e[2] for e in due], np.uint32),
            "cnt": np.asarray([e[3] for e in due], np.uint32),
            "due": np.asarray([e[0] for e in due], np.uint64),
        }
        return OK, n, m, rows


def push_alg_bytes(n_txn, n_sel, nnz_sel):
    """dcc_abortq_push_alg_bytes as documented in dcc.h: the select with one
    per-txn array (src) plus cnt (4 B) and due (8 B) written per parked txn."""
    return 4 * (n_txn + 1) + n_txn + 18 * nnz_sel + 4 * (n_sel + 1) + 16 * n_sel + 12 * n_sel


def pop_alg_bytes(n_q, nnz_q, n_due, nnz_due):
    """dcc_abortq_pop_alg_bytes as documented in dcc.h."""
    flags = 8 * n_q + 4 * (n_q + 1)
    if n_due == 0:
        return flags
    return flags + 24 * n_q + 18 * nnz_q + 4 * (n_due + 1) + 4 * (n_q - n_due + 1) + 32 * n_q
