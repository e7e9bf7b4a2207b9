"""Replays of CC_ALG TIMESTAMP with one txn in flight at a time: the parity
references of dcc_tso_validate_epoch.

The txns of the batch run in index order.  Each calls get_row for its accesses
in list order (storage/row.cpp:239-282: WR sends P_REQ then R_REQ, RD / SCAN
send R_REQ, XP sends nothing), then commits or aborts before the next txn
starts (TxnManager::cleanup, system/txn.cpp:747-761, newest access first:
cleanup_row turns the WR of an aborted txn into XP, txn.cpp:700-704, so
return_row sends XP_REQ for it and W_REQ for the WR of a committed one,
row.cpp:380-390).

Three restatements, independent of each other:

  replay_literal  Row_ts::access (concurrency_control/row_ts.cpp:167-266) with
                  its three request queues, min_pts / min_rts / min_wts and
                  update_buffer.  It raises if any request returns WAIT or a
                  read or write request is buffered: in this model none is.
  replay          the comparisons alone: wts / rts as running maxima.
  replay_rounds   the rounds fixed point the GPU engine runs (certain and
                  possible prefix maxima per row), for the number of rounds.

All return (rc u8[n], conflict u32[n]) and update `rows`, a dict
key -> (wts, rts) that the caller carries from epoch to epoch (absent: (0, 0)).
"""
from __future__ import annotations

import numpy as np

from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RD, SCAN, WR, XP

U64_MAX = (1 << 64) - 1
R_REQ, W_REQ, P_REQ, XP_REQ = 0, 1, 2, 3  # TsType, row_ts.h
RCOK, ABORT, WAIT = 0, 1, 2


def live(rows):
    """`rows` without the rows at (0, 0), which read the same as rows never seen
    (a replay enters a row when it first touches it)."""
    return {int(k): (int(w), int(r)) for k, (w, r) in rows.items() if (w, r) != (0, 0)}


def _lists(batch, ts):
    off = np.asarray(batch.offsets).astype(np.int64).tolist()
    keys = np.asarray(batch.keys).astype(np.uint64).tolist()
    at = np.asarray(batch.acctype).tolist()
    tsl = [int(v) for v in np.asarray(ts, np.uint64).tolist()]
    assert len(tsl) >= len(off) - 1
    return off, keys, at, tsl


class RowTs:
    """Row_ts (row_ts.h / row_ts.cpp).  A queue is a Python list whose index 0
    is the head of the reference's singly linked list."""

    def __init__(self, wts=0, rts=0):  # Row_ts::init, row_ts.cpp:25-40
        self.wts = wts
        self.rts = rts
        self.min_wts = U64_MAX
        self.min_rts = U64_MAX
        self.min_pts = U64_MAX
        self.readreq = []
        self.writereq = []
        self.prereq = []

    def buffer_req(self, typ, txn, ts):  # row_ts.cpp:64-90
        if typ != P_REQ:
            raise AssertionError(f"txn {txn}: a {'read' if typ == R_REQ else 'write'} request is buffered")
        self.prereq.insert(0, (txn, ts))
        if ts < self.min_pts:
            self.min_pts = ts

    def debuffer_txn(self, queue, txn):  # row_ts.cpp:112-126: the first entry of `txn`
        for q, (t, _) in enumerate(queue):
            if t == txn:
                return queue.pop(q)
        raise AssertionError("debuffer_req: no entry of the txn")  # assert(req != NULL), :117

    @staticmethod
    def debuffer_ts(queue, ts):  # row_ts.cpp:127-144: every entry with req->ts <= ts
        out = [e for e in queue if e[1] <= ts]
        queue[:] = [e for e in queue if e[1] > ts]
        return out

    @staticmethod
    def cal_min(queue):  # row_ts.cpp:148-165
        m = U64_MAX
        for _, ts in queue:
            if ts < m:
                m = ts
        return m

    def access(self, txn, typ, ts):  # row_ts.cpp:167-266
        if typ == R_REQ:
            if ts < self.wts:  # :176
                return ABORT
            if ts > self.min_pts:  # :178
                self.buffer_req(R_REQ, txn, ts)
                return WAIT
            if self.rts < ts:  # :188
                self.rts = ts
            return RCOK
        if typ == P_REQ:
            if ts < self.rts:  # :193
                return ABORT
            if ts < self.wts:  # :200 (TS_TWR false)
                return ABORT
            self.buffer_req(P_REQ, txn, ts)  # :204
            return RCOK
        if typ == W_REQ:
            if ts > self.min_pts:  # :224
                self.buffer_req(W_REQ, txn, ts)
                return RCOK
            if ts > self.min_rts:  # :230
                self.buffer_req(W_REQ, txn, ts)
                return RCOK
            if self.wts < ts:  # :238
                self.wts = ts
            self.debuffer_txn(self.prereq, txn)  # :241
            self.update_buffer()
            return RCOK
        assert typ == XP_REQ
        self.debuffer_txn(self.prereq, txn)  # :250
        self.update_buffer()
        return RCOK

    def update_buffer(self):  # row_ts.cpp:268-323
        while True:
            new_min_pts = self.cal_min(self.prereq)
            assert new_min_pts >= self.min_pts  # :272
            if new_min_pts > self.min_pts:
                self.min_pts = new_min_pts
            else:
                break
            ready_read = self.debuffer_ts(self.readreq, self.min_pts)  # :277
            if not ready_read:
                break
            for _, rts in ready_read:  # :281-292
                if self.rts < rts:
                    self.rts = rts
            new_min_rts = self.cal_min(self.readreq)  # :296
            if new_min_rts > self.min_rts:
                self.min_rts = new_min_rts
            else:
                break
            ready_write = self.debuffer_ts(self.writereq, self.min_rts)  # :301
            if not ready_write:
                break
            young = min(ready_write, key=lambda e: e[1])  # :303-315
            for t, _ in ready_write:
                self.debuffer_txn(self.prereq, t)
            if self.wts < young[1]:  # :318
                self.wts = young[1]


def replay_literal(batch, ts, rows=None):
    off, keys, at, tsl = _lists(batch, ts)
    n = len(off) - 1
    rows = {} if rows is None else rows
    mgr = {}  # key -> RowTs, from `rows` on first touch

    def manager(k):
        m = mgr.get(k)
        if m is None:
            w, r = rows.get(k, (0, 0))
            m = mgr[k] = RowTs(int(w), int(r))
        return m

    rc = [RC_RCOK] * n
    conflict = [ACCESS_NONE] * n
    for i in range(n):
        t = tsl[i]
        made = []  # txn->accesses: the accesses whose get_row returned RCOK
        res = RCOK
        for a in range(off[i], off[i + 1]):
            k, ty = keys[a], at[a]
            if ty == XP:
                manager(k)  # the row is touched, no request is made
                made.append((k, ty))
                continue
            m = manager(k)
            if ty == WR:  # row.cpp:252-256
                res = m.access(i, P_REQ, t)
            if res == RCOK:  # row.cpp:257-258: WR && RCOK, RD, SCAN
                assert ty in (WR, RD, SCAN), f"access type {ty}"
                res = m.access(i, R_REQ, t)
            if res == WAIT:
                raise AssertionError(f"txn {i}: access {a - off[i]} returned WAIT")
            if res == ABORT:
                rc[i] = RC_ABORT
                conflict[i] = a - off[i]
                break
            made.append((k, ty))
        for k, ty in reversed(made):  # cleanup, txn.cpp:759-761
            if ty == WR:
                r2 = mgr[k].access(i, XP_REQ if res == ABORT else W_REQ, t)
                assert r2 == RCOK  # row.cpp:389
    for k, m in mgr.items():
        if m.prereq or m.readreq or m.writereq:
            raise AssertionError(f"row {k}: requests left in its queues")
        rows[k] = (m.wts, m.rts)
    return np.asarray(rc, np.uint8), np.asarray(conflict, np.uint32)


def replay(batch, ts, rows=None):
    off, keys, at, tsl = _lists(batch, ts)
    n = len(off) - 1
    rows = {} if rows is None else rows
    rc = [RC_RCOK] * n
    conflict = [ACCESS_NONE] * n
    get = rows.get
    for i in range(n):
        t = tsl[i]
        wrs = []
        ok = True
        for a in range(off[i], off[i + 1]):
            k, ty = keys[a], at[a]
            w, r = get(k, (0, 0))
            if ty == XP:
                rows[k] = (w, r)
                continue
            if t < w or (ty == WR and t < r):
                rc[i] = RC_ABORT
                conflict[i] = a - off[i]
                ok = False
                break
            if r < t:
                rows[k] = (w, t)
            else:
                rows[k] = (w, r)
            if ty == WR:
                wrs.append(k)
        if ok:
            for k in wrs:
                w, r = rows[k]
                if w < t:
                    rows[k] = (t, r)
    return np.asarray(rc, np.uint8), np.asarray(conflict, np.uint32)


def replay_rounds(batch, ts, rows=None):
    """The engine's fixed point; returns (rc, conflict, rounds)."""
    off, keys, at, tsl = _lists(batch, ts)
    n = len(off) - 1
    rows = {} if rows is None else rows
    UND, COM, ABO = 0, 1, 2
    state = [UND] * n
    prog = [0] * n
    seg = {}  # key -> its accesses (txn, position, type) in index order
    for i in range(n):
        for a in range(off[i], off[i + 1]):
            seg.setdefault(keys[a], []).append((i, a - off[i], at[a]))
            rows.setdefault(keys[a], (0, 0))
    rounds = 0
    left = n
    while left:
        rounds += 1
        bdef, bpos = {}, {}
        for k, accs in seg.items():
            w0, r0 = rows[k]
            de = pe = max(w0, r0)
            dw = pw = w0
            for i, q, ty in accs:
                if ty != XP:
                    bdef[(i, q)], bpos[(i, q)] = (de, pe) if ty == WR else (dw, pw)
                    if q < prog[i]:
                        de = max(de, tsl[i])
                    if state[i] == UND or q < prog[i]:
                        pe = max(pe, tsl[i])
                    if ty == WR and state[i] == COM:
                        dw = max(dw, tsl[i])
                    if ty == WR and state[i] != ABO:
                        pw = max(pw, tsl[i])
        left = 0
        for i in range(n):
            if state[i] != UND:
                continue
            L = off[i + 1] - off[i]
            p = prog[i]
            while p < L and (at[off[i] + p] == XP or tsl[i] >= bpos[(i, p)]):
                p += 1
            prog[i] = p
            if p == L:
                state[i] = COM
            elif tsl[i] < bdef[(i, p)]:
                state[i] = ABO
            else:
                left += 1
    for k, accs in seg.items():
        w, r = rows[k]
        for i, q, ty in accs:
            if ty != XP and q < prog[i]:
                r = max(r, tsl[i])
                if ty == WR and state[i] == COM:
                    w = max(w, tsl[i])
        rows[k] = (w, r)
    rc = [RC_RCOK if s == COM else RC_ABORT for s in state]
    conflict = [ACCESS_NONE if s == COM else p for s, p in zip(state, prog)]
    return np.asarray(rc, np.uint8), np.asarray(conflict, np.uint32), rounds
