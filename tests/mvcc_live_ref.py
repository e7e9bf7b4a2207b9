"""Replays of CC_ALG MVCC with txns in flight, as the engine models it
(include/dcc.h): the parity references of dcc_mvcc_access_epoch
and dcc_mvcc_finish.

The state is two per-txn arrays over a batch the caller keeps: rc[i] in
{WD_RUN, RC_RCOK, RC_WAIT, RC_ABORT, WD_GONE} and pos[i].  A txn that is not
GONE holds one pending prewrite (ts[i]) on the row of each WR access in [0, pos);
a WAIT txn has a buffered read on the row of access pos and, if that access is a
WR, that access's prewrite too.  An epoch only sends requests: the RUN txns run
in index order, each from pos on.  A finish commits or aborts the txns the
caller names and promotes buffered reads.  Rows and versions live in `state`, a
dict the caller carries from call to call.

Three restatements, independent of each other:

  Literal (class)   Row_mvcc with its buffers (concurrency_control/row_mvcc.cpp):
                    readreq_mvcc / prereq_mvcc with buffer_req (:95-109),
                    debuffer_req for both types (:115-171), the full conflict()
                    (:198-240), access (:242-334) and update_buffer (:336-364), on
                    mvcc_ref.RowMvcc's histories.  The txns' cleanup is
                    txn.cpp:759-761, newest access first.  It keeps the buffers
                    from call to call, so it is an object; `state`: key -> LiveRow.
  epoch / finish    the closed forms: per row rts, the versions in install order
                    and, recomputed from (rc, pos) at every call, the pending
                    prewrites' timestamps.  `state`: key -> [rts, [versions]],
                    mvcc_ref's shape (rows_of, versions_of and trim apply).
  rounds_epoch /    what the GPU engine runs: the certain / possible rounds over
  rounds_finish     the accesses sorted by (row, static before dynamic), and for
                    the finish one sort by (row, ts, txn) and one exclusive prefix.

Each call takes (batch, ts, rc, pos, ..., vts, state) and returns new arrays:
  epoch   -> (rc, pos, conflict, stats)          [rounds_epoch: stats["rounds"]]
  finish  -> (rc, pos, n_left, n_promoted)
vts (u64[nnz] or None) is updated in place, as the engine does.  Malformed
states raise ValueError (the engine's DCC_EINVAL) before anything changes.

The three facts the closed forms rest on are asserted by the literal replay
after every request:
  1. every pending prewrite of a row is at or above the row's latest version;
  2. an installed version is at or above the row's latest version (so a row's
     versions are non-decreasing in install order, across finishes);
  3. a write timestamp is in the row's read history.
"""
from __future__ import annotations

from bisect import bisect_right

import numpy as np

from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RC_WAIT, VTS_BASE, VTS_NONE, WD_GONE, WD_RUN, WR, XP
from mvcc_ref import ABORT, P_REQ, R_REQ, RCOK, W_REQ, WAIT, XP_REQ, RowMvcc
from waitdie_ref import check_state

U64_MAX = (1 << 64) - 1


def _lists(batch, ts, rc, pos, leave=None):
    off = np.asarray(batch.offsets).astype(np.int64).tolist()
    keys = np.asarray(batch.keys).astype(np.uint64).tolist()
    at = [int(v) & 3 for v in np.asarray(batch.acctype).tolist()]
    n = len(off) - 1
    if ts is None or rc is None or pos is None:
        raise ValueError("null ts / rc / pos")
    tsl = [int(v) for v in np.asarray(ts, np.uint64).tolist()]
    rcl = [int(v) for v in np.asarray(rc, np.uint8).tolist()]
    posl = [int(v) for v in np.asarray(pos, np.uint32).tolist()]
    if min(len(tsl), len(rcl), len(posl)) < n:
        raise ValueError("ts / rc / pos shorter than the batch")
    check_state(off, keys, rcl, posl)
    for i in range(n):
        if rcl[i] != WD_GONE and not 0 < tsl[i] < U64_MAX:
            raise ValueError(f"txn {i}: ts outside [1, 2^64-2]")
    lv = None
    if leave is not None:
        lv = [int(v) != 0 for v in np.asarray(leave, np.uint8).tolist()][:n]
        if len(lv) < n:
            raise ValueError("leave shorter than the batch")
        if any(lv[i] and rcl[i] == RC_WAIT for i in range(n)):
            raise ValueError("a WAIT txn cannot leave")
    return off, keys, at, tsl[:n], rcl[:n], posl[:n], lv


def _out(rc, pos):
    return np.asarray(rc, np.uint8), np.asarray(pos, np.uint32)


def _stats(off, at, rc_in, pos_in, rc):
    run = [i for i in range(len(rc_in)) if rc_in[i] == WD_RUN]
    nwr = [sum(at[a] == WR for a in range(off[i] + pos_in[i], off[i + 1])) for i in run]
    return {"n_commit": sum(rc[i] == RC_RCOK for i in run), "n_abort": sum(rc[i] == RC_ABORT for i in run),
            "n_survivors": sum(rc[i] == RC_WAIT for i in run), "nnz_w": sum(nwr),
            "n_readonly": sum(c == 0 for c in nwr)}


def held_prewrites(off, at, rc, pos, i):
    """The accesses of txn i that hold a pending prewrite."""
    if rc[i] == WD_GONE:
        return []
    top = pos[i] + (1 if rc[i] == RC_WAIT else 0)
    return [a for a in range(off[i], off[i] + top) if at[a] == WR]


# ------------------------------------------------------------------ literal
class LiveRow(RowMvcc):
    """Row_mvcc with both buffers.  readreq: (txn, ts), index 0 the head."""

    def __init__(self):
        super().__init__()
        self.readreq = []

    def check(self):
        latest = self.writehis[0] if self.writehis else 0
        for _, p in self.prereq:
            if p < latest:
                raise AssertionError(f"a pending prewrite {p} lies below the row's latest version {latest}")

    def debuffer_reads(self):  # debuffer_req(R_REQ, NULL), :143-167; the return queue is a stack
        min_pts = U64_MAX
        for _, p in self.prereq:
            if p < min_pts:
                min_pts = p
        ready, stay = [], []
        for req in self.readreq:
            (ready if req[1] <= min_pts else stay).append(req)
        self.readreq = stay
        ready.reverse()
        return ready

    def update_buffer(self):  # :336-364 -> [(txn, version)]
        out = []
        for txn, ts in self.debuffer_reads():
            v = VTS_BASE
            for w in self.writehis:
                if not w > ts:
                    v = w
                    break
            self.insert_history(self.readhis, ts)
            out.append((txn, v))
        return out

    def access(self, txn, typ, ts):  # :242-334
        if typ == R_REQ:
            if self.conflict(R_REQ, ts):
                self.readreq.insert(0, (txn, ts))  # buffer_req(R_REQ), STACK_PUSH
                return WAIT, None
            return super().access(txn, typ, ts)
        if typ == P_REQ:
            r = super().access(txn, typ, ts)
            self.check()
            return r
        if typ == W_REQ and self.writehis and ts < self.writehis[0]:
            raise AssertionError(f"txn {txn}: installs version {ts} below the row's latest {self.writehis[0]}")
        super().access(txn, typ, ts)  # W_REQ: raises if ts is not in the read history
        self.check()
        return RCOK, self.update_buffer()


class Literal:
    """The literal replay: the rows with their buffers persist in the object."""

    def __init__(self):
        self.state = {}

    def row(self, k):
        return self.state.setdefault(k, LiveRow())

    def buffers_match(self, batch, ts, rc, pos):
        """The rows' buffers are what (rc, pos) say they are."""
        off, keys, at, tsl, rcl, posl, _ = _lists(batch, ts, rc, pos)
        pre, rd = {}, {}
        for i in range(len(rcl)):
            for a in held_prewrites(off, at, rcl, posl, i):
                pre.setdefault(keys[a], []).append((i, tsl[i]))
            if rcl[i] == RC_WAIT:
                rd.setdefault(keys[off[i] + posl[i]], []).append((i, tsl[i]))
        for k, m in self.state.items():
            assert sorted(m.prereq) == sorted(pre.get(k, [])), f"row {k}: prewrites {m.prereq} vs {pre.get(k)}"
            assert sorted(m.readreq) == sorted(rd.get(k, [])), f"row {k}: buffered reads"
        assert all(k in self.state for k in list(pre) + list(rd))

    def epoch(self, batch, ts, rc, pos, vts=None):
        off, keys, at, tsl, rcl, posl, _ = _lists(batch, ts, rc, pos)
        n = len(rcl)
        rc_in, pos_in = list(rcl), list(posl)
        conflict = [ACCESS_NONE] * n
        for i in range(n):
            if rcl[i] != WD_RUN:
                continue
            t = tsl[i]
            q = posl[i]
            L = off[i + 1] - off[i]
            res = RCOK
            while q < L:
                a = off[i] + q
                k, ty = keys[a], at[a]
                if ty != XP:  # row.cpp:239-282
                    m = self.row(k)
                    if ty == WR:
                        res, _ = m.access(i, P_REQ, t)
                    if res == RCOK:
                        res, v = m.access(i, R_REQ, t)
                        if res == RCOK and vts is not None:
                            vts[a] = v
                    if res != RCOK:
                        break
                q += 1
            posl[i] = q
            if res == RCOK:
                rcl[i] = RC_RCOK
            else:
                rcl[i] = RC_WAIT if res == WAIT else RC_ABORT
                conflict[i] = q
        return _out(rcl, posl) + (np.asarray(conflict, np.uint32), _stats(off, at, rc_in, pos_in, rcl))

    def finish(self, batch, ts, rc, pos, leave, vts=None):
        """The leavers released one at a time in index order, newest access
        first (txn.cpp:759-761)."""
        off, keys, at, tsl, rcl, posl, lv = _lists(batch, ts, rc, pos, leave)
        n = len(rcl)
        left = prom = 0
        for i in range(n):
            if not lv[i] or rcl[i] == WD_GONE:
                continue
            left += 1
            typ = W_REQ if rcl[i] == RC_RCOK else XP_REQ
            for a in reversed(held_prewrites(off, at, rcl, posl, i)):
                _, ready = self.row(keys[a]).access(i, typ, tsl[i])
                for j, v in ready:  # restart_txn -> get_row_post_wait
                    assert rcl[j] == RC_WAIT and keys[off[j] + posl[j]] == keys[a] and not lv[j]
                    if vts is not None and at[off[j] + posl[j]] != XP:
                        vts[off[j] + posl[j]] = v
                    rcl[j] = WD_RUN
                    posl[j] += 1
                    prom += 1
            rcl[i] = WD_GONE
        return _out(rcl, posl) + (left, prom)


# -------------------------------------------------------------- closed form
def _pending(off, keys, at, rc, pos, skip=None):
    """key -> the timestamps' owners of the pending prewrites: [txn, ...]."""
    out = {}
    for i in range(len(rc)):
        if skip is not None and skip[i]:
            continue
        for a in held_prewrites(off, at, rc, pos, i):
            out.setdefault(keys[a], []).append(i)
    return out


def _version(vers, t):
    p = bisect_right(vers, t)
    return (vers[p - 1] if p else VTS_BASE), bool(p and p < len(vers))


def epoch(batch, ts, rc, pos, vts=None, state=None, info=None):
    """info (a dict, optional) counts 'late': reads of a version that is not
    the row's latest."""
    off, keys, at, tsl, rcl, posl, _ = _lists(batch, ts, rc, pos)
    state = {} if state is None else state
    n = len(rcl)
    rc_in, pos_in = list(rcl), list(posl)
    minpre = {k: min(tsl[i] for i in v) for k, v in _pending(off, keys, at, rcl, posl).items()}
    conflict = [ACCESS_NONE] * n
    late = 0
    for i in range(n):
        if rcl[i] != WD_RUN:
            continue
        t = tsl[i]
        q = posl[i]
        L = off[i + 1] - off[i]
        stop = None
        while q < L:
            a = off[i] + q
            k, ty = keys[a], at[a]
            if ty != XP:
                row = state.setdefault(k, [0, []])
                if ty == WR:
                    if t < row[0]:
                        stop = RC_ABORT
                        break
                    minpre[k] = min(minpre.get(k, U64_MAX), t)
                if minpre.get(k, U64_MAX) < t:
                    stop = RC_WAIT
                    break
                v, old = _version(row[1], t)
                late += old
                if vts is not None:
                    vts[a] = v
                row[0] = max(row[0], t)
            q += 1
        posl[i] = q
        rcl[i] = RC_RCOK if stop is None else stop
        if stop is not None:
            conflict[i] = q
    if info is not None:
        info["late"] = info.get("late", 0) + late
    return _out(rcl, posl) + (np.asarray(conflict, np.uint32), _stats(off, at, rc_in, pos_in, rcl))


def finish(batch, ts, rc, pos, leave, vts=None, state=None, info=None):
    """Install every committing leaver's versions, then promote."""
    off, keys, at, tsl, rcl, posl, lv = _lists(batch, ts, rc, pos, leave)
    state = {} if state is None else state
    n = len(rcl)
    left = prom = late = 0
    for i in range(n):
        if lv[i] and rcl[i] == RC_RCOK:
            for a in held_prewrites(off, at, rcl, posl, i):
                vers = state.setdefault(keys[a], [0, []])[1]
                assert not vers or vers[-1] <= tsl[i], "a row's versions are non-decreasing in install order"
                vers.append(tsl[i])
    gone = [lv[i] or rcl[i] == WD_GONE for i in range(n)]
    minpre = {k: min(tsl[i] for i in v) for k, v in _pending(off, keys, at, rcl, posl, skip=gone).items()}
    for i in range(n):
        if lv[i] and rcl[i] != WD_GONE:
            left += 1
            rcl[i] = WD_GONE
        elif rcl[i] == RC_WAIT:
            a = off[i] + posl[i]
            k = keys[a]
            if tsl[i] <= minpre.get(k, U64_MAX):
                row = state.setdefault(k, [0, []])
                v, old = _version(row[1], tsl[i])
                late += old
                if vts is not None and at[a] != XP:
                    vts[a] = v
                row[0] = max(row[0], tsl[i])
                rcl[i] = WD_RUN
                posl[i] += 1
                prom += 1
    if info is not None:
        info["late"] = info.get("late", 0) + late
    return _out(rcl, posl) + (left, prom)


# ------------------------------------------------------- the engine's passes
UND, OK, WAITS, ABORTS = 0, 1, 2, 3
NOCAP = 0xFF


def rounds_epoch(batch, ts, rc, pos, vts=None, state=None):
    off, keys, at, tsl, rcl, posl, _ = _lists(batch, ts, rc, pos)
    state = {} if state is None else state
    n = len(rcl)
    rc_in, pos_in = list(rcl), list(posl)
    # the sort: (row, static before dynamic), stable in batch order
    ent = []
    for i in range(n):
        held = set(held_prewrites(off, at, rcl, posl, i))
        for a in range(off[i], off[i + 1]):
            q = a - off[i]
            dyn = rcl[i] == WD_RUN and q >= posl[i]
            if dyn or a in held:
                ent.append((keys[a], 1 if dyn else 0, a, i, q))
    ent.sort(key=lambda e: (e[0], e[1]))
    st = {i: [UND, NOCAP, posl[i]] for i in range(n) if rcl[i] == WD_RUN}  # state, cap, progress
    rounds = 0
    while True:
        rounds += 1
        flags = {}
        cur = None
        for k, dyn, a, i, q in ent:
            if k != cur:
                cur = k
                r0 = state.get(k, [0, []])[0]
                ec = ep = r0
                mc = mp = U64_MAX
            t, nx, wr = tsl[i], at[a] != XP, at[a] == WR
            if not dyn:
                mc, mp = min(mc, t), min(mp, t)
                continue
            s, cap, p = st[i]
            if s == UND and q >= p:
                flags[a] = (wr and t < ec, nx and mc < t, wr and t < ep, nx and mp < t)
            cex = nx and (s == OK or q < p)
            cpr = wr and (s == OK or q < p or (s == WAITS and q == p))
            pex = cex or (s == UND and nx and q < cap)
            ppr = cpr or (s == UND and wr and q <= cap)
            if cex:
                ec = max(ec, t)
            if pex:
                ep = max(ep, t)
            if cpr:
                mc = min(mc, t)
            if ppr:
                mp = min(mp, t)
        left = 0
        for i, w in st.items():
            if w[0] != UND:
                continue
            L = off[i + 1] - off[i]
            fl = [flags[off[i] + q] for q in range(w[2], L)]
            stops = [x for x, f in enumerate(fl) if f[2] or f[3]]
            if not stops:
                st[i] = [OK, 0, L]
                continue
            x = stops[0]
            ca, cw, pa, _ = fl[x]
            s = ABORTS if ca else (WAITS if cw and not pa else UND)
            cert = [y for y, f in enumerate(fl) if f[0] or f[1]]
            st[i] = [s, w[2] + cert[0] if cert else NOCAP, w[2] + x]
            left += s == UND
        if not left:
            break
        assert rounds <= n + len(keys) + 2, "the fixed point did not converge"
    conflict = [ACCESS_NONE] * n
    for i, (s, _, p) in st.items():
        rcl[i] = {OK: RC_RCOK, WAITS: RC_WAIT, ABORTS: RC_ABORT}[s]
        posl[i] = p
        if s != OK:
            conflict[i] = p
    # the final pass: versions by the fast path or a search, the rows' rts
    cur = None
    for k, dyn, a, i, q in ent:
        row = state.setdefault(k, [0, []])
        if dyn and at[a] != XP and (st[i][0] == OK or q < st[i][2]):
            t = tsl[i]
            latest = row[1][-1] if row[1] else 0
            if vts is not None:
                vts[a] = latest if t >= latest else _version(row[1], t)[0]
            row[0] = max(row[0], t)
    stats = _stats(off, at, rc_in, pos_in, rcl)
    stats["rounds"] = rounds
    return _out(rcl, posl) + (np.asarray(conflict, np.uint32), stats)


def rounds_finish(batch, ts, rc, pos, leave, vts=None, state=None):
    off, keys, at, tsl, rcl, posl, lv = _lists(batch, ts, rc, pos, leave)
    state = {} if state is None else state
    n = len(rcl)
    INST, PRE, READ = 1, 2, 4
    ent = []
    for i in range(n):
        stays = rcl[i] != WD_GONE and not lv[i]
        for a in range(off[i], off[i + 1]):
            q = a - off[i]
            wr, atp = at[a] == WR, rcl[i] == RC_WAIT and q == posl[i]
            kind = INST if lv[i] and rcl[i] == RC_RCOK and wr else 0
            if stays and wr and (q < posl[i] or atp):
                kind |= PRE
            if stays and atp:
                kind |= READ
            ent.append((keys[a], tsl[i], i, a, kind))
    ent.sort(key=lambda e: (e[0], e[1], e[2]))
    # the versions to install, compacted in sorted order, merged by rank: old
    # elements before new ones of a key
    for k, t, i, a, kind in ent:
        if kind & INST:
            state.setdefault(k, [0, []])[1].append(t)
    for row in state.values():
        assert all(x <= y for x, y in zip(row[1], row[1][1:])), "the merged store is not in (key, ts) order"
    prom = 0
    cur = None
    for k, t, i, a, kind in ent:
        if k != cur:
            cur, minpre = k, U64_MAX
        if kind & READ and not minpre < t:
            row = state.setdefault(k, [0, []])
            if vts is not None and at[a] != XP:
                vts[a] = _version(row[1], t)[0]
            row[0] = max(row[0], t)
            rcl[i] = WD_RUN
            posl[i] += 1
            prom += 1
        if kind & PRE:
            minpre = min(minpre, t)
    left = 0
    for i in range(n):
        if lv[i] and rcl[i] != WD_GONE:
            left += 1
            rcl[i] = WD_GONE
    return _out(rcl, posl) + (left, prom)


def new_vts(batch):
    return np.full(max(int(batch.nnz), 0), VTS_NONE, np.uint64)
