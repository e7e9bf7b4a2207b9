"""Replays of CC_ALG WAIT_DIE as the engine models it (include/dcc.h): the
parity references of dcc_waitdie_lock_epoch and dcc_waitdie_release.

The lock state is two per-txn arrays over a batch the caller keeps: rc[i] in
{WD_RUN, RC_RCOK, RC_WAIT, RC_ABORT, WD_GONE} and pos[i].  A non-GONE txn owns
its accesses [0, pos): one owner entry (type, ts) per access on the access's
row; a WAIT txn also has one waiter entry, on the row of access pos.  An epoch
only acquires: the RUN txns run in index order, each calling lock_get for its
accesses from pos on.  A release removes the txns the caller names and promotes
waiters.

Three restatements, independent of each other:

  replay_literal  Row_lock in WAIT_DIE mode (concurrency_control/
                  row_lock.cpp): the owner list, the waiter list in descending
                  ts, lock_type, lock_get (:46-216), lock_release with its
                  promotion loop (:219-372) and the waiter removal behind its
                  assert(false) (:289-303); the reference's asserts on distinct
                  txns / timestamps (:106-107) compiled out, ties in the waiter
                  list broken by txn index (lower index nearer the head).
  replay          the closed forms over four per-row aggregates: any owner, any
                  EX owner, the least owner ts, the largest waiter ts.
  replay_rounds   what the GPU engine runs: the certain / possible rounds over
                  the accesses sorted by (row, static before dynamic) -- an
                  undecided txn's accesses counting as possible owners only
                  below its first certain conflict -- and for the release one
                  sort and one segmented scan.

Each takes (batch, ts, rc, pos) and returns new arrays:
  *_epoch    -> (rc, pos, conflict, stats)    [replay_rounds_epoch: stats["rounds"]]
  *_release  -> (rc, pos, n_left, n_promoted)
Malformed states raise ValueError (the engine's DCC_EINVAL).

The three claims the closed forms rest on are asserted where they apply:
  1. a lock granted and released inside one txn's turn restores the row exactly
     and promotes nothing (replay_literal_epoch, on every died txn);
  2. releasing the leavers one at a time, in any order, with literal
     lock_release -- promotions included, a leaver promoted on the way being
     released as an owner -- ends in the state of the batch rule
     (replay_literal_release, which runs two orders);
  3. decisions need only the four aggregates (replay_epoch keeps nothing else).
"""
from __future__ import annotations

import numpy as np

from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RC_WAIT, RD, SCAN, WD_GONE, WD_RUN

MAX_LEN = 64  # MAX_ROW_PER_TXN
KEY_RESERVED = (1 << 64) - 1
U64_MAX = (1 << 64) - 1
LOCK_EX, LOCK_SH, LOCK_NONE = 0, 1, 2  # lock_t, row_lock.h
STATES = (WD_RUN, RC_RCOK, RC_WAIT, RC_ABORT, WD_GONE)


def lock_of(ty):
    """row.cpp:228: RD / SCAN request LOCK_SH, every other access LOCK_EX."""
    return LOCK_SH if ty in (RD, SCAN) else LOCK_EX


def conflict_lock(l1, l2):  # row_lock.cpp:374-381
    if l1 == LOCK_NONE or l2 == LOCK_NONE:
        return False
    return l1 == LOCK_EX or l2 == LOCK_EX


def _lists(batch, ts, rc, pos):
    off = np.asarray(batch.offsets).astype(np.int64).tolist()
    keys = np.asarray(batch.keys).astype(np.uint64).tolist()
    at = np.asarray(batch.acctype).tolist()
    n = len(off) - 1
    if ts is None or rc is None or pos is None:
        raise ValueError("null ts / rc / pos")
    tsl = [int(v) for v in np.asarray(ts, np.uint64).tolist()]
    rcl = [int(v) for v in np.asarray(rc, np.uint8).tolist()]
    posl = [int(v) for v in np.asarray(pos, np.uint32).tolist()]
    if min(len(tsl), len(rcl), len(posl)) < n:
        raise ValueError("ts / rc / pos shorter than the batch")
    check_state(off, keys, rcl, posl)
    return off, keys, at, tsl[:n], rcl[:n], posl[:n]


def check_state(off, keys, rc, pos):
    """The rejections of both calls."""
    n = len(off) - 1
    if n and (off[0] != 0 or off[n] != len(keys)):
        raise ValueError("malformed offsets")
    for i in range(n):
        L = off[i + 1] - off[i]
        if L < 0:
            raise ValueError("malformed offsets")
        if L > MAX_LEN:
            raise ValueError("a txn longer than MAX_ROW_PER_TXN")
    if any(k == KEY_RESERVED for k in keys):
        raise ValueError("the reserved key")
    for i in range(n):
        L = off[i + 1] - off[i]
        if rc[i] not in STATES:
            raise ValueError(f"txn {i}: rc byte {rc[i]:#x}")
        if rc[i] == WD_GONE:
            continue
        if pos[i] > L:
            raise ValueError(f"txn {i}: pos > len")
        if rc[i] == RC_RCOK and pos[i] != L:
            raise ValueError(f"txn {i}: RCOK with pos != len")
        if rc[i] == RC_WAIT and pos[i] >= L:
            raise ValueError(f"txn {i}: WAIT with pos >= len")


def _out(rc, pos):
    return np.asarray(rc, np.uint8), np.asarray(pos, np.uint32)


def _stats(off, at, rc_in, pos_in, rc):
    """The epoch's counts: decisions of the RUN txns; EX requests are the EX
    accesses at or past pos of the RUN txns."""
    run = [i for i in range(len(rc_in)) if rc_in[i] == WD_RUN]
    nex = [sum(lock_of(at[a]) == LOCK_EX for a in range(off[i] + pos_in[i], off[i + 1])) for i in run]
    return {"n_commit": sum(rc[i] == RC_RCOK for i in run), "n_abort": sum(rc[i] == RC_ABORT for i in run),
            "n_survivors": sum(rc[i] == RC_WAIT for i in run), "nnz_w": sum(nex),
            "n_readonly": sum(c == 0 for c in nex)}


# ------------------------------------------------------------------ literal
class RowLock:
    """Row_lock (row_lock.h / row_lock.cpp) under CC_ALG == WAIT_DIE.  An entry
    is (txn, type, ts); owners[0] is the top of the reference's stack,
    waiters[0] its waiters_head."""

    def __init__(self):  # Row_lock::init, :24-44
        self.owners = []
        self.waiters = []
        self.lock_type = LOCK_NONE

    def lock_get(self, typ, txn, ts):  # :52-216
        conflict = conflict_lock(self.lock_type, typ)  # :69
        if not conflict and self.waiters and ts < self.waiters[0][2]:  # :73-77
            conflict = True
        if conflict:  # :91-151
            canwait = True
            for _, _, ots in self.owners:  # :103-118, the asserts of :106-107 compiled out
                if ts > ots:
                    canwait = False
                    break
            if not canwait:
                return RC_ABORT  # :150
            # :133-141 keeps the list in descending ts; among equal ts the
            # lower txn index is nearer the head (the engine's rule: the
            # reference's order there depends on arrival)
            q = 0
            while q < len(self.waiters) and (ts < self.waiters[q][2] or
                                             (ts == self.waiters[q][2] and self.waiters[q][0] < txn)):
                q += 1
            self.waiters.insert(q, (txn, typ, ts))
            return RC_WAIT  # :146
        self.owners.insert(0, (txn, typ, ts))  # :177-181
        self.lock_type = typ  # :194
        return RC_RCOK

    def lock_release(self, txn):
        """:219-372.  Returns the txns promoted, in promotion order."""
        for q, en in enumerate(self.owners):  # :261-267
            if en[0] == txn:
                self.owners.pop(q)  # :270-273
                if not self.owners:
                    self.lock_type = LOCK_NONE  # :274-287
                break
        else:  # :289-303, behind assert(false)
            for q, en in enumerate(self.waiters):
                if en[0] == txn:
                    self.waiters.pop(q)
                    break
            else:
                raise AssertionError("lock_release: the txn has no entry")  # ASSERT(en), :294
        promoted = []
        while self.waiters and not conflict_lock(self.lock_type, self.waiters[0][1]):  # :317
            en = self.waiters.pop(0)  # :318
            self.owners.insert(0, en)  # :332
            self.lock_type = en[1]  # :353
            promoted.append(en[0])  # restart_txn, :347
        return promoted

    def image(self):
        return (sorted(self.owners), list(self.waiters), self.lock_type)

    def derived_lock_type(self):
        if any(t == LOCK_EX for _, t, _ in self.owners):
            return LOCK_EX
        return LOCK_SH if self.owners else LOCK_NONE

    def invariant(self):
        """lock_type is what the owner entries say, and waiters exist only
        behind a head that conflicts with it."""
        assert self.lock_type == self.derived_lock_type()
        assert not self.waiters or conflict_lock(self.lock_type, self.waiters[0][1])


def _build_rows(off, keys, at, ts, rc, pos):
    """The Row_lock of every row from the (rc, pos) state."""
    rows = {}
    n = len(off) - 1
    for i in range(n):
        if rc[i] == WD_GONE:
            continue
        for q in range(pos[i]):
            a = off[i] + q
            rows.setdefault(keys[a], RowLock()).owners.append((i, lock_of(at[a]), ts[i]))
    for r in rows.values():
        r.lock_type = r.derived_lock_type()
    wait = [(-ts[i], i) for i in range(n) if rc[i] == RC_WAIT]
    for _, i in sorted(wait):  # descending ts, lower index nearer the head
        a = off[i] + pos[i]
        rows.setdefault(keys[a], RowLock()).waiters.append((i, lock_of(at[a]), ts[i]))
    return rows


def replay_literal_epoch(batch, ts, rc, pos):
    off, keys, at, tsl, rcl, posl = _lists(batch, ts, rc, pos)
    n = len(off) - 1
    rows = _build_rows(off, keys, at, tsl, rcl, posl)
    rc_in, pos_in = list(rcl), list(posl)
    conflict = [ACCESS_NONE] * n
    for i in range(n):
        if rc_in[i] != WD_RUN:
            continue
        before = {}
        gained = []
        res = RC_RCOK
        q = pos_in[i]
        while q < off[i + 1] - off[i]:
            a = off[i] + q
            row = rows.setdefault(keys[a], RowLock())
            before.setdefault(keys[a], row.image())
            res = row.lock_get(lock_of(at[a]), i, tsl[i])
            if res != RC_RCOK:
                break
            gained.append(keys[a])
            q += 1
        if res == RC_RCOK:
            rcl[i], posl[i] = RC_RCOK, q
        elif res == RC_WAIT:
            rcl[i], posl[i], conflict[i] = RC_WAIT, q, q
        else:
            # TxnManager::cleanup (system/txn.cpp): return_row, newest access
            # first, for the accesses of this turn; the carried prefix stays
            # (deferred cleanup)
            for k in reversed(gained):
                assert rows[k].lock_release(i) == [], "claim 1: a release inside the turn promoted a waiter"
            for k, img in before.items():
                assert rows[k].image() == img, "claim 1: the row is not restored"
            rcl[i], conflict[i] = RC_ABORT, q
    for r in rows.values():
        r.invariant()
    return _out(rcl, posl) + (np.asarray(conflict, np.uint32), _stats(off, at, rc_in, pos_in, rcl))


def _release_in_order(off, keys, at, tsl, rcl, posl, order):
    rows = _build_rows(off, keys, at, tsl, rcl, posl)
    rcl, posl = list(rcl), list(posl)
    promoted = set()
    for i in order:
        entries = list(range(posl[i])) if rcl[i] != WD_GONE else []
        if rcl[i] == RC_WAIT:  # still queued (a leaver promoted on the way owns the access by now)
            entries.append(posl[i])
        for q in reversed(entries):  # cleanup: newest access first
            for j in rows[keys[off[i] + q]].lock_release(i):
                # restart_txn -> get_row_post_wait (row.cpp:313-321): the
                # waiter resumes behind the access it waited for
                assert rcl[j] == RC_WAIT
                promoted.add(j)
                rcl[j], posl[j] = WD_RUN, posl[j] + 1
        rcl[i] = WD_GONE
    for r in rows.values():
        r.invariant()
        assert not any(rcl[t] == WD_GONE for t, _, _ in r.owners + r.waiters)
    return rcl, posl, rows, promoted


def replay_literal_release(batch, ts, rc, pos, leave, order=None):
    """One leaver at a time, in `order` (a permutation of the leavers; index
    order by default) and, for claim 2, in the reverse order too."""
    off, keys, at, tsl, rcl, posl = _lists(batch, ts, rc, pos)
    if leave is None:
        raise ValueError("null leave")
    lv = [i for i, v in enumerate(np.asarray(leave).tolist()[:len(rcl)]) if v]
    order = lv if order is None else [int(i) for i in order]
    assert sorted(order) == lv
    r1, p1, rows1, prom1 = _release_in_order(off, keys, at, tsl, rcl, posl, order)
    r2, p2, rows2, _ = _release_in_order(off, keys, at, tsl, rcl, posl, order[::-1])
    live = [i for i in range(len(r1)) if r1[i] != WD_GONE]
    assert r1 == r2 and [p1[i] for i in live] == [p2[i] for i in live], "claim 2: the order of the releases shows"
    assert {k: r.image() for k, r in rows1.items() if r.owners or r.waiters} == \
        {k: r.image() for k, r in rows2.items() if r.owners or r.waiters}, "claim 2: row states differ"
    n_left = sum(rcl[i] != WD_GONE for i in lv)
    n_prom = sum(r1[i] == WD_RUN and rcl[i] == RC_WAIT for i in range(len(r1)))
    # the state left in the Row_locks is the state the arrays describe
    again = _build_rows(off, keys, at, tsl, r1, p1)
    assert {k: r.image() for k, r in rows1.items() if r.owners or r.waiters} == \
        {k: r.image() for k, r in again.items()}
    for i in lv:
        p1[i] = posl[i]  # pos of a GONE txn is ignored: left as it was
    return _out(r1, p1) + (n_left, n_prom)


# -------------------------------------------------------------- closed forms
def replay_epoch(batch, ts, rc, pos):
    off, keys, at, tsl, rcl, posl = _lists(batch, ts, rc, pos)
    n = len(off) - 1
    rc_in, pos_in = list(rcl), list(posl)
    agg = {}  # row -> (owner entries, EX owner entries, least owner ts, largest waiter ts | -1)
    for i in range(n):
        if rcl[i] == WD_GONE:
            continue
        for q in range(posl[i]):
            a = off[i] + q
            c, x, lo, hi = agg.get(keys[a], (0, 0, U64_MAX, -1))
            agg[keys[a]] = (c + 1, x + (lock_of(at[a]) == LOCK_EX), min(lo, tsl[i]), hi)
        if rcl[i] == RC_WAIT:
            k = keys[off[i] + posl[i]]
            c, x, lo, hi = agg.get(k, (0, 0, U64_MAX, -1))
            agg[k] = (c, x, lo, max(hi, tsl[i]))
    conflict = [ACCESS_NONE] * n
    for i in range(n):
        if rc_in[i] != WD_RUN:
            continue
        t = tsl[i]
        undo = {}
        q = pos_in[i]
        L = off[i + 1] - off[i]
        while q < L:
            a = off[i] + q
            k, ex = keys[a], lock_of(at[a]) == LOCK_EX
            c, x, lo, hi = agg.get(k, (0, 0, U64_MAX, -1))
            if not (x > 0 or (ex and c > 0) or t < hi):
                undo.setdefault(k, (c, x, lo, hi))
                agg[k] = (c + 1, x + ex, min(lo, t), hi)
                q += 1
                continue
            conflict[i] = q
            if c > 0 and t > lo:  # dies; what it gained in this turn leaves no trace
                agg.update(undo)
                rcl[i] = RC_ABORT
            else:
                agg[k] = (c, x, lo, max(hi, t))
                rcl[i], posl[i] = RC_WAIT, q
            break
        else:
            rcl[i], posl[i] = RC_RCOK, L
    return _out(rcl, posl) + (np.asarray(conflict, np.uint32), _stats(off, at, rc_in, pos_in, rcl))


def replay_release(batch, ts, rc, pos, leave):
    off, keys, at, tsl, rcl, posl = _lists(batch, ts, rc, pos)
    if leave is None:
        raise ValueError("null leave")
    n = len(off) - 1
    lv = np.asarray(leave).tolist()
    n_left = 0
    for i in range(n):
        if lv[i]:
            n_left += rcl[i] != WD_GONE
            rcl[i] = WD_GONE
    own = {}  # row -> (owner entries, EX owner entries) of the stayers
    queue = {}  # row -> its staying waiters
    for i in range(n):
        if rcl[i] == WD_GONE:
            continue
        for q in range(posl[i]):
            a = off[i] + q
            c, x = own.get(keys[a], (0, 0))
            own[keys[a]] = (c + 1, x + (lock_of(at[a]) == LOCK_EX))
        if rcl[i] == RC_WAIT:
            queue.setdefault(keys[off[i] + posl[i]], []).append((-tsl[i], i))
    n_prom = 0
    for k, w in queue.items():
        c, x = own.get(k, (0, 0))
        if x:
            continue
        w.sort()
        all_sh = True
        for rank, (_, i) in enumerate(w, 1):
            all_sh = all_sh and lock_of(at[off[i] + posl[i]]) == LOCK_SH
            if (rank == 1 and c == 0) or all_sh:
                rcl[i], posl[i] = WD_RUN, posl[i] + 1
                n_prom += 1
            else:
                break
    return _out(rcl, posl) + (n_left, n_prom)


# ------------------------------------------------------- the engine's passes
def replay_rounds_epoch(batch, ts, rc, pos):
    off, keys, at, tsl, rcl, posl = _lists(batch, ts, rc, pos)
    n = len(off) - 1
    rc_in, pos_in = list(rcl), list(posl)
    OWN, WAITER, DYN = 0, 1, 2
    seg = {}  # row -> its accesses (dynamic?, txn, position, kind), static before dynamic
    for i in range(n):
        if rcl[i] == WD_GONE:
            continue
        for q in range(off[i + 1] - off[i]):
            if q < posl[i]:
                kind = OWN
            elif rcl[i] == RC_WAIT and q == posl[i]:
                kind = WAITER
            elif rcl[i] == WD_RUN:
                kind = DYN
            else:
                continue
            seg.setdefault(keys[off[i] + q], []).append((kind == DYN, i, q, kind))
    for accs in seg.values():
        accs.sort(key=lambda e: e[0])  # stable: (txn, position) order within each half
    UND, OK, WT, AB = 0, 1, 2, 3
    state = {i: UND for i in range(n) if rcl[i] == WD_RUN}
    prog = {i: posl[i] for i in state}
    # the first access at or past the progress with a certain conflict, once one
    # is known: the txn owns nothing from there on and waits there at the latest
    cap = {i: MAX_LEN for i in state}
    rounds = 0
    left = len(state)
    while left or rounds == 0:
        rounds += 1
        assert rounds <= n + len(keys) + 2, "the fixed point did not converge"
        flags = {}
        for k, accs in seg.items():
            c_any = c_ex = p_any = p_ex = False
            c_min = p_min = U64_MAX
            c_w = p_w = -1
            o_txn, o_any, o_ex = -1, False, False  # the txn's own accesses below its progress
            for _, i, q, kind in accs:
                ex = lock_of(at[off[i] + q]) == LOCK_EX
                t = tsl[i]
                if kind == DYN and o_txn != i:
                    o_txn, o_any, o_ex = i, False, False
                if kind == DYN and state[i] == UND and q >= prog[i]:
                    cc = c_ex or (ex and c_any) or t < c_w or o_ex or (ex and o_any)
                    pc = p_ex or (ex and p_any) or t < p_w
                    flags[(i, q)] = (cc, t > c_min, pc, t > p_min)
                s = state.get(i)
                certain_owner = kind == OWN or (kind == DYN and ((s == OK) or (s == WT and q < prog[i])))
                possible_owner = certain_owner or (kind == DYN and s == UND and q < cap[i])
                certain_waiter = kind == WAITER or (kind == DYN and s == WT and q == prog[i])
                possible_waiter = certain_waiter or (kind == DYN and s == UND and prog[i] <= q <= cap[i])
                if certain_owner:
                    c_any, c_ex, c_min = True, c_ex or ex, min(c_min, t)
                if possible_owner:
                    p_any, p_ex, p_min = True, p_ex or ex, min(p_min, t)
                if certain_waiter:
                    c_w = max(c_w, t)
                if possible_waiter:
                    p_w = max(p_w, t)
                if kind == DYN and s == UND and q < prog[i]:
                    o_any, o_ex = True, o_ex or ex
        left = 0
        for i in state:
            if state[i] != UND:
                continue
            L = off[i + 1] - off[i]
            p = prog[i]
            cap[i] = min([q for q in range(p, L) if flags[(i, q)][0]], default=MAX_LEN)
            while p < L and not flags[(i, p)][2]:
                p += 1
            prog[i] = p
            if p == L:
                state[i] = OK
                continue
            cc, cd, _, pd = flags[(i, p)]
            if cc and cd:
                state[i] = AB
            elif cc and not pd:
                state[i] = WT
            else:
                left += 1
    conflict = [ACCESS_NONE] * n
    for i, s in state.items():
        if s == OK:
            rcl[i], posl[i] = RC_RCOK, prog[i]
        elif s == WT:
            rcl[i], posl[i], conflict[i] = RC_WAIT, prog[i], prog[i]
        else:
            rcl[i], conflict[i] = RC_ABORT, prog[i]
    st = _stats(off, at, rc_in, pos_in, rcl)
    st["rounds"] = rounds
    return _out(rcl, posl) + (np.asarray(conflict, np.uint32), st)


def replay_rounds_release(batch, ts, rc, pos, leave):
    """One sort of the staying static accesses by (row, owners before waiters,
    ~ts, txn index) and one exclusive segmented scan of (owners, EX owners,
    waiters, a waiter that is EX)."""
    off, keys, at, tsl, rcl, posl = _lists(batch, ts, rc, pos)
    if leave is None:
        raise ValueError("null leave")
    n = len(off) - 1
    lv = np.asarray(leave).tolist()
    n_left = sum(bool(lv[i]) and rcl[i] != WD_GONE for i in range(n))
    for i in range(n):
        if lv[i]:
            rcl[i] = WD_GONE
    recs = []
    for i in range(n):
        if rcl[i] == WD_GONE:
            continue
        for q in range(posl[i]):
            recs.append((keys[off[i] + q], 0, U64_MAX - tsl[i], i, q))
        if rcl[i] == RC_WAIT:
            recs.append((keys[off[i] + posl[i]], 1, U64_MAX - tsl[i], i, posl[i]))
    recs.sort(key=lambda e: e[:4])
    n_prom = 0
    prev = None
    for k, w, _, i, q in recs:
        if k != prev:
            any_own = ex_own = some_ex = False
            cnt = 0
            prev = k
        ex = lock_of(at[off[i] + q]) == LOCK_EX
        if not w:
            any_own, ex_own = True, ex_own or ex
            continue
        if not ex_own and ((cnt == 0 and not any_own) or (not some_ex and not ex)):
            rcl[i], posl[i] = WD_RUN, posl[i] + 1
            n_prom += 1
        cnt += 1
        some_ex = some_ex or ex
    return _out(rcl, posl) + (n_left, n_prom)
