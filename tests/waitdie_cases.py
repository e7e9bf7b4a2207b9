"""Known answers and histories of the WAIT_DIE calls (dcc_waitdie_lock_epoch,
dcc_waitdie_release), worked by hand from concurrency_control/row_lock.cpp:

  lock_get  conflict iff lock_type conflicts with the request (:69, :374-381)
            or the request's ts < the waiter head's ts (:73-77); no conflict:
            owner (:171-196); conflict: die if ts > some owner's ts (:103-118,
            :150), else wait in descending ts (:119-146)
  release   the leaver's entries go (:261-303); while the head does not
            conflict with lock_type it becomes an owner (:317-357)

A case is (name, txns, ts, rc0, steps): txns a list of lists of (key, access
type), rc0 the initial rc (pos starts at 0), steps a list of
  ("epoch", rc, pos, conflict)           the state and ordinals after an epoch
  ("release", leavers, rc, pos, n_prom)  the state after these txns left
  ("admit", txns)                        GONE txns admitted as (RUN, 0)
"""
import numpy as np

from deneva_amd import ACCESS_NONE as NONE
from deneva_amd import RC_ABORT as AB
from deneva_amd import RC_RCOK as OK
from deneva_amd import RC_WAIT as WT
from deneva_amd import RD, SCAN, WD_GONE as GONE, WD_RUN as RUN, WR, XP

from tso_cases import make_ts

A, B, C, K = 11, 22, 33, 5

TS_FAMILIES = ("permuted", "jitter", "tied", "span63")

KATS = [
    # 1: T0 owns K (EX).  T1 conflicts; 5 > 10 is false: it waits.
    ("older_waits", [[(K, WR)], [(K, WR)]], [10, 5], [RUN, RUN],
     [("epoch", [OK, WT], [1, 0], [NONE, 0])]),
    # 2: the same with the ts swapped: 10 > 5, T1 dies.
    ("younger_dies", [[(K, WR)], [(K, WR)]], [5, 10], [RUN, RUN],
     [("epoch", [OK, AB], [1, 0], [NONE, 0])]),
    # 3: T0 SH owner.  T1 (EX, ts 5) conflicts, 5 > 10 false: waits.  T2 (SH, ts
    # 3) does not conflict with SH but 3 < the head's 5 (:74): conflict, 3 > 10
    # false: waits.  T3 (SH, ts 7): 7 < 5 false: owner.  T4 (SH, ts 4): 4 < 5:
    # conflict, 4 > min(10, 7) false: waits.  Queue: T1 (5), T4 (4), T2 (3).
    # 3a: T0 and T3 leave: lock_type NONE, the head T1 (EX) becomes the owner,
    # T4 conflicts with EX.  3b: T1 at pos 1 == len turns RCOK.  3c: T1 leaves:
    # T4 and T2 (both SH) are promoted.
    ("head_rule_and_promotion",
     [[(K, RD)], [(K, WR)], [(K, RD)], [(K, RD)], [(K, RD)]], [10, 5, 3, 7, 4], [RUN] * 5,
     [("epoch", [OK, WT, WT, OK, WT], [1, 0, 0, 1, 0], [NONE, 0, 0, NONE, 0]),
      ("release", [0, 3], [GONE, RUN, WT, GONE, WT], [1, 1, 0, 1, 0], 1),
      ("epoch", [GONE, OK, WT, GONE, WT], [1, 1, 0, 1, 0], [NONE] * 5),
      ("release", [1], [GONE, GONE, RUN, GONE, RUN], [1, 1, 1, 1, 1], 2)]),
    # 4: T1 gains A, dies on B (5 > 1) and releases A at once: T2 finds A free.
    ("died_txn_leaves_no_trace",
     [[(B, WR)], [(A, WR), (B, WR)], [(A, WR)]], [1, 5, 9], [RUN] * 3,
     [("epoch", [OK, AB, OK], [1, 0, 1], [NONE, 1, NONE])]),
    # 5: T1 gains A and waits on B (5 > 9 false), keeping A.  T2 (ts 7) meets
    # T1's A: 7 > 5, dies.  T3 (SH, ts 2) meets the EX owner: 2 > 5 false: waits.
    ("waiter_keeps_its_prefix",
     [[(B, WR)], [(A, WR), (B, WR)], [(A, WR)], [(A, RD)]], [9, 5, 7, 2], [RUN] * 4,
     [("epoch", [OK, WT, AB, WT], [1, 1, 0, 0], [NONE, 1, 0, 0])]),
    # 6: RD then WR of one row: the WR meets the txn's own SH entry; 5 > 5 is
    # false: it waits on itself.
    ("self_wait", [[(A, RD), (A, WR)]], [5], [RUN],
     [("epoch", [WT], [1], [1])]),
    # 6a: with an older SH owner in front the WR dies (5 > 1).
    ("self_conflict_dies", [[(A, RD)], [(A, RD), (A, WR)]], [1, 5], [RUN] * 2,
     [("epoch", [OK, AB], [1, 0], [NONE, 1])]),
    # 7: T1 gains A, waits on B.  T0 leaves: T1 is promoted to (RUN, 2).  T3 is
    # admitted.  Epoch 2: T1 requests C, owned by T2 (ts 1): 5 > 1, it dies as
    # (ABORT, 2) and still owns A and B (deferred cleanup); T3 (ts 3) meets T1's
    # A: 3 > 5 false: waits.  T1 leaves: T3 is promoted.
    ("deferred_cleanup",
     [[(B, WR)], [(A, WR), (B, WR), (C, WR)], [(C, WR)], [(A, WR)]], [9, 5, 1, 3], [RUN, RUN, RUN, GONE],
     [("epoch", [OK, WT, OK, GONE], [1, 1, 1, 0], [NONE, 1, NONE, NONE]),
      ("release", [0], [GONE, RUN, OK, GONE], [1, 2, 1, 0], 1),
      ("admit", [3]),
      ("epoch", [GONE, AB, OK, WT], [1, 2, 1, 0], [NONE, 2, NONE, 0]),
      ("release", [1], [GONE, GONE, OK, RUN], [1, 2, 1, 1], 1)]),
    # two SH requests of one txn on one row are two entries; SCAN is SH, XP is
    # EX.  T1 (XP, ts 4) meets them: 4 > 6 false: waits.  T0 leaves: promoted.
    ("two_entries_scan_xp",
     [[(A, RD), (A, SCAN)], [(A, XP)]], [6, 4], [RUN] * 2,
     [("epoch", [OK, WT], [2, 0], [NONE, 0]),
      ("release", [0], [GONE, RUN], [2, 1], 1)]),
    # ties: T1 and T2 (ts 5 both) wait behind T0 (5 > 7 false); among equal ts
    # the lower index is the head.  T0 leaves: only T1 (EX) is promoted.
    ("tied_waiters", [[(A, WR)], [(A, WR)], [(A, WR)]], [7, 5, 5], [RUN] * 3,
     [("epoch", [OK, WT, WT], [1, 0, 0], [NONE, 0, 0]),
      ("release", [0], [GONE, RUN, WT], [1, 1, 0], 1)]),
]


def new_state(n, rc=RUN):
    return np.full(n, rc, np.uint8), np.zeros(n, np.uint32)


def admit(rc, pos, idx):
    for i in idx:
        assert rc[i] == GONE
        rc[i], pos[i] = RUN, 0


def hot_batch(rng, n, max_len, n_keys, types=(RD, WR, XP, SCAN), p_sh=0.6):
    """Ragged random txns, lengths 0 .. max_len, rows drawn with replacement
    (a txn may name a row more than once), all four access types."""
    import deneva_amd as d
    lens = rng.integers(0, max_len + 1, size=n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    m = int(off[-1])
    keys = rng.integers(0, n_keys, size=m).astype(np.uint64) * np.uint64(7) + np.uint64(1)
    sh = [t for t in types if t in (RD, SCAN)]
    ex = [t for t in types if t not in (RD, SCAN)]
    at = np.where(rng.random(m) < p_sh, rng.choice(sh, size=m), rng.choice(ex, size=m)).astype(np.uint8)
    return d.EpochBatch(off, keys, at)


def history(rng, b, ts, replay_epoch, replay_release, epochs=6, p_start=0.5):
    """A multi-epoch history over one batch: admissions before every epoch, a
    release after it whose leavers come from every state plus a random mask.
    Returns the steps [("epoch", rc_in, pos_in, expect) | ("release", rc_in,
    pos_in, leave, expect)], the expectations computed by the given replays."""
    n = b.n_txn
    rc, pos = new_state(n, GONE)
    steps = []
    p_leave = {OK: 0.7, AB: 0.8, WT: 0.1, RUN: 0.05, GONE: 0.1}
    for e in range(epochs):
        adm = np.nonzero((rc == GONE) & (rng.random(n) < (p_start if e == 0 else 0.3)))[0]
        admit(rc, pos, adm)
        exp = replay_epoch(b, ts, rc, pos)
        steps.append(("epoch", rc.copy(), pos.copy(), exp))
        rc, pos = exp[0].copy(), exp[1].copy()
        u = rng.random(n)
        leave = (u < np.asarray([p_leave[int(s)] for s in rc])).astype(np.uint8)
        exp = replay_release(b, ts, rc, pos, leave)
        steps.append(("release", rc.copy(), pos.copy(), leave, exp))
        rc, pos = exp[0].copy(), exp[1].copy()
    return steps


def outcomes(steps):
    """(RCOK, ABORT, WAIT) decisions over the epochs of a history."""
    c = [0, 0, 0]
    for s in steps:
        if s[0] == "epoch":
            st = s[3][3]
            c[0] += st["n_commit"]
            c[1] += st["n_abort"]
            c[2] += st["n_survivors"]
    return tuple(c)


__all__ = ["KATS", "TS_FAMILIES", "make_ts", "new_state", "admit", "hot_batch", "history", "outcomes"]
