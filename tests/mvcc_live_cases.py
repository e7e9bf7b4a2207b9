"""Hand cases and random histories of MVCC with txns in flight, shared by the
CPU reference tests (test_mvcc_live_ref.py) and the GPU parity tests
(test_gpu_mvcc_live.py).

A hand case is (name, txns, ts, rc0, steps); a step is
  ("admit", [txn, ...])                                GONE -> (RUN, 0)
  ("epoch", rc, pos, conflict, vts)                    the state after it
  ("finish", [leaver, ...], rc, pos, n_promoted, vts)  the state after it
vts is the caller-kept versions array (N: never written).
"""
import numpy as np

from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RC_WAIT, RD, SCAN, VTS_NONE, WD_GONE, WD_RUN, WR, XP
from helpers import make_batch
from mvcc_ref import rows_of, trim, versions_of
import mvcc_live_ref as ref

A, B, C = 11, 22, 33
RUN, OK, WT, AB, GONE, NONE, N = WD_RUN, RC_RCOK, RC_WAIT, RC_ABORT, WD_GONE, ACCESS_NONE, VTS_NONE

KATS = [
    # 1: T0 prewrites A at 5 and reads the base row.  T1 (ts 9) finds a pending
    # prewrite below 9: buffered.  T0 commits: version 5 is installed, T1 is
    # promoted, reads it and, at pos == len, turns RCOK in the next epoch.
    ("commit_promotes_reader", [[(A, WR)], [(A, RD)]], [5, 9], [RUN, RUN],
     [("epoch", [OK, WT], [1, 0], [NONE, 0], [0, N]),
      ("finish", [0], [GONE, RUN], [1, 1], 1, [0, 5]),
      ("epoch", [GONE, OK], [1, 1], [NONE, NONE], [0, 5])]),
    # 2: T0 reads B at 8.  T1 (ts 5) prewrites A, then its P_REQ on B aborts
    # (5 < 8): it keeps A's prewrite, so T2 (ts 9) is buffered behind an aborted
    # txn.  T1's release (XP_REQ) promotes T2, which reads the old version.
    ("abort_promotes_reader_old_version", [[(B, RD)], [(A, WR), (B, WR)], [(A, RD)]], [8, 5, 9], [RUN] * 3,
     [("epoch", [OK, AB, WT], [1, 1, 0], [NONE, 1, 0], [0, 0, N, N]),
      ("finish", [1], [OK, GONE, RUN], [1, 1, 1], 1, [0, 0, N, 0])]),
    # 3: prewrites at 3 (T0) and 7 (T1, itself buffered behind 3 at its own
    # R_REQ).  T2 (ts 5) lies between them, T3 (ts 9) above both.  A finish in
    # which nobody goes promotes nobody.  T0's commit promotes T1 and T2 (both
    # read 3); T3 stays behind T1's prewrite until T1 commits, then reads 7.
    ("between_two_prewrites", [[(A, WR)], [(A, WR)], [(A, RD)], [(A, SCAN)]], [3, 7, 5, 9], [RUN] * 4,
     [("epoch", [OK, WT, WT, WT], [1, 0, 0, 0], [NONE, 0, 0, 0], [0, N, N, N]),
      ("finish", [], [OK, WT, WT, WT], [1, 0, 0, 0], 0, [0, N, N, N]),
      ("finish", [0], [GONE, RUN, RUN, WT], [1, 1, 1, 0], 2, [0, 3, 3, N]),
      ("epoch", [GONE, OK, OK, WT], [1, 1, 1, 0], [NONE, NONE, NONE, NONE], [0, 3, 3, N]),
      ("finish", [1, 2], [GONE, GONE, GONE, RUN], [1, 1, 1, 1], 1, [0, 3, 3, 7])]),
    # 4: T1's WR passes P_REQ (7 >= rts 3) and waits at its own R_REQ; the
    # prewrite it made blocks T2 (ts 9) even once T0 is gone.
    ("waiting_writer_blocks_reader", [[(A, WR)], [(A, WR), (B, RD)], [(A, RD)]], [3, 7, 9], [RUN] * 3,
     [("epoch", [OK, WT, WT], [1, 0, 0], [NONE, 0, 0], [0, N, N, N]),
      ("finish", [0], [GONE, RUN, WT], [1, 1, 0], 1, [0, 3, N, N]),
      ("epoch", [GONE, OK, WT], [1, 2, 0], [NONE, NONE, NONE], [0, 3, 0, N])]),
    # 5: equal timestamps never block or abort each other.
    ("ties_pass", [[(A, WR)], [(A, WR)], [(A, RD)]], [5, 5, 5], [RUN] * 3,
     [("epoch", [OK, OK, OK], [1, 1, 1], [NONE, NONE, NONE], [0, 0, 0]),
      ("finish", [0, 1, 2], [GONE, GONE, GONE], [1, 1, 1], 0, [0, 0, 0])]),
    # 6: T1 aborted in epoch 1 and was not released: T3, admitted later, still
    # waits behind its prewrite on A.
    ("deferred_prewrite_blocks", [[(B, RD)], [(A, WR), (B, WR)], [], [(A, RD)]], [8, 5, 1, 6], [RUN, RUN, RUN, GONE],
     [("epoch", [OK, AB, OK, GONE], [1, 1, 0, 0], [NONE, 1, NONE, NONE], [0, 0, N, N]),
      ("admit", [3]),
      ("epoch", [OK, AB, OK, WT], [1, 1, 0, 0], [NONE, NONE, NONE, 0], [0, 0, N, N]),
      ("finish", [1, 2], [OK, GONE, GONE, RUN], [1, 1, 0, 1], 1, [0, 0, N, 0]),
      ("epoch", [OK, GONE, GONE, OK], [1, 1, 0, 1], [NONE, NONE, NONE, NONE], [0, 0, N, 0])]),
    # 7: a txn's own prewrite never blocks its later accesses of the row, XP
    # sends nothing, and a WR below rts aborts at its ordinal.
    ("own_prewrite_xp_and_abort_ordinal", [[(A, WR), (A, RD), (A, XP), (A, WR)], [(B, RD), (C, XP), (A, WR)]],
     [9, 4], [RUN, RUN],
     [("epoch", [OK, AB], [4, 2], [NONE, 2], [0, 0, N, 0, 0, N, N])]),
]


def new_state(n, rc=RUN):
    return np.full(n, rc, np.uint8), np.zeros(n, np.uint32)


def admit(rc, pos, idx):
    for i in idx:
        assert rc[i] == GONE
        rc[i], pos[i] = RUN, 0


FAMILIES = ("index", "jitter", "permuted", "tied", "wrap")


def make_ts(rng, n, family):
    i = np.arange(n, dtype=np.uint64)
    if family == "index":
        return i + np.uint64(1)
    if family == "jitter":
        return i * np.uint64(8) + rng.integers(1, 17, size=n).astype(np.uint64)
    if family == "permuted":
        return rng.permutation(n).astype(np.uint64) + np.uint64(1)
    if family == "tied":
        return i // np.uint64(3) + np.uint64(1)
    assert family == "wrap"  # across 2^63
    return np.uint64((1 << 63) - n // 2) + i


def hot_batch(rng, n, max_len, n_rows, min_len=1, key_base=0, key_step=1):
    """Ragged random txns over n_rows rows, all four access types; a txn names
    a row it already named with probability 0.2."""
    txns = []
    for _ in range(n):
        t = []
        for _ in range(int(rng.integers(min_len, max_len + 1))):
            if t and rng.random() < 0.2:
                k = t[int(rng.integers(len(t)))][0]
            else:
                k = key_base + key_step * int(rng.integers(n_rows))
            t.append((k, int(rng.choice([RD, WR, XP, SCAN], p=[.5, .3, .1, .1]))))
        txns.append(t)
    return make_batch(txns)


def history(seed, family, epochs=8, per_epoch=60, n_rows=40, max_len=4, batch=None, p_leave=0.6, trim_after=5):
    """A history over one batch of epochs * per_epoch txns: per_epoch txns are
    admitted before every epoch; after it p_leave of the RCOK / ABORT txns
    leave, and in a second finish a sixth of the RUN ones (promoted by the
    first); a trim follows the finishes of epoch `trim_after`, at the least ts
    still to come or in flight.  Driven by the
    closed form.  Returns (batch, ts, steps, totals); a step is
      ("epoch", rc_in, pos_in, vts_in, expect, vts_out, rows, versions)
      ("finish", rc_in, pos_in, leave, vts_in, expect, vts_out, rows, versions)
      ("trim", floor, dropped, rows, versions)
    and totals counts RCOK / ABORT / WAIT decisions, promotions and reads of a
    version that is not the row's latest."""
    rng = np.random.default_rng(seed)
    n = epochs * per_epoch
    b = batch if batch is not None else hot_batch(rng, n, max_len, n_rows)
    assert b.n_txn == n
    ts = make_ts(rng, n, family)
    rc, pos = new_state(n, GONE)
    vts = ref.new_vts(b)
    state = {}
    steps = []
    info = {}
    tot = {"rcok": 0, "abort": 0, "wait": 0, "promoted": 0, "late": 0, "run_leavers": 0, "trimmed": 0}
    snap = lambda: (rows_of(state), versions_of(state))
    for e in range(epochs):
        admit(rc, pos, range(e * per_epoch, (e + 1) * per_epoch))
        vin = vts.copy()
        exp = ref.epoch(b, ts, rc, pos, vts, state, info)
        steps.append(("epoch", rc.copy(), pos.copy(), vin, exp, vts.copy()) + snap())
        rc, pos = exp[0].copy(), exp[1].copy()
        tot["rcok"] += exp[3]["n_commit"]
        tot["abort"] += exp[3]["n_abort"]
        tot["wait"] += exp[3]["n_survivors"]
        for second in (False, True):
            u = rng.random(n)
            leave = ((rc == RUN) & (u < 1 / 6) if second else np.isin(rc, [OK, AB]) & (u < p_leave)).astype(np.uint8)
            tot["run_leavers"] += int(((rc == RUN) & (leave != 0)).sum())
            vin = vts.copy()
            exp = ref.finish(b, ts, rc, pos, leave, vts, state, info)
            steps.append(("finish", rc.copy(), pos.copy(), leave, vin, exp, vts.copy()) + snap())
            rc, pos = exp[0].copy(), exp[1].copy()
            tot["promoted"] += exp[3]
        if e + 1 == trim_after:
            live = np.ones(n, bool)
            live[:(e + 1) * per_epoch] = rc[:(e + 1) * per_epoch] != GONE
            floor = int(ts[live].min()) if live.any() else 0
            dropped = trim(state, floor)
            tot["trimmed"] += dropped
            steps.append(("trim", floor, dropped) + snap())
    tot["late"] = info.get("late", 0)
    return b, ts, steps, tot


def five_outcomes(tot):
    assert min(tot["rcok"], tot["abort"], tot["wait"], tot["promoted"], tot["late"]) > 0, \
        f"the history misses an outcome: {tot}"
