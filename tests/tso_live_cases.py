"""Hand cases and random histories of TIMESTAMP with txns in flight, shared by
the CPU reference tests (test_tso_live_ref.py) and the GPU parity tests
(test_gpu_tso_live.py).

A hand case is (name, txns, ts, rc0, steps); a step is
  ("seed", {key: (wts, rts)})                           dcc_tso_rows_set
  ("admit", [txn, ...])                                 GONE -> (RUN, 0)
  ("epoch", rc, pos, conflict, rows)                    the state after it
  ("finish", [leaver, ...], rc, pos, n_promoted, rows)  the state after it
rows: key -> (wts, rts) of every row that is not (0, 0).
"""
import numpy as np

from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RC_WAIT, RD, SCAN, WD_GONE, WD_RUN, WR, XP
from mvcc_live_cases import FAMILIES as TS_FAMILIES, admit, hot_batch, make_ts, new_state
import tso_live_ref as ref

A, B, C = 11, 22, 33
RUN, OK, WT, AB, GONE, NONE = WD_RUN, RC_RCOK, RC_WAIT, RC_ABORT, WD_GONE, ACCESS_NONE
U = (1 << 64) - 1

KATS = [
    # 1: against a seeded wts of 5 a read at 4 aborts at its ordinal, a read at
    # 5 passes (the test is strict) and raises rts.
    ("read_below_seeded_wts", [[(B, RD), (A, RD)], [(A, RD)], [(A, SCAN)]], [4, 5, 3], [RUN] * 3,
     [("seed", {A: (5, 0)}),
      ("epoch", [AB, OK, AB], [1, 1, 0], [1, NONE, 0], {A: (5, 5), B: (0, 4)})]),
    # 2: T0 prewrites A at 5 and reads it.  T1 (ts 9) finds a pending prewrite
    # below 9: buffered.  T0 commits: wts = 5, T1 is promoted and raises rts to
    # 9.  A later WR at 7 aborts on rts, a later RD at 3 on wts.
    ("commit_promotes_reader_and_raises_wts", [[(A, WR)], [(A, RD)], [(A, WR)], [(A, RD)]], [5, 9, 7, 3],
     [RUN, RUN, GONE, GONE],
     [("epoch", [OK, WT, GONE, GONE], [1, 0, 0, 0], [NONE, 0, NONE, NONE], {A: (0, 5)}),
      ("finish", [0], [GONE, RUN, GONE, GONE], [1, 1, 0, 0], 1, {A: (5, 9)}),
      ("admit", [2, 3]),
      ("epoch", [GONE, OK, AB, AB], [1, 1, 0, 0], [NONE, NONE, 0, 0], {A: (5, 9)})]),
    # 3: T0 reads B at 8.  T1 (ts 5) prewrites A, then its P_REQ on B aborts
    # (5 < 8): it keeps A's prewrite, so T2 (ts 9) is buffered behind an aborted
    # txn.  T1's release (XP_REQ) promotes T2 and leaves wts alone.
    ("abort_release_promotes_without_wts", [[(B, RD)], [(A, WR), (B, WR)], [(A, RD)]], [8, 5, 9], [RUN] * 3,
     [("epoch", [OK, AB, WT], [1, 1, 0], [NONE, 1, 0], {A: (0, 5), B: (0, 8)}),
      ("finish", [1], [OK, GONE, RUN], [1, 1, 1], 1, {A: (0, 9), B: (0, 8)})]),
    # 4: WR at 3 (T0), 7 (T1) and 5 (T2) on one row: T1 and T2 wait at their own
    # R_REQ behind 3, each holding its prewrite.  A finish in which nobody goes
    # promotes nobody.  Finishing the 3 promotes 5 (the least remaining
    # prewrite is its own) and leaves 7 behind it; finishing 5 promotes 7.
    ("between_two_prewrites", [[(A, WR)], [(A, WR)], [(A, WR)]], [3, 7, 5], [RUN] * 3,
     [("epoch", [OK, WT, WT], [1, 0, 0], [NONE, 0, 0], {A: (0, 3)}),
      ("finish", [], [OK, WT, WT], [1, 0, 0], 0, {A: (0, 3)}),
      ("finish", [0], [GONE, WT, RUN], [1, 0, 1], 1, {A: (3, 5)}),
      ("epoch", [GONE, WT, OK], [1, 0, 1], [NONE, NONE, NONE], {A: (3, 5)}),
      ("finish", [2], [GONE, RUN, GONE], [1, 1, 1], 1, {A: (5, 7)})]),
    # 5: T1's WR passes P_REQ (7 >= rts 3) and waits at its own R_REQ; the
    # prewrite it made blocks T2 (ts 9) even once T0 is gone.
    ("waiting_writer_blocks_reader", [[(A, WR)], [(A, WR), (B, RD)], [(A, RD)]], [3, 7, 9], [RUN] * 3,
     [("epoch", [OK, WT, WT], [1, 0, 0], [NONE, 0, 0], {A: (0, 3)}),
      ("finish", [0], [GONE, RUN, WT], [1, 1, 0], 1, {A: (3, 7)}),
      ("epoch", [GONE, OK, WT], [1, 2, 0], [NONE, NONE, NONE], {A: (3, 7), B: (0, 7)})]),
    # 6: equal timestamps never block or abort each other.
    ("ties_pass", [[(A, WR)], [(A, WR)], [(A, RD)]], [5, 5, 5], [RUN] * 3,
     [("epoch", [OK, OK, OK], [1, 1, 1], [NONE, NONE, NONE], {A: (0, 5)}),
      ("finish", [0, 1, 2], [GONE, GONE, GONE], [1, 1, 1], 0, {A: (5, 5)})]),
    # 7: T1 aborted in epoch 1 and was not released: T3, admitted later, still
    # waits behind its prewrite on A.
    ("deferred_prewrite_blocks", [[(B, RD)], [(A, WR), (B, WR)], [], [(A, RD)]], [8, 5, 1, 6], [RUN, RUN, RUN, GONE],
     [("epoch", [OK, AB, OK, GONE], [1, 1, 0, 0], [NONE, 1, NONE, NONE], {A: (0, 5), B: (0, 8)}),
      ("admit", [3]),
      ("epoch", [OK, AB, OK, WT], [1, 1, 0, 0], [NONE, NONE, NONE, 0], {A: (0, 5), B: (0, 8)}),
      ("finish", [1, 2], [OK, GONE, GONE, RUN], [1, 1, 0, 1], 1, {A: (0, 6), B: (0, 8)}),
      ("epoch", [OK, GONE, GONE, OK], [1, 1, 0, 1], [NONE, NONE, NONE, NONE], {A: (0, 6), B: (0, 8)})]),
    # 8: a txn's own prewrite never blocks its later accesses of the row, XP
    # sends nothing, and a WR below rts aborts at its ordinal.
    ("own_prewrite_xp_and_abort_ordinal", [[(A, WR), (A, RD), (A, XP), (A, WR)], [(B, RD), (C, XP), (A, WR)]],
     [9, 4], [RUN, RUN],
     [("epoch", [OK, AB], [4, 2], [NONE, 2], {A: (0, 9), B: (0, 4)})]),
    # 9: a finish in which nobody goes, on a state with waiters and an aborted txn.
    ("nobody_goes", [[(A, WR)], [(A, RD)], [(A, WR)]], [5, 9, 2], [RUN] * 3,
     [("epoch", [OK, WT, AB], [1, 0, 0], [NONE, 0, 0], {A: (0, 5)}),
      ("finish", [], [OK, WT, AB], [1, 0, 0], 0, {A: (0, 5)})]),
    # 10: ts 0 and UINT64_MAX as writers and as readers.  A prewrite at 0 blocks
    # every larger read; one at UINT64_MAX blocks nobody, as no prewrite would.
    # Behind the commits (wts(B) = rts(A) = UINT64_MAX) a read at 0 aborts on
    # wts and a write at 0 on rts.
    ("ts_zero_and_max", [[(A, WR)], [(A, RD)], [(B, WR)], [(B, RD)], [(B, RD)], [(B, RD)], [(A, WR)]],
     [0, U, U, 0, U, 0, 0], [RUN] * 5 + [GONE] * 2,
     [("epoch", [OK, WT, OK, OK, OK, GONE, GONE], [1, 0, 1, 1, 1, 0, 0], [NONE, 0, NONE, NONE, NONE, NONE, NONE],
       {B: (0, U)}),
      ("finish", [0, 2], [GONE, RUN, GONE, OK, OK, GONE, GONE], [1, 1, 1, 1, 1, 0, 0], 1, {A: (0, U), B: (U, U)}),
      ("admit", [5, 6]),
      ("epoch", [GONE, OK, GONE, OK, OK, AB, AB], [1, 1, 1, 1, 1, 0, 0], [NONE, NONE, NONE, NONE, NONE, 0, 0],
       {A: (0, U), B: (U, U)})]),
]

# the five of mvcc_live_cases.py, and "permuted" timestamps over rows seeded
# with (wts, rts) on either side of each other
FAMILIES = TS_FAMILIES + ("seeded",)
# histories per family whose totals together show every outcome (found on the CPU)
SEEDS = {f: (100, 101, 102, 103) for f in FAMILIES}


def seed_rows(rng, n, n_rows, key_base=0, key_step=1):
    """(wts, rts) in [0, n] for about half of the rows; wts above rts in some,
    which no run of the calls produces."""
    rows = {}
    for r in range(n_rows):
        if rng.random() < 0.5:
            rows[key_base + key_step * r] = (int(rng.integers(0, n + 1)), int(rng.integers(0, n + 1)))
    return rows


def history(seed, family, epochs=8, per_epoch=60, n_rows=40, max_len=4, batch=None, p_leave=0.6):
    """A history over one batch of epochs * per_epoch txns: per_epoch txns are
    admitted before every epoch; after it p_leave of the RCOK / ABORT txns
    leave, and in a second finish a sixth of the RUN ones (promoted by the
    first).  Driven by the closed form.  Returns (batch, ts, rows0, steps,
    totals); rows0 are the seeded rows and a step is
      ("epoch", rc_in, pos_in, expect, rows)
      ("finish", rc_in, pos_in, leave, expect, rows)
    totals counts the decisions, the aborts by cause (tso_live_ref.epoch's
    info), promotions and the finishes that promoted nobody."""
    rng = np.random.default_rng(seed)
    n = epochs * per_epoch
    b = batch if batch is not None else hot_batch(rng, n, max_len, n_rows)
    assert b.n_txn == n
    ts = make_ts(rng, n, "permuted" if family == "seeded" else family)
    rows0 = seed_rows(rng, n, n_rows) if family == "seeded" else {}
    rc, pos = new_state(n, GONE)
    state = {k: list(v) for k, v in rows0.items()}
    steps = []
    tot = {"rcok": 0, "abort": 0, "wait": 0, "promoted": 0, "zero_prom": 0, "run_leavers": 0, "ab_rts": 0,
           "ab_wts_rd": 0, "ab_wts_wr": 0, "ab_wts_wr_only": 0}
    for e in range(epochs):
        admit(rc, pos, range(e * per_epoch, (e + 1) * per_epoch))
        exp = ref.epoch(b, ts, rc, pos, state, tot)
        steps.append(("epoch", rc.copy(), pos.copy(), exp, ref.rows_of(state)))
        rc, pos = exp[0].copy(), exp[1].copy()
        tot["rcok"] += exp[3]["n_commit"]
        tot["abort"] += exp[3]["n_abort"]
        tot["wait"] += exp[3]["n_survivors"]
        for second in (False, True):
            u = rng.random(n)
            leave = ((rc == RUN) & (u < 1 / 6) if second else np.isin(rc, [OK, AB]) & (u < p_leave)).astype(np.uint8)
            tot["run_leavers"] += int(((rc == RUN) & (leave != 0)).sum())
            exp = ref.finish(b, ts, rc, pos, leave, state)
            steps.append(("finish", rc.copy(), pos.copy(), leave, exp, ref.rows_of(state)))
            rc, pos = exp[0].copy(), exp[1].copy()
            tot["promoted"] += exp[3]
            tot["zero_prom"] += exp[3] == 0
    return b, ts, rows0, steps, tot


OUTCOMES = ("rcok", "ab_rts", "ab_wts_rd", "ab_wts_wr", "wait", "promoted", "zero_prom")


def all_outcomes(tot, family=None):
    """RCOK, an abort on rts, an abort on wts by a read and by a write, WAIT, a
    promotion and a finish with zero promotions.  Rows reached by the calls
    alone keep rts >= wts (a committed writer's own read raised rts first), so
    there a write below wts is below rts too; only seeded rows show a write
    that aborts on wts alone."""
    assert min(tot[k] for k in OUTCOMES) > 0, f"the histories miss an outcome: {tot}"
    if family == "seeded":
        assert tot["ab_wts_wr_only"] > 0, tot
