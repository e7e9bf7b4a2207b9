"""The three restatements of TIMESTAMP with txns in flight (tso_live_ref.py)
held against each other after every call: the literal Row_ts with its queues,
the closed forms and the engine's passes.  No GPU."""
import numpy as np
import pytest

from deneva_amd import RC_ABORT, RC_RCOK, RC_WAIT, RD, WD_GONE, WD_RUN, WR
from helpers import make_batch
import tso_live_ref as ref
from tso_live_cases import FAMILIES, KATS, SEEDS, admit, all_outcomes, history, new_state


def same(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b)), f"{what}: {np.asarray(a)} vs {np.asarray(b)}"


class Three:
    """The three replays side by side, each with its own rows."""

    def __init__(self, b, ts, rows=None):
        self.b, self.ts = b, ts
        self.seed(rows or {})

    def seed(self, rows):
        self.lit = ref.Literal(rows)
        self.closed = {k: list(v) for k, v in rows.items()}
        self.passes = {k: list(v) for k, v in rows.items()}

    def rows(self):
        return ref.rows_of(self.lit.state)

    def agree(self, outs, what):
        for k in range(len(outs[0])):
            for o in outs[1:]:
                if isinstance(outs[0][k], dict):
                    assert {x: o[k][x] for x in outs[0][k]} == outs[0][k], what
                else:
                    same(outs[0][k], o[k], what)
        assert ref.rows_of(self.lit.state) == ref.rows_of(self.closed) == ref.rows_of(self.passes), what + " rows"

    def epoch(self, rc, pos):
        outs = [self.lit.epoch(self.b, self.ts, rc, pos),
                ref.epoch(self.b, self.ts, rc, pos, self.closed),
                ref.rounds_epoch(self.b, self.ts, rc, pos, self.passes)]
        self.agree(outs, "epoch")
        self.lit.buffers_match(self.b, self.ts, outs[0][0], outs[0][1])
        return outs[2]

    def finish(self, rc, pos, leave, order=None):
        outs = [self.lit.finish(self.b, self.ts, rc, pos, leave, order),
                ref.finish(self.b, self.ts, rc, pos, leave, self.closed),
                ref.rounds_finish(self.b, self.ts, rc, pos, leave, self.passes)]
        self.agree(outs, "finish")
        self.lit.buffers_match(self.b, self.ts, outs[0][0], outs[0][1])
        return outs[0]


@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_hand_cases(case):
    _, txns, ts, rc0, steps = case
    b = make_batch(txns)
    ts = np.asarray(ts, np.uint64)
    t = Three(b, ts)
    rc, pos = np.asarray(rc0, np.uint8), np.zeros(len(txns), np.uint32)
    for s in steps:
        if s[0] == "seed":
            t.seed(s[1])
        elif s[0] == "admit":
            admit(rc, pos, s[1])
        elif s[0] == "epoch":
            rc, pos, cf, _ = t.epoch(rc, pos)
            assert (rc.tolist(), pos.tolist(), cf.tolist(), t.rows()) == (s[1], s[2], s[3], s[4])
        else:
            leave = np.zeros(len(txns), np.uint8)
            leave[s[1]] = 1
            rc, pos, left, prom = t.finish(rc, pos, leave)
            assert (rc.tolist(), pos.tolist(), left, prom, t.rows()) == (s[2], s[3], len(s[1]), s[4], s[5])


@pytest.mark.parametrize("family", FAMILIES)
def test_histories(family):
    """Eight epochs with two finishes after each, in every ts family and over
    seeded rows; duplicate rows in a txn, all four access types, RUN leavers.
    The literal replay releases the leavers of every other finish in reverse
    order.  Each family's histories show RCOK, an abort on rts, an abort on wts
    by a read and by a write, WAIT, a promotion and a finish that promotes
    nobody."""
    seen = {"run_leavers": 0, "rounds": 0}
    total = {}
    for seed in SEEDS[family]:
        b, ts, rows0, steps, tot = history(seed, family)
        for k, v in tot.items():
            total[k] = total.get(k, 0) + v
        t = Three(b, ts, rows0)
        for q, s in enumerate(steps):
            if s[0] == "epoch":
                got = t.epoch(s[1], s[2])
                for k in range(3):
                    same(got[k], s[3][k], "epoch against the driver")
                seen["rounds"] = max(seen["rounds"], got[3]["rounds"])
            else:
                order = list(reversed(range(b.n_txn))) if q % 2 else None
                got = t.finish(s[1], s[2], s[3], order)
                assert (got[2], got[3]) == (s[4][2], s[4][3])
            assert t.rows() == s[-1]
        seen["run_leavers"] += tot["run_leavers"]
    all_outcomes(total, family)
    assert seen["run_leavers"] > 0 and seen["rounds"] > 2


def test_the_literal_replay_raises_where_a_fact_fails():
    """The three facts are checked, not assumed."""
    m = ref.LiveRowTs()  # 1: a committing writer whose prewrite is not the row's least
    m.prereq, m.min_pts = [(0, 3), (1, 5)], 3
    with pytest.raises(AssertionError, match="W_REQ at 5, min_pts 3"):
        m.access(1, ref.W_REQ, 5)
    m = ref.LiveRowTs()  # 2: a buffered write
    m.prereq, m.min_pts = [(1, 5)], 5
    m.writereq, m.min_wts = [(2, 7)], 7
    with pytest.raises(AssertionError, match="a write request is buffered"):
        m.access(1, ref.XP_REQ, 5)
    m = ref.LiveRowTs()  # 2: the write branch of update_buffer
    m.prereq, m.min_pts = [(1, 5), (2, 7)], 5
    m.readreq, m.min_rts = [(3, 6)], 6
    m.writereq, m.min_wts = [(2, 7)], 7
    with pytest.raises(AssertionError, match="performed a buffered write"):
        m._access(1, ref.XP_REQ, 5)
    m = ref.LiveRowTs()  # 3: a stale cached minimum
    m.prereq, m.min_pts = [(1, 5)], 4
    with pytest.raises(AssertionError, match="cached minimum"):
        m.access(2, ref.R_REQ, 3)
    m = ref.LiveRowTs()  # 3: a buffered read at or below min_pts
    m.prereq, m.min_pts = [(1, 5)], 5
    m.readreq, m.min_rts = [(2, 5)], 5
    with pytest.raises(AssertionError, match="not above min_pts"):
        m.access(3, ref.R_REQ, 1)


def test_rejections_and_any_ts():
    b = make_batch([[(1, WR)], [(1, RD)]])
    ts = np.asarray([5, 9], np.uint64)
    rc, pos = new_state(2)
    # 0 and UINT64_MAX are ordinary timestamps
    for any_ts in ([0, 9], [5, (1 << 64) - 1]):
        for f in (ref.epoch, ref.rounds_epoch, ref.Literal().epoch):
            assert f(b, np.asarray(any_ts, np.uint64), rc, pos)[0].tolist() == [RC_RCOK, RC_WAIT]
    # a WAIT txn cannot leave
    e = ref.epoch(b, ts, rc, pos)
    assert e[0].tolist() == [RC_RCOK, RC_WAIT]
    for f in (ref.finish, ref.rounds_finish, ref.Literal().finish):
        with pytest.raises(ValueError):
            f(b, ts, e[0], e[1], np.asarray([0, 1], np.uint8))
    for bad in ((np.asarray([7, WD_RUN], np.uint8), pos), (rc, np.asarray([2, 0], np.uint32)),
                (np.asarray([RC_RCOK, WD_RUN], np.uint8), pos),
                (np.asarray([RC_WAIT, WD_RUN], np.uint8), np.asarray([1, 0], np.uint32))):
        for f in (ref.epoch, ref.rounds_epoch, ref.Literal().epoch):
            with pytest.raises(ValueError):
                f(b, ts, *bad)
    assert RD != WR and RC_ABORT != WD_GONE
