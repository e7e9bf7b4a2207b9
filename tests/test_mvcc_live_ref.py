"""The three restatements of MVCC with txns in flight (mvcc_live_ref.py) held
against each other after every call: the literal Row_mvcc with its buffers, the
closed forms and the engine's passes.  No GPU."""
import numpy as np
import pytest

from deneva_amd import RC_RCOK, RC_WAIT, RD, VTS_NONE, WD_GONE, WD_RUN, WR
from helpers import make_batch
from mvcc_ref import rows_of, trim, trim_literal, versions_of
import mvcc_live_ref as ref
from mvcc_live_cases import FAMILIES, KATS, admit, five_outcomes, history, new_state


def same(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b)), f"{what}: {np.asarray(a)} vs {np.asarray(b)}"


class Three:
    """The three replays side by side, each with its own rows and versions."""

    def __init__(self, b, ts):
        self.b, self.ts = b, ts
        self.lit = ref.Literal()
        self.closed, self.passes = {}, {}
        self.vts = [ref.new_vts(b) for _ in range(3)]

    def agree(self, outs, what):
        for k in range(len(outs[0])):
            for o in outs[1:]:
                if isinstance(outs[0][k], dict):
                    assert {x: o[k][x] for x in outs[0][k]} == outs[0][k], what
                else:
                    same(outs[0][k], o[k], what)
        same(self.vts[0], self.vts[1], what + " vts literal / closed")
        same(self.vts[0], self.vts[2], what + " vts literal / passes")
        assert rows_of(self.lit.state) == rows_of(self.closed) == rows_of(self.passes), what + " rows"
        assert versions_of(self.lit.state) == versions_of(self.closed) == versions_of(self.passes), what

    def epoch(self, rc, pos):
        outs = [self.lit.epoch(self.b, self.ts, rc, pos, self.vts[0]),
                ref.epoch(self.b, self.ts, rc, pos, self.vts[1], self.closed),
                ref.rounds_epoch(self.b, self.ts, rc, pos, self.vts[2], self.passes)]
        self.agree(outs, "epoch")
        self.lit.buffers_match(self.b, self.ts, outs[0][0], outs[0][1])
        return outs[2]

    def finish(self, rc, pos, leave):
        outs = [self.lit.finish(self.b, self.ts, rc, pos, leave, self.vts[0]),
                ref.finish(self.b, self.ts, rc, pos, leave, self.vts[1], self.closed),
                ref.rounds_finish(self.b, self.ts, rc, pos, leave, self.vts[2], self.passes)]
        self.agree(outs, "finish")
        self.lit.buffers_match(self.b, self.ts, outs[0][0], outs[0][1])
        return outs[0]

    def trim(self, floor):
        got = [trim_literal(self.lit.state, floor), trim(self.closed, floor), trim(self.passes, floor)]
        assert got[0] == got[1] == got[2]
        return got[0]


@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_hand_cases(case):
    _, txns, ts, rc0, steps = case
    b = make_batch(txns)
    ts = np.asarray(ts, np.uint64)
    t = Three(b, ts)
    rc, pos = np.asarray(rc0, np.uint8), np.zeros(len(txns), np.uint32)
    for s in steps:
        if s[0] == "admit":
            admit(rc, pos, s[1])
        elif s[0] == "epoch":
            rc, pos, cf, _ = t.epoch(rc, pos)
            assert (rc.tolist(), pos.tolist(), cf.tolist(), t.vts[0].tolist()) == (s[1], s[2], s[3], s[4])
        else:
            leave = np.zeros(len(txns), np.uint8)
            leave[s[1]] = 1
            rc, pos, left, prom = t.finish(rc, pos, leave)
            assert (rc.tolist(), pos.tolist(), left, prom, t.vts[0].tolist()) == (s[2], s[3], len(s[1]), s[4], s[5])


@pytest.mark.parametrize("family", FAMILIES)
def test_histories(family):
    """Eight epochs with two finishes after each and a trim in between, in every ts
    family; duplicate rows in a txn, all four access types, RUN leavers.  Each
    family's history shows RCOK, ABORT, WAIT, a promotion and a read of a
    version that is not the row's latest."""
    seen = {"trimmed": 0, "run_leavers": 0, "rounds": 0}
    for seed in range(4):
        b, ts, steps, tot = history(100 + seed, family)
        five_outcomes(tot)
        t = Three(b, ts)
        for s in steps:
            if s[0] == "epoch":
                got = t.epoch(s[1], s[2])
                for k in range(3):
                    same(got[k], s[4][k], "epoch against the driver")
                seen["rounds"] = max(seen["rounds"], got[3]["rounds"])
            elif s[0] == "finish":
                got = t.finish(s[1], s[2], s[3])
                assert (got[2], got[3]) == (s[5][2], s[5][3])
            else:
                assert t.trim(s[1]) == s[2]
            assert (rows_of(t.closed), versions_of(t.closed)) == (s[-2], s[-1])
            if s[0] != "trim":
                same(t.vts[1], s[-3], "vts against the driver")
        seen["trimmed"] += tot["trimmed"]
        seen["run_leavers"] += tot["run_leavers"]
    assert seen["run_leavers"] > 0 and seen["rounds"] > 2
    if family in ("index", "jitter", "wrap"):
        assert seen["trimmed"] > 0


def test_the_literal_replay_raises_where_the_closed_form_would_be_wrong():
    """The three facts are checked, not assumed."""
    m = ref.LiveRow()
    m.writehis = [9]
    m.prereq = [(0, 5)]
    with pytest.raises(AssertionError, match="below the row's latest version"):
        m.check()
    m = ref.LiveRow()
    m.readhis, m.writehis, m.prereq = [9, 5], [9], [(1, 5)]
    with pytest.raises(AssertionError, match="below the row's latest"):
        m.access(1, ref.W_REQ, 5)
    m = ref.LiveRow()
    m.prereq = [(1, 5)]
    with pytest.raises(AssertionError, match="not in the read history"):
        m.access(1, ref.W_REQ, 5)


def test_rejections():
    b = make_batch([[(1, WR)], [(1, RD)]])
    ts = np.asarray([5, 9], np.uint64)
    rc, pos = new_state(2)
    for bad_ts in ([0, 9], [5, (1 << 64) - 1]):
        for f in (ref.epoch, ref.rounds_epoch, ref.Literal().epoch):
            with pytest.raises(ValueError):
                f(b, np.asarray(bad_ts, np.uint64), rc, pos)
    # the ts of a GONE txn is not looked at
    ref.epoch(b, np.asarray([0, 9], np.uint64), np.asarray([WD_GONE, WD_RUN], np.uint8), pos)
    # a WAIT txn cannot leave
    e = ref.epoch(b, ts, rc, pos)
    assert e[0].tolist() == [RC_RCOK, RC_WAIT]
    for f in (ref.finish, ref.rounds_finish, ref.Literal().finish):
        with pytest.raises(ValueError):
            f(b, ts, e[0], e[1], np.asarray([0, 1], np.uint8))
    for bad in ((np.asarray([7, WD_RUN], np.uint8), pos), (rc, np.asarray([2, 0], np.uint32)),
                (np.asarray([RC_RCOK, WD_RUN], np.uint8), pos), (np.asarray([RC_WAIT, WD_RUN], np.uint8), np.asarray([1, 0], np.uint32))):
        with pytest.raises(ValueError):
            ref.epoch(b, ts, *bad)
    assert ref.new_vts(b).tolist() == [VTS_NONE] * 2 and RD != WR
