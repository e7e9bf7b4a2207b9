"""The three restatements of WAIT_DIE (waitdie_ref.py) agree with one another
and with the hand-worked answers (waitdie_cases.py); every random family shows
all three outcomes.  No GPU."""
import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RC_WAIT, RD, WD_GONE, WD_RUN, WR
from helpers import make_batch
from waitdie_cases import KATS, TS_FAMILIES, admit, history, hot_batch, make_ts, new_state, outcomes
from waitdie_ref import (replay_epoch, replay_literal_epoch, replay_literal_release, replay_release,
                         replay_rounds_epoch, replay_rounds_release)

FORMS = {"literal": (replay_literal_epoch, replay_literal_release),
         "closed": (replay_epoch, replay_release),
         "rounds": (replay_rounds_epoch, replay_rounds_release)}


def same_epoch(a, b):
    keys = ("n_commit", "n_abort", "n_survivors", "nnz_w", "n_readonly")
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and
            all(a[3][k] == b[3][k] for k in keys))


def same_release(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(case, form):
    epoch, release = FORMS[form]
    _, txns, ts, rc0, steps = case
    b = make_batch(txns)
    ts = np.asarray(ts, np.uint64)
    rc, pos = np.asarray(rc0, np.uint8), np.zeros(len(txns), np.uint32)
    for s in steps:
        if s[0] == "admit":
            admit(rc, pos, s[1])
        elif s[0] == "epoch":
            rc, pos, cf, st = epoch(b, ts, rc, pos)
            assert (rc.tolist(), pos.tolist(), cf.tolist()) == (s[1], s[2], s[3])
        else:
            leave = np.zeros(len(txns), np.uint8)
            leave[s[1]] = 1
            rc, pos, n_left, n_prom = release(b, ts, rc, pos, leave)
            assert (rc.tolist(), pos.tolist(), n_left, n_prom) == (s[2], s[3], len(s[1]), s[4])


@pytest.mark.parametrize("family", TS_FAMILIES)
def test_forms_agree_on_histories(family):
    """Random ragged batches with all four access types and rows named more
    than once per txn; six epoch + release pairs with admissions and leavers of
    every state.  The literal releases run in a random order and its reverse."""
    total = np.zeros(3, np.int64)
    for seed in range(12):
        rng = np.random.default_rng(1000 * TS_FAMILIES.index(family) + seed)
        n = int(rng.integers(5, 60))
        b = hot_batch(rng, n, 6, max(2, n // 3))
        ts = make_ts(rng, n, family)
        steps = history(rng, b, ts, replay_epoch, replay_release)
        total += outcomes(steps)
        for s in steps:
            if s[0] == "epoch":
                _, rc, pos, exp = s
                assert same_epoch(replay_literal_epoch(b, ts, rc, pos), exp)
                assert same_epoch(replay_rounds_epoch(b, ts, rc, pos), exp)
            else:
                _, rc, pos, leave, exp = s
                order = rng.permutation(np.nonzero(leave)[0])
                assert same_release(replay_literal_release(b, ts, rc, pos, leave, order), exp)
                assert same_release(replay_rounds_release(b, ts, rc, pos, leave), exp)
    assert total.min() > 0, f"(RCOK, ABORT, WAIT) = {total.tolist()}: an outcome is missing"
    assert total.min() * 10 > total.sum(), f"(RCOK, ABORT, WAIT) = {total.tolist()}: an outcome is rare"


def test_larger_history_closed_against_rounds():
    rng = np.random.default_rng(77)
    n = 600
    b = hot_batch(rng, n, 8, 150)
    ts = make_ts(rng, n, "permuted")
    steps = history(rng, b, ts, replay_epoch, replay_release, epochs=3)
    assert min(outcomes(steps)) > 0
    for s in steps:
        if s[0] == "epoch":
            assert same_epoch(replay_rounds_epoch(b, ts, s[1], s[2]), s[3])
        else:
            assert same_release(replay_rounds_release(b, ts, s[1], s[2], s[3]), s[4])


def test_rounds_of_a_chain_and_of_duplicates():
    """Txn i names row i - 1 then row i, all EX, ts falling: an odd txn waits
    on its first row, so the next one finds its second row free -- which is
    known only once the odd one is decided: a round per txn.  Eight SH
    requests of one row never conflict with each other (one round); a WR behind
    seven RD is a possible conflict in round 1 and a certain one, on the txn
    itself, in round 2."""
    n = 40
    b = make_batch([[(0, WR)]] + [[(i - 1, WR), (i, WR)] for i in range(1, n)])
    ts = np.arange(n, 0, -1).astype(np.uint64)
    rc, pos = new_state(n)
    exp = replay_epoch(b, ts, rc, pos)
    assert exp[0].tolist() == [RC_RCOK if i % 2 == 0 else RC_WAIT for i in range(n)]
    got = replay_rounds_epoch(b, ts, rc, pos)
    assert same_epoch(got, exp) and n - 1 <= got[3]["rounds"] <= n + 1
    got = replay_rounds_epoch(make_batch([[(3, RD)] * 8]), np.asarray([4], np.uint64), *new_state(1))
    assert got[0].tolist() == [RC_RCOK] and got[1].tolist() == [8] and got[3]["rounds"] == 1
    got = replay_rounds_epoch(make_batch([[(3, RD)] * 7 + [(3, WR)]]), np.asarray([4], np.uint64), *new_state(1))
    assert got[0].tolist() == [RC_WAIT] and got[1].tolist() == [7] and got[3]["rounds"] == 2


def test_run_at_len_turns_rcok_and_non_run_is_unchanged():
    b = make_batch([[(1, WR)], [(1, WR), (2, RD)], [], [(2, WR)], [(9, RD)]])
    ts = np.asarray([5, 6, 7, 8, 9], np.uint64)
    rc = np.asarray([WD_RUN, RC_ABORT, WD_RUN, WD_GONE, RC_RCOK], np.uint8)
    pos = np.asarray([1, 1, 0, 77, 1], np.uint32)
    for epoch, _ in FORMS.values():
        r, p, c, st = epoch(b, ts, rc, pos)
        assert r.tolist() == [RC_RCOK, RC_ABORT, RC_RCOK, WD_GONE, RC_RCOK]
        assert p.tolist() == [1, 1, 0, 77, 1] and np.all(c == d.ACCESS_NONE)
        assert (st["n_commit"], st["n_abort"], st["n_survivors"], st["nnz_w"], st["n_readonly"]) == (2, 0, 0, 0, 2)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_malformed_states_raise(form):
    epoch, release = FORMS[form]
    b = make_batch([[(1, RD), (2, WR)], [(3, WR)]])
    ts = np.asarray([1, 2], np.uint64)
    leave = np.zeros(2, np.uint8)
    bad = [([WD_RUN, 0x12], [0, 0]),        # an rc byte outside the five states
           ([WD_RUN, 1], [0, 0]),
           ([WD_RUN, WD_RUN], [3, 0]),      # pos > len
           ([RC_RCOK, WD_RUN], [1, 0]),     # RCOK with pos != len
           ([RC_WAIT, WD_RUN], [2, 0]),     # WAIT with pos >= len
           ([RC_ABORT, WD_RUN], [3, 0])]
    for rc, pos in bad:
        with pytest.raises(ValueError):
            epoch(b, ts, np.asarray(rc, np.uint8), np.asarray(pos, np.uint32))
        with pytest.raises(ValueError):
            release(b, ts, np.asarray(rc, np.uint8), np.asarray(pos, np.uint32), leave)
    rc, pos = new_state(2)
    for args in ((None, rc, pos), (ts, None, pos), (ts, rc, None)):
        with pytest.raises(ValueError):
            epoch(b, *args)
    with pytest.raises(ValueError):
        release(b, ts, rc, pos, None)
    keys = b.keys.copy()
    keys[1] = d.KEY_RESERVED
    with pytest.raises(ValueError):
        epoch(d.EpochBatch(b.offsets, keys, b.acctype), ts, rc, pos)
    off = b.offsets.copy()
    off[1] = 4  # [0, 4, 3]: decreases
    with pytest.raises(ValueError):
        epoch(d.EpochBatch(off, b.keys, b.acctype), ts, rc, pos)
    long = make_batch([[(q, RD) for q in range(65)], []])
    with pytest.raises(ValueError):
        epoch(long, ts, rc, pos)
    # GONE ignores pos
    epoch(b, ts, np.asarray([WD_GONE, WD_RUN], np.uint8), np.asarray([99, 0], np.uint32))
