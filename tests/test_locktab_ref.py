"""CPU: the reference of the lock table that lives across epochs
(locktab_ref.LockTable) against an independent composition of the existing
replay (nowait_ref.replay with the table's rows as its held list), and against
hand-worked known answers."""
import numpy as np
import pytest

from deneva_amd import RC_ABORT, RC_RCOK, RD, WR
from helpers import make_batch
from locktab_cases import kat_steps, random_sequences
from locktab_ref import LockTable, OverRelease, held_list, lock_of
from nowait_ref import LOCK_EX, LOCK_SH, replay


def test_against_replay_with_held_list():
    """Before each epoch the export becomes a held list (a row with count c: c
    entries of its type) for nowait_ref.replay; the decisions must be equal and
    so must the state after adding the commits' requests to the export."""
    for steps, _ in random_sequences():
        ref = LockTable()
        for st in steps:
            if st["kind"] == "release":
                assert ref.release(st["batch"], st["sel"], st["want"]) == (st["n"], st["nnz"])
                assert ref.export() == st["state"]
                continue
            b = st["batch"]
            before = ref.export()
            erc, ecf = replay(b, held_list(before))
            rc, cf = ref.lock_epoch(b)
            assert np.array_equal(rc, erc) and np.array_equal(cf, ecf)
            assert np.array_equal(rc, st["rc"]) and np.array_equal(cf, st["conflict"])
            # the commits applied by hand: owner_cnt++, lock_type = type per request
            want = {k: list(v) for k, v in before.items()}
            ok = np.repeat(erc == RC_RCOK, np.diff(b.offsets.astype(np.int64)))
            for k, t in zip(b.keys[ok].tolist(), b.acctype[ok].tolist()):
                e = want.setdefault(k, [None, 0])
                e[0] = lock_of(t)
                e[1] += 1
            assert ref.export() == {k: tuple(v) for k, v in want.items()}


def test_sequences_exercise_the_table():
    """A table that forgets its rows, or never frees one, would not pass."""
    for steps, f in random_sequences():
        assert f["commits"] > 0 and f["aborts"] > 0
        assert f["changed"] >= 100, f
        assert f["regrants"] >= 100, f


def test_known_answers():
    ref = LockTable()
    for st in kat_steps():
        if st["kind"] == "epoch":
            rc, cf = ref.lock_epoch(st["batch"])
            assert rc.tolist() == st["rc"].tolist() and cf.tolist() == st["conflict"].tolist()
        else:
            assert ref.release(st["batch"], st["sel"], st["want"]) == (st["n"], st["nnz"])
        assert ref.export() == st["state"]


def test_counts_and_seeding():
    ref = LockTable()
    ref.lock_epoch(make_batch([[(5, RD), (5, RD)]]))
    assert ref.export() == {5: (LOCK_SH, 2)}
    ref.acquire_rows([5, 6, 6], [RD, RD, WR])  # EX if any entry of the row is EX
    assert ref.export() == {5: (LOCK_SH, 3), 6: (LOCK_EX, 2)}
    ref.release_rows([6, 5, 6])
    assert ref.export() == {5: (LOCK_SH, 2)}
    ref.clear()
    assert ref.export() == {}


def test_over_release_changes_nothing():
    ref = LockTable()
    ref.lock_epoch(make_batch([[(1, RD)], [(2, WR)]]))
    state = ref.export()
    two = make_batch([[(1, RD)], [(1, RD)]])  # each alone would pass; together they must not
    for bad in (lambda: ref.release(two), lambda: ref.release_rows([9]), lambda: ref.release_rows([2, 1, 2])):
        with pytest.raises(OverRelease):
            bad()
        assert ref.export() == state
    assert ref.release(two, np.array([RC_RCOK, RC_ABORT], np.uint8)) == (1, 1)
    with pytest.raises(OverRelease):  # a row at count 0
        ref.release_rows([1])
    assert ref.export() == {2: (LOCK_EX, 1)}
