"""CPU: the restatements of CC_ALG MVCC (mvcc_ref.py) agree with each other
and with the hand-derived known answers (mvcc_cases.py)."""
import numpy as np
import pytest

from deneva_amd import RC_ABORT, RC_RCOK, RD, SCAN, VTS_BASE, VTS_NONE, WR, XP
from helpers import make_batch, random_batch
from mvcc_cases import KATS, TS_FAMILIES, epoch_base, make_ts
from mvcc_ref import against_timestamp, replay, replay_literal, rows_of, trim, trim_literal, versions_of
import tso_ref


def both(b, ts, lit, clo, info=None):
    """One epoch through both replays on their carried states."""
    la = replay_literal(b, ts, lit)
    lb = replay(b, ts, clo, info)
    for x, y, what in zip(la, lb, ("rc", "conflict", "vts")):
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{what} differs at {bad[:5]}: literal {x[bad[:5]]} closed form {y[bad[:5]]}"
    assert rows_of(lit) == rows_of(clo)
    assert versions_of(lit) == versions_of(clo)
    return la


@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(case):
    _, txns, ts, rc, conflict, vts, rows, versions = case
    lit, clo = {}, {}
    grc, gcf, gv = both(make_batch(txns), np.asarray(ts, np.uint64), lit, clo)
    assert grc.tolist() == rc and gcf.tolist() == conflict and gv.tolist() == vts
    assert rows_of(clo) == rows and versions_of(clo) == versions


@pytest.mark.parametrize("family", TS_FAMILIES)
def test_random_families(family):
    """Three chained epochs per case; the family's replay shows both outcomes,
    a late read of a non-latest version and a base-row read."""
    rng = np.random.default_rng(TS_FAMILIES.index(family) + 77)
    commits = aborts = 0
    info = {}
    for it in range(25):
        nk = int(rng.integers(1, 40))
        types = (RD, WR) if it % 2 else (RD, WR, XP, SCAN)
        lit, clo = {}, {}
        for e in range(3):
            b = random_batch(rng, int(rng.integers(1, 60)), int(rng.integers(1, 10)), nk,
                             p_write=float(rng.random()), types=types, unique=bool(it % 3))
            ts = make_ts(rng, b.n_txn, family, base=epoch_base(family, e, b.n_txn))
            rc, cf, vts = both(b, ts, lit, clo, info)
            commits += int((rc == RC_RCOK).sum())
            aborts += int((rc == RC_ABORT).sum())
            at = np.asarray(b.acctype)
            off = np.asarray(b.offsets).astype(np.int64)
            ab = np.nonzero(rc == RC_ABORT)[0]
            assert np.all(at[off[ab] + cf[ab]] == WR)  # only a WR aborts a txn
            assert np.all(vts[at == XP] == VTS_NONE)
        if it % 5 == 0:  # a trim in the middle of the ts range, then one more epoch on what it kept
            floor = int(np.median(ts))
            assert trim_literal(lit, floor) == trim(clo, floor)
            assert versions_of(lit) == versions_of(clo) and rows_of(lit) == rows_of(clo)
            b = random_batch(rng, 30, 6, nk, p_write=0.3, types=types, unique=False)
            both(b, make_ts(rng, b.n_txn, family, base=floor), lit, clo)
    assert commits > 0 and aborts > 0, "the family yields one outcome only"
    assert info["late"] > 0, "no late read returned a non-latest version"
    assert info["base"] > 0, "no read returned the base row"


def test_trim():
    # row 1: versions 10, 20, 30, 40; row 2: 25; row 3: none
    txns = [[(1, WR)], [(1, WR)], [(2, WR)], [(1, WR)], [(1, WR)], [(3, RD)]]
    ts = np.asarray([10, 20, 25, 30, 40, 5], np.uint64)
    for floor, left, dropped in ((5, [(1, 10), (1, 20), (1, 30), (1, 40), (2, 25)], 0),
                                 (10, [(1, 10), (1, 20), (1, 30), (1, 40), (2, 25)], 0),
                                 (11, [(1, 10), (1, 20), (1, 30), (1, 40), (2, 25)], 0),
                                 (21, [(1, 20), (1, 30), (1, 40), (2, 25)], 1),   # the newest below the floor stays
                                 (35, [(1, 30), (1, 40), (2, 25)], 2),
                                 (1000, [(1, 40), (2, 25)], 3)):
        lit, clo = {}, {}
        both(make_batch(txns), ts, lit, clo)
        assert trim_literal(lit, floor) == trim(clo, floor) == dropped
        assert versions_of(lit) == versions_of(clo) == left
        assert trim_literal(lit, floor) == trim(clo, floor) == 0  # idempotent
        assert rows_of(lit) == rows_of(clo) == {1: (40, 40), 2: (25, 25), 3: (0, 5)}
    # a read below the floor gets what the kept versions give: ts 15 saw 10, now the base row
    lit, clo = {}, {}
    both(make_batch(txns), ts, lit, clo)
    trim_literal(lit, 35), trim(clo, 35)
    _, _, vts = both(make_batch([[(1, RD)], [(1, RD)]]), np.asarray([15, 36], np.uint64), lit, clo)
    assert vts.tolist() == [VTS_BASE, 30]


def test_aborts_against_timestamp():
    """Same batch and ts on fresh state through both references (see
    mvcc_ref.against_timestamp): one-access txns, where the rule holds for
    every txn, and ragged txns, where it holds up to the first txn the two
    engines decide differently."""
    rng = np.random.default_rng(5)
    seen = 0
    for it in range(40):
        one = it % 2 == 0
        n = 120
        if one:
            b = make_batch([[(int(rng.integers(0, 6)), int(rng.choice([RD, WR, XP, SCAN], p=[.4, .4, .1, .1])))]
                            for _ in range(n)])
        else:
            b = random_batch(rng, n, 6, 12, p_write=0.4, types=(RD, WR, XP, SCAN), unique=False)
        ts = make_ts(rng, b.n_txn, ("jitter", "permuted", "tied", "span63")[it % 4])
        mv = replay(b, ts, {})
        tr = tso_ref.replay(b, ts, {})
        seen += against_timestamp(b, mv[0], mv[1], tr[0], tr[1], every=one)
    assert seen > 0


def test_timestamp_rule_is_not_a_theorem_past_a_divergence():
    """Why against_timestamp stops at the first divergence for ragged txns.  T1
    (ts 5) reads row 1 below its version 10: TIMESTAMP aborts it there, MVCC
    goes on and reads row 2 (rts 5).  So T2 (ts 3) aborts at its WR of row 2 in
    MVCC only, and its RD of row 3 is made in TIMESTAMP only (rts 3).  T3
    (ts 2) WR row 3: TIMESTAMP aborts it on ts < rts, MVCC reaches the same WR
    against rts 0 and commits."""
    b = make_batch([[(1, WR)], [(1, RD), (2, RD)], [(2, WR), (3, RD)], [(3, WR)]])
    ts = np.asarray([10, 5, 3, 2], np.uint64)
    lit, clo = {}, {}
    mrc, mcf, _ = both(b, ts, lit, clo)
    trc, tcf = tso_ref.replay(b, ts, {})
    assert trc.tolist() == [RC_RCOK, RC_ABORT, RC_RCOK, RC_ABORT] and tcf.tolist()[3] == 0
    assert mrc.tolist() == [RC_RCOK, RC_RCOK, RC_ABORT, RC_RCOK]
    assert against_timestamp(b, mrc, mcf, trc, tcf, every=False) == 0
    with pytest.raises(AssertionError):
        against_timestamp(b, mrc, mcf, trc, tcf, every=True)
