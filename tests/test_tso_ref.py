"""CPU: the restatements of CC_ALG TIMESTAMP (tso_ref.py) agree with each
other and with the hand-derived known answers (tso_cases.py)."""
import numpy as np
import pytest

from deneva_amd import RC_ABORT, RC_RCOK, RD, SCAN, WR, XP
from helpers import chain_batch, make_batch, random_batch
from tso_cases import KATS, TS_FAMILIES, make_ts, seed_rows
from tso_ref import live, replay, replay_literal, replay_rounds


def all_three(b, ts, seed):
    ra, rb, rr = dict(seed), dict(seed), dict(seed)
    la = replay_literal(b, ts, ra)
    lb = replay(b, ts, rb)
    lr = replay_rounds(b, ts, rr)
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
    assert np.array_equal(la[0], lr[0]) and np.array_equal(la[1], lr[1])
    assert live(ra) == live(rb) == live(rr)
    return la[0], la[1], live(ra), lr[2]


@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(case):
    _, txns, ts, seed, rc, conflict, rows = case
    grc, gcf, grows, _ = all_three(make_batch(txns), np.asarray(ts, np.uint64), seed)
    assert grc.tolist() == rc and gcf.tolist() == conflict
    assert grows == live(rows)


@pytest.mark.parametrize("family", TS_FAMILIES)
def test_random_families(family):
    rng = np.random.default_rng(TS_FAMILIES.index(family) + 31)
    commits = aborts = 0
    for it in range(40):
        nk = int(rng.integers(1, 60))
        types = (RD, WR) if it % 2 else (RD, WR, XP, SCAN)
        b = random_batch(rng, int(rng.integers(1, 80)), int(rng.integers(1, 12)), nk,
                         p_write=float(rng.random()), types=types, unique=bool(it % 3))
        ts = make_ts(rng, b.n_txn, family)
        seed = seed_rows(rng, nk, ts) if it % 4 == 0 else {}
        rc, _, _, _ = all_three(b, ts, seed)
        commits += int((rc == RC_RCOK).sum())
        aborts += int((rc == RC_ABORT).sum())
    assert commits > 0 and aborts > 0, "the family yields one outcome only"


def test_index_order_commits_in_one_round():
    rng = np.random.default_rng(3)
    b = random_batch(rng, 200, 10, 50, p_write=0.5, types=(RD, WR, XP, SCAN), unique=False)
    rc, _, _, rounds = all_three(b, make_ts(rng, b.n_txn, "index"), {})
    assert np.all(rc == RC_RCOK) and rounds == 1


def test_chain_needs_a_round_per_txn():
    """Txn i reads key i-1 and writes key i, ts decreasing: txn i commits iff
    txn i-1 aborted, which the rounds learn one txn at a time."""
    n = 40
    b = chain_batch(n)
    ts = np.arange(n, 0, -1).astype(np.uint64) + np.uint64(100)
    rc, cf, _, rounds = all_three(b, ts, {})
    assert rc.tolist() == [RC_RCOK if i % 2 == 0 else RC_ABORT for i in range(n)]
    assert all(cf[i] == 0 for i in range(1, n, 2))
    assert rounds >= n - 1


def test_state_carries_across_epochs():
    rng = np.random.default_rng(9)
    ra, rb = {}, {}
    base = 1000
    for e in range(4):
        b = random_batch(rng, 60, 8, 30, p_write=0.4)
        ts = make_ts(rng, b.n_txn, "jitter", base=base)
        base += b.n_txn
        la, lb = replay_literal(b, ts, ra), replay(b, ts, rb)
        assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and live(ra) == live(rb)
        assert 0 < int((la[0] == RC_RCOK).sum()) < b.n_txn
