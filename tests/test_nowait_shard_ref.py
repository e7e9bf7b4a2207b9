"""CPU: the key-sharded NO_WAIT protocol in plain Python (nowait_shard_ref.py,
DESIGN.md §8p) against the literal Row_lock replay (nowait_ref.py): the same
RC and the same conflict ordinal for every rank count, and what the design
claims about a self-conflicting txn's handling."""
import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RD, SCAN, WR, XP
from helpers import chain_batch, make_batch, random_batch
from nowait_cases import KATS
from nowait_ref import replay
from nowait_shard_cases import directed, self_conflict_and_live_locks
from nowait_shard_ref import RanksDisagree, sharded_epoch

RANKS = [1, 2, 3, 4, 8]


def held_arrays(held):
    if held is None:
        return None
    return (np.array([k for k, _ in held], np.uint64), np.array([t for _, t in held], np.uint8))


def check(b, held, R, selfc="round1"):
    erc, ecf = replay(b, held)
    rc, cf, info = sharded_epoch(b, held, R, d.key_shard, selfc=selfc)
    assert rc.tolist() == erc.tolist()
    assert cf.tolist() == ecf.tolist()
    assert sum(info["own"]) == b.nnz
    assert info["collectives"] == (info["rounds"] + 1 + (selfc == "pre") if b.n_txn else 0)
    return rc, cf, info


@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(case, R):
    _, txns, held, rc, conflict = case
    grc, gcf, _ = check(make_batch(txns), held_arrays(held), R)
    assert grc.tolist() == rc and gcf.tolist() == conflict


@pytest.mark.parametrize("R", RANKS)
def test_directed(R):
    for name, txns, held in directed(d.key_shard, R):
        check(make_batch(txns), held_arrays(held), R)


@pytest.mark.parametrize("R", [2, 3, 4])
def test_directed_answers(R):
    """The directed cases decide what their docstrings say."""
    cases = {name: (txns, held) for name, txns, held in directed(d.key_shard, R)}
    N = d.ACCESS_NONE
    for held, at in ((0, 1), (1, 2)):
        rc, cf = replay(make_batch(cases[f"self_conflict_live_locks_held{held}"][0]),
                        held_arrays(cases[f"self_conflict_live_locks_held{held}"][1]))
        assert rc.tolist() == [RC_ABORT, RC_RCOK, RC_ABORT] and cf.tolist() == [at, N, 1]
    for mirror in (0, 1):
        rc, cf = replay(make_batch(cases[f"first_conflict_elsewhere_mirror{mirror}"][0]))
        assert rc.tolist() == [RC_RCOK, RC_ABORT] and cf.tolist() == [N, 1]
    rc, cf = replay(make_batch(cases["killed_here_blocked_there"][0]))
    assert rc.tolist() == [RC_RCOK, RC_ABORT, RC_RCOK, RC_ABORT] and cf.tolist() == [N, 0, N, 0]
    _, _, info = sharded_epoch(make_batch(cases["killed_here_blocked_there"][0]), None, R, d.key_shard)
    assert info["rounds"] == 3
    _, _, info = sharded_epoch(make_batch(cases["one_shard_only"][0]), held_arrays(cases["one_shard_only"][1]),
                               R, d.key_shard)
    assert sorted(info["own"])[:-1] == [0] * (R - 1) and sorted(info["own_held"])[:-1] == [0] * (R - 1)


@pytest.mark.parametrize("R", RANKS)
def test_random(R):
    rng = np.random.default_rng(100 + R)
    for it in range(10):
        nk = int(rng.integers(1, 60))
        types = (RD, WR) if it % 3 else (RD, WR, XP, SCAN)
        b = random_batch(rng, int(rng.integers(1, 250)), int(rng.integers(1, 10)), nk,
                         p_write=float(rng.random()) * 0.6, types=types, unique=bool(it % 2))
        held = None
        if it >= 5:
            hk = rng.choice(nk, size=int(rng.integers(0, nk + 1)), replace=False).astype(np.uint64)
            held = (hk, rng.integers(0, 4, size=hk.size).astype(np.uint8))
        check(b, held, R)


@pytest.mark.parametrize("R", [2, 3])
def test_chain_past_the_tag_wrap(R):
    """Consecutive rows of the chain fall on different shards; the fixed point
    needs more rounds than there are round tags, so the words are retagged."""
    b = chain_batch(150)
    sh = [d.key_shard(k, R) for k in range(150)]
    assert any(sh[i] != sh[i + 1] for i in range(149))
    _, _, info = check(b, None, R)
    assert info["rounds"] > 62


@pytest.mark.parametrize("R", RANKS)
def test_self_conflict_handling(R):
    """a stale round-1 word of a self-conflicting txn on another
    rank only blocks for round 1.  Telling every rank before any word is
    published gives the same decisions in at most one round less; telling
    nobody makes the ranks' state bytes part."""
    rng = np.random.default_rng(7 + R)
    batches = [(make_batch(t), held_arrays(h)) for with_held in (False, True)
               for t, h in [self_conflict_and_live_locks(d.key_shard, R, with_held)]]
    for it in range(8):  # repeated rows inside a txn: unique=False
        batches.append((random_batch(rng, 120, 8, int(rng.integers(2, 30)), p_write=0.4, unique=False), None))
    for b, held in batches:
        _, _, chosen = check(b, held, R, selfc="round1")
        _, _, pre = check(b, held, R, selfc="pre")
        assert pre["rounds"] <= chosen["rounds"] <= pre["rounds"] + 1
    if R > 1:
        b, held = batches[0]
        with pytest.raises(RanksDisagree):
            sharded_epoch(b, held, R, d.key_shard, selfc="silent")
