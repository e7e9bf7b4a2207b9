"""The isolation-level replay (nowait_iso_ref.py) against the known answers,
against nowait_ref.replay at SERIALIZABLE, against the closed forms, and the
conditions on the inputs of the GPU tests (test_gpu_nowait_iso.py)."""
import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RD, SCAN, WR, XP
from helpers import chain_batch, make_batch, random_batch
import nowait_ref
from nowait_iso_cases import (CARRY_SEEDS, KATS, N_TXN_EDGES, YCSB_THETAS, answer, carry, chain_variant, hot_row,
                              length_batch, ntxn_batch, random_draws)
from nowait_iso_ref import LEVELS, RCL, RUL, SER, Table, closed_form, replay


def held_arrays(held):
    if held is None:
        return None
    return (np.array([k for k, _ in held], np.uint64), np.array([t for _, t in held], np.uint8))


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def families():
    """Random ragged batches: duplicate rows, all four access types, held prefixes."""
    rng = np.random.default_rng(23)
    for it in range(40):
        nk = int(rng.integers(1, 300))
        b = random_batch(rng, int(rng.integers(1, 400)), int(rng.integers(1, 20)), nk,
                         p_write=float(rng.random()), types=(RD, WR, XP, SCAN), unique=bool(it % 2))
        held = None
        if it % 4 >= 2:
            hk = rng.integers(0, nk, size=int(rng.integers(0, nk // 2 + 1))).astype(np.uint64)  # rows may repeat
            held = (hk, rng.integers(0, 4, size=hk.size).astype(np.uint8))
        yield b, held
    yield from ((b, h) for _, b, h in random_draws())


@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(case):
    _, txns, held, _ = case
    for level in LEVELS:
        rc, cf = replay(make_batch(txns), held_arrays(held), level)
        erc, ecf = answer(case, level)
        assert rc.tolist() == erc and cf.tolist() == ecf, level
        if level != SER:
            assert same(closed_form(make_batch(txns), held_arrays(held), level), (rc, cf))


def test_serializable_is_nowait_ref():
    for b, held in families():
        assert same(replay(b, held, SER), nowait_ref.replay(b, held))


@pytest.mark.parametrize("level", [RCL, RUL])
def test_replay_equals_closed_form(level):
    for b, held in families():
        assert same(replay(b, held, level), closed_form(b, held, level))


def test_read_uncommitted_without_held_commits_all():
    for b, _ in families():
        rc, _ = replay(b, None, RUL)
        assert np.all(rc == RC_RCOK)


def test_table_form_equals_held_form():
    """An epoch on a carried table decides as the same epoch with the table's export as `held`."""
    from locktab_ref import held_list
    rng = np.random.default_rng(5)
    t = Table()
    for e in range(6):
        level = LEVELS[int(rng.integers(0, 3))]
        b = random_batch(rng, 300, 8, 200, p_write=0.3, types=(RD, WR, XP, SCAN), unique=False)
        want = replay(b, held_list(t.export()), level)
        assert same(t.lock_epoch(b, level), want)


def differs(b, held=None):
    """The READ_COMMITTED decisions are not the serializable ones, and both outcomes occur."""
    s, r = replay(b, held, SER), replay(b, held, RCL)
    return bool(np.any(s[0] != r[0]))


def test_gpu_inputs_tell_the_levels_apart():
    """A library that ignores the flag fails every READ_COMMITTED input of the
    GPU tests.  Two of them cannot tell the levels apart by construction, and
    the GPU tests pair each with one that does: chain_batch (a reader of a
    committed writer's row aborts at either level; its variant with a
    read-then-write txn 0 flips every decision) and the all-writers hot row
    (no reads; the every-third-reads form differs)."""
    for _, b, held in random_draws():
        assert differs(b, held)
        rc = replay(b, held, RCL)[0]
        assert 0 < int((rc == RC_ABORT).sum()) < b.n_txn
    for L in (1, 2, 16, 17, 64):
        assert differs(length_batch(L)), L
    for n in N_TXN_EDGES:
        assert differs(ntxn_batch(n)), n
    for n in (1025, 2051):
        assert differs(hot_row(n, True))
        assert not differs(hot_row(n, False))
    assert not differs(chain_batch(300))
    assert differs(chain_variant(300))
    for theta in YCSB_THETAS:
        b = d.gen_ycsb(n_txn=8192, zipf_theta=theta)
        assert differs(b)
        rc = replay(b, None, RCL)[0]
        assert 0 < int((rc == RC_ABORT).sum()) < b.n_txn
    held = None
    for seed in CARRY_SEEDS:
        b = d.gen_ycsb(n_txn=8192, zipf_theta=0.8, table_size=1 << 14, seed=seed)
        assert differs(b, held)
        rc = replay(b, held, RCL)[0]
        assert 0 < int((rc == RC_ABORT).sum()) < b.n_txn
        held = carry(b, rc)
