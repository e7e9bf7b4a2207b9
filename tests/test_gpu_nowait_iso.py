"""GPU parity of the NO_WAIT lock epoch at READ_COMMITTED and READ_UNCOMMITTED
(DCC_ISO_*, nowait.hip) against the literal replay with the levels' releases
(nowait_iso_ref.py): RC, the request each aborted txn aborted at, the counts
and alg_bytes, bit-exact.  test_nowait_iso_ref.py checks on the CPU that the
inputs used here tell READ_COMMITTED from SERIALIZABLE."""
import ctypes as C
import functools

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RD, SCAN, WR, _abi
from deneva_amd.engine import _ptr
from helpers import chain_batch, make_batch
import nowait_ref
from nowait_iso_cases import (CARRY_SEEDS, KATS, N_TXN_EDGES, YCSB_THETAS, answer, carry, chain_variant, hot_row,
                              length_batch, ntxn_batch, random_draws)
from nowait_iso_ref import LEVELS, RCL, RUL, SER, replay

pytestmark = pytest.mark.gpu

NEW = (RCL, RUL)
IDS = {SER: "ser", RCL: "rc", RUL: "ru"}


def held_arrays(held):
    if held is None:
        return None
    return (np.array([k for k, _ in held], np.uint64), np.array([t for _, t in held], np.uint8))


def check(eng, b, level, held=None, ref=None, dev=False, run_batch=None, want_conflict=True):
    """Run `b` (or run_batch, another form of the same epoch) at `level` and
    compare with the replay of `b`.  Returns (rc, conflict, stats)."""
    erc, ecf = ref if ref is not None else replay(b, held, level)
    bb = run_batch if run_batch is not None else b
    h = held
    if dev:
        import torch
        bb = bb.to_torch("cuda:0")
        if held is not None:
            h = (torch.from_numpy(np.ascontiguousarray(held[0], np.uint64).view(np.int64)).to("cuda:0"),
                 torch.from_numpy(np.ascontiguousarray(held[1], np.uint8)).to("cuda:0"))
    rc, cf, st = eng.nowait_lock_epoch(bb, held=h, isolation=level, want_conflict=want_conflict)
    if dev:
        rc = rc.cpu().numpy()
        cf = cf.cpu().numpy().view(np.uint32) if cf is not None else None
    rc = np.asarray(rc)
    bad = np.nonzero(rc != erc)[0]
    assert bad.size == 0, f"rc mismatch at {bad[:10]} (gpu {rc[bad[:10]]} replay {erc[bad[:10]]})"
    if want_conflict:
        cf = np.asarray(cf)
        bad = np.nonzero(cf != ecf)[0]
        assert bad.size == 0, f"conflict mismatch at {bad[:10]} (gpu {cf[bad[:10]]} replay {ecf[bad[:10]]})"
    else:
        assert cf is None
    assert st["n_commit"] == int((erc == RC_RCOK).sum())
    assert st["n_abort"] == int((erc == RC_ABORT).sum())
    at = np.asarray(b.acctype)
    ex = (at != RD) & (at != SCAN)
    assert st["nnz_w"] == int(ex.sum())
    exc = np.concatenate([[0], np.cumsum(ex)])
    off = np.asarray(b.offsets).astype(np.int64)
    assert st["n_readonly"] == int((exc[off[1:]] == exc[off[:-1]]).sum())
    hn = 0 if held is None else int(np.asarray(held[0]).size)
    if b.n_txn:
        assert st["alg_bytes"] == d.nowait_iso_alg_bytes(b.n_txn, b.nnz, hn, want_conflict, level)
    if level == RUL:
        assert st["rounds"] == 0
    return rc, cf, st


@functools.lru_cache(maxsize=None)
def ycsb(theta, level):
    b = d.gen_ycsb(n_txn=8192, zipf_theta=theta)
    return b, replay(b, None, level)


def test_alg_bytes():
    n, m = 1000, 16000
    for wc in (False, True):
        base = d.nowait_alg_bytes(n, m, wc)
        assert d.nowait_iso_alg_bytes(n, m, 0, wc, SER) == base
        assert d.nowait_iso_alg_bytes(n, m, 0, wc, RCL) == base
        assert d.nowait_iso_alg_bytes(n, m, 5, wc, RUL) == base
        assert d.nowait_iso_alg_bytes(n, m, 0, wc, RUL) == base - 16 * m


@pytest.mark.parametrize("level", LEVELS, ids=[IDS[x] for x in LEVELS])
@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(engine, case, level):
    _, txns, held, _ = case
    erc, ecf = answer(case, level)
    for dev in (False, True):
        rc, cf, _ = check(engine, make_batch(txns), level, held_arrays(held), dev=dev)
        assert rc.tolist() == erc and cf.tolist() == ecf


@pytest.mark.parametrize("level", NEW, ids=[IDS[x] for x in NEW])
def test_empty_and_zero_length(engine, level):
    rc, cf, st = engine.nowait_lock_epoch(make_batch([]), isolation=level)
    assert len(rc) == 0 and len(cf) == 0 and st["n_commit"] == 0 and st["n_abort"] == 0
    check(engine, make_batch([[], [(1, WR)], [], [(1, RD)], [], []]), level)
    check(engine, make_batch([[], [], []]), level)
    check(engine, make_batch([[], [(1, RD)], []]), level, held_arrays([(1, WR)]))


@pytest.mark.parametrize("level", NEW, ids=[IDS[x] for x in NEW])
def test_without_conflict_output(engine, level):
    b, ref = ycsb(0.6, level)
    check(engine, b, level, ref=ref, want_conflict=False)
    hk = np.unique(b.keys[:500])
    check(engine, b, level, (hk, np.where(hk % 3 == 0, WR, RD).astype(np.uint8)), want_conflict=False)


@pytest.mark.parametrize("L", [1, 2, 16, 17, 64])
def test_txn_lengths(engine, L):
    """P = 1 .. 64 lanes per txn; a read of a row that is not in the table in
    the first, a middle and the last lane of a txn."""
    b = length_batch(L)
    assert np.all(np.diff(b.offsets) == L)
    check(engine, b, RCL)
    hk = np.arange(0, 40 * L, 7, dtype=np.uint64)
    held = (hk, np.where(hk % 2 == 0, WR, RD).astype(np.uint8))
    check(engine, b, RCL, held)
    check(engine, b, RUL, held)


@pytest.mark.parametrize("level", NEW, ids=[IDS[x] for x in NEW])
def test_length_65_rejected(engine, level):
    long = make_batch([[(1, RD)], [(100 + q, RD) for q in range(65)], [(2, WR)]])
    for bb in (long, long.to_torch("cuda:0")):
        with pytest.raises(d.DccError) as e:
            engine.nowait_lock_epoch(bb, isolation=level)
        assert e.value.code == _abi.DCC_EINVAL
    check(engine, make_batch([[(1, RD)], [(1, WR)], [(1, RD)]]), level)  # the context still works


@pytest.mark.parametrize("n", N_TXN_EDGES)
def test_txn_counts(engine, n):
    b = ntxn_batch(n)
    check(engine, b, RCL)
    check(engine, b, RUL, held_arrays([(3, WR), (5, RD), (1000, RD)]))


@pytest.mark.parametrize("readers", [False, True], ids=["writers", "every_third_reads"])
@pytest.mark.parametrize("n", [1025, 2051])
def test_one_hot_row(engine, n, readers):
    """Every txn but the winners is blocked in round 1: the staged list's flush
    seam (1,024 txns) and a long kill list."""
    b = hot_row(n, readers)
    rc, cf, _ = check(engine, b, RCL)
    first_wr = 1 if readers else 0
    assert rc[first_wr] == RC_RCOK and np.all(rc[first_wr + 1:] == RC_ABORT) and np.all(cf[first_wr + 1:] == 0)
    rc, _, _ = check(engine, b, RUL)
    assert np.all(rc == RC_RCOK)


def test_more_rounds_than_tags(engine):
    for b in (chain_batch(300), chain_variant(300)):
        _, _, st = check(engine, b, RCL)
        assert st["rounds"] > 62
        rc, _, st = check(engine, b, RUL)
        assert np.all(rc == RC_RCOK) and st["rounds"] == 0


@pytest.mark.parametrize("level", NEW, ids=[IDS[x] for x in NEW])
def test_random(engine, level):
    for it, b, held in random_draws():
        check(engine, b, level, held, dev=it in (3, 8))


@pytest.mark.parametrize("level", NEW, ids=[IDS[x] for x in NEW])
@pytest.mark.parametrize("theta", YCSB_THETAS)
def test_ycsb_8192_forms(engine, theta, level):
    b, ref = ycsb(theta, level)
    if level == RCL:  # the condition on the input, before anything runs on the GPU
        assert 0 < int((ref[0] == RC_RCOK).sum()) < ref[0].size, "the replay yields one outcome only"
    check(engine, b, level, ref=ref)
    check(engine, b, level, ref=ref, dev=True)
    c = engine.compact_host_batch(b)
    assert c.keys.dtype == np.uint32 and c.meta.get("acctype_2bit")
    check(engine, b, level, ref=ref, run_batch=c)


def test_held_rows_carried_over_epochs(engine):
    """Epoch e+1's held prefix is what epoch e's committed txns still hold at
    READ_COMMITTED: their EX rows."""
    held = None
    for e, seed in enumerate(CARRY_SEEDS):
        b = d.gen_ycsb(n_txn=8192, zipf_theta=0.8, table_size=1 << 14, seed=seed)
        ref = replay(b, held, RCL)
        assert 0 < int((ref[0] == RC_RCOK).sum()) < ref[0].size
        rc, _, _ = check(engine, b, RCL, held, ref=ref, dev=e == 2)
        held = carry(b, rc)
        assert held[0].size > 0
        check(engine, b, RUL, held)


def test_both_bits(engine):
    b, _ = ycsb(0.6, RCL)
    with pytest.raises(d.DccError) as e:
        engine.nowait_lock_epoch(b, isolation=RCL | RUL)
    assert e.value.code == _abi.DCC_EINVAL
    check(engine, b, RCL, ref=ycsb(0.6, RCL)[1])


@pytest.mark.parametrize("level", NEW, ids=[IDS[x] for x in NEW])
def test_sharded_not_supported(level):
    b, ref = ycsb(0.6, level)
    with d.Engine(0) as solo:
        solo.set_option(_abi.OPT_COMM_SOLO, 1)
        solo.comm_init(0, 1, d.comm_unique_id())
        c0 = solo.comm_calls
        with pytest.raises(d.DccError) as e:
            solo.nowait_lock_epoch(b, shard=True, isolation=level)
        assert e.value.code == _abi.DCC_ENOTSUP and solo.comm_calls == c0
        check(solo, b, level, ref=ref)  # unflagged: the level runs
    with d.Engine(devices=[0, 0]) as m:
        with pytest.raises(d.DccError) as e:
            m.nowait_lock_epoch(b, shard=True, isolation=level)
        assert e.value.code == _abi.DCC_ENOTSUP
        # without the shard flag: the whole epoch on rank 0, at the level asked for
        check(m, b, level, ref=ref)
        check(m, b, level, ref=ref, dev=True)


def test_waitdie_not_supported(engine):
    b = make_batch([[(1, RD)], [(1, WR)]])
    ts = np.asarray([5, 6], np.uint64)
    for level in NEW:
        rc = np.full(2, d.WD_RUN, np.uint8)
        pos = np.zeros(2, np.uint32)
        cb = b.to_c(level)
        e = _abi.lib.dcc_waitdie_lock_epoch(engine._h, C.byref(cb), _ptr(ts), _ptr(rc), _ptr(pos), None, None)
        assert e == _abi.DCC_ENOTSUP
        assert np.all(rc == d.WD_RUN) and np.all(pos == 0)
        leave = np.ones(2, np.uint8)
        e = _abi.lib.dcc_waitdie_release(engine._h, C.byref(cb), _ptr(ts), _ptr(rc), _ptr(pos), _ptr(leave), None,
                                         None, None)
        assert e == _abi.DCC_ENOTSUP
        assert np.all(rc == d.WD_RUN) and np.all(pos == 0)
    # without a bit the same epoch runs
    rc, pos, _, _ = engine.waitdie_lock_epoch(b, ts, np.full(2, d.WD_RUN, np.uint8), np.zeros(2, np.uint32))
    assert len(rc) == 2


def test_reserve_and_alternating_levels(engine):
    """The READ_COMMITTED table is the smaller one: a serializable call right
    after it equals nowait_ref.replay, so nothing of it is left behind."""
    b = d.gen_ycsb(n_txn=8192, zipf_theta=0.99)
    engine.reserve(b.n_txn, b.nnz)
    hk = np.unique(b.keys[:2000])
    held = (hk, np.where(hk % 3 == 0, WR, RD).astype(np.uint8))
    refs = {lv: replay(b, held, lv) for lv in LEVELS}
    sref = nowait_ref.replay(b, held)
    assert np.array_equal(refs[SER][0], sref[0]) and np.array_equal(refs[SER][1], sref[1])
    for lv in (RCL, SER, RUL, SER, RCL, RUL, RCL, SER):
        check(engine, b, lv, held, ref=refs[lv])
    for lv in (RCL, SER, RUL, SER):  # and without held rows: READ_UNCOMMITTED builds no table
        check(engine, b, lv)
