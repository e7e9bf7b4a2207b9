"""GPU parity of the NO_WAIT lock epoch (dcc_nowait_lock_epoch, nowait.hip)
against the literal Row_lock replay (nowait_ref.py): RC, the request each
aborted txn aborted at, and the commit / abort counts, bit-exact."""
import functools

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RD, SCAN, WR, XP, _abi
from helpers import chain_batch, make_batch, random_batch
from nowait_cases import KATS
from nowait_ref import replay

pytestmark = pytest.mark.gpu


def held_arrays(held):
    if held is None:
        return None
    return (np.array([k for k, _ in held], np.uint64), np.array([t for _, t in held], np.uint8))


def check(eng, b, held=None, ref=None, dev=False, run_batch=None):
    """Run `b` (or run_batch, another form of the same epoch) and compare with
    the replay of `b`.  Returns (rc, conflict, stats) as numpy / dict."""
    erc, ecf = ref if ref is not None else replay(b, held)
    bb = run_batch if run_batch is not None else b
    h = held
    if dev:
        import torch
        bb = bb.to_torch("cuda:0")
        if held is not None:
            h = (torch.from_numpy(np.ascontiguousarray(held[0], np.uint64).view(np.int64)).to("cuda:0"),
                 torch.from_numpy(np.ascontiguousarray(held[1], np.uint8)).to("cuda:0"))
    rc, cf, st = eng.nowait_lock_epoch(bb, held=h)
    if dev:
        rc, cf = rc.cpu().numpy(), cf.cpu().numpy().view(np.uint32)
    rc, cf = np.asarray(rc), np.asarray(cf)
    bad = np.nonzero(rc != erc)[0]
    assert bad.size == 0, f"rc mismatch at {bad[:10]} (gpu {rc[bad[:10]]} replay {erc[bad[:10]]})"
    bad = np.nonzero(cf != ecf)[0]
    assert bad.size == 0, f"conflict mismatch at {bad[:10]} (gpu {cf[bad[:10]]} replay {ecf[bad[:10]]})"
    assert st["n_commit"] == int((erc == RC_RCOK).sum())
    assert st["n_abort"] == int((erc == RC_ABORT).sum())
    at = np.asarray(b.acctype)
    ex = (at != RD) & (at != SCAN)
    assert st["nnz_w"] == int(ex.sum())
    exc = np.concatenate([[0], np.cumsum(ex)])
    off = np.asarray(b.offsets).astype(np.int64)
    assert st["n_readonly"] == int((exc[off[1:]] == exc[off[:-1]]).sum())
    if b.n_txn:
        assert st["alg_bytes"] == d.nowait_alg_bytes(b.n_txn, b.nnz, True)
    return rc, cf, st


@functools.lru_cache(maxsize=None)
def ycsb(n_txn, theta):
    b = d.gen_ycsb(n_txn=n_txn, zipf_theta=theta)
    return b, replay(b)


def both_outcomes(ref):
    erc = ref[0]
    assert 0 < int((erc == RC_RCOK).sum()) < erc.size, "the replay yields one outcome only"


@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(engine, case):
    _, txns, held, rc, conflict = case
    grc, gcf, _ = check(engine, make_batch(txns), held_arrays(held))
    assert grc.tolist() == rc and gcf.tolist() == conflict


def test_known_answers_device(engine):
    for _, txns, held, rc, conflict in KATS:
        grc, gcf, _ = check(engine, make_batch(txns), held_arrays(held), dev=True)
        assert grc.tolist() == rc and gcf.tolist() == conflict


def test_empty_and_zero_length(engine):
    rc, cf, st = engine.nowait_lock_epoch(make_batch([]))
    assert len(rc) == 0 and len(cf) == 0 and st["n_commit"] == 0 and st["n_abort"] == 0
    check(engine, make_batch([[], [(1, WR)], [], [(1, RD)], [], []]))
    check(engine, make_batch([[], [], []]))


def test_without_conflict_output(engine):
    b, ref = ycsb(8192, 0.6)
    rc, cf, st = engine.nowait_lock_epoch(b, want_conflict=False)
    assert cf is None and np.array_equal(np.asarray(rc), ref[0])
    assert st["alg_bytes"] == d.nowait_alg_bytes(b.n_txn, b.nnz, False)


def test_random(engine):
    rng = np.random.default_rng(11)
    for it in range(12):
        nk = int(rng.integers(1, 2000))
        types = (RD, WR) if it % 3 else (RD, WR, XP, SCAN)
        b = random_batch(rng, int(rng.integers(1, 5000)), int(rng.integers(1, 64)), nk,
                         p_write=float(rng.random()), types=types, unique=bool(it % 2))
        held = None
        if it >= 6:  # a random held prefix over distinct keys
            hk = rng.choice(nk, size=int(rng.integers(0, nk + 1)), replace=False).astype(np.uint64)
            held = (hk, rng.integers(0, 4, size=hk.size).astype(np.uint8))
        check(engine, b, held, dev=it in (3, 8))


def test_lengths_at_the_limit(engine):
    rng = np.random.default_rng(5)
    n = 300
    keys = rng.integers(0, 40000, size=(n, 64))
    at = np.where(rng.random((n, 64)) < 0.03, WR, RD)
    b = make_batch([list(zip(keys[i].tolist(), at[i].tolist())) for i in range(n)])
    assert np.all(np.diff(b.offsets) == 64)
    ref = replay(b)
    both_outcomes(ref)
    check(engine, b, ref=ref)
    # one txn of 65 accesses
    long = make_batch([[(1, RD)], [(100 + q, RD) for q in range(65)], [(2, WR)]])
    for bb in (long, long.to_torch("cuda:0")):
        with pytest.raises(d.DccError) as e:
            engine.nowait_lock_epoch(bb)
        assert e.value.code == _abi.DCC_EINVAL


def test_malformed_batches(engine):
    good = make_batch([[(1, RD)], [(2, WR), (3, RD)]])
    off = good.offsets.copy()
    off[1] = 4  # [0, 4, 3]: decreases
    with pytest.raises(d.DccError) as e:
        engine.nowait_lock_epoch(d.EpochBatch(off, good.keys, good.acctype))
    assert e.value.code == _abi.DCC_EINVAL
    keys = good.keys.copy()
    keys[1] = d.KEY_RESERVED
    with pytest.raises(d.DccError) as e:
        engine.nowait_lock_epoch(d.EpochBatch(good.offsets, keys, good.acctype))
    assert e.value.code == _abi.DCC_EINVAL
    with pytest.raises(d.DccError) as e:
        engine.nowait_lock_epoch(good, held=(np.array([d.KEY_RESERVED], np.uint64), np.array([WR], np.uint8)))
    assert e.value.code == _abi.DCC_EINVAL
    check(engine, good)  # the context still works


@pytest.mark.parametrize("all_wr", [False, True])
def test_one_hot_row(engine, all_wr):
    """20,000 one-access txns on one row, across many workgroups."""
    n = 20000
    at = np.full(n, WR if all_wr else RD, np.uint8)
    at[10000] = WR
    b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, 77, np.uint64), at)
    rc, cf, _ = check(engine, b)
    if all_wr:
        assert rc[0] == RC_RCOK and np.all(rc[1:] == RC_ABORT) and np.all(cf[1:] == 0)
    else:
        assert rc[10000] == RC_ABORT and cf[10000] == 0 and int((rc == RC_RCOK).sum()) == n - 1


def test_more_rounds_than_tags(engine):
    _, _, st = check(engine, chain_batch(300))
    assert st["rounds"] > 62


def test_ycsb_c2_forms(engine):
    """65,536 x 16 at theta 0.9: host, device and compact batches."""
    b, ref = ycsb(65536, 0.9)
    both_outcomes(ref)
    assert int(((ref[0] == RC_ABORT) & (ref[1] > 0)).sum()) > 0  # not every abort is at request 0
    check(engine, b, ref=ref)
    check(engine, b, ref=ref, dev=True)
    c = engine.compact_host_batch(b)
    assert c.keys.dtype == np.uint32 and c.meta.get("acctype_2bit")
    check(engine, b, ref=ref, run_batch=c)


@pytest.mark.parametrize("theta", [0.0, 0.6, 0.99])
def test_ycsb_8192(engine, theta):
    b, ref = ycsb(8192, theta)
    both_outcomes(ref)
    check(engine, b, ref=ref)


def test_tpcc(engine):
    b = d.gen_tpcc(n_txn=16384, num_wh=128)
    ref = replay(b)
    both_outcomes(ref)
    check(engine, b, ref=ref)


def test_held_rows_carried_over_epochs(engine):
    """Epoch e+1's held prefix is the requests of epoch e's committed txns."""
    held = None
    for e in range(4):
        b = d.gen_ycsb(n_txn=8192, zipf_theta=0.8, table_size=1 << 14, seed=70 + e)
        ref = replay(b, held)
        both_outcomes(ref)
        rc, _, _ = check(engine, b, held, ref=ref, dev=e == 2)
        per_req = np.repeat(rc == RC_RCOK, np.diff(b.offsets.astype(np.int64)))
        held = (b.keys[per_req].copy(), b.acctype[per_req].copy())
        assert held[0].size > 0


def test_multi_context_runs_on_rank0(engine):
    b, ref = ycsb(8192, 0.6)
    with d.Engine(devices=[0, 0]) as m:
        check(m, b, ref=ref)
        check(m, b, ref=ref, dev=True)


def test_two_rank_communicator_not_supported():
    b, _ = ycsb(8192, 0.6)
    with d.Engine(0) as eng:
        eng.comm_init_host(0, 2, lambda buf: None)
        with pytest.raises(d.DccError) as e:
            eng.nowait_lock_epoch(b)
        assert e.value.code == _abi.DCC_ENOTSUP
        eng.comm_destroy()
        check(eng, b, ref=ycsb(8192, 0.6)[1])


def test_reserve_and_repeat(engine):
    """After reserve, a second identical call returns identical outputs (no
    state of the first is left in the lock table)."""
    b, ref = ycsb(8192, 0.99)
    engine.reserve(b.n_txn, b.nnz)
    hk = np.unique(b.keys[:2000])
    held = (hk, np.where(hk % 3 == 0, WR, RD).astype(np.uint8))
    ref = replay(b, held)
    r1 = check(engine, b, held, ref=ref)
    r2 = check(engine, b, held, ref=ref)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    # and an epoch without held rows right after one with them
    check(engine, b, ref=ycsb(8192, 0.99)[1])


def test_external_stream(engine):
    import torch
    b, ref = ycsb(8192, 0.6)
    s = torch.cuda.Stream(device="cuda:0")
    engine.set_stream(s.cuda_stream)
    try:
        check(engine, b, ref=ref)
    finally:
        engine.set_stream(None)
