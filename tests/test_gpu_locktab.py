"""GPU parity of the NO_WAIT lock table that lives across epochs (dcc_locktab_*,
locktab.hip) against the literal reference (locktab_ref.py): after every call
RC, the request each aborted txn aborted at, the stats and the whole exported
state, bit-exact."""
import ctypes as C

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RD, SCAN, WR, _abi
from helpers import chain_batch, make_batch
from locktab_cases import kat_steps, random_sequences
from locktab_ref import LockTable, OverRelease, held_list
from nowait_ref import LOCK_EX, LOCK_SH

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def state_of(lt, dev=False):
    """The table's export as {row: (lock_type, owner_cnt)}."""
    k, t, c = lt.export(device=DEV if dev else None)
    if dev:
        k, t, c = k.cpu().numpy().view(np.uint64), t.cpu().numpy(), c.cpu().numpy().view(np.uint32)
    out = {int(a): (int(b), int(x)) for a, b, x in zip(k, t, c)}
    assert len(out) == len(k), "a row exported twice"
    assert lt.size()[0] == len(out)
    return out


def epoch(lt, ref, b, dev=False, run_batch=None, expect=None):
    """One epoch on the table and on the reference; everything compared.
    run_batch: another form of the same epoch."""
    erc, ecf = expect if expect is not None else ref.lock_epoch(b)
    bb = run_batch if run_batch is not None else b
    if dev:
        bb = bb.to_torch(DEV)
    rc, cf, st = lt.lock_epoch(bb)
    if dev:
        rc, cf = rc.cpu().numpy(), cf.cpu().numpy().view(np.uint32)
    rc, cf = np.asarray(rc), np.asarray(cf)
    bad = np.nonzero(rc != erc)[0]
    assert bad.size == 0, f"rc mismatch at {bad[:10]} (gpu {rc[bad[:10]]} reference {erc[bad[:10]]})"
    bad = np.nonzero(cf != ecf)[0]
    assert bad.size == 0, f"conflict mismatch at {bad[:10]} (gpu {cf[bad[:10]]} reference {ecf[bad[:10]]})"
    assert st["n_commit"] == int((erc == RC_RCOK).sum()) and st["n_abort"] == int((erc == RC_ABORT).sum())
    at = np.asarray(b.acctype)
    ex = (at != RD) & (at != SCAN)
    assert st["nnz_w"] == int(ex.sum())
    exc = np.concatenate([[0], np.cumsum(ex)])
    off = np.asarray(b.offsets).astype(np.int64)
    assert st["n_readonly"] == int((exc[off[1:]] == exc[off[:-1]]).sum())
    if b.n_txn:
        granted = int(np.diff(off)[erc == RC_RCOK].sum())
        assert st["alg_bytes"] == d.locktab_epoch_alg_bytes(b.n_txn, b.nnz, granted, True)
    return rc, cf, st


def release(lt, ref, b, sel=None, want=RC_RCOK, dev=False, run_batch=None):
    en, em = ref.release(b, sel, want)
    bb = run_batch if run_batch is not None else b
    s = sel
    if dev:
        import torch
        bb = bb.to_torch(DEV)
        s = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).to(DEV)
    n, m, st = lt.release(bb, s, want)
    assert (n, m) == (en, em)
    assert st["n_commit"] == en and st["n_abort"] == b.n_txn - en
    if b.n_txn:
        assert st["alg_bytes"] == d.locktab_release_alg_bytes(b.n_txn, en, em)
    return st


def run_steps(eng, lt, steps, dev=False, compact=False):
    ref = LockTable()
    for st in steps:
        b = st["batch"]
        rb = eng.compact_host_batch(b) if compact else None
        if st["kind"] == "epoch":
            epoch(lt, ref, b, dev=dev, run_batch=rb)
        else:
            release(lt, ref, b, st["sel"], st["want"], dev=dev, run_batch=rb)
        assert ref.export() == st["state"]
        assert state_of(lt, dev) == st["state"]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_known_answers(engine, dev):
    with engine.locktab(64) as lt:
        run_steps(engine, lt, kat_steps(), dev=dev)


@pytest.mark.parametrize("s", range(8))
def test_random_sequences(engine, s):
    """Sequences 1 and 4 from device batches, 6 from the compact batch form."""
    steps, f = random_sequences()[s]
    # on the reference: a table that forgets or never frees would not pass
    assert f["commits"] > 0 and f["aborts"] > 0 and f["changed"] >= 100 and f["regrants"] >= 100, f
    with engine.locktab(1 << 16) as lt:
        run_steps(engine, lt, steps, dev=s in (1, 4), compact=s == 6)


def test_equal_to_the_epoch_with_a_held_list(engine):
    """dcc_nowait_lock_epoch(batch, held = the export, a row of count c as c
    entries) decides what the table epoch decides."""
    steps, _ = random_sequences()[2]
    ref = LockTable()
    with engine.locktab(1 << 16) as lt:
        for st in steps:
            if st["kind"] == "release":
                release(lt, ref, st["batch"], st["sel"], st["want"])
                continue
            held = held_list(state_of(lt))
            orc, ocf, _ = engine.nowait_lock_epoch(st["batch"], held=held if held[0].size else None)
            rc, cf, _ = epoch(lt, ref, st["batch"])
            assert np.array_equal(np.asarray(orc), rc) and np.array_equal(np.asarray(ocf), cf)


@pytest.mark.parametrize("length", [1, 16, 17, 64])
def test_tile_edges(engine, length):
    """Txn counts around the wave (64) and the workgroup (256) for txn lengths
    at and around the lane groups (P = 1, 16, 32, 64)."""
    rng = np.random.default_rng(100 + length)
    ref = LockTable()
    with engine.locktab(1 << 16) as lt:
        for n in (1, 63, 64, 65, 255, 256, 257):
            keys = rng.integers(0, 40 * n * length + 64, size=(n, length)).astype(np.uint64)
            at = np.where(rng.random((n, length)) < 0.1, WR, RD).astype(np.uint8)
            b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32) * length, keys.reshape(-1), at.reshape(-1))
            rc, _, _ = epoch(lt, ref, b, dev=n == 65)
            assert state_of(lt) == ref.export()
            # a second epoch on the same rows meets the first one's locks
            rc2, _, _ = epoch(lt, ref, b)
            assert state_of(lt) == ref.export()
            release(lt, ref, b, rc2, dev=n == 255)
            release(lt, ref, b, rc)
            assert state_of(lt) == ref.export() == {}


def test_empty_and_zero_length(engine):
    ref = LockTable()
    with engine.locktab(64) as lt:
        rc, cf, st = lt.lock_epoch(make_batch([]))
        assert len(rc) == 0 and len(cf) == 0 and st["n_commit"] == 0
        assert lt.release(make_batch([]))[:2] == (0, 0)
        b = make_batch([[], [(1, WR)], [], [(1, RD)], [], []])
        rc, _, _ = epoch(lt, ref, b)
        epoch(lt, ref, make_batch([[], [], []]))
        assert state_of(lt) == ref.export() == {1: (LOCK_EX, 1)}
        release(lt, ref, b, rc)
        assert state_of(lt) == {}


def test_too_long_txn_leaves_the_table(engine):
    ref = LockTable()
    with engine.locktab(256) as lt:
        epoch(lt, ref, make_batch([[(1, RD)], [(2, WR)]]))
        before = state_of(lt)
        long = make_batch([[(1, RD)], [(100 + q, RD) for q in range(65)], [(3, WR)]])
        for bb in (long, long.to_torch(DEV)):
            with pytest.raises(d.DccError) as e:
                lt.lock_epoch(bb)
            assert e.value.code == _abi.DCC_EINVAL
            assert state_of(lt) == before
        keys = long.keys.copy()
        keys[0] = d.KEY_RESERVED
        with pytest.raises(d.DccError) as e:
            lt.lock_epoch(d.EpochBatch(np.array([0, 1], np.uint32), keys[:1], long.acctype[:1]))
        assert e.value.code == _abi.DCC_EINVAL
        assert state_of(lt) == before
        epoch(lt, ref, make_batch([[(1, RD)], [(2, RD)]]))
        assert state_of(lt) == ref.export()


def test_counts(engine):
    n = 20000
    ref = LockTable()
    with engine.locktab(n) as lt:  # room is counted in requests: an upper bound on the new rows
        twice = make_batch([[(5, RD), (5, RD)]])
        epoch(lt, ref, twice)
        assert state_of(lt) == {5: (LOCK_SH, 2)}
        release(lt, ref, twice)
        # 20,000 one-access readers of one row, across many workgroups
        readers = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, 77, np.uint64), np.full(n, RD, np.uint8))
        rc, _, _ = epoch(lt, ref, readers)
        assert np.all(rc == RC_RCOK) and state_of(lt) == {77: (LOCK_SH, n)}
        writers = make_batch([[(77, WR)]] * 300)
        rc, cf, _ = epoch(lt, ref, writers)
        assert np.all(rc == RC_ABORT) and np.all(cf == 0) and state_of(lt) == {77: (LOCK_SH, n)}
        st = release(lt, ref, readers)
        assert st["n_commit"] == n and state_of(lt) == {}
        rc, _, _ = epoch(lt, ref, writers)
        assert rc[0] == RC_RCOK and np.all(rc[1:] == RC_ABORT) and state_of(lt) == {77: (LOCK_EX, 1)}


def test_more_rounds_than_tags_with_seeded_rows(engine):
    ref = LockTable()
    with engine.locktab(1024) as lt:
        lt.acquire_rows([0], [RD])
        ref.acquire_rows([0], [RD])
        rc, cf, st = epoch(lt, ref, chain_batch(300))
        assert st["rounds"] > 62
        assert rc[0] == RC_ABORT and cf[0] == 0 and rc[1] == RC_RCOK  # txn 0 writes the SH-held row 0
        assert state_of(lt) == ref.export()


def test_release_errors(engine):
    """Each is DCC_EINVAL with the table as it was; the valid release that
    follows succeeds, so the failed ones left no release scratch behind."""
    ref = LockTable()
    with engine.locktab(256) as lt:
        held = make_batch([[(1, RD), (2, WR)], [(1, RD)], [(3, RD)]])
        epoch(lt, ref, held)
        release(lt, ref, held, np.array([RC_ABORT, RC_ABORT, RC_RCOK], np.uint8))  # 3 goes to count 0
        before = state_of(lt)
        assert before == {1: (LOCK_SH, 2), 2: (LOCK_EX, 1)}
        never = make_batch([[(1, RD), (99, RD)]])
        at_zero = make_batch([[(3, RD)], [(1, RD)]])
        together = make_batch([[(2, WR)], [(1, RD)], [(2, WR)]])  # 2 is held once
        for bad in (never, at_zero, together):
            with pytest.raises(OverRelease):
                ref.release(bad)
            for bb in (bad, bad.to_torch(DEV)):
                with pytest.raises(d.DccError) as e:
                    lt.release(bb)
                assert e.value.code == _abi.DCC_EINVAL
                assert state_of(lt) == before
        with pytest.raises(d.DccError) as e:
            lt.release_rows(np.array([2, 1, 2], np.uint64))
        assert e.value.code == _abi.DCC_EINVAL and state_of(lt) == before
        off = held.offsets.copy()
        off[1] = 4  # [0, 4, 3, 4]: decreases
        for mal in (d.EpochBatch(off, held.keys, held.acctype),
                    d.EpochBatch(off, held.keys, held.acctype).to_torch(DEV)):
            with pytest.raises(d.DccError) as e:
                lt.release(mal)
            assert e.value.code == _abi.DCC_EINVAL
            assert state_of(lt) == before
        # selected by rc, the same batch passes: only its first txn releases row 2
        release(lt, ref, together, np.array([RC_RCOK, RC_RCOK, RC_ABORT], np.uint8))
        assert state_of(lt) == ref.export() == {1: (LOCK_SH, 1)}
        release(lt, ref, make_batch([[(1, RD)]]))
        assert state_of(lt) == {}


def test_room_and_rebuild(engine):
    """cap_rows 1024 (2048 slots, at most 1024 in use): released rows keep
    their slots, so epochs over moving key ranges fill the table up until the
    held rows are rebuilt into the other buffer."""
    rng = np.random.default_rng(9)
    ref = LockTable()
    with engine.locktab(1024) as lt:
        prev = None
        for e in range(10):
            keys = np.stack([rng.choice(300, size=10, replace=False) + 150 * e for _ in range(30)]).astype(np.uint64)
            at = np.where(rng.random((30, 10)) < 0.05, WR, RD).astype(np.uint8)
            b = d.EpochBatch(np.arange(31, dtype=np.uint32) * 10, keys.reshape(-1), at.reshape(-1))
            rc, _, _ = epoch(lt, ref, b, dev=e % 3 == 1)
            assert state_of(lt) == ref.export()
            if prev is not None:
                release(lt, ref, prev[0], prev[1])
                assert state_of(lt) == ref.export()
            prev = (b, rc)
            rows, slots, _ = lt.size()
            assert rows <= slots <= 1024
        assert lt.size()[2] >= 1
        # 1,100 requests cannot fit beside the held rows, rebuilt or not
        before, rebuilds = state_of(lt), lt.size()[2]
        assert len(before) > 0
        big = d.EpochBatch(np.arange(1101, dtype=np.uint32), np.arange(5000, 6100, dtype=np.uint64),
                           np.full(1100, RD, np.uint8))
        for bb in (big, big.to_torch(DEV)):
            with pytest.raises(d.DccError) as e:
                lt.lock_epoch(bb)
            assert e.value.code == _abi.DCC_ERANGE
            assert state_of(lt) == before and lt.size()[2] == rebuilds
        with pytest.raises(d.DccError) as e:
            lt.acquire_rows(big.keys, big.acctype)
        assert e.value.code == _abi.DCC_ERANGE and state_of(lt) == before
        epoch(lt, ref, make_batch([[(5000, WR)]]))
        assert state_of(lt) == ref.export()


def test_acquire_release_rows_and_clear(engine):
    import torch
    ref = LockTable()
    with engine.locktab(4096) as lt:
        rng = np.random.default_rng(3)
        keys = rng.integers(0, 500, size=3000).astype(np.uint64)
        at = rng.integers(0, 4, size=3000).astype(np.uint8)
        lt.acquire_rows(keys[:2000], at[:2000])
        lt.acquire_rows(torch.from_numpy(keys[2000:].view(np.int64)).to(DEV), torch.from_numpy(at[2000:]).to(DEV))
        ref.acquire_rows(keys, at)
        assert state_of(lt) == state_of(lt, dev=True) == ref.export()
        b = make_batch([[(int(k), RD)] for k in range(0, 520, 7)])
        epoch(lt, ref, b)
        perm = rng.permutation(3000)
        lt.release_rows(keys[perm[:1500]])
        lt.release_rows(torch.from_numpy(keys[perm[1500:]].view(np.int64)).to(DEV))
        ref.release_rows(keys)
        assert state_of(lt) == ref.export()
        with pytest.raises(d.DccError) as e:
            lt.acquire_rows(np.array([1, d.KEY_RESERVED], np.uint64), np.array([RD, RD], np.uint8))
        assert e.value.code == _abi.DCC_EINVAL and state_of(lt) == ref.export()
        with pytest.raises(d.DccError) as e:  # export into too little room
            n = C.c_uint64(0)
            code = _abi.lib.dcc_locktab_export(lt._handle(), None, None, None, 0, 0, C.byref(n))
            raise d.DccError(code, "export")
        assert e.value.code == _abi.DCC_ERANGE and n.value == len(ref.export()) > 0
        lt.clear()
        assert state_of(lt) == {} and lt.size()[:2] == (0, 0)
        ref.clear()
        epoch(lt, ref, b)
        assert state_of(lt) == ref.export()


def test_profiled_calls(engine):
    ref = LockTable()
    b = d.gen_ycsb(n_txn=4096, zipf_theta=0.9, table_size=1 << 14)
    engine.set_profiling(True)
    try:
        with engine.locktab(1 << 17) as lt:
            rc, _, st = epoch(lt, ref, b)
            p = lt.pass_ms()
            assert p["seed"] > 0 and p["grant"] > 0 and p["rebuild"] == 0
            assert p["seed"] <= st["phase_ms"][0] and p["grant"] <= st["phase_ms"][3]
            st = release(lt, ref, b, rc)
            assert all(x >= 0 for x in st["phase_ms"]) and st["device_ms"] > 0
            assert state_of(lt) == {}
    finally:
        engine.set_profiling(False)


def test_table_alive_at_destroy():
    with d.Engine(0) as eng:
        lt = eng.locktab(1024)
        lt.lock_epoch(make_batch([[(1, WR)]]))
    assert lt._q is None  # freed with its context


def test_two_tables_on_one_context(engine):
    ra, rb = LockTable(), LockTable()
    with engine.locktab(256) as a, engine.locktab(256) as b:
        w = make_batch([[(7, WR)], [(8, RD)]])
        epoch(a, ra, w)
        assert state_of(b) == {}
        rc, _, _ = epoch(b, rb, w)  # b does not see a's locks
        assert np.all(rc == RC_RCOK)
        rc, _, _ = epoch(a, ra, w)
        assert rc.tolist() == [RC_ABORT, RC_RCOK]
        release(b, rb, w)
        assert state_of(b) == {} and state_of(a) == ra.export() == {7: (LOCK_EX, 1), 8: (LOCK_SH, 2)}


def test_multi_context_runs_on_rank0():
    steps, _ = random_sequences()[5]
    with d.Engine(devices=[0, 0]) as m:
        with m.locktab(1 << 16) as lt:
            run_steps(m, lt, steps[:6])
            run_steps_dev = kat_steps()
            lt.clear()
            run_steps(m, lt, run_steps_dev, dev=True)


def test_two_rank_communicator_not_supported():
    b = make_batch([[(1, WR)], [(1, RD)]])
    with d.Engine(0) as eng:
        lt = eng.locktab(64)
        eng.comm_init_host(0, 2, lambda buf: None)
        with pytest.raises(d.DccError) as e:
            lt.lock_epoch(b)
        assert e.value.code == _abi.DCC_ENOTSUP
        eng.comm_destroy()
        epoch(lt, LockTable(), b)


def test_ycsb_hold_two_epochs(engine):
    """16,384 x 16 at theta 0.9: four epochs, each epoch's commits held for two."""
    ref = LockTable()
    done = []
    with engine.locktab(1 << 20) as lt:
        for e in range(4):
            b = d.gen_ycsb(n_txn=16384, zipf_theta=0.9, seed=300 + e)
            rc, _, _ = epoch(lt, ref, b, dev=e % 2 == 1)
            assert 0 < int((rc == RC_RCOK).sum()) < rc.size
            done.append((b, rc))
            if e >= 2:
                release(lt, ref, *done[e - 2], dev=e == 3)
            assert state_of(lt, dev=e == 2) == ref.export()
