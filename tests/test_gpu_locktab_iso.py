"""GPU parity of the lock table that lives across epochs at the isolation
levels (dcc_locktab_lock_epoch / dcc_locktab_release with DCC_ISO_*) against
the table-carrying replay (nowait_iso_ref.Table): RC, conflict ordinals, the
counts and the whole exported state after every call, bit-exact."""
import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RD, SCAN, WR, XP, _abi
from helpers import make_batch, random_batch
from nowait_iso_ref import LEVELS, RCL, RUL, SER, Table
from nowait_ref import LOCK_EX, LOCK_SH

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def state_of(lt):
    k, t, c = lt.export()
    out = {int(a): (int(b), int(x)) for a, b, x in zip(k, t, c)}
    assert len(out) == len(k), "a row exported twice"
    assert lt.size()[0] == len(out)
    return out


def epoch(lt, ref, b, level, dev=False):
    """One epoch on the table and on the reference; everything compared."""
    erc, ecf = ref.lock_epoch(b, level)
    rc, cf, st = lt.lock_epoch(b.to_torch(DEV) if dev else b, isolation=level)
    if dev:
        rc, cf = rc.cpu().numpy(), cf.cpu().numpy().view(np.uint32)
    rc, cf = np.asarray(rc), np.asarray(cf)
    bad = np.nonzero(rc != erc)[0]
    assert bad.size == 0, f"rc mismatch at {bad[:10]} (gpu {rc[bad[:10]]} reference {erc[bad[:10]]})"
    bad = np.nonzero(cf != ecf)[0]
    assert bad.size == 0, f"conflict mismatch at {bad[:10]} (gpu {cf[bad[:10]]} reference {ecf[bad[:10]]})"
    assert st["n_commit"] == int((erc == RC_RCOK).sum()) and st["n_abort"] == int((erc == RC_ABORT).sum())
    if level == RUL:
        assert st["rounds"] == 0
    if b.n_txn:
        at = np.asarray(b.acctype)
        stays = np.repeat(erc == RC_RCOK, np.diff(np.asarray(b.offsets).astype(np.int64)))
        if level == RCL:
            stays = stays & (at != RD) & (at != SCAN)
        granted = 0 if level == RUL else int(stays.sum())
        assert st["alg_bytes"] == d.locktab_epoch_alg_bytes(b.n_txn, b.nnz, granted, True)
    assert state_of(lt) == ref.export()
    return rc, cf


def release(lt, ref, b, sel, level, dev=False):
    en, em = ref.release(b, sel, RC_RCOK, level)
    bb, s = b, sel
    if dev:
        import torch
        bb = b.to_torch(DEV)
        s = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).to(DEV)
    n, m, st = lt.release(bb, s, RC_RCOK, isolation=level)
    assert (n, m) == (en, em)
    assert st["n_commit"] == en and st["n_abort"] == b.n_txn - en
    assert state_of(lt) == ref.export()


def test_hand_case(engine):
    with engine.locktab(64) as lt:
        ref = Table()
        a = make_batch([[(1, RD), (2, WR)]])
        rc_a, _ = epoch(lt, ref, a, RCL)
        assert state_of(lt) == {2: (LOCK_EX, 1)}
        b = make_batch([[(1, WR)], [(2, RD)]])
        rc, cf = epoch(lt, ref, b, RCL)
        assert rc.tolist() == [RC_RCOK, RC_ABORT] and cf.tolist() == [ACCESS_NONE, 0]
        assert state_of(lt) == {1: (LOCK_EX, 1), 2: (LOCK_EX, 1)}
        n, m, _ = lt.release(a, rc_a, RC_RCOK, isolation=RCL)
        ref.release(a, rc_a, RC_RCOK, RCL)
        assert (n, m) == (1, 1)
        assert state_of(lt) == {1: (LOCK_EX, 1)} == ref.export()


def test_read_of_a_row_held_in_the_table_only(engine):
    """No request of the epoch writes rows 7 and 9: only the table knows that they are held."""
    with engine.locktab(64) as lt:
        ref = Table()
        lt.acquire_rows(np.array([7, 9], np.uint64), np.array([WR, RD], np.uint8))
        ref.acquire_rows([7, 9], [WR, RD])
        b = make_batch([[(3, RD), (4, RD), (7, RD)], [(9, RD), (3, RD)], [(3, RD), (9, SCAN), (7, SCAN), (7, RD)],
                        [(4, WR), (9, WR)]])
        for level, dev in ((RCL, False), (RCL, True), (RUL, False)):
            rc, cf = epoch(lt, ref, b, level, dev=dev)
            assert rc.tolist() == [RC_ABORT, RC_RCOK, RC_ABORT, RC_ABORT]
            assert cf.tolist() == [2, ACCESS_NONE, 2, 1]
            assert state_of(lt) == {7: (LOCK_EX, 1), 9: (LOCK_SH, 1)}


def test_read_uncommitted_leaves_the_table_alone(engine):
    rng = np.random.default_rng(3)
    with engine.locktab(1 << 14) as lt:
        ref = Table()
        first = random_batch(rng, 500, 8, 300, p_write=0.3, types=(RD, WR, XP, SCAN), unique=False)
        rc0, _ = epoch(lt, ref, first, SER)
        before = state_of(lt)
        assert before
        b = random_batch(rng, 2000, 12, 300, p_write=0.3, types=(RD, WR, XP, SCAN), unique=False)
        rc, _ = epoch(lt, ref, b, RUL)
        assert 0 < int((rc == RC_RCOK).sum()) < b.n_txn
        assert state_of(lt) == before
        n, m, _ = lt.release(b, rc, RC_RCOK, isolation=RUL)  # a valid no-op
        assert (n, m) == (int((rc == RC_RCOK).sum()), 0)
        assert state_of(lt) == before
        release(lt, ref, first, rc0, SER)
        assert state_of(lt) == {}


@pytest.mark.parametrize("s", range(3))
def test_random_histories(engine, s):
    """Six epochs of 2,000 txns at random levels; each epoch's commits are
    released two epochs later at that epoch's level."""
    rng = np.random.default_rng(40 + s)
    with engine.locktab(1 << 16) as lt:
        ref = Table()
        past = []
        seen = set()
        for e in range(6):
            level = LEVELS[int(rng.integers(0, 3))] if e >= 3 else LEVELS[(e + s) % 3]  # every level occurs
            seen.add(level)
            b = random_batch(rng, 2000, int(rng.integers(2, 20)), int(rng.integers(3000, 20000)),
                             p_write=0.3, types=(RD, WR, XP, SCAN), unique=bool(e % 2))
            rc, _ = epoch(lt, ref, b, level, dev=e == 4)
            assert 0 < int((rc == RC_RCOK).sum())
            past.append((b, rc, level))
            if e >= 2:
                pb, prc, pl = past[e - 2]
                release(lt, ref, pb, prc, pl, dev=e == 3)
        assert seen == set(LEVELS)


def test_over_release(engine):
    with engine.locktab(64) as lt:
        ref = Table()
        a = make_batch([[(1, RD), (2, WR)], [(3, WR)]])
        rc, _ = epoch(lt, ref, a, RCL)
        before = state_of(lt)
        assert before == {2: (LOCK_EX, 1), 3: (LOCK_EX, 1)}
        twice = make_batch([[(2, WR)], [(5, RD), (2, WR)]])  # row 2 is held once
        with pytest.raises(d.DccError) as e:
            lt.release(twice, None, isolation=RCL)
        assert e.value.code == _abi.DCC_EINVAL and state_of(lt) == before
        # the read of row 1 was released at once: releasing it again at SERIALIZABLE names a row the table lacks
        with pytest.raises(d.DccError) as e:
            lt.release(a, rc, RC_RCOK)
        assert e.value.code == _abi.DCC_EINVAL and state_of(lt) == before
        with pytest.raises(d.DccError) as e:
            lt.release(a, rc, RC_RCOK, isolation=RCL | RUL)
        assert e.value.code == _abi.DCC_EINVAL and state_of(lt) == before
        release(lt, ref, a, rc, RCL)
        assert state_of(lt) == {}


def test_failed_epoch_leaves_the_table(engine):
    with engine.locktab(256) as lt:
        ref = Table()
        epoch(lt, ref, make_batch([[(1, RD), (2, WR)], [(3, WR), (4, RD)]]), RCL)
        before = state_of(lt)
        long = make_batch([[(5, WR)], [(100 + q, WR) for q in range(65)], [(2, RD)]])
        for level in (RCL, RUL):
            with pytest.raises(d.DccError) as e:
                lt.lock_epoch(long, isolation=level)
            assert e.value.code == _abi.DCC_EINVAL and state_of(lt) == before
        epoch(lt, ref, make_batch([[(2, RD)], [(1, WR)]]), RCL)  # the table still works
