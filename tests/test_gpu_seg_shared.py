"""TIMESTAMP, MVCC and WAIT_DIE share one set of epoch workspaces (dcc_ctx.h
SegWork), and with NO_WAIT one rounds loop: on one context,
big, tiny and big epochs of the four engines in turn, each of which finds the
counters, ring, tile flags and aggregates the engine before it left.  Every
call is compared bit for bit with its engine's replay."""
import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RD, SCAN, WR
from tso_cases import make_ts
from waitdie_cases import new_state
import test_gpu_mvcc as mv
import test_gpu_nowait as nw
import test_gpu_tso as ts_
import test_gpu_waitdie as wd

pytestmark = pytest.mark.gpu

HOT = np.asarray([3, 9, 1 << 40], np.uint64)  # a few hot rows: more than two rounds per epoch


def hot_txns(seed, m, per_txn=1):
    """m accesses on the hot rows, per_txn to a txn (the last one takes what is
    left), ts = index with jitter."""
    rng = np.random.default_rng(seed)
    keys = rng.choice(HOT, size=m, p=[0.5, 0.3, 0.2])
    at = rng.choice(np.asarray([RD, WR, SCAN], np.uint8), size=m, p=[0.5, 0.4, 0.1])
    off = np.concatenate([np.arange(0, m, per_txn), [m]]).astype(np.uint32)
    return d.EpochBatch(off, keys, at), make_ts(rng, off.size - 1, "jitter")


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_engines_in_turn_on_one_context(dev):
    with d.Engine(0) as eng:
        rows = {}  # the TIMESTAMP rows, as the replays leave them
        eng.tso_rows_clear()

        def tso(b, t):
            rc, cf = ts_.replay(b, t, rows)
            return ts_.run(eng, b, t, (rc, cf, rows), dev=dev)

        # 1. TIMESTAMP, three tiles, the last one partial
        b1, t1 = hot_txns(1, 2 * ts_.TS_TILE + 1)
        assert b1.nnz == 2049
        rc1, _, st = tso(b1, t1)
        assert st["rounds"] > 2 and 0 < int((rc1 == RC_RCOK).sum()) < b1.n_txn
        # 2. / 3. WAIT_DIE epoch and release at 3 accesses
        b2, t2 = hot_txns(2, 3)
        r, p, _, _ = wd.check_epoch(eng, b2, t2, *new_state(3), dev=dev)
        wd.check_release(eng, b2, t2, r, p, wd.leave_of(r, [RC_RCOK, RC_ABORT]), dev=dev)
        # 4. MVCC, two tiles; a read never stops its txn, so one-access txns
        # take two rounds: two accesses each, where the second one is executed
        # or not with the first
        b4, t4 = hot_txns(4, ts_.TS_TILE + 1, per_txn=2)
        assert b4.nnz == 1025
        _, _, _, st = mv.step(eng, mv.fresh(eng), b4, t4, dev=dev)
        assert st["rounds"] > 2
        # 5. WAIT_DIE, one full tile
        b5, t5 = hot_txns(5, wd.TILE)
        assert b5.nnz == 1024
        exp = wd.replay_epoch(b5, t5, *new_state(b5.n_txn))
        wd.three_outcomes(exp)
        _, _, _, st = wd.check_epoch(eng, b5, t5, *new_state(b5.n_txn), exp=exp, dev=dev)
        assert st["rounds"] > 2
        # 6. TIMESTAMP at one access
        b6, t6 = hot_txns(6, 1)
        tso(b6, t6 + np.uint64(5000))
        # 7. NO_WAIT
        b7, _ = hot_txns(7, 1025)
        ref = nw.replay(b7)
        nw.both_outcomes(ref)
        _, _, st = nw.check(eng, b7, ref=ref, dev=dev)
        assert st["rounds"] > 2
        # 8. TIMESTAMP at 2,049 again, on the rows the calls before left and
        # with ts above theirs: the decisions of the first call
        rc8, _, st = tso(b1, t1 + np.uint64(10000))
        assert st["rounds"] > 2 and np.array_equal(rc8, rc1)
