"""WAIT_DIE and MVCC with txns in flight share one skeleton (live_txn.h,
DESIGN.md §8s): one counter layout, one check, one state rule, which the
WAIT_DIE carry applies too.  On one context the two engines' calls in turn,
each of which finds the counters, ring words, tile flags, flag bytes and host
staging the other engine left, every call compared bit for bit with its
replay; and the (rc, pos) rule at its three doors, which accept and reject the
same states."""
import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RC_WAIT, RD, WD_GONE, WD_RUN, WR, _abi
from helpers import make_batch
from waitdie_cases import new_state
import mvcc_live_ref as mref
import test_gpu_mvcc_live as ml
import test_gpu_waitdie as wd
import test_gpu_waitdie_carry as wc
from test_gpu_seg_shared import hot_txns
from waitdie_carry_ref import carry

pytestmark = pytest.mark.gpu

TILE = wd.TILE
assert TILE == ml.TILE
# hot_txns seeds, chosen on the replays: every multi-tile epoch takes more than
# two rounds and has RCOK, ABORT and WAIT txns
SEED_WD_1, SEED_ML_2, SEED_WD_5, SEED_ML_6, SEED_ML_7, SEED_WD_8 = 1, 1, 5, 6, 4, 8


def three(st):
    assert min(st["n_commit"], st["n_abort"], st["n_survivors"]) > 0, ml.outcomes(st)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_engines_in_turn_on_one_context(dev):
    with d.Engine(0) as eng:
        # 1. WAIT_DIE epoch, two tiles
        b1, t1 = hot_txns(SEED_WD_1, TILE + 1)
        e1 = wd.check_epoch(eng, b1, t1, *new_state(b1.n_txn), dev=dev)
        three(e1[3])
        assert e1[3]["rounds"] > 2
        # 2. MVCC access epoch, two tiles, two accesses per txn
        b2, t2 = hot_txns(SEED_ML_2, TILE + 1, per_txn=2)
        run2 = ml.Run(eng, b2, t2)
        e2 = run2.epoch(*ml.new_state(b2.n_txn), dev=dev)
        three(e2[3])
        assert e2[3]["rounds"] > 2
        # 3. WAIT_DIE release of the first state
        r3 = wd.check_release(eng, b1, t1, e1[0], e1[1], wd.leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=dev)
        assert r3[3] > 0
        # 4. MVCC finish of every RCOK and ABORT txn
        f4 = run2.finish(e2[0], e2[1], ml.leave_of(e2[0], [RC_RCOK, RC_ABORT]), dev=dev)
        assert f4[2] > 0
        # 5. WAIT_DIE epoch at 3 accesses
        b5, t5 = hot_txns(SEED_WD_5, 3)
        wd.check_epoch(eng, b5, t5, *new_state(3), dev=dev)
        # 6. MVCC access epoch at 1 access
        b6, t6 = hot_txns(SEED_ML_6, 1)
        ml.Run(eng, b6, t6).epoch(*ml.new_state(1), dev=dev)
        # 7. MVCC access epoch, three tiles, on a promoted state.  Before it
        # an epoch of every other txn and the finish of its RCOK and ABORT
        # txns, which promotes readers; the txns in between are admitted then
        b7, t7 = hot_txns(SEED_ML_7, 2 * TILE + 1, per_txn=2)
        run7 = ml.Run(eng, b7, t7)
        rc7, pos7 = ml.new_state(b7.n_txn)
        rc7[1::2] = WD_GONE
        e7 = run7.epoch(rc7, pos7, dev=dev)
        f7 = run7.finish(e7[0], e7[1], ml.leave_of(e7[0], [RC_RCOK, RC_ABORT]), dev=dev)
        assert f7[3] > 0 and int((f7[0] == WD_RUN).sum()) == f7[3]
        rc7, pos7 = f7[0].copy(), f7[1].copy()
        ml.admit(rc7, pos7, range(1, b7.n_txn, 2))
        g7 = run7.epoch(rc7, pos7, dev=dev)
        three(g7[3])
        assert g7[3]["rounds"] > 2
        # 8. WAIT_DIE epoch, one full tile
        b8, t8 = hot_txns(SEED_WD_8, TILE)
        e8 = wd.check_epoch(eng, b8, t8, *new_state(b8.n_txn), dev=dev)
        three(e8[3])
        assert e8[3]["rounds"] > 2


# ------------------------------------------------- one rule at three doors
STATES = (WD_RUN, RC_RCOK, RC_WAIT, RC_ABORT, WD_GONE, 0x12)


def rule_cases():
    """(rc, len, pos) of the middle txn: every state byte and 0x12, len 0 .. 2,
    pos 0, len - 1, len and len + 1."""
    return [(rc, L, p) for rc in STATES for L in (0, 1, 2) for p in sorted({0, max(L - 1, 0), L, L + 1})]


def rule_batch(rc, L, p):
    b = make_batch([[(10, RD)], [(20 + q, WR) for q in range(L)], [(30, RD)]])
    return (b, np.asarray([5, 6, 7], np.uint64), np.asarray([WD_RUN, rc, WD_RUN], np.uint8),
            np.asarray([0, p, 0], np.uint32))


def accepts(fn):
    try:
        fn()
    except ValueError:
        return False
    return True


def test_one_state_rule_at_three_doors(engine):
    assert len(rule_cases()) == len(set(rule_cases())) == 6 * 9
    n_acc = 0
    for rc_m, L, p_m in rule_cases():
        b, ts, rc, pos = rule_batch(rc_m, L, p_m)
        what = f"rc {rc_m:#x} len {L} pos {p_m}"
        ok = [accepts(lambda: wd.replay_epoch(b, ts, rc, pos)), accepts(lambda: mref.epoch(b, ts, rc, pos)),
              accepts(lambda: carry(b, ts, rc, pos))]
        assert ok[0] == ok[1] == ok[2], f"{what}: the references disagree {ok}"
        if ok[0]:
            n_acc += 1
            wd.check_epoch(engine, b, ts, rc, pos)
            ml.Run(engine, b, ts).epoch(rc, pos)
            wc.check(engine, b, ts, rc, pos, modes=(False,))
            continue
        bad_rc = rc_m == 0x12
        doors = [
            (lambda r, p: engine.waitdie_lock_epoch(b, ts, r, p),
             "waitdie: an rc byte is none of the five states" if bad_rc else
             "waitdie: a pos does not fit its state (pos > len, RCOK below len, WAIT at len)"),
            (lambda r, p: engine.mvcc_access_epoch(b, ts, r, p),
             "mvcc: an rc byte is none of the five states" if bad_rc else
             "mvcc: a pos does not fit its state (pos > len, RCOK below len, WAIT at len)"),
            (lambda r, p: engine.waitdie_carry(b, ts, r, p),
             "waitdie_carry: an rc byte outside the five states" if bad_rc else
             "waitdie_carry: pos does not fit its txn's state"),
        ]
        for call, msg in doors:
            r, p = rc.copy(), pos.copy()
            with pytest.raises(d.DccError) as e:
                call(r, p)
            assert e.value.code == _abi.DCC_EINVAL and msg in str(e.value), (what, str(e.value))
            assert np.array_equal(r, rc) and np.array_equal(p, pos), what
    # RUN: pos <= len; RCOK: pos == len; WAIT: pos < len; ABORT: pos <= len; GONE: any
    assert n_acc == 6 + 3 + 3 + 6 + 9
