"""Which rejection wins when a call breaks several rules at once: the code and
the context's message of dcc_nowait_lock_epoch, dcc_locktab_lock_epoch,
dcc_waitdie_lock_epoch and dcc_waitdie_release for such calls, what a rejected
call leaves untouched, and that the next valid call matches the replay
(nowait_iso_ref.py).  The calls go to the library as given, so that a null
pointer or a nonzero output word reaches it.  The literals are the library's
own; the order among them is what this file pins.

Two rules of the issue's list cannot be broken through the C ABI:
dcc_locktab_lock_epoch passes no held list, and dcc_waitdie_release answers a
null `leave` itself, without a message."""
import ctypes as C

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RC_WAIT, RD, WD_RUN, WR, _abi
from deneva_amd._abi import lib
from deneva_amd.engine import _ptr
from helpers import make_batch
from nowait_iso_ref import LEVELS, RCL, RUL, SER, Table, replay

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, ENOTSUP = _abi.DCC_EINVAL, _abi.DCC_ENOTSUP
BOTH = RCL | RUL
SHARD = _abi.SHARD_SELF
M_BOTH = "nowait: both isolation bits set"
M_SER_ONLY = "nowait: a key-sharded epoch is SERIALIZABLE only"
M_RANKS = "nowait: more than one rank takes the whole epoch with DCC_SHARD_SELF and no lock table"
M_HELD_NULL = "nowait: null held keys/acctype"
M_HELD_KEY = "nowait: held key equal to DCC_KEY_RESERVED"
M_OFF = "batch: malformed offsets"
M_KEY = "batch: key equal to DCC_KEY_RESERVED"
M_WD_ISO = "waitdie: an isolation level below SERIALIZABLE"
M_WD_RANKS = "waitdie: single-GPU engine"
M_WD_RC = "waitdie: an rc byte is none of the five states"


def bad_offsets(b):
    """The batch with offsets that run backwards at txn 1; offsets[0] and offsets[n] stay sound."""
    off = b.offsets.copy()
    off[1] = off[2] + 1
    return d.EpochBatch(off, b.keys, b.acctype)


def reserved_key(b, at=1):
    keys = b.keys.copy()
    keys[at] = d.KEY_RESERVED
    return d.EpochBatch(b.offsets, keys, b.acctype)


GOOD = make_batch([[(1, RD)], [(2, WR), (3, RD)], [(2, RD), (9, WR)], [(7, RD)]])
EMPTY = make_batch([])
BAD_OFF = bad_offsets(GOOD)
BAD_KEY = reserved_key(GOOD)
LONG_BAD_KEY = reserved_key(make_batch([[(1, RD)], [(100 + q, RD) for q in range(65)], [(2, WR)]]), at=40)
HELD = (np.array([7, 9], np.uint64), np.array([WR, RD], np.uint8))
HELD_BAD_KEY = (np.array([7, d.KEY_RESERVED], np.uint64), np.array([WR, RD], np.uint8))
HELD_NULL = "null"  # n = 2 with null keys and access types


def message(eng):
    return lib.dcc_last_error(eng._h).decode()


def held_struct(held, keep):
    if held is None:
        return None
    if held is HELD_NULL:
        return C.byref(_abi.CalvinHeld(2, None, None))
    keep.extend(held)
    return C.byref(_abi.CalvinHeld(int(held[0].shape[0]), _ptr(held[0]), _ptr(held[1])))


def outputs(b):
    """rc and conflict arrays of the batch's kind, filled with 0xEE bytes."""
    n = max(b.n_txn, 1)
    rc, cf = np.full(n, 0xEE, np.uint8), np.full(n, 0xEEEEEEEE, np.uint32)
    if b.on_device:
        import torch
        return torch.from_numpy(rc).to(DEV), torch.from_numpy(cf.view(np.int32)).to(DEV)
    return rc, cf


def host(b, rc, cf):
    if b.on_device:
        rc, cf = rc.cpu().numpy(), cf.cpu().numpy().view(np.uint32)
    return rc[:b.n_txn], cf[:b.n_txn]


def nowait_call(eng, b, flags=0, held=None):
    """dcc_nowait_lock_epoch as given: (code, rc, conflict)."""
    rc, cf = outputs(b)
    keep = []
    cb = b.to_c(flags)
    st = _abi.Stats()
    code = lib.dcc_nowait_lock_epoch(eng._h, C.byref(cb), held_struct(held, keep), _ptr(rc), _ptr(cf), C.byref(st))
    return (code,) + host(b, rc, cf)


def rejected(eng, b, flags, held, code, msg):
    """The call fails with `code` and `msg`.  Its outputs are untouched, unless it is the held list's
    reserved key found by the build of an epoch that is not key-sharded, behind the decisions."""
    got, rc, cf = nowait_call(eng, b, flags, held)
    assert (got, message(eng)) == (code, msg)
    if msg != M_HELD_KEY or (flags & SHARD):
        assert np.all(rc == 0xEE) and np.all(cf == 0xEEEEEEEE), "a rejected call wrote its outputs"


def still_works(eng, level=SER, flags=0):
    erc, ecf = replay(GOOD, HELD, level)
    code, rc, cf = nowait_call(eng, GOOD, flags | level, HELD)
    assert code == _abi.DCC_OK
    assert rc.tolist() == erc.tolist() and cf.tolist() == ecf.tolist()


# (batch, flags, held, code, message) on one context without a communicator
ONE_CONTEXT = [
    ("both_bits+null_held", GOOD, BOTH, HELD_NULL, EINVAL, M_BOTH),
    ("both_bits+malformed_offsets+reserved_held_key", BAD_OFF, BOTH, HELD_BAD_KEY, EINVAL, M_BOTH),
    ("shard_flag+both_bits", GOOD, SHARD | BOTH, None, EINVAL, M_BOTH),
    ("empty+null_held", EMPTY, 0, HELD_NULL, EINVAL, M_HELD_NULL),
    ("empty+both_bits+null_held", EMPTY, BOTH, HELD_NULL, EINVAL, M_BOTH),
    ("malformed_offsets+reserved_held_key", BAD_OFF, 0, HELD_BAD_KEY, EINVAL, M_OFF),
    ("malformed_offsets+reserved_held_key@rc", BAD_OFF, RCL, HELD_BAD_KEY, EINVAL, M_OFF),
    ("malformed_offsets+reserved_held_key@ru", BAD_OFF, RUL, HELD_BAD_KEY, EINVAL, M_OFF),
    ("malformed_offsets+reserved_key", bad_offsets(BAD_KEY), 0, None, EINVAL, M_OFF),
    ("reserved_key+reserved_held_key", BAD_KEY, 0, HELD_BAD_KEY, EINVAL, M_KEY),
    ("65_accesses+reserved_key", LONG_BAD_KEY, 0, None, EINVAL, M_KEY),
    ("65_accesses+reserved_key@rc", LONG_BAD_KEY, RCL, None, EINVAL, M_KEY),
    ("65_accesses+reserved_key@ru", LONG_BAD_KEY, RUL, HELD, EINVAL, M_KEY),
    ("reserved_held_key", GOOD, 0, HELD_BAD_KEY, EINVAL, M_HELD_KEY),
]


@pytest.mark.parametrize("case", ONE_CONTEXT, ids=[c[0] for c in ONE_CONTEXT])
def test_one_context(engine, case):
    _, b, flags, held, code, msg = case
    for bb in (b, b.to_torch(DEV)) if b.n_txn and (held is None or held is HELD_NULL) else (b,):
        rejected(engine, bb, flags, held, code, msg)
    still_works(engine, flags & BOTH if (flags & BOTH) != BOTH else SER)


def test_communicator_of_one_rank(engine):
    """Key-sharded on a communicator: the level's rejection comes before the held list's and before
    any collective; the counted reserved held key after the batch's own errors."""
    with d.Engine(0) as solo:
        solo.set_option(_abi.OPT_COMM_SOLO, 1)
        solo.comm_init(0, 1, d.comm_unique_id())
        c0 = solo.comm_calls
        for level in (RCL, RUL):
            rejected(solo, GOOD, SHARD | level, HELD_NULL, ENOTSUP, M_SER_ONLY)
            rejected(solo, EMPTY, SHARD | level, None, ENOTSUP, M_SER_ONLY)
        rejected(solo, GOOD, SHARD | BOTH, HELD_NULL, EINVAL, M_BOTH)
        rejected(solo, GOOD, SHARD, HELD_NULL, EINVAL, M_HELD_NULL)
        rejected(solo, BAD_OFF, SHARD, HELD_BAD_KEY, EINVAL, M_OFF)
        rejected(solo, BAD_KEY, SHARD, HELD_BAD_KEY, EINVAL, M_KEY)
        rejected(solo, LONG_BAD_KEY, SHARD, HELD_BAD_KEY, EINVAL, M_KEY)
        rejected(solo, GOOD, SHARD, HELD_BAD_KEY, EINVAL, M_HELD_KEY)
        assert solo.comm_calls == c0, "a rejected call reached a collective"
        still_works(solo, flags=SHARD)
        assert solo.comm_calls > c0


def test_communicator_of_two_ranks(engine):
    """More than one rank and no shard flag: that rejection comes first."""
    with d.Engine(0) as eng:
        eng.comm_init_host(0, 2, lambda buf: None)
        rejected(eng, GOOD, BOTH, HELD_NULL, ENOTSUP, M_RANKS)
        rejected(eng, EMPTY, RCL, HELD_NULL, ENOTSUP, M_RANKS)
        rejected(eng, GOOD, SHARD | BOTH, None, EINVAL, M_BOTH)
        rejected(eng, GOOD, SHARD | RCL, HELD_NULL, ENOTSUP, M_SER_ONLY)
        ts, rc, pos = wd_state(GOOD.n_txn)
        for b in (BAD_OFF, EMPTY):
            assert wd_epoch(eng, b, ts, rc, pos) == ENOTSUP and message(eng) == M_WD_RANKS
            assert wd_release(eng, b, ts, rc, pos, np.ones(4, np.uint8)) == (ENOTSUP, 77, 77)
            assert message(eng) == M_WD_RANKS
        eng.comm_destroy()
        still_works(eng)


def test_multi_gpu_context(engine):
    """One process, several GPUs: the shard flag with a level is DCC_ENOTSUP before anything else of
    the call is looked at, both bits included (one context: DCC_EINVAL, test_one_context)."""
    with d.Engine(devices=[0, 0]) as m:
        for b, flags, held in ((GOOD, SHARD | BOTH, None), (GOOD, SHARD | RCL, HELD_NULL),
                               (EMPTY, SHARD | RUL, None), (BAD_OFF, SHARD | BOTH, HELD_BAD_KEY)):
            rejected(m, b, flags, held, ENOTSUP, M_SER_ONLY)
        code, _, _ = nowait_call(m, GOOD, SHARD, HELD_NULL)
        assert (code, message(m)) == (EINVAL, M_HELD_NULL)
        still_works(m, flags=SHARD)
        still_works(m, RCL)


# ------------------------------------------------------------- lock table
def state_of(lt):
    k, t, c = lt.export()
    return {int(a): (int(b), int(x)) for a, b, x in zip(k, t, c)}


def locktab_call(lt, b, flags):
    rc, cf = outputs(b)
    cb = b.to_c(flags)
    st = _abi.Stats()
    code = lib.dcc_locktab_lock_epoch(lt._handle(), C.byref(cb), _ptr(rc), _ptr(cf), C.byref(st))
    return (code,) + host(b, rc, cf)


LOCKTAB = [
    ("both_bits+malformed_offsets", BAD_OFF, BOTH, M_BOTH),
    ("both_bits+empty", EMPTY, BOTH, M_BOTH),
    ("malformed_offsets+reserved_key", bad_offsets(BAD_KEY), SER, M_OFF),
    ("malformed_offsets+reserved_key@rc", bad_offsets(BAD_KEY), RCL, M_OFF),
    ("65_accesses+reserved_key", LONG_BAD_KEY, SER, M_KEY),
    ("65_accesses+reserved_key@rc", LONG_BAD_KEY, RCL, M_KEY),
    ("65_accesses+reserved_key@ru", LONG_BAD_KEY, RUL, M_KEY),
]


def test_lock_table_untouched(engine):
    with engine.locktab(256) as lt:
        ref = Table()
        lt.acquire_rows(*HELD)
        ref.acquire_rows(*HELD)
        for level in LEVELS:
            before = state_of(lt)
            assert before == ref.export() and before
            for _, b, flags, msg in LOCKTAB:
                for bb in (b, b.to_torch(DEV)) if b.n_txn else (b,):
                    code, rc, cf = locktab_call(lt, bb, flags)
                    assert (code, message(engine)) == (EINVAL, msg)
                    assert np.all(rc == 0xEE) and np.all(cf == 0xEEEEEEEE)
                    assert state_of(lt) == before and lt.size()[0] == len(before)
            erc, ecf = ref.lock_epoch(GOOD, level)
            code, rc, cf = locktab_call(lt, GOOD, level)
            assert code == _abi.DCC_OK and rc.tolist() == erc.tolist() and cf.tolist() == ecf.tolist()
            assert state_of(lt) == ref.export()


# --------------------------------------------------------------- WAIT_DIE
def wd_state(n):
    return np.arange(1, n + 1, dtype=np.uint64), np.full(n, WD_RUN, np.uint8), np.zeros(n, np.uint32)


def wd_epoch(eng, b, ts, rc, pos, flags=0):
    cb = b.to_c(flags)
    st = _abi.Stats()
    return lib.dcc_waitdie_lock_epoch(eng._h, C.byref(cb), _ptr(ts), _ptr(rc), _ptr(pos), None, C.byref(st))


def wd_release(eng, b, ts, rc, pos, leave, flags=0):
    """(code, left, promoted); both words hold 77 before the call."""
    cb = b.to_c(flags)
    st = _abi.Stats()
    left, prom = C.c_uint64(77), C.c_uint64(77)
    code = lib.dcc_waitdie_release(eng._h, C.byref(cb), _ptr(ts), _ptr(rc), _ptr(pos), _ptr(leave), C.byref(left),
                                   C.byref(prom), C.byref(st))
    return code, int(left.value), int(prom.value)


def to_dev(*arrs):
    import torch
    return [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else
                             a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV) for a in arrs]


# (batch, flags, rc, pos, code, message, the release's out words after the call)
WAITDIE = [
    ("bad_rc+malformed_offsets", BAD_OFF, 0, [WD_RUN, WD_RUN, 0x12, WD_RUN], [0, 0, 0, 0], EINVAL, M_OFF, 0),
    ("bad_rc+reserved_key", BAD_KEY, 0, [0x12, WD_RUN, WD_RUN, WD_RUN], [0, 0, 0, 0], EINVAL, M_KEY, 0),
    ("bad_rc+bad_pos", GOOD, 0, [WD_RUN, RC_RCOK, WD_RUN, 0xFF], [0, 1, 0, 0], EINVAL, M_WD_RC, 0),
    ("level+bad_rc+malformed_offsets", BAD_OFF, RCL, [WD_RUN, 1, WD_RUN, WD_RUN], [0, 0, 0, 0], ENOTSUP, M_WD_ISO, 77),
    ("level+empty", EMPTY, RUL, [], [], ENOTSUP, M_WD_ISO, 77),
]


@pytest.mark.parametrize("case", WAITDIE, ids=[c[0] for c in WAITDIE])
def test_waitdie(engine, case):
    _, b, flags, rc0, pos0, code, msg, out = case
    n = len(rc0)
    ts = np.arange(1, max(n, 1) + 1, dtype=np.uint64)
    for dev in (False, True) if b.n_txn else (False,):
        rc, pos = np.asarray(rc0 or [0], np.uint8), np.asarray(pos0 or [0], np.uint32)
        leave = np.ones(max(n, 1), np.uint8)
        bb, args = b, [ts, rc, pos, leave]
        if dev:
            bb, args = b.to_torch(DEV), to_dev(ts, rc, pos, leave)
        assert wd_epoch(engine, bb, *args[:3], flags=flags) == code and message(engine) == msg
        assert wd_release(engine, bb, *args, flags=flags) == (code, out, out) and message(engine) == msg
        if dev:
            rc, pos = args[1].cpu().numpy(), args[2].cpu().numpy().view(np.uint32)
        assert rc[:n].tolist() == rc0 and pos[:n].tolist() == pos0, "a rejected call changed the state"


def test_waitdie_null_leave_and_empty(engine):
    ts, rc, pos = wd_state(GOOD.n_txn)
    assert wd_epoch(engine, EMPTY, ts, rc, pos) == _abi.DCC_OK  # leaves a message of its own: none
    before = message(engine)
    # the entry point answers a null array itself: no message, the out words untouched
    assert wd_release(engine, BAD_OFF, ts, rc, pos, None) == (EINVAL, 77, 77) and message(engine) == before
    assert wd_release(engine, EMPTY, ts, rc, pos, None) == (EINVAL, 77, 77) and message(engine) == before
    # the empty batch: zeros in left / promoted
    assert wd_release(engine, EMPTY, ts, rc, pos, np.ones(4, np.uint8)) == (_abi.DCC_OK, 0, 0)
    assert np.all(rc == WD_RUN) and np.all(pos == 0)
    # the context still works: txn 2 reads row 2 behind txn 1's write and is younger: it dies
    assert wd_epoch(engine, GOOD, ts, rc, pos) == _abi.DCC_OK
    assert rc.tolist() == [RC_RCOK, RC_RCOK, RC_ABORT, RC_RCOK] and pos.tolist() == [1, 2, 0, 1]
    assert wd_release(engine, GOOD, ts, rc, pos, np.array([0, 1, 0, 0], np.uint8)) == (_abi.DCC_OK, 1, 0)
    assert RC_WAIT not in rc.tolist()
