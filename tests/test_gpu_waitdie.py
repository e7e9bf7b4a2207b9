"""GPU parity of the WAIT_DIE calls (dcc_waitdie_lock_epoch, dcc_waitdie_release,
waitdie.hip) against the closed-form replay (waitdie_ref.py): rc, pos, the
conflict ordinals and the counts after every call, bit-exact."""
import functools
import os
import re

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RC_WAIT, RD, SCAN, WD_GONE, WD_RUN, WR, XP, _abi
from helpers import make_batch
from waitdie_cases import KATS, admit, history, hot_batch, make_ts, new_state, outcomes
from waitdie_ref import replay_epoch, replay_release, replay_rounds_epoch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constant(name):
    src = open(os.path.join(ROOT, "deneva_amd", "csrc", "waitdie.hip")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


WD_T = kernel_constant("WD_T")          # threads per workgroup
WD_ITEMS = kernel_constant("WD_ITEMS")  # sorted accesses per thread
TILE = WD_T * WD_ITEMS                  # accesses per scan tile
WD_RING = kernel_constant("WD_RING")    # undecided-count ring


def to_dev(ts, rc, pos, leave=None):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(ts, np.uint64).view(np.int64)).to("cuda:0"),
           torch.from_numpy(np.array(rc, np.uint8)).to("cuda:0"),
           torch.from_numpy(np.array(pos, np.uint32).view(np.int32)).to("cuda:0")]
    if leave is not None:
        out.append(torch.from_numpy(np.ascontiguousarray(leave, np.uint8)).to("cuda:0"))
    return out


def from_dev(rc, pos):
    return rc.cpu().numpy(), pos.cpu().numpy().view(np.uint32)


def differ(what, got, exp):
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    assert bad.size == 0, f"{what} differs at {bad[:10]} (gpu {np.asarray(got)[bad[:10]]} replay {np.asarray(exp)[bad[:10]]})"


def check_epoch(eng, b, ts, rc, pos, exp=None, dev=False, run_batch=None, want_conflict=True):
    """One epoch from the state (rc, pos), which is not changed; compared with
    exp = replay_epoch's result.  Returns (rc, pos, conflict, stats) as numpy."""
    exp = exp if exp is not None else replay_epoch(b, ts, rc, pos)
    bb = run_batch if run_batch is not None else b
    if dev:
        bb = bb.to_torch("cuda:0")
        t, r, p = to_dev(ts, rc, pos)
        r, p, cf, st = eng.waitdie_lock_epoch(bb, t, r, p, want_conflict=want_conflict)
        r, p = from_dev(r, p)
        cf = cf.cpu().numpy().view(np.uint32) if cf is not None else None
    else:
        r, p = np.array(rc, np.uint8), np.array(pos, np.uint32)
        r, p, cf, st = eng.waitdie_lock_epoch(bb, np.asarray(ts, np.uint64), r, p, want_conflict=want_conflict)
    differ("rc", r, exp[0])
    differ("pos", p, exp[1])
    if want_conflict:
        differ("conflict", cf, exp[2])
    else:
        assert cf is None
    for k in ("n_commit", "n_abort", "n_survivors", "nnz_w", "n_readonly"):
        assert st[k] == exp[3][k], (k, st[k], exp[3][k])
    if b.n_txn:
        n, m = b.n_txn, b.nnz
        assert st["alg_bytes"] == d.waitdie_alg_bytes(n, m, want_conflict)
        assert d.waitdie_alg_bytes(n, m, True) == 4 * (n + 1) + 13 * n + 9 * m + 24 * m + 5 * n + 4 * n
    return r, p, cf, st


def check_release(eng, b, ts, rc, pos, leave, exp=None, dev=False, run_batch=None):
    exp = exp if exp is not None else replay_release(b, ts, rc, pos, leave)
    bb = run_batch if run_batch is not None else b
    if dev:
        bb = bb.to_torch("cuda:0")
        t, r, p, lv = to_dev(ts, rc, pos, leave)
        left, prom, st = eng.waitdie_release(bb, t, r, p, lv)
        r, p = from_dev(r, p)
    else:
        r, p = np.array(rc, np.uint8), np.array(pos, np.uint32)
        left, prom, st = eng.waitdie_release(bb, np.asarray(ts, np.uint64), r, p, np.asarray(leave, np.uint8))
    differ("rc", r, exp[0])
    differ("pos", p, exp[1])
    assert (left, prom) == (exp[2], exp[3])
    assert st["n_commit"] == exp[2] and st["n_survivors"] == exp[3]
    return r, p, left, prom


def three_outcomes(exp):
    st = exp[3]
    assert min(st["n_commit"], st["n_abort"], st["n_survivors"]) > 0, \
        f"the replay misses an outcome: {st['n_commit']} RCOK, {st['n_abort']} ABORT, {st['n_survivors']} WAIT"


def leave_of(rc, states):
    return np.isin(rc, states).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ycsb(n_txn):
    """A YCSB theta 0.9 batch, ts = index with jitter, and the replay of: an
    epoch, the release of every RCOK and ABORT txn, a second epoch."""
    b = d.gen_ycsb(n_txn=n_txn, zipf_theta=0.9)
    ts = make_ts(np.random.default_rng(n_txn), n_txn, "jitter")
    rc, pos = new_state(n_txn)
    e1 = replay_epoch(b, ts, rc, pos)
    leave = leave_of(e1[0], [RC_RCOK, RC_ABORT])
    r1 = replay_release(b, ts, e1[0], e1[1], leave)
    e2 = replay_epoch(b, ts, r1[0], r1[1])
    return b, ts, e1, leave, r1, e2


# ------------------------------------------------------------ known answers
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(engine, case, dev):
    _, txns, ts, rc0, steps = case
    b = make_batch(txns)
    ts = np.asarray(ts, np.uint64)
    rc, pos = np.asarray(rc0, np.uint8), np.zeros(len(txns), np.uint32)
    for s in steps:
        if s[0] == "admit":
            admit(rc, pos, s[1])
        elif s[0] == "epoch":
            rc, pos, cf, _ = check_epoch(engine, b, ts, rc, pos, dev=dev)
            assert (rc.tolist(), pos.tolist(), cf.tolist()) == (s[1], s[2], s[3])
        else:
            leave = np.zeros(len(txns), np.uint8)
            leave[s[1]] = 1
            rc, pos, left, prom = check_release(engine, b, ts, rc, pos, leave, dev=dev)
            assert (rc.tolist(), pos.tolist(), left, prom) == (s[2], s[3], len(s[1]), s[4])


# ---------------------------------------------------------------- the edges
def test_empty_zero_length_gone_and_run_at_len(engine):
    e = make_batch([])
    z = np.zeros(0, np.uint64)
    rc, pos, cf, st = engine.waitdie_lock_epoch(e, z, np.zeros(0, np.uint8), np.zeros(0, np.uint32))
    assert len(rc) == 0 and len(pos) == 0 and len(cf) == 0 and st["n_commit"] == 0
    assert engine.waitdie_release(e, z, np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint8))[:2] == (0, 0)
    # zero-length txns: a RUN one turns RCOK at pos 0 == len
    b = make_batch([[], [(1, WR)], [], [(1, RD)], []])
    ts = np.asarray([5, 4, 3, 2, 1], np.uint64)
    r, p, cf, st = check_epoch(engine, b, ts, *new_state(5))
    assert r.tolist() == [RC_RCOK, RC_RCOK, RC_RCOK, RC_WAIT, RC_RCOK] and st["rounds"] >= 1
    _, _, _, st = check_epoch(engine, make_batch([[], [], []]), ts[:3], *new_state(3), dev=True)
    assert st["n_commit"] == 3 and st["rounds"] == 1 and st["n_readonly"] == 3
    check_release(engine, make_batch([[], [], []]), ts[:3], *new_state(3), np.asarray([1, 0, 1], np.uint8))
    # all GONE: nothing runs, whatever pos holds
    rc, pos = new_state(5, WD_GONE)
    pos[:] = [7, 0, 99, 1, 2]
    for dev in (False, True):
        r, p, cf, st = check_epoch(engine, b, ts, rc, pos, dev=dev)
        assert np.all(r == WD_GONE) and p.tolist() == pos.tolist() and np.all(cf == ACCESS_NONE)
        assert st["n_commit"] == st["n_abort"] == st["n_survivors"] == 0 and st["rounds"] == 1
        _, _, left, prom = check_release(engine, b, ts, rc, pos, np.ones(5, np.uint8), dev=dev)
        assert (left, prom) == (0, 0)
    # RUN at pos == len (a promoted waiter at its last access), next to every other state
    b = make_batch([[(1, WR)], [(1, WR), (2, RD)], [], [(2, WR)], [(9, RD)]])
    rc = np.asarray([WD_RUN, RC_ABORT, WD_RUN, WD_GONE, RC_RCOK], np.uint8)
    pos = np.asarray([1, 1, 0, 77, 1], np.uint32)
    r, p, cf, _ = check_epoch(engine, b, ts, rc, pos)
    assert r.tolist() == [RC_RCOK, RC_ABORT, RC_RCOK, WD_GONE, RC_RCOK] and p.tolist() == pos.tolist()


def test_lanes_per_txn_and_the_length_limit(engine):
    """Txn lengths 1, 2, 16, 17 and 64 in one batch (64 lanes per txn), then a
    txn of 65: DCC_EINVAL with rc / pos as they were."""
    rng = np.random.default_rng(5)
    lens = [1, 2, 16, 17, 64] * 40
    txns = [[(int(k), int(t)) for k, t in zip(rng.integers(0, 300, size=L), rng.choice([RD, WR, XP, SCAN], size=L,
                                                                                        p=[.6, .2, .1, .1]))]
            for L in lens]
    b = make_batch(txns)
    ts = make_ts(rng, b.n_txn, "permuted")
    rc, pos = new_state(b.n_txn)
    e1 = replay_epoch(b, ts, rc, pos)
    three_outcomes(e1)
    assert int(((e1[0] != RC_RCOK) & (e1[2] > 32)).sum()) > 0  # stops in the upper lanes too
    check_epoch(engine, b, ts, rc, pos, exp=e1)
    r1 = check_release(engine, b, ts, e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=True)
    check_epoch(engine, b, ts, r1[0], r1[1], dev=True)
    long = make_batch([[(1, RD)], [(100 + q, WR) for q in range(65)], [(2, WR)]])
    t3 = np.asarray([9, 8, 7], np.uint64)
    for dev in (False, True):
        rc, pos = new_state(3)
        if dev:
            bb = long.to_torch("cuda:0")
            args = to_dev(t3, rc, pos, np.ones(3, np.uint8))
        else:
            bb, args = long, [t3, rc, pos, np.ones(3, np.uint8)]
        for call in (lambda: engine.waitdie_lock_epoch(bb, *args[:3]), lambda: engine.waitdie_release(bb, *args)):
            with pytest.raises(d.DccError) as e:
                call()
            assert e.value.code == _abi.DCC_EINVAL
            r, p = from_dev(args[1], args[2]) if dev else (args[1], args[2])
            assert np.all(r == WD_RUN) and np.all(p == 0)


# ------------------------------------------------------------- tile seams
def one_row(rng, n_own, n_wait, n_dyn, key=77):
    """One row: n_own SH owners (RCOK txns), n_wait static waiters (EX, older
    than every owner), n_dyn RUN txns of mixed types."""
    n = n_own + n_wait + n_dyn
    at = np.full(n, RD, np.uint8)
    at[n_own:n_own + n_wait] = WR
    at[n_own + n_wait:] = rng.choice(np.asarray([RD, WR, SCAN, XP], np.uint8), size=n_dyn, p=[.6, .2, .1, .1])
    perm = rng.permutation(n).astype(np.uint64)
    ts = np.empty(n, np.uint64)
    ts[:n_own] = np.uint64(10 * n) + perm[:n_own]
    ts[n_own:n_own + n_wait] = np.uint64(1) + perm[n_own:n_own + n_wait]
    ts[n_own + n_wait:] = np.uint64(5 * n) + np.uint64(10) * perm[n_own + n_wait:]
    rc = np.full(n, WD_RUN, np.uint8)
    rc[:n_own] = RC_RCOK
    rc[n_own:n_own + n_wait] = RC_WAIT
    pos = np.zeros(n, np.uint32)
    pos[:n_own] = 1
    # shuffle the txns so that static and dynamic accesses interleave in batch order
    order = rng.permutation(n)
    b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, key, np.uint64), at[order])
    return b, ts[order], rc[order], pos[order]


@pytest.mark.parametrize("n", [TILE + 1, 2 * TILE + 3])
def test_one_row_across_tiles(engine, n):
    """One row named by n one-access RUN txns: its segment crosses the tile
    seams; then the same row with waiters to release."""
    rng = np.random.default_rng(n)
    b, ts, rc, pos = one_row(rng, 0, 0, n)
    e1 = check_epoch(engine, b, ts, rc, pos)
    assert e1[3]["n_survivors"] > 0 and e1[3]["n_commit"] > 0
    r1 = check_release(engine, b, ts, e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]))
    assert r1[3] > 0
    check_epoch(engine, b, ts, r1[0], r1[1], dev=True)


@pytest.mark.parametrize("m", [TILE - 1, TILE, TILE + 1])
def test_batch_of_a_tile(engine, m):
    """m accesses in all, one per txn, on three hot rows."""
    rng = np.random.default_rng(m)
    keys = rng.choice(np.asarray([3, 9, 1 << 40], np.uint64), size=m, p=[0.5, 0.3, 0.2])
    at = rng.choice(np.asarray([RD, WR, SCAN], np.uint8), size=m, p=[0.7, 0.2, 0.1])
    b = d.EpochBatch(np.arange(m + 1, dtype=np.uint32), keys, at)
    ts = make_ts(rng, m, "permuted")
    e1 = check_epoch(engine, b, ts, *new_state(m))
    three_outcomes(e1)
    r1 = check_release(engine, b, ts, e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]))
    check_epoch(engine, b, ts, r1[0], r1[1])


@pytest.mark.parametrize("n_own,n_wait,n_dyn", [(TILE - 3, 0, 40), (TILE - 20, 17, 40), (TILE + 5, 9, TILE),
                                                (5, TILE + 2, 30)])
def test_static_and_dynamic_across_a_seam(engine, n_own, n_wait, n_dyn):
    """The row's static accesses end, and its dynamic ones begin, on either
    side of a tile seam; waiters beyond a tile for the release's scan."""
    rng = np.random.default_rng(n_own + n_wait)
    b, ts, rc, pos = one_row(rng, n_own, n_wait, n_dyn)
    e1 = check_epoch(engine, b, ts, rc, pos)
    assert e1[3]["n_abort"] > 0 and e1[3]["n_commit"] + e1[3]["n_survivors"] > 0
    leave = leave_of(e1[0], [RC_RCOK, RC_ABORT])
    r1 = check_release(engine, b, ts, e1[0], e1[1], leave, dev=True)
    assert r1[3] > 0
    check_epoch(engine, b, ts, r1[0], r1[1])


# ------------------------------------------------------------------ rounds
def test_chain_of_100_rounds(engine):
    """Txn i names row i - 1 then row i (EX), ts falling: it is decided a
    round after txn i - 1: more rounds than the undecided-count ring holds and
    than one host batch of rounds."""
    n = 100
    assert n > WD_RING
    b = make_batch([[(0, WR)]] + [[(i - 1, WR), (i, WR)] for i in range(1, n)])
    ts = np.arange(n, 0, -1).astype(np.uint64)
    rc, pos = new_state(n)
    exp = replay_epoch(b, ts, rc, pos)
    assert exp[0].tolist() == [RC_RCOK if i % 2 == 0 else RC_WAIT for i in range(n)]
    _, _, _, st = check_epoch(engine, b, ts, rc, pos, exp=exp)
    assert n - 1 <= st["rounds"] <= n + 1
    assert st["rounds"] == replay_rounds_epoch(b, ts, rc, pos)[3]["rounds"]


def test_one_row_eight_times_in_a_txn(engine):
    """Own accesses below the progress count as owners for the txn itself: RD
    x 8 passes, a WR behind seven RD waits on the txn itself, with an older SH
    owner in front it dies; each next to other txns of the row."""
    K = 3
    cases = [([[(K, RD)] * 8], [4]),
             ([[(K, RD)] * 7 + [(K, WR)]], [4]),
             ([[(K, RD)], [(K, RD)] * 7 + [(K, WR)], [(K, RD)]], [1, 4, 9]),
             ([[(K, RD)], [(K, RD)] * 7 + [(K, WR)], [(K, RD)], [(K, WR)] * 8, [(K, SCAN)] * 8], [9, 4, 2, 1, 3])]
    for txns, ts in cases:
        b = make_batch(txns)
        ts = np.asarray(ts, np.uint64)
        rc, pos = new_state(len(txns))
        _, _, _, st = check_epoch(engine, b, ts, rc, pos)
        assert st["rounds"] == replay_rounds_epoch(b, ts, rc, pos)[3]["rounds"]
    rng = np.random.default_rng(8)
    b = hot_batch(rng, 500, 8, 40)  # rows drawn with replacement: many duplicates
    ts = make_ts(rng, 500, "tied")
    e1 = check_epoch(engine, b, ts, *new_state(500))
    three_outcomes(e1)


def test_hot_row_of_20000(engine):
    """20,000 one-access txns on one row, distinct ts in random order."""
    n = 20000
    rng = np.random.default_rng(17)
    at = rng.choice(np.asarray([RD, WR], np.uint8), size=n, p=[0.8, 0.2])
    b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, 77, np.uint64), at)
    ts = make_ts(rng, n, "permuted")
    e1 = check_epoch(engine, b, ts, *new_state(n))
    three_outcomes(e1)
    r1 = check_release(engine, b, ts, e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=True)
    assert r1[3] > 0


# -------------------------------------------------------------------- YCSB
@pytest.mark.parametrize("form", ["host", "device", "compact"])
def test_ycsb_epoch_release_epoch(engine, form):
    """8,192 x 16 at theta 0.9: an epoch, the release of every RCOK and ABORT
    txn, a second epoch; host, device and compact batches."""
    b, ts, e1, leave, r1, e2 = ycsb(8192)
    three_outcomes(e1)
    assert r1[3] > 0 and e2[3]["n_commit"] > 0
    kw = {"dev": form == "device"}
    if form == "compact":
        kw["run_batch"] = engine.compact_host_batch(b)
        assert kw["run_batch"].keys.dtype == np.uint32 and kw["run_batch"].meta.get("acctype_2bit")
    rc, pos = new_state(b.n_txn)
    _, _, _, st = check_epoch(engine, b, ts, rc, pos, exp=e1, **kw)
    assert st["rounds"] > 1
    check_release(engine, b, ts, e1[0], e1[1], leave, exp=r1, **kw)
    check_epoch(engine, b, ts, r1[0], r1[1], exp=e2, **kw)


def test_without_conflict_output(engine):
    b, ts, e1, _, _, _ = ycsb(8192)
    rc, pos = new_state(b.n_txn)
    check_epoch(engine, b, ts, rc, pos, exp=e1, want_conflict=False)
    check_epoch(engine, b, ts, rc, pos, exp=e1, want_conflict=False, dev=True)


@pytest.mark.parametrize("family", ["permuted", "tied", "span63"])
def test_six_epoch_histories(engine, family):
    """2,000 txns, six epoch + release pairs with admissions, leavers of every
    state and a random leave mask: compared after each of the twelve calls."""
    rng = np.random.default_rng(len(family))
    n = 2000
    b = hot_batch(rng, n, 8, 500)
    ts = make_ts(rng, n, family)
    steps = history(rng, b, ts, replay_epoch, replay_release)
    assert len(steps) == 12 and min(outcomes(steps)) > 0
    proms = 0
    for q, s in enumerate(steps):
        dev = q % 4 >= 2
        if s[0] == "epoch":
            check_epoch(engine, b, ts, s[1], s[2], exp=s[3], dev=dev)
        else:
            proms += check_release(engine, b, ts, s[1], s[2], s[3], exp=s[4], dev=dev)[3]
    assert proms > 0


# ---------------------------------------------------------------- rejections
def test_rejections_leave_rc_and_pos(engine):
    b = make_batch([[(1, RD), (2, WR)], [(3, WR)], [(2, RD)]])
    ts = np.asarray([1, 2, 3], np.uint64)
    leave = np.asarray([1, 0, 0], np.uint8)
    off = b.offsets.copy()
    off[1] = 4  # [0, 4, 3, 4]: decreases
    keys = b.keys.copy()
    keys[1] = d.KEY_RESERVED
    ok_rc, ok_pos = [WD_RUN, WD_RUN, WD_RUN], [0, 0, 0]
    bad = [(b, [WD_RUN, 0x12, WD_RUN], [0, 0, 0]),        # rc bytes outside the five states
           (b, [WD_RUN, 1, WD_RUN], [0, 0, 0]),
           (b, [WD_RUN, 0xFF, WD_RUN], [0, 0, 0]),
           (b, [WD_RUN, WD_RUN, WD_RUN], [3, 0, 0]),      # pos > len
           (b, [RC_ABORT, WD_RUN, WD_RUN], [3, 0, 0]),
           (b, [RC_RCOK, WD_RUN, WD_RUN], [1, 0, 0]),     # RCOK with pos != len
           (b, [RC_WAIT, WD_RUN, WD_RUN], [2, 0, 0]),     # WAIT with pos >= len
           (d.EpochBatch(off, b.keys, b.acctype), ok_rc, ok_pos),
           (d.EpochBatch(b.offsets, keys, b.acctype), ok_rc, ok_pos)]
    for bb, rc0, pos0 in bad:
        for dev in (False, True):
            if dev:
                run_b = bb.to_torch("cuda:0")
                args = to_dev(ts, rc0, pos0, leave)
            else:
                run_b = bb
                args = [ts, np.asarray(rc0, np.uint8), np.asarray(pos0, np.uint32), leave]
            for call in (lambda: engine.waitdie_lock_epoch(run_b, *args[:3]),
                         lambda: engine.waitdie_release(run_b, *args)):
                with pytest.raises(d.DccError) as e:
                    call()
                assert e.value.code == _abi.DCC_EINVAL
                r, p = from_dev(args[1], args[2]) if dev else (args[1], args[2])
                assert r.tolist() == rc0 and p.tolist() == pos0
    # NULL ts / rc / pos / leave
    rc, pos = new_state(3)
    for args in ((None, rc, pos), (ts, None, pos), (ts, rc, None)):
        with pytest.raises(d.DccError) as e:
            engine.waitdie_lock_epoch(b, *args)
        assert e.value.code == _abi.DCC_EINVAL
        with pytest.raises(d.DccError) as e:
            engine.waitdie_release(b, *args, leave)
        assert e.value.code == _abi.DCC_EINVAL
    with pytest.raises(d.DccError) as e:
        engine.waitdie_release(b, ts, rc, pos, None)
    assert e.value.code == _abi.DCC_EINVAL
    assert np.all(rc == WD_RUN) and np.all(pos == 0)
    # a GONE txn's pos is ignored, and the context still works
    check_epoch(engine, b, ts, np.asarray([WD_GONE, WD_RUN, WD_RUN], np.uint8), np.asarray([99, 0, 0], np.uint32))


def test_reserve_and_repeat(engine):
    b, ts, e1, leave, r1, e2 = ycsb(8192)
    engine.reserve(b.n_txn, b.nnz)
    rc, pos = new_state(b.n_txn)
    a = check_epoch(engine, b, ts, rc, pos, exp=e1, dev=True)
    c = check_epoch(engine, b, ts, rc, pos, exp=e1, dev=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], c[:3]))
    for _ in range(2):
        check_release(engine, b, ts, e1[0], e1[1], leave, exp=r1, dev=True)
        check_epoch(engine, b, ts, r1[0], r1[1], exp=e2)


# ----------------------------------------------------------------- multi-GPU
def device_count():
    import torch
    return torch.cuda.device_count()


@pytest.mark.parametrize("devices", [[0, 0], [0, 1]], ids=["one_device_twice", "two_devices"])
def test_multi_context_runs_on_rank0(devices):
    if max(devices) >= device_count():
        pytest.skip("needs two devices")
    b, ts, e1, leave, r1, e2 = ycsb(8192)
    rc, pos = new_state(b.n_txn)
    with d.Engine(devices=devices) as m:
        check_epoch(m, b, ts, rc, pos, exp=e1)
        check_release(m, b, ts, e1[0], e1[1], leave, exp=r1, dev=True)
        check_epoch(m, b, ts, r1[0], r1[1], exp=e2, dev=True)


def test_two_rank_communicator_not_supported():
    b, ts, e1, leave, _, _ = ycsb(8192)
    rc, pos = new_state(b.n_txn)
    with d.Engine(0) as eng:
        eng.comm_init_host(0, 2, lambda buf: None)
        with pytest.raises(d.DccError) as e:
            eng.waitdie_lock_epoch(b, ts, rc, pos)
        assert e.value.code == _abi.DCC_ENOTSUP
        with pytest.raises(d.DccError) as e:
            eng.waitdie_release(b, ts, rc, pos, leave)
        assert e.value.code == _abi.DCC_ENOTSUP
        assert np.all(rc == WD_RUN) and np.all(pos == 0)
        eng.comm_destroy()
        check_epoch(eng, b, ts, rc, pos, exp=e1)
