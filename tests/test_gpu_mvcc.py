"""GPU parity of the MVCC epoch (dcc_mvcc_validate_epoch, mvcc.hip) against the
closed-form replay of Row_mvcc (mvcc_ref.py), carried across the calls: RC, the
WR each aborted txn aborted at, the version every access read, the counts and,
after every call, (latest version, rts) of every touched row and the whole
version store, bit-exact."""
import functools
import os
import re

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RD, SCAN, VTS_BASE, VTS_NONE, WR, XP, _abi
from helpers import make_batch, random_batch
from mvcc_cases import KATS, TS_FAMILIES, epoch_base, make_ts
from mvcc_ref import against_timestamp, replay, rows_of, trim, versions_of
import tso_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constant(name):
    src = open(os.path.join(ROOT, "deneva_amd", "csrc", "mvcc.hip")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


TS_T = kernel_constant("TS_T")          # threads per workgroup
TS_ITEMS = kernel_constant("TS_ITEMS")  # sorted accesses per thread
TS_TILE = TS_T * TS_ITEMS               # accesses per scan / compaction / trim tile


def check_state(eng, keys, state):
    """mvcc_rows_get over `keys` and mvcc_versions() equal the replay's state."""
    k = np.unique(np.asarray(keys, np.uint64))
    rows = rows_of(state)
    if k.size:
        w, r = eng.mvcc_rows_get(k)
        ew = np.asarray([rows.get(int(x), (0, 0))[0] for x in k], np.uint64)
        er = np.asarray([rows.get(int(x), (0, 0))[1] for x in k], np.uint64)
        bad = np.nonzero((w != ew) | (r != er))[0]
        assert bad.size == 0, (f"row state differs at keys {k[bad[:5]]}: gpu {list(zip(w[bad[:5]], r[bad[:5]]))} "
                               f"replay {list(zip(ew[bad[:5]], er[bad[:5]]))}")
    vk, vt = eng.mvcc_versions()
    ev = versions_of(state)
    assert eng.mvcc_versions_size == len(ev) == vk.size
    ek = np.asarray([x[0] for x in ev], np.uint64)
    et = np.asarray([x[1] for x in ev], np.uint64)
    bad = np.nonzero((vk != ek) | (vt != et))[0]
    assert bad.size == 0, f"version store differs at {bad[:5]}: gpu {list(zip(vk[bad[:5]], vt[bad[:5]]))}"


def step(eng, state, b, ts, dev=False, run_batch=None, want_conflict=True, want_vts=True, info=None):
    """One call on the engine's state as it stands, which `state` mirrors; the
    replay advances `state`.  Returns (rc, conflict, vts, stats)."""
    erc, ecf, evts = replay(b, ts, state, info)
    bb = run_batch if run_batch is not None else b
    tt = np.ascontiguousarray(ts, np.uint64)
    if dev:
        import torch
        bb = bb.to_torch("cuda:0")
        tt = torch.from_numpy(tt.view(np.int64)).to("cuda:0")
    rc, cf, vts, st = eng.mvcc_validate_epoch(bb, tt, want_conflict=want_conflict, want_vts=want_vts)
    if dev:
        rc = rc.cpu().numpy()
        cf = cf.cpu().numpy().view(np.uint32) if cf is not None else None
        vts = vts.cpu().numpy().view(np.uint64) if vts is not None else None
    rc = np.asarray(rc)
    bad = np.nonzero(rc != erc)[0]
    assert bad.size == 0, f"rc mismatch at {bad[:10]} (gpu {rc[bad[:10]]} replay {erc[bad[:10]]})"
    if want_conflict:
        cf = np.asarray(cf)
        bad = np.nonzero(cf != ecf)[0]
        assert bad.size == 0, f"conflict mismatch at {bad[:10]} (gpu {cf[bad[:10]]} replay {ecf[bad[:10]]})"
    else:
        assert cf is None
    if want_vts:
        vts = np.asarray(vts)
        bad = np.nonzero(vts != evts)[0]
        assert bad.size == 0, f"vts mismatch at {bad[:10]} (gpu {vts[bad[:10]]} replay {evts[bad[:10]]})"
    else:
        assert vts is None and st["n_survivors"] == 0
    assert st["n_commit"] == int((erc == RC_RCOK).sum())
    assert st["n_abort"] == int((erc == RC_ABORT).sum())
    at = np.asarray(b.acctype)
    wr = at == WR
    assert st["nnz_w"] == int(wr.sum())
    wc = np.concatenate([[0], np.cumsum(wr)])
    off = np.asarray(b.offsets).astype(np.int64)
    assert st["n_readonly"] == int((wc[off[1:]] == wc[off[:-1]]).sum())
    if b.n_txn:
        n, m = b.n_txn, b.nnz
        assert st["alg_bytes"] == d.mvcc_alg_bytes(n, m, want_conflict, want_vts)
        assert d.mvcc_alg_bytes(n, m, True, True) == d.tso_alg_bytes(n, m, True) + 8 * m
    check_state(eng, b.keys, state)
    return rc, cf, vts, st


def fresh(eng):
    eng.mvcc_clear()
    assert eng.mvcc_rows_size == 0 and eng.mvcc_versions_size == 0
    return {}


def slow_path(info):
    assert info.get("late", 0) > 0, "no late read returned a non-latest version"
    assert info.get("base", 0) > 0, "no read returned the base row"


# ------------------------------------------------------------ known answers
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(engine, case, dev):
    _, txns, ts, rc, conflict, vts, rows, versions = case
    state = fresh(engine)
    b = make_batch(txns)
    grc, gcf, gv, _ = step(engine, state, b, np.asarray(ts, np.uint64), dev=dev)
    assert grc.tolist() == rc and gcf.tolist() == conflict and gv.tolist() == vts
    assert rows_of(state) == rows and versions_of(state) == versions
    vk, vt = engine.mvcc_versions()
    assert list(zip(vk.tolist(), vt.tolist())) == versions
    if rows:
        keys = np.asarray(sorted(rows), np.uint64)
        w, r = engine.mvcc_rows_get(keys)
        assert [(int(a), int(c)) for a, c in zip(w, r)] == [rows[int(k)] for k in keys]


def test_empty_epoch(engine):
    state = fresh(engine)
    rc, cf, vts, st = engine.mvcc_validate_epoch(make_batch([]), np.zeros(0, np.uint64))
    assert len(rc) == 0 and len(cf) == 0 and len(vts) == 0 and st["n_commit"] == 0
    _, _, _, st = step(engine, state, make_batch([[], [], []]), np.asarray([3, 2, 1], np.uint64))
    assert st["n_commit"] == 3 and st["rounds"] == 1


# ------------------------------------------------------------------ random
@pytest.mark.parametrize("n", [1, 5, 1001, 8192])
@pytest.mark.parametrize("family", TS_FAMILIES)
def test_random_ragged(engine, n, family):
    """Three chained epochs over 64 keys; the middle one as a device batch."""
    rng = np.random.default_rng(n + 13 * TS_FAMILIES.index(family))
    state = fresh(engine)
    info = {}
    commits = aborts = 0
    for e in range(3):
        types = (RD, WR) if e == 1 else (RD, WR, XP, SCAN)
        b = random_batch(rng, n, 8, 64, p_write=0.2 + 0.15 * e, types=types, unique=e != 2)
        ts = make_ts(rng, b.n_txn, family, base=epoch_base(family, e, n))
        rc, _, _, _ = step(engine, state, b, ts, dev=e == 1, info=info)
        commits += int((rc == RC_RCOK).sum())
        aborts += int((rc == RC_ABORT).sum())
    assert commits > 0
    if n >= 1001:
        assert aborts > 0, "the replay yields one outcome only"
        slow_path(info)


# ----------------------------------------------- one row across the tiles
@pytest.mark.parametrize("kind", ["wr", "rd_one_wr", "mixed"])
@pytest.mark.parametrize("m", [TS_T - 1, TS_T, TS_T + 1, TS_TILE - 1, TS_TILE, TS_TILE + 1, 2 * TS_TILE + 1])
def test_one_hot_row(engine, m, kind):
    """m one-access txns on one row, permuted ts: the row's segment crosses the
    tile seams of the decision scan and of the commit compaction, the late
    reads search a list as long as the segment, and ts == dw ties (a second
    epoch at the same timestamps) go to the search."""
    rng = np.random.default_rng(m)
    at = np.full(m, WR if kind == "wr" else RD, np.uint8)
    if kind == "mixed":
        at = rng.choice(np.asarray([RD, WR, XP, SCAN], np.uint8), size=m)
    b = d.EpochBatch(np.arange(m + 1, dtype=np.uint32), np.full(m, 77, np.uint64), at)
    ts = make_ts(rng, m, "permuted")
    if kind == "rd_one_wr":  # one early WR at the lowest ts: it commits, every RD behind it sees it
        at[0] = WR
        lo = int(np.argmin(ts))
        ts[0], ts[lo] = ts[lo], ts[0]
    state = fresh(engine)
    info = {}
    rc, cf, _, st = step(engine, state, b, ts, info=info)
    assert np.all(cf[rc == RC_ABORT] == 0)
    if kind != "rd_one_wr":
        assert 0 < int((rc == RC_RCOK).sum()) < m and versions_of(state)
    else:
        assert np.all(rc == RC_RCOK) and len(versions_of(state)) == 1 and st["n_survivors"] == 0
    # readers at the same timestamps: most lie at or below the row's latest
    # version, and one on every version's own ts (dw == ts, a tie)
    rd = d.EpochBatch(b.offsets, b.keys, np.full(m, RD, np.uint8))
    rc, _, vts, st = step(engine, state, rd, np.sort(ts), info=info)
    assert np.all(rc == RC_RCOK) and st["n_survivors"] > 0
    assert int((vts == np.sort(ts)).sum()) == len(set(v for _, v in versions_of(state)))


# -------------------------------------------------------------- merge seams
def writers(keys, base):
    """One WR txn per key, ts in index order from base."""
    keys = np.asarray(keys, np.uint64)
    b = d.EpochBatch(np.arange(keys.size + 1, dtype=np.uint32), keys, np.full(keys.size, WR, np.uint8))
    return b, np.uint64(base) + np.arange(keys.size, dtype=np.uint64)


def test_merge_seams(engine):
    state = fresh(engine)
    step(engine, state, *writers([100, 200, 300], 10))                # into an empty store
    before = engine.mvcc_versions()
    b0 = make_batch([[(100, RD)], [(200, WR)], [(150, RD)]])
    rc, _, _, _ = step(engine, state, b0, np.asarray([50, 5, 50], np.uint64))  # zero commits
    assert rc.tolist() == [RC_RCOK, RC_ABORT, RC_RCOK]
    after = engine.mvcc_versions()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    step(engine, state, *writers([1, 2, 3], 100))                     # all below the store's keys
    step(engine, state, *writers([1000, 2000, 1 << 40], 200))         # all above
    step(engine, state, *writers([50, 150, 250, 1500, (1 << 40) + 1], 300))  # strictly interleaved
    step(engine, state, *writers([100, 100, 1, 1 << 40], 400))        # behind the old versions of their keys
    assert len(versions_of(state)) == 18


@pytest.mark.parametrize("big_first", [True, False], ids=["store_big", "epoch_big"])
def test_merge_more_than_a_workgroup_with_one(engine, big_first):
    rng = np.random.default_rng(8)
    many = rng.permutation(np.arange(1, 5 * TS_TILE, dtype=np.uint64) * np.uint64(3))[:2 * TS_TILE + 7]
    state = fresh(engine)
    first, second = (many, [3 * TS_TILE]) if big_first else ([3 * TS_TILE], many)
    step(engine, state, *writers(first, 10))
    step(engine, state, *writers(second, 10 + len(first)))
    assert engine.mvcc_versions_size == many.size + 1


def test_keys_with_wide_bit_patterns(engine):
    """The sort packs the varying key bits: the epoch's versions must still come
    out in raw key order (the store, and the lookups' binary searches, rest on it)."""
    rng = np.random.default_rng(3)
    pool = np.asarray([1, 2, 1 << 20, (1 << 20) + 1, 1 << 33, (1 << 33) | 5, 1 << 62, (1 << 63) | 1,
                       (1 << 63) | (1 << 20), (1 << 64) - 2], np.uint64)
    state = fresh(engine)
    info = {}
    for e in range(2):
        n = 600
        b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), rng.choice(pool, size=n),
                         rng.choice(np.asarray([RD, WR], np.uint8), size=n))
        step(engine, state, b, make_ts(rng, n, "jitter", base=1000 + 300 * e), info=info)
    slow_path(info)


# --------------------------------------------------------------------- trim
def trim_both(eng, state, floor, touched):
    want = trim(state, floor)
    assert eng.mvcc_trim(floor) == want
    check_state(eng, touched, state)
    return want


def test_trim(engine):
    rng = np.random.default_rng(12)
    state = fresh(engine)
    assert engine.mvcc_trim(100) == 0  # an empty store
    n = 4 * TS_TILE + 5
    b = random_batch(rng, n, 3, 40, p_write=0.6, unique=False)
    ts = make_ts(rng, n, "index", base=1000)  # every txn commits
    step(engine, state, b, ts)
    total = len(versions_of(state))
    assert total > 2 * TS_TILE  # the trim's compaction crosses tile seams
    assert trim_both(engine, state, 1, b.keys) == 0                      # below every version
    mid = 1000 + n // 2
    dropped = trim_both(engine, state, mid, b.keys)                      # in the middle
    assert 0 < dropped < total
    assert trim_both(engine, state, mid, b.keys) == 0                    # idempotent
    # an epoch behind the trim: reads just above the floor land on the kept
    # newest-below-floor versions, writers go on
    info = {}
    b2 = random_batch(rng, 500, 3, 40, p_write=0.2, unique=False)
    step(engine, state, b2, make_ts(rng, 500, "permuted", base=mid), info=info)
    assert info["late"] > 0
    rows = [r for r in state.values() if r[1]]
    trim_both(engine, state, (1 << 64) - 2, np.concatenate([b.keys, b2.keys]))  # above every version
    assert engine.mvcc_versions_size == len(rows) and all(len(r[1]) == 1 for r in rows)
    step(engine, state, b2, make_ts(rng, 500, "jitter", base=mid + 600))  # the context still works


# --------------------------------------------------------------- rejections
def test_rejected_calls_leave_rows_and_versions(engine):
    state = fresh(engine)
    good = make_batch([[(1, WR)], [(2, WR), (3, RD)], [(1, RD)]])
    ts = np.asarray([10, 11, 5], np.uint64)
    step(engine, state, good, ts)
    keys = np.asarray([1, 2, 3, 4, 100], np.uint64)
    rows0, ver0, size0 = engine.mvcc_rows_get(keys), engine.mvcc_versions(), engine.mvcc_rows_size
    off = good.offsets.copy()
    off[1] = 4  # [0, 4, 3, 4]: decreases
    rk = good.keys.copy()
    rk[1] = d.KEY_RESERVED
    long = make_batch([[(1, RD)], [(100 + q, WR) for q in range(65)]])
    bad = [(good, np.asarray([10, 0, 12], np.uint64)),
           (good, np.asarray([10, (1 << 64) - 1, 12], np.uint64)),
           (d.EpochBatch(good.offsets, rk, good.acctype), ts),
           (d.EpochBatch(off, good.keys, good.acctype), ts),
           (long, np.asarray([20, 21], np.uint64)),
           (good, None)]
    for dev in (False, True):
        for bb, tt in bad:
            if dev and tt is None:
                continue
            if dev:
                import torch
                bb = bb.to_torch("cuda:0")
                tt = torch.from_numpy(tt.view(np.int64)).to("cuda:0")
            with pytest.raises(d.DccError) as e:
                engine.mvcc_validate_epoch(bb, tt)
            assert e.value.code == _abi.DCC_EINVAL
            rows1, ver1 = engine.mvcc_rows_get(keys), engine.mvcc_versions()
            assert engine.mvcc_rows_size == size0
            assert all(np.array_equal(x, y) for x, y in zip(rows0 + ver0, rows1 + ver1))
    step(engine, state, good, ts + np.uint64(10))  # the context still works


# -------------------------------------------------------------------- other
@functools.lru_cache(maxsize=None)
def ycsb(n_txn=8192, theta=0.9):
    b = d.gen_ycsb(n_txn=n_txn, zipf_theta=theta)
    rng = np.random.default_rng(n_txn)
    ts = np.uint64(1000) + np.arange(n_txn, dtype=np.uint64) + rng.integers(0, 65, size=n_txn).astype(np.uint64)
    return b, ts


def test_ycsb_8192_jitter_forms(engine):
    """8,192 x 16 at theta 0.9 with jitter: host, device and compact batches,
    each on a cleared engine, then once more on the state the last one left."""
    b, ts = ycsb()
    c = engine.compact_host_batch(b)
    for kw in ({}, {"dev": True}, {"run_batch": c}):
        state = fresh(engine)
        info = {}
        rc, cf, _, st = step(engine, state, b, ts, info=info, **kw)
        assert 0 < int((rc == RC_RCOK).sum()) < b.n_txn and st["rounds"] > 1
        assert int(((rc == RC_ABORT) & (cf > 0)).sum()) > 0  # not every abort is at access 0
        slow_path(info)
    step(engine, state, b, ts + np.uint64(4000), info=info)


def test_without_vts_and_without_conflict(engine):
    b, ts = ycsb()
    for dev in (False, True):
        state = fresh(engine)
        step(engine, state, b, ts, dev=dev, want_vts=False)
        step(engine, state, b, ts + np.uint64(3000), dev=dev, want_conflict=False)
        step(engine, state, b, ts + np.uint64(6000), dev=dev, want_conflict=False, want_vts=False)


def test_clear(engine):
    state = fresh(engine)
    b, ts = writers([5, 6, 7], 10)
    step(engine, state, b, ts)
    assert engine.mvcc_rows_size == 3 and engine.mvcc_versions_size == 3
    state = fresh(engine)
    w, r = engine.mvcc_rows_get(np.asarray([5, 6], np.uint64))
    assert w.tolist() == [0, 0] and r.tolist() == [0, 0]
    rc, _, vts, _ = step(engine, state, make_batch([[(5, WR)]]), np.asarray([3], np.uint64))  # 3 < the old rts 10
    assert rc.tolist() == [RC_RCOK] and vts.tolist() == [VTS_BASE]


def test_reserve_and_repeat(engine):
    b, ts = ycsb()
    engine.reserve(b.n_txn, b.nnz)
    r1 = step(engine, fresh(engine), b, ts)
    r2 = step(engine, fresh(engine), b, ts)
    assert all(np.array_equal(x, y) for x, y in zip(r1[:3], r2[:3]))


def test_multi_context_runs_on_rank0():
    b, ts = ycsb()
    with d.Engine(devices=[0, 0]) as m:
        state = {}
        step(m, state, b, ts)
        step(m, state, b, ts + np.uint64(2000), dev=True)
        assert m.mvcc_rows_size == np.unique(b.keys).size
        assert m.mvcc_trim(3000) == trim(state, 3000)
        check_state(m, b.keys, state)


def test_two_rank_communicator_not_supported():
    b, ts = ycsb()
    with d.Engine(0) as eng:
        eng.comm_init_host(0, 2, lambda buf: None)
        with pytest.raises(d.DccError) as e:
            eng.mvcc_validate_epoch(b, ts)
        assert e.value.code == _abi.DCC_ENOTSUP
        eng.comm_destroy()
        step(eng, {}, b, ts)


def test_table_growth_keeps_values():
    """A fresh context's row table starts small: an epoch over many new rows
    makes it grow by rehash, with the rows decided before in place."""
    with d.Engine(0) as eng:
        state = {}
        b0, ts0 = writers(np.arange(1, 1500), 10)
        step(eng, state, b0, ts0)
        b = d.gen_ycsb(n_txn=8192, zipf_theta=0.0, table_size=1 << 22, seed=5)  # ~131,000 new rows
        step(eng, state, b, make_ts(np.random.default_rng(2), b.n_txn, "jitter", base=3000))
        assert eng.mvcc_rows_size > 100000
        check_state(eng, np.arange(0, 1600, dtype=np.uint64), state)


# ------------------------------------------------- against the TIMESTAMP engine
@pytest.mark.parametrize("one_access", [True, False], ids=["one_access", "ragged"])
def test_aborts_against_timestamp(engine, one_access):
    """Same batch and ts on fresh state through both engines, and through both
    references (mvcc_ref.against_timestamp has the rule and where it holds)."""
    rng = np.random.default_rng(41)
    n = 3000
    if one_access:
        b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), rng.integers(0, 20, size=n).astype(np.uint64),
                         rng.choice(np.asarray([RD, WR, XP, SCAN], np.uint8), size=n, p=[.4, .4, .1, .1]))
    else:
        b = random_batch(rng, n, 6, 200, p_write=0.4, types=(RD, WR, XP, SCAN), unique=False)
    ts = make_ts(rng, b.n_txn, "jitter")
    mrc, mcf, _, _ = step(engine, fresh(engine), b, ts)
    engine.tso_rows_clear()
    trc, tcf, _ = engine.tso_validate_epoch(b, ts)
    rr = tso_ref.replay(b, ts, {})
    assert np.array_equal(trc, rr[0]) and np.array_equal(tcf, rr[1])
    mr = replay(b, ts, {})
    applied = against_timestamp(b, mrc, mcf, trc, tcf, every=one_access)
    assert applied == against_timestamp(b, mr[0], mr[1], rr[0], rr[1], every=one_access)
    assert applied > 0
