"""GPU parity of the TIMESTAMP epoch (dcc_tso_validate_epoch, tso.hip) against
the replays of Row_ts (tso_ref.py): RC, the access each aborted txn aborted at,
the counts and, after every call, the (wts, rts) of every touched row,
bit-exact."""
import functools
import os
import re

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RD, SCAN, WR, XP, _abi
from helpers import chain_batch, make_batch, random_batch
from tso_cases import KATS, TS_FAMILIES, make_ts, seed_rows
from tso_ref import live, replay, replay_literal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constant(name):
    src = open(os.path.join(ROOT, "deneva_amd", "csrc", "tso.hip")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


TS_T = kernel_constant("TS_T")          # threads per workgroup
TS_ITEMS = kernel_constant("TS_ITEMS")  # sorted accesses per thread
TS_TILE = TS_T * TS_ITEMS               # accesses per scan tile


def set_rows(eng, rows):
    eng.tso_rows_clear()
    if rows:
        k = np.fromiter(rows.keys(), np.uint64, len(rows))
        eng.tso_rows_set(k, np.asarray([rows[int(x)][0] for x in k], np.uint64),
                         np.asarray([rows[int(x)][1] for x in k], np.uint64))


def check_rows(eng, keys, rows):
    """rows_get of every key of `keys` equals the replay's state."""
    k = np.unique(np.asarray(keys, np.uint64))
    w, r = eng.tso_rows_get(k)
    ew = np.asarray([rows.get(int(x), (0, 0))[0] for x in k], np.uint64)
    er = np.asarray([rows.get(int(x), (0, 0))[1] for x in k], np.uint64)
    bad = np.nonzero((w != ew) | (r != er))[0]
    assert bad.size == 0, (f"row state differs at keys {k[bad[:5]]}: gpu {list(zip(w[bad[:5]], r[bad[:5]]))} "
                           f"replay {list(zip(ew[bad[:5]], er[bad[:5]]))}")


def run(eng, b, ts, ref, dev=False, run_batch=None, want_conflict=True):
    """One call on the table as it stands; compares with ref = (rc, conflict,
    rows after).  Returns (rc, conflict, stats)."""
    erc, ecf, rows = ref
    bb = run_batch if run_batch is not None else b
    tt = np.ascontiguousarray(ts, np.uint64)
    if dev:
        import torch
        bb = bb.to_torch("cuda:0")
        tt = torch.from_numpy(tt.view(np.int64)).to("cuda:0")
    rc, cf, st = eng.tso_validate_epoch(bb, tt, want_conflict=want_conflict)
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
    wr = at == WR
    assert st["nnz_w"] == int(wr.sum())
    wc = np.concatenate([[0], np.cumsum(wr)])
    off = np.asarray(b.offsets).astype(np.int64)
    assert st["n_readonly"] == int((wc[off[1:]] == wc[off[:-1]]).sum())
    if b.n_txn:
        assert st["alg_bytes"] == d.tso_alg_bytes(b.n_txn, b.nnz, want_conflict)
        n, m = b.n_txn, b.nnz
        assert d.tso_alg_bytes(n, m, True) == 4 * (n + 1) + 8 * n + 9 * m + 24 * m + n + 4 * n
    check_rows(eng, b.keys, rows)
    return rc, cf, st


def reference(b, ts, seed=None):
    rows = dict(seed or {})
    rc, cf = replay(b, ts, rows)
    return rc, cf, rows


def check(eng, b, ts, seed=None, ref=None, **kw):
    """A call on a table holding exactly `seed`."""
    ref = ref if ref is not None else reference(b, ts, seed)
    set_rows(eng, seed)
    return run(eng, b, ts, ref, **kw)


def both_outcomes(ref):
    erc = ref[0]
    assert 0 < int((erc == RC_RCOK).sum()) < erc.size, "the replay yields one outcome only"


@functools.lru_cache(maxsize=None)
def ycsb(n_txn, theta, family, jitter=64):
    b = d.gen_ycsb(n_txn=n_txn, zipf_theta=theta)
    rng = np.random.default_rng(n_txn + jitter)
    if family == "jitter":
        ts = np.uint64(1000) + np.arange(n_txn, dtype=np.uint64) + \
            rng.integers(0, jitter + 1, size=n_txn).astype(np.uint64)
    else:
        ts = make_ts(rng, n_txn, family)
    return b, ts, reference(b, ts)


# ------------------------------------------------------------ known answers
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(engine, case, dev):
    _, txns, ts, seed, rc, conflict, rows = case
    b = make_batch(txns)
    ts = np.asarray(ts, np.uint64)
    ref = reference(b, ts, seed)
    assert ref[0].tolist() == rc and ref[1].tolist() == conflict and live(ref[2]) == live(rows)
    grc, gcf, _ = check(engine, b, ts, seed, ref=ref, dev=dev)
    assert grc.tolist() == rc and gcf.tolist() == conflict
    keys = np.asarray(sorted(rows), np.uint64)
    w, r = engine.tso_rows_get(keys)
    assert [(int(a), int(c)) for a, c in zip(w, r)] == [rows[int(k)] for k in keys]


def test_empty_zero_length_and_xp_only(engine):
    engine.tso_rows_clear()
    rc, cf, st = engine.tso_validate_epoch(make_batch([]), np.zeros(0, np.uint64))
    assert len(rc) == 0 and len(cf) == 0 and st["n_commit"] == 0 and st["n_abort"] == 0
    ts6 = np.asarray([5, 4, 3, 2, 1, 0], np.uint64)
    ref = reference(make_batch([[], [(1, WR)], [], [(1, RD)], [], []]), ts6)
    assert ref[0].tolist() == [RC_RCOK, RC_RCOK, RC_RCOK, RC_ABORT, RC_RCOK, RC_RCOK]
    check(engine, make_batch([[], [(1, WR)], [], [(1, RD)], [], []]), ts6, ref=ref)
    _, _, st = check(engine, make_batch([[], [], []]), ts6[:3])
    assert st["n_commit"] == 3 and st["rounds"] == 1
    # XP alone makes no request: every txn commits against any row state
    seed = {1: (50, 60), 2: (70, 0)}
    xb = make_batch([[(1, XP)], [(2, XP), (1, XP), (3, XP)], [(2, XP)]])
    rc, _, st = check(engine, xb, np.asarray([3, 2, 1], np.uint64), seed)
    assert np.all(rc == RC_RCOK) and st["rounds"] == 1 and st["nnz_w"] == 0
    w, r = engine.tso_rows_get(np.asarray([1, 2, 3], np.uint64))
    assert w.tolist() == [50, 70, 0] and r.tolist() == [60, 0, 0]


# ------------------------------------------------------------------ random
@pytest.mark.parametrize("n", [1, 5, 1001, 8192])
def test_random_ragged(engine, n):
    rng = np.random.default_rng(n)
    commits = aborts = 0
    for it, family in enumerate(TS_FAMILIES):
        nk = max(2, n // 3)
        types = (RD, WR) if it % 2 else (RD, WR, XP, SCAN)
        b = random_batch(rng, n, 8, nk, p_write=0.3 + 0.1 * it, types=types, unique=bool(it % 2))
        ts = make_ts(rng, b.n_txn, family)
        seed = seed_rows(rng, nk, ts) if it in (1, 2) else {}
        ref = reference(b, ts, seed)
        if n <= 1001:  # the literal Row_ts::access with its queues agrees
            lrows = dict(seed)
            lrc, lcf = replay_literal(b, ts, lrows)
            assert np.array_equal(lrc, ref[0]) and np.array_equal(lcf, ref[1]) and live(lrows) == live(ref[2])
        check(engine, b, ts, seed, ref=ref, dev=it == 3)
        commits += int((ref[0] == RC_RCOK).sum())
        aborts += int((ref[0] == RC_ABORT).sum())
    assert commits > 0
    if n >= 5:
        assert aborts > 0, "the replay yields one outcome only"


def test_lengths_at_the_limit(engine):
    rng = np.random.default_rng(5)
    n = 300
    keys = rng.integers(0, 40000, size=(n, 64))
    at = np.where(rng.random((n, 64)) < 0.1, WR, RD)
    b = make_batch([list(zip(keys[i].tolist(), at[i].tolist())) for i in range(n)])
    assert np.all(np.diff(b.offsets) == 64)
    ts = make_ts(rng, n, "permuted")
    ref = reference(b, ts)
    both_outcomes(ref)
    assert int(((ref[0] == RC_ABORT) & (ref[1] > 32)).sum()) > 0  # aborts in the upper lanes too
    check(engine, b, ts, ref=ref)
    # one txn of 65 accesses: rejected, the table as it was
    rows = ref[2]
    long = make_batch([[(1, RD)], [(100 + q, WR) for q in range(65)], [(2, WR)]])
    for bb, tt in ((long, np.asarray([9, 8, 7], np.uint64)), (long.to_torch("cuda:0"), None)):
        if tt is None:
            import torch
            tt = torch.tensor([9, 8, 7], dtype=torch.int64, device="cuda:0")
        size = engine.tso_rows_size
        with pytest.raises(d.DccError) as e:
            engine.tso_validate_epoch(bb, tt)
        assert e.value.code == _abi.DCC_EINVAL
        assert engine.tso_rows_size == size
        check_rows(engine, np.concatenate([b.keys, long.keys]), rows)


# ----------------------------------------------- segments across many tiles
@pytest.mark.parametrize("kind", ["wr", "rd_one_wr", "mixed"])
def test_one_hot_row(engine, kind):
    """20,000 one-access txns on one row, permuted ts: the row's segment spans
    ten 2,048-pair sort tiles and twenty scan tiles."""
    n = 20000
    rng = np.random.default_rng(17)
    at = np.full(n, WR if kind == "wr" else RD, np.uint8)
    if kind == "rd_one_wr":
        at[10000] = WR
    if kind == "mixed":
        at = rng.choice(np.asarray([RD, WR, XP, SCAN], np.uint8), size=n)
    b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, 77, np.uint64), at)
    ts = make_ts(rng, n, "permuted")
    ref = reference(b, ts)
    both_outcomes(ref)
    rc, cf, st = check(engine, b, ts, ref=ref)
    assert st["rounds"] > 1
    assert np.all(cf[rc == RC_ABORT] == 0)


@pytest.mark.parametrize("m", sorted({TS_T - 1, TS_T, TS_T + 1, TS_TILE - 1, TS_TILE, TS_TILE + 1,
                                      2 * TS_TILE - 1, 2 * TS_TILE, 2 * TS_TILE + 1,
                                      TS_TILE * TS_TILE // 256 + 1}))
def test_scan_tile_and_workgroup_sizes(engine, m):
    """m accesses in all (one per txn), at the workgroup size TS_T and the scan
    tile TS_TILE +- 1, two tiles +- 1 and past 4 tiles: three hot rows whose
    segments start and end at every offset against the tile seams."""
    rng = np.random.default_rng(m)
    keys = rng.choice(np.asarray([3, 9, 1 << 40], np.uint64), size=m, p=[0.5, 0.3, 0.2])
    at = rng.choice(np.asarray([RD, WR, SCAN], np.uint8), size=m, p=[0.5, 0.4, 0.1])
    b = d.EpochBatch(np.arange(m + 1, dtype=np.uint32), keys, at)
    ts = make_ts(rng, m, "jitter")
    ref = reference(b, ts)
    both_outcomes(ref)
    check(engine, b, ts, ref=ref)
    # and n_txn at the same sizes with two accesses each (two lanes per txn)
    b2 = d.EpochBatch(np.arange(0, 2 * m + 1, 2, dtype=np.uint32),
                      np.stack([keys, np.arange(m, dtype=np.uint64) + np.uint64(100)], 1).reshape(-1),
                      np.stack([at, np.full(m, WR, np.uint8)], 1).reshape(-1))
    check(engine, b2, ts)


def test_chain_of_300_rounds(engine):
    """Txn i reads key i-1 and writes key i with decreasing ts: txn i commits
    iff txn i-1 aborted, which takes a round per txn."""
    n = 300
    b = chain_batch(n)
    ts = np.arange(n, 0, -1).astype(np.uint64) + np.uint64(100)
    ref = reference(b, ts)
    assert ref[0].tolist() == [RC_RCOK if i % 2 == 0 else RC_ABORT for i in range(n)]
    _, _, st = check(engine, b, ts, ref=ref)
    assert n - 1 <= st["rounds"] <= n + 1


def test_index_order_one_round(engine):
    b, _, _ = ycsb(8192, 0.9, "jitter")
    ts = make_ts(None, b.n_txn, "index")
    ref = reference(b, ts)
    assert np.all(ref[0] == RC_RCOK)
    _, _, st = check(engine, b, ts, ref=ref)
    assert st["n_abort"] == 0 and st["rounds"] == 1


def test_ycsb_8192_jitter(engine):
    b, ts, ref = ycsb(8192, 0.9, "jitter")
    both_outcomes(ref)
    assert int(((ref[0] == RC_ABORT) & (ref[1] > 0)).sum()) > 0  # not every abort is at access 0
    _, _, st = check(engine, b, ts, ref=ref)
    assert st["rounds"] > 1


def test_ycsb_c2_forms(engine):
    """65,536 x 16 at theta 0.9: host, device and compact batches."""
    b, ts, ref = ycsb(65536, 0.9, "jitter")
    both_outcomes(ref)
    check(engine, b, ts, ref=ref)
    check(engine, b, ts, ref=ref, dev=True)
    c = engine.compact_host_batch(b)
    assert c.keys.dtype == np.uint32 and c.meta.get("acctype_2bit")
    check(engine, b, ts, ref=ref, run_batch=c)


def test_tpcc(engine):
    b = d.gen_tpcc(n_txn=2048, num_wh=4)
    ts = make_ts(np.random.default_rng(4), b.n_txn, "jitter")
    ref = reference(b, ts)
    both_outcomes(ref)
    check(engine, b, ts, ref=ref)


# ------------------------------------------------------------- the row table
def test_four_chained_epochs(engine):
    """ts continue across the epochs; the table carries wts / rts, nothing is
    set in between."""
    engine.tso_rows_clear()
    rows = {}
    named = set()
    base = 1000
    rng = np.random.default_rng(21)
    for e in range(4):
        b = d.gen_ycsb(n_txn=4096, zipf_theta=0.8, table_size=1 << 14, seed=70 + e)
        named.update(b.keys.tolist())
        ts = make_ts(rng, b.n_txn, "jitter", base=base)
        base += b.n_txn
        rc, cf = replay(b, ts, rows)
        both_outcomes((rc,))
        run(engine, b, ts, (rc, cf, rows), dev=e == 2)
    # every row an accepted batch names is in the table, reached or not
    assert len(rows) < len(named) and engine.tso_rows_size == len(named)


def test_rows_set_get_clear(engine):
    engine.tso_rows_clear()
    assert engine.tso_rows_size == 0
    w, r = engine.tso_rows_get(np.asarray([1, 2, 1 << 63], np.uint64))
    assert w.tolist() == [0, 0, 0] and r.tolist() == [0, 0, 0]
    big = (1 << 64) - 2
    engine.tso_rows_set(np.asarray([5, 6, big], np.uint64), np.asarray([50, 0, big], np.uint64),
                        np.asarray([7, 60, 1], np.uint64))
    assert engine.tso_rows_size == 3
    engine.tso_rows_set(np.asarray([6], np.uint64), np.asarray([61], np.uint64), np.asarray([62], np.uint64))
    assert engine.tso_rows_size == 3  # overwritten, not added
    w, r = engine.tso_rows_get(np.asarray([big, 4, 6, 5], np.uint64))
    assert w.tolist() == [big, 0, 61, 50] and r.tolist() == [1, 0, 62, 7]
    # the seeds decide: ts 55 reads row 5 (wts 50), may not write row 6 (rts 62)
    b = make_batch([[(5, RD)], [(6, WR)], [(5, WR)]])
    rc, cf, _ = check(engine, b, np.asarray([55, 55, 49], np.uint64), {5: (50, 7), 6: (61, 62)})
    assert rc.tolist() == [RC_RCOK, RC_ABORT, RC_ABORT] and cf.tolist() == [ACCESS_NONE, 0, 0]
    with pytest.raises(d.DccError) as e:
        engine.tso_rows_set(np.asarray([9, d.KEY_RESERVED], np.uint64), np.zeros(2, np.uint64),
                            np.zeros(2, np.uint64))
    assert e.value.code == _abi.DCC_EINVAL
    engine.tso_rows_clear()
    assert engine.tso_rows_size == 0
    w, r = engine.tso_rows_get(np.asarray([5, 6], np.uint64))
    assert w.tolist() == [0, 0] and r.tolist() == [0, 0]


def test_table_growth_keeps_values():
    """A fresh context's table starts small: an epoch over many new rows makes
    it grow by rehash, with the rows seeded and decided before in place."""
    with d.Engine(0) as eng:
        rows = {int(k): (int(k) + 5, int(k) + 9) for k in range(1, 1500)}
        set_rows(eng, rows)
        b0 = make_batch([[(3, WR), (7, RD)], [(1400, RD)]])
        ts0 = np.asarray([5000, 1402], np.uint64)
        rc, cf = replay(b0, ts0, rows)
        assert rc.tolist() == [RC_RCOK, RC_ABORT]
        run(eng, b0, ts0, (rc, cf, rows))
        before = eng.tso_rows_size
        rng = np.random.default_rng(2)
        b = d.gen_ycsb(n_txn=8192, zipf_theta=0.0, table_size=1 << 22, seed=5)  # ~131,000 new rows
        ts = make_ts(rng, b.n_txn, "jitter", base=3000)
        rc, cf = replay(b, ts, rows)
        both_outcomes((rc,))
        run(eng, b, ts, (rc, cf, rows))
        assert eng.tso_rows_size > before + 100000
        check_rows(eng, np.arange(0, 1600, dtype=np.uint64), rows)


def test_rejected_calls_leave_the_table(engine):
    good = make_batch([[(1, RD)], [(2, WR), (3, RD)]])
    ts = np.asarray([10, 11], np.uint64)
    seed = {1: (4, 5), 2: (6, 7), 40: (8, 9)}
    check(engine, good, ts, seed)
    rows = reference(good, ts, seed)[2]
    size = engine.tso_rows_size
    off = good.offsets.copy()
    off[1] = 4  # [0, 4, 3]: decreases
    keys = good.keys.copy()
    keys[1] = d.KEY_RESERVED
    bad = [(d.EpochBatch(off, good.keys, good.acctype), ts),
           (d.EpochBatch(good.offsets, keys, good.acctype), ts),
           (good, None)]
    for bb, tt in bad:
        with pytest.raises(d.DccError) as e:
            engine.tso_validate_epoch(bb, tt)
        assert e.value.code == _abi.DCC_EINVAL
        assert engine.tso_rows_size == size
        check_rows(engine, [1, 2, 3, 40, 4], rows)
    run(engine, good, ts + np.uint64(10), reference(good, ts + np.uint64(10), rows))  # the context still works


def test_without_conflict_output(engine):
    b, ts, ref = ycsb(8192, 0.9, "jitter")
    check(engine, b, ts, ref=ref, want_conflict=False)
    check(engine, b, ts, ref=ref, want_conflict=False, dev=True)


def test_multi_context_runs_on_rank0():
    b, ts, ref = ycsb(8192, 0.9, "jitter")
    with d.Engine(devices=[0, 0]) as m:
        check(m, b, ts, ref=ref)
        check(m, b, ts, ref=ref, dev=True)
        assert m.tso_rows_size == np.unique(b.keys).size


def test_two_rank_communicator_not_supported():
    b, ts, ref = ycsb(8192, 0.9, "jitter")
    with d.Engine(0) as eng:
        eng.comm_init_host(0, 2, lambda buf: None)
        with pytest.raises(d.DccError) as e:
            eng.tso_validate_epoch(b, ts)
        assert e.value.code == _abi.DCC_ENOTSUP
        eng.comm_destroy()
        check(eng, b, ts, ref=ref)


def test_reserve_and_repeat(engine):
    """After reserve, repeated calls on the same seed give the same outputs;
    a call on the table the first one left sees its wts / rts."""
    b, ts, ref = ycsb(8192, 0.9, "permuted")
    both_outcomes(ref)
    engine.reserve(b.n_txn, b.nnz)
    r1 = check(engine, b, ts, ref=ref)
    r2 = check(engine, b, ts, ref=ref)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    again = reference(b, ts, ref[2])
    assert int((again[0] == RC_ABORT).sum()) > int((ref[0] == RC_ABORT).sum())
    run(engine, b, ts, again)
