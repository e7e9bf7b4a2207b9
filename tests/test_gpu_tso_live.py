"""GPU parity of TIMESTAMP with txns in flight (dcc_tso_access_epoch,
dcc_tso_finish, tso_live.hip) against the closed-form replay (tso_live_ref.py,
which test_tso_live_ref.py holds against the literal Row_ts): rc, pos, the
conflict ordinals, the counts and the rows' (wts, rts) after every call,
bit-exact."""
import functools
import os
import re

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RC_WAIT, RD, SCAN, WD_GONE, WD_RUN, WR, XP, _abi
from helpers import make_batch
import tso_live_ref as ref
from tso_live_cases import KATS, admit, history, hot_batch, make_ts, new_state, seed_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constant(name, file):
    src = open(os.path.join(ROOT, "deneva_amd", "csrc", file)).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


TILE = kernel_constant("TS_T", "tso_live.hip") * kernel_constant("TS_ITEMS", "tso_live.hip")  # accesses per scan tile
RING = kernel_constant("SEG_RING", "seg_rounds.h")  # undecided-count ring


@pytest.fixture(autouse=True)
def clean_rows(request):
    if "engine" in request.fixturenames:
        request.getfixturevalue("engine").tso_rows_clear()
    yield


def differ(what, got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what} differs at {bad[:10]} (gpu {got[bad[:10]]} replay {exp[bad[:10]]})"


def to_dev(a, dt):
    import torch
    view = {np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}[dt]
    return torch.from_numpy(np.ascontiguousarray(a, dt).view(view).copy()).to("cuda:0")


def from_dev(t, dt):
    return t.cpu().numpy().view(dt)


def engine_rows(eng, keys):
    keys = np.unique(np.asarray(keys, np.uint64))
    if not keys.size:
        return {}
    w, r = eng.tso_rows_get(keys)
    return {int(k): (int(a), int(b)) for k, a, b in zip(keys, w, r) if (a, b) != (0, 0)}


def set_rows(eng, rows):
    eng.tso_rows_clear()
    if rows:
        k = np.asarray(list(rows), np.uint64)
        eng.tso_rows_set(k, np.asarray([rows[int(x)][0] for x in k], np.uint64),
                         np.asarray([rows[int(x)][1] for x in k], np.uint64))


class Run:
    """The engine next to the closed form over one batch: every call is made on
    both and everything they leave is compared."""

    def __init__(self, eng, b, ts, run_batch=None, rows=None):
        set_rows(eng, rows)
        self.eng, self.b, self.ts = eng, b, np.asarray(ts, np.uint64)
        self.run_batch = run_batch if run_batch is not None else b
        self.state = {int(k): list(v) for k, v in (rows or {}).items()}
        self.seeded = [int(k) for k in (rows or {})]

    def same_rows(self, exp=None):
        keys = np.concatenate([np.asarray(self.b.keys, np.uint64), np.asarray(self.seeded, np.uint64)])
        assert engine_rows(self.eng, keys) == (exp if exp is not None else ref.rows_of(self.state))

    def call(self, dev, rc, pos, leave, fn):
        """fn(batch, ts, rc, pos[, leave]) on host arrays or device tensors;
        returns rc, pos as numpy and what fn returned."""
        if dev:
            args = [to_dev(self.ts, np.uint64), to_dev(rc, np.uint8), to_dev(pos, np.uint32)]
            if leave is not None:
                args.append(to_dev(leave, np.uint8))
            out = fn(self.run_batch.to_torch("cuda:0"), *args)
            return from_dev(args[1], np.uint8), from_dev(args[2], np.uint32), out
        r, p = np.array(rc, np.uint8), np.array(pos, np.uint32)
        args = [self.ts, r, p] + ([np.asarray(leave, np.uint8)] if leave is not None else [])
        return r, p, fn(self.run_batch, *args)

    def epoch(self, rc, pos, dev=False, exp=None, want_conflict=True):
        """exp: (replay's result, rows) computed before."""
        if exp is None:
            exp = (ref.epoch(self.b, self.ts, rc, pos, self.state), ref.rows_of(self.state))
        e = exp[0]
        r, p, out = self.call(dev, rc, pos, None, lambda b, t, r, p: self.eng.tso_access_epoch(b, t, r, p, want_conflict))
        cf, st = out[2], out[3]
        if cf is not None and dev:
            cf = from_dev(cf, np.uint32)
        differ("rc", r, e[0])
        differ("pos", p, e[1])
        if want_conflict:
            differ("conflict", cf, e[2])
        else:
            assert cf is None
        for k in ("n_commit", "n_abort", "n_survivors", "nnz_w", "n_readonly"):
            assert st[k] == e[3][k], (k, st[k], e[3][k])
        self.same_rows(exp[1])
        n, m = self.b.n_txn, self.b.nnz
        if n:
            assert st["alg_bytes"] == d.tso_access_alg_bytes(n, m, want_conflict) == d.waitdie_alg_bytes(n, m, want_conflict)
        return r, p, cf, st

    def finish(self, rc, pos, leave, dev=False, exp=None):
        if exp is None:
            exp = (ref.finish(self.b, self.ts, rc, pos, leave, self.state), ref.rows_of(self.state))
        e = exp[0]
        r, p, out = self.call(dev, rc, pos, leave, lambda b, t, r, p, lv: self.eng.tso_finish(b, t, r, p, lv))
        left, prom, st = out
        differ("rc", r, e[0])
        differ("pos", p, e[1])
        assert (left, prom) == (e[2], e[3])
        assert st["n_commit"] == e[2] and st["n_survivors"] == e[3]
        self.same_rows(exp[1])
        return r, p, left, prom


def leave_of(rc, states):
    return np.isin(rc, states).astype(np.uint8)


def outcomes(st):
    return st["n_commit"], st["n_abort"], st["n_survivors"]


# ------------------------------------------------------------ the hand cases
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_hand_cases(engine, case, dev):
    _, txns, ts, rc0, steps = case
    seed = steps[0][1] if steps[0][0] == "seed" else None
    run = Run(engine, make_batch(txns), ts, rows=seed)
    rc, pos = np.asarray(rc0, np.uint8), np.zeros(len(txns), np.uint32)
    for s in steps:
        if s[0] == "seed":
            continue
        if s[0] == "admit":
            admit(rc, pos, s[1])
        elif s[0] == "epoch":
            rc, pos, cf, _ = run.epoch(rc, pos, dev=dev)
            assert (rc.tolist(), pos.tolist(), cf.tolist()) == (s[1], s[2], s[3])
            run.same_rows(s[4])
        else:
            leave = np.zeros(len(txns), np.uint8)
            leave[s[1]] = 1
            rc, pos, left, prom = run.finish(rc, pos, leave, dev=dev)
            assert (rc.tolist(), pos.tolist(), left, prom) == (s[2], s[3], len(s[1]), s[4])
            run.same_rows(s[5])


# ---------------------------------------------------------------- the edges
def test_empty_zero_length_gone_and_run_at_len(engine):
    e = make_batch([])
    z = np.zeros(0, np.uint64)
    rc, pos, cf, st = engine.tso_access_epoch(e, z, np.zeros(0, np.uint8), np.zeros(0, np.uint32))
    assert len(rc) == 0 and len(pos) == 0 and len(cf) == 0 and st["n_commit"] == 0
    assert engine.tso_finish(e, z, np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint8))[:2] == (0, 0)
    # zero-length txns: a RUN one turns RCOK at pos 0 == len
    b = make_batch([[], [(1, WR)], [], [(1, RD)], []])
    ts = np.asarray([5, 1, 3, 2, 4], np.uint64)
    run = Run(engine, b, ts)
    r, p, cf, st = run.epoch(*new_state(5))
    assert r.tolist() == [RC_RCOK, RC_RCOK, RC_RCOK, RC_WAIT, RC_RCOK] and st["rounds"] >= 1
    z3 = make_batch([[], [], []])
    run = Run(engine, z3, ts[:3])
    _, _, _, st = run.epoch(*new_state(3), dev=True)
    assert st["n_commit"] == 3 and st["rounds"] == 1 and st["n_readonly"] == 3
    run.finish(*new_state(3), np.asarray([1, 0, 1], np.uint8))
    # all GONE: nothing runs, whatever pos and ts hold
    run = Run(engine, b, np.asarray([0, 1, (1 << 64) - 1, 2, 0], np.uint64))
    rc, pos = new_state(5, WD_GONE)
    pos[:] = [7, 0, 99, 1, 2]
    for dev in (False, True):
        r, p, cf, st = run.epoch(rc, pos, dev=dev)
        assert np.all(r == WD_GONE) and p.tolist() == pos.tolist() and np.all(cf == ACCESS_NONE)
        assert outcomes(st) == (0, 0, 0) and st["rounds"] == 1
        assert run.finish(rc, pos, np.ones(5, np.uint8), dev=dev)[2:] == (0, 0)
    # RUN at pos == len (a promoted read at its last access), next to every other state
    b = make_batch([[(1, WR)], [(1, WR), (2, RD)], [], [(2, WR)], [(9, RD)]])
    ts = np.asarray([5, 4, 3, 2, 1], np.uint64)
    rc = np.asarray([WD_RUN, RC_ABORT, WD_RUN, WD_GONE, RC_RCOK], np.uint8)
    pos = np.asarray([1, 1, 0, 77, 1], np.uint32)
    r, p, cf, _ = Run(engine, b, ts).epoch(rc, pos)
    assert r.tolist() == [RC_RCOK, RC_ABORT, RC_RCOK, WD_GONE, RC_RCOK] and p.tolist() == pos.tolist()


def mixed_batch(rng, lens, n_rows):
    return make_batch([[(int(k), int(t)) for k, t in zip(rng.integers(0, n_rows, size=L),
                                                         rng.choice([RD, WR, XP, SCAN], size=L, p=[.5, .3, .1, .1]))]
                       for L in lens])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches(engine, n):
    """One wave of txns, one short of it, one more: over 8 seeded rows."""
    rng = np.random.default_rng(n)
    b = mixed_batch(rng, rng.integers(0, 5, size=n).tolist() if n > 1 else [3], 8)
    run = Run(engine, b, make_ts(rng, n, "permuted"), rows=seed_rows(rng, n, 8))
    e1 = run.epoch(*new_state(n), dev=n == 64)
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=n == 64)
    run.epoch(f1[0], f1[1])


@pytest.mark.parametrize("maxlen", [1, 2, 4, 8, 16, 32, 64])
def test_lanes_per_txn(engine, maxlen):
    """1, 2, .. 64 lanes per txn: the longest txn decides; shorter ones beside
    it, stops in the upper lanes too."""
    rng = np.random.default_rng(maxlen)
    lens = [maxlen, max(maxlen // 2 + 1, 1), 1, maxlen] * 30
    n_rows = 400 * maxlen  # few conflicts, so that long txns get far
    b = mixed_batch(rng, lens, n_rows)
    seeded = {int(k): (int(rng.integers(0, len(lens))), int(rng.integers(0, len(lens))))
              for k in rng.choice(n_rows, size=n_rows // 20, replace=False)}
    run = Run(engine, b, make_ts(rng, b.n_txn, "permuted"), rows=seeded)
    e1 = run.epoch(*new_state(b.n_txn))
    assert e1[3]["n_commit"] > 0 and e1[3]["n_abort"] > 0
    if maxlen >= 4:
        assert int(((e1[0] != RC_RCOK) & (e1[2] >= maxlen // 2)).sum()) > 0
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=True)
    run.epoch(f1[0], f1[1], dev=True)


def test_the_length_limit(engine):
    """A txn of 65 accesses: DCC_EINVAL with rc / pos and the rows as they were."""
    run = Run(engine, make_batch([[(1, RD)]]), [1], rows={1: (3, 4), 100: (5, 6)})
    long = make_batch([[(1, RD)], [(100 + q, WR) for q in range(65)], [(2, WR)]])
    t3 = np.asarray([9, 8, 7], np.uint64)
    for dev in (False, True):
        rc, pos = new_state(3)
        if dev:
            bb = long.to_torch("cuda:0")
            args = [to_dev(t3, np.uint64), to_dev(rc, np.uint8), to_dev(pos, np.uint32), to_dev(np.ones(3), np.uint8)]
        else:
            bb, args = long, [t3, rc, pos, np.ones(3, np.uint8)]
        for call in (lambda: engine.tso_access_epoch(bb, *args[:3]), lambda: engine.tso_finish(bb, *args)):
            with pytest.raises(d.DccError) as e:
                call()
            assert e.value.code == _abi.DCC_EINVAL
            r, p = (from_dev(args[1], np.uint8), from_dev(args[2], np.uint32)) if dev else (args[1], args[2])
            assert np.all(r == WD_RUN) and np.all(p == 0)
    assert engine_rows(engine, [1, 2, 100, 101]) == {1: (3, 4), 100: (5, 6)}


# ------------------------------------------------------------- tile seams
@pytest.mark.parametrize("n", [TILE + 1, 2 * TILE + 3])
@pytest.mark.parametrize("shape", ["low_prewrite", "all_wr"])
def test_one_row_across_tiles(engine, n, shape):
    """One row named by n one-access RUN txns, its segment across the tile
    seams: one low prewrite in front of readers that all wait, or writers
    only, whose aborts and waits depend on all that ran before.  The row's wts
    is seeded below every ts but a few, which abort on it."""
    rng = np.random.default_rng(n)
    if shape == "low_prewrite":
        at = np.full(n, RD, np.uint8)
        at[0] = WR
        ts = np.uint64(10) + np.concatenate([[0], 1 + rng.permutation(n - 1)]).astype(np.uint64)
        ts[[5, TILE // 2, TILE - 1, TILE]] = [1, 2, 3, 4]  # below the seeded wts, on both sides of the seam
    else:
        at = np.full(n, WR, np.uint8)
        ts = make_ts(rng, n, "permuted") + np.uint64(10)
    b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, 77, np.uint64), at)
    run = Run(engine, b, ts, rows={77: (5, 0)})
    e1 = run.epoch(*new_state(n))
    if shape == "low_prewrite":
        assert outcomes(e1[3]) == (1, 4, n - 5)
    else:
        assert min(outcomes(e1[3])) > 0
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=True)
    assert f1[3] > 0
    run.epoch(f1[0], f1[1], dev=True)


@pytest.mark.parametrize("m", [TILE - 1, TILE, TILE + 1])
def test_batch_of_a_tile(engine, m):
    """m accesses in all, one per txn, on three hot rows, one with a seeded wts."""
    rng = np.random.default_rng(m)
    keys = rng.choice(np.asarray([3, 9, 1 << 40], np.uint64), size=m, p=[0.5, 0.3, 0.2])
    at = rng.choice(np.asarray([RD, WR, SCAN], np.uint8), size=m, p=[0.7, 0.2, 0.1])
    b = d.EpochBatch(np.arange(m + 1, dtype=np.uint32), keys, at)
    # the first third in random order (aborts), the rest rising above it (waits)
    ts = np.arange(1, m + 1).astype(np.uint64)
    ts[:m // 3] = rng.permutation(ts[:m // 3])
    run = Run(engine, b, ts, rows={9: (m // 6, 0)})
    e1 = run.epoch(*new_state(m))
    assert min(outcomes(e1[3])) > 0
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]))
    assert f1[3] > 0
    run.epoch(f1[0], f1[1])


def one_row(rng, n_static, n_dyn, key=77):
    """One row named by n_static WR txns, their ts rising with the index from
    4 * n_dyn on, between n_dyn txns of mixed types whose ts lie on both sides
    of the least of those."""
    n = n_static + n_dyn
    is_dyn = np.zeros(n, bool)
    is_dyn[rng.choice(n, size=n_dyn, replace=False)] = True
    at = np.full(n, WR, np.uint8)
    at[is_dyn] = rng.choice(np.asarray([RD, WR, SCAN, XP], np.uint8), size=n_dyn, p=[.5, .3, .1, .1])
    ts = np.empty(n, np.uint64)
    ts[~is_dyn] = np.uint64(4 * n_dyn) + np.arange(n_static, dtype=np.uint64)
    ts[is_dyn] = np.uint64(1) + rng.permutation(8 * n_dyn)[:n_dyn].astype(np.uint64)
    return d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, key, np.uint64), at), ts, is_dyn


@pytest.mark.parametrize("n_static,n_dyn", [(TILE - 3, 40), (TILE, 40), (TILE + 5, TILE), (5, TILE + 2)])
def test_static_and_dynamic_across_a_seam(engine, n_static, n_dyn):
    """A first epoch of the writers alone leaves one RCOK and the others
    buffered at their own reads, each holding its prewrite: the static entries
    of the second epoch, which admits the rest.  The row's static prewrites
    end, and its dynamic accesses begin, on either side of a tile seam; the
    row's seeded wts reaches the dynamic accesses across it."""
    rng = np.random.default_rng(n_static + n_dyn)
    b, ts, is_dyn = one_row(rng, n_static, n_dyn)
    run = Run(engine, b, ts, rows={77: (n_dyn // 2, 0)})
    rc = np.where(is_dyn, WD_GONE, WD_RUN).astype(np.uint8)
    e0 = run.epoch(rc, np.zeros(b.n_txn, np.uint32))
    assert outcomes(e0[3]) == (1, 0, n_static - 1)
    rc, pos = e0[0].copy(), e0[1].copy()
    admit(rc, pos, np.nonzero(is_dyn)[0])
    e1 = run.epoch(rc, pos, dev=True)
    assert min(outcomes(e1[3])) > 0
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=True)
    assert f1[3] > 0
    run.epoch(f1[0], f1[1])


# ------------------------------------------------------------------ finish
@pytest.mark.parametrize("middle", [False, True], ids=["all_at_once", "a_prewrite_in_the_middle"])
def test_finish_promotes_a_row_of_buffered_reads(engine, middle):
    """1,026 buffered reads on one row behind one prewrite, whose commit
    promotes them all; with a second prewrite that stays in the middle of their
    timestamps only the reads at or below it go."""
    n = TILE + 2
    rng = np.random.default_rng(n + middle)
    at = np.asarray([WR, WR] + [RD] * n, np.uint8)
    rts = np.uint64(10) + rng.permutation(n).astype(np.uint64)
    ts = np.concatenate([np.asarray([1, 10 + n // 2 if middle else 5 * n], np.uint64), rts])
    rc = np.asarray([RC_RCOK, RC_RCOK] + [RC_WAIT] * n, np.uint8)
    pos = np.asarray([1, 1] + [0] * n, np.uint32)
    b = d.EpochBatch(np.arange(n + 3, dtype=np.uint32), np.full(n + 2, 5, np.uint64), at)
    for dev in (False, True):
        run = Run(engine, b, ts)
        leave = np.zeros(n + 2, np.uint8)
        leave[0] = 1
        f = run.finish(rc, pos, leave, dev=dev)
        assert f[3] == (int((rts <= ts[1]).sum()) if middle else n)
        assert engine_rows(engine, [5]) == {5: (1, int(rts[rts <= ts[1]].max()))}
        run.epoch(f[0], f[1], dev=dev)


# ------------------------------------------------------------------ rounds
def test_chain_of_100_rounds(engine):
    """Txn i reads row i - 1 and writes row i, ts rising: whether txn i - 1 made
    its prewrite decides txn i, a round later: more rounds than the
    undecided-count ring holds and than one host batch of rounds."""
    n = 100
    assert n > RING
    b = make_batch([[(0, WR)]] + [[(i - 1, RD), (i, WR)] for i in range(1, n)])
    ts = np.arange(1, n + 1).astype(np.uint64)
    rc, pos = new_state(n)
    run = Run(engine, b, ts)
    _, _, _, st = run.epoch(rc, pos)
    exp = ref.rounds_epoch(b, ts, rc, pos)
    assert exp[0].tolist() == [RC_RCOK if i % 2 == 0 else RC_WAIT for i in range(n)]
    assert n - 1 <= st["rounds"] <= n + 1 and st["rounds"] == exp[3]["rounds"]


def test_one_row_eight_times_in_a_txn(engine):
    """A txn's own prewrites and reads never stop it, next to other txns of
    the row that they do stop."""
    K = 3
    cases = [([[(K, RD)] * 8], [4]),
             ([[(K, RD)] * 7 + [(K, WR)]], [4]),
             ([[(K, RD)], [(K, WR)] * 7 + [(K, RD)], [(K, RD)]], [1, 4, 9]),
             ([[(K, RD)], [(K, RD)] * 7 + [(K, WR)], [(K, RD)], [(K, WR)] * 8, [(K, SCAN)] * 8], [9, 4, 2, 1, 3])]
    for txns, ts in cases:
        b = make_batch(txns)
        ts = np.asarray(ts, np.uint64)
        run = Run(engine, b, ts)
        rc, pos = new_state(len(txns))
        r, p, _, st = run.epoch(rc, pos)
        assert st["rounds"] == ref.rounds_epoch(b, ts, rc, pos)[3]["rounds"]
        run.finish(r, p, leave_of(r, [RC_RCOK, RC_ABORT]), dev=True)
    rng = np.random.default_rng(8)
    b = hot_batch(rng, 500, 8, 40)  # many duplicate rows within a txn
    run = Run(engine, b, make_ts(rng, 500, "permuted"))
    e1 = run.epoch(*new_state(500))
    assert min(outcomes(e1[3])) > 0


# -------------------------------------------------------------------- YCSB
@functools.lru_cache(maxsize=None)
def ycsb(n_txn):
    """A YCSB theta 0.9 batch, ts = index with jitter, and the replay of: an
    epoch, the finish of every RCOK and ABORT txn, a second epoch."""
    b = d.gen_ycsb(n_txn=n_txn, zipf_theta=0.9)
    ts = make_ts(np.random.default_rng(n_txn), n_txn, "jitter")
    rc, pos = new_state(n_txn)
    state = {}
    snap = lambda r: (r, ref.rows_of(state))
    e1 = snap(ref.epoch(b, ts, rc, pos, state))
    leave = leave_of(e1[0][0], [RC_RCOK, RC_ABORT])
    f1 = snap(ref.finish(b, ts, e1[0][0], e1[0][1], leave, state))
    e2 = snap(ref.epoch(b, ts, f1[0][0], f1[0][1], state))
    return b, ts, e1, leave, f1, e2


@pytest.mark.parametrize("form", ["host", "device", "compact"])
def test_ycsb_epoch_finish_epoch(engine, form):
    """4,096 x 16 at theta 0.9: an epoch, the finish of every RCOK and ABORT
    txn, a second epoch; host, device and compact batches."""
    b, ts, e1, leave, f1, e2 = ycsb(4096)
    assert e1[0][3]["n_commit"] > 0 and e1[0][3]["n_survivors"] > 0 and f1[0][3] > 0 and min(outcomes(e2[0][3])) > 0
    dev = form == "device"
    cb = engine.compact_host_batch(b) if form == "compact" else None
    if cb is not None:
        assert cb.keys.dtype == np.uint32 and cb.meta.get("acctype_2bit")
    run = Run(engine, b, ts, run_batch=cb)
    _, _, _, st = run.epoch(*new_state(b.n_txn), exp=e1, dev=dev)
    assert st["rounds"] > 1
    run.finish(e1[0][0], e1[0][1], leave, exp=f1, dev=dev)
    run.epoch(f1[0][0], f1[0][1], exp=e2, dev=dev, want_conflict=form != "device")


@pytest.mark.parametrize("family", ["permuted", "tied", "seeded"])
def test_six_epoch_histories(engine, family):
    """2,000 txns over 400 rows admitted over six epochs, two finishes after
    each (the second has RUN leavers): compared after every call."""
    b, ts, rows0, steps, tot = history(len(family), family, epochs=6, per_epoch=334, n_rows=400, max_len=8)
    assert min(tot[k] for k in ("rcok", "ab_rts", "ab_wts_rd", "ab_wts_wr", "wait", "promoted", "run_leavers")) > 0
    assert family != "seeded" or tot["ab_wts_wr_only"] > 0
    run = Run(engine, b, ts, rows=rows0)
    for q, s in enumerate(steps):
        dev = q % 4 >= 2
        if s[0] == "epoch":
            run.epoch(s[1], s[2], exp=(s[3], s[4]), dev=dev)
        else:
            run.finish(s[1], s[2], s[3], exp=(s[4], s[5]), dev=dev)


def test_keys_across_the_u64_range(engine):
    """Keys from 1 to 2^64 - 2 that leave the epoch's sort its bit: they vary in
    63 bits; varying in all 64 is DCC_ENOTSUP for the epoch and fine for the
    finish."""
    rng = np.random.default_rng(64)
    n = 600
    rows = np.concatenate([np.asarray([1, (1 << 64) - 2, 1 << 63, (1 << 63) - 1], np.uint64),
                           rng.integers(1, (1 << 64) - 1, size=36, dtype=np.uint64)]) | np.uint64(1 << 20)
    rows[1] = (1 << 64) - 2
    b = hot_batch(rng, n, 4, len(rows))
    b = d.EpochBatch(b.offsets, rows[np.asarray(b.keys, np.int64)], b.acctype)
    vary = np.bitwise_or.reduce(b.keys) & ~np.bitwise_and.reduce(b.keys)
    assert bin(int(vary)).count("1") == 63
    seeded = {int(k): (int(rng.integers(0, n)), int(rng.integers(0, n))) for k in rows[::3]}
    run = Run(engine, b, make_ts(rng, n, "permuted"), rows=seeded)
    e1 = run.epoch(*new_state(n))
    assert min(outcomes(e1[3])) > 0
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=True)
    run.epoch(f1[0], f1[1], dev=True)
    keys = np.asarray(b.keys).copy()
    keys[0] ^= np.uint64(1 << 20)
    b64 = d.EpochBatch(b.offsets, keys, b.acctype)
    rc, pos = new_state(n)
    with pytest.raises(d.DccError) as e:
        engine.tso_access_epoch(b64, run.ts, rc, pos)
    assert e.value.code == _abi.DCC_ENOTSUP and np.all(rc == WD_RUN) and np.all(pos == 0)
    run.same_rows()
    run = Run(engine, b64, run.ts)
    st0 = np.where(np.arange(n) % 2 == 0, RC_RCOK, WD_GONE).astype(np.uint8)
    lens = np.diff(np.asarray(b64.offsets).astype(np.int64)).astype(np.uint32)
    run.finish(st0, lens, leave_of(st0, [RC_RCOK]))


# ----------------------------------------------- interplay with other calls
def test_one_at_a_time_equals_validate_epoch(engine):
    """64 txns run one at a time as (an epoch with one RUN txn, its finish) give
    dcc_tso_validate_epoch's rc, conflict ordinals and rows, over seeded rows."""
    rng = np.random.default_rng(64)
    n = 64
    b = hot_batch(rng, n, 6, 12)
    ts = make_ts(rng, n, "permuted")
    seeded = {k: v for k, v in seed_rows(rng, n // 4, 12).items()}
    set_rows(engine, seeded)
    rc, pos = new_state(n, WD_GONE)
    out_rc, out_cf = np.empty(n, np.uint8), np.empty(n, np.uint32)
    for i in range(n):
        rc[i], pos[i] = WD_RUN, 0
        _, _, cf, st = engine.tso_access_epoch(b, ts, rc, pos)
        assert rc[i] in (RC_RCOK, RC_ABORT) and st["n_survivors"] == 0
        out_rc[i], out_cf[i] = rc[i], cf[i]
        leave = np.zeros(n, np.uint8)
        leave[i] = 1
        assert engine.tso_finish(b, ts, rc, pos, leave)[:2] == (1, 0)
        assert rc[i] == WD_GONE
    rows = engine_rows(engine, np.arange(12))
    set_rows(engine, seeded)
    vrc, vcf, _ = engine.tso_validate_epoch(b, ts)
    assert 0 < int((vrc == RC_ABORT).sum()) < n
    differ("rc", out_rc, vrc)
    differ("conflict", out_cf, vcf)
    assert engine_rows(engine, np.arange(12)) == rows


def test_a_carried_population_decides_the_same(engine):
    """dcc_waitdie_carry moves a TIMESTAMP population unchanged: the carried
    batch decides, through src, what the uncompacted one decides."""
    rng = np.random.default_rng(3)
    n = 1500
    b = hot_batch(rng, n, 6, 200)
    ts = make_ts(rng, n, "jitter")
    run = Run(engine, b, ts)
    e1 = run.epoch(*new_state(n))
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]))
    assert f1[3] > 0
    rc, pos = f1[0], f1[1]
    exp = ref.epoch(b, ts, rc, pos, run.state)
    got, cts, crc, cpos, src, kept, _ = engine.waitdie_carry(b, ts, rc, pos)
    assert kept == int((rc != WD_GONE).sum()) == got.n_txn and 0 < kept < n
    r, p, cf, _ = engine.tso_access_epoch(got, cts, crc, cpos)
    differ("rc", r, exp[0][src])
    differ("pos", p, exp[1][src])
    differ("conflict", cf, exp[2][src])
    run.same_rows()


# ---------------------------------------------------------------- rejections
def test_rejections_leave_everything(engine):
    b = make_batch([[(1, RD), (2, WR)], [(3, WR)], [(2, RD)]])
    ts = np.asarray([1, 2, 3], np.uint64)
    # something in the rows first
    run = Run(engine, b, ts, rows={7: (8, 9)})
    e1 = run.epoch(*new_state(3))
    assert e1[0].tolist() == [RC_RCOK, RC_RCOK, RC_WAIT]
    run.finish(e1[0], e1[1], np.asarray([0, 1, 0], np.uint8))
    leave = np.asarray([1, 0, 0], np.uint8)
    off = b.offsets.copy()
    off[1] = 4  # [0, 4, 3, 4]: decreases
    keys = b.keys.copy()
    keys[1] = d.KEY_RESERVED
    ok_rc, ok_pos = [WD_RUN, WD_RUN, WD_RUN], [0, 0, 0]
    bad = [(b, ts, [WD_RUN, 0x12, WD_RUN], [0, 0, 0]),        # rc bytes outside the five states
           (b, ts, [WD_RUN, 1, WD_RUN], [0, 0, 0]),
           (b, ts, [WD_RUN, 0xFF, WD_RUN], [0, 0, 0]),
           (b, ts, [WD_RUN, WD_RUN, WD_RUN], [3, 0, 0]),      # pos > len
           (b, ts, [RC_ABORT, WD_RUN, WD_RUN], [3, 0, 0]),
           (b, ts, [RC_RCOK, WD_RUN, WD_RUN], [1, 0, 0]),     # RCOK with pos != len
           (b, ts, [RC_WAIT, WD_RUN, WD_RUN], [2, 0, 0]),     # WAIT with pos >= len
           (d.EpochBatch(off, b.keys, b.acctype), ts, ok_rc, ok_pos),
           (d.EpochBatch(b.offsets, keys, b.acctype), ts, ok_rc, ok_pos)]
    calls = [(bb, t, r, p, leave, True) for bb, t, r, p in bad]
    calls.append((b, ts, [RC_WAIT, WD_RUN, WD_RUN], [1, 0, 0], leave, False))  # a WAIT leaver: the finish only
    for bb, t, rc0, pos0, lv, both in calls:
        t = np.asarray(t, np.uint64)
        for dev in (False, True):
            if dev:
                run_b = bb.to_torch("cuda:0")
                args = [to_dev(t, np.uint64), to_dev(rc0, np.uint8), to_dev(pos0, np.uint32), to_dev(lv, np.uint8)]
            else:
                run_b = bb
                args = [t, np.asarray(rc0, np.uint8), np.asarray(pos0, np.uint32), lv]
            fns = [lambda: engine.tso_finish(run_b, *args)]
            if both:
                fns.append(lambda: engine.tso_access_epoch(run_b, *args[:3]))
            for call in fns:
                with pytest.raises(d.DccError) as e:
                    call()
                assert e.value.code == _abi.DCC_EINVAL
                r, p = (from_dev(args[1], np.uint8), from_dev(args[2], np.uint32)) if dev else (args[1], args[2])
                assert r.tolist() == rc0 and p.tolist() == pos0
                run.same_rows()
    # NULL ts / rc / pos / leave
    rc, pos = new_state(3)
    for args in ((None, rc, pos), (ts, None, pos), (ts, rc, None)):
        with pytest.raises(d.DccError) as e:
            engine.tso_access_epoch(b, *args)
        assert e.value.code == _abi.DCC_EINVAL
        with pytest.raises(d.DccError) as e:
            engine.tso_finish(b, *args, leave)
        assert e.value.code == _abi.DCC_EINVAL
    with pytest.raises(d.DccError) as e:
        engine.tso_finish(b, ts, rc, pos, None)
    assert e.value.code == _abi.DCC_EINVAL
    assert np.all(rc == WD_RUN) and np.all(pos == 0)
    run.same_rows()
    # a GONE txn's pos is ignored, 0 and UINT64_MAX are timestamps, and the context still works
    run.ts = np.asarray([0, 0, (1 << 64) - 1], np.uint64)
    run.epoch(np.asarray([WD_GONE, WD_RUN, WD_RUN], np.uint8), np.asarray([99, 0, 0], np.uint32))


def test_reserve_and_repeat(engine):
    b, ts, e1, leave, f1, e2 = ycsb(4096)
    engine.reserve(b.n_txn, b.nnz)
    for _ in range(2):
        run = Run(engine, b, ts)
        run.epoch(*new_state(b.n_txn), exp=e1, dev=True)
        run.finish(e1[0][0], e1[0][1], leave, exp=f1, dev=True)
        run.epoch(f1[0][0], f1[0][1], exp=e2)


# ----------------------------------------------------------------- multi-GPU
def test_multi_context_runs_on_rank0():
    b, ts, e1, leave, f1, e2 = ycsb(4096)
    with d.Engine(devices=[0, 0]) as m:
        run = Run(m, b, ts)
        run.epoch(*new_state(b.n_txn), exp=e1)
        run.finish(e1[0][0], e1[0][1], leave, exp=f1, dev=True)
        run.epoch(f1[0][0], f1[0][1], exp=e2, dev=True)


def test_two_rank_communicator_not_supported():
    b, ts, e1, leave, _, _ = ycsb(4096)
    rc, pos = new_state(b.n_txn)
    with d.Engine(0) as eng:
        eng.comm_init_host(0, 2, lambda buf: None)
        with pytest.raises(d.DccError) as e:
            eng.tso_access_epoch(b, ts, rc, pos)
        assert e.value.code == _abi.DCC_ENOTSUP
        with pytest.raises(d.DccError) as e:
            eng.tso_finish(b, ts, rc, pos, leave)
        assert e.value.code == _abi.DCC_ENOTSUP
        assert np.all(rc == WD_RUN) and np.all(pos == 0)
        eng.comm_destroy()
