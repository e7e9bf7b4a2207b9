"""GPU parity of MVCC with txns in flight (dcc_mvcc_access_epoch, dcc_mvcc_finish,
mvcc_live.hip) against the closed-form replay (mvcc_live_ref.py): rc, pos, the
conflict ordinals, the counts, the versions read, the rows and the exported
store after every call, bit-exact."""
import functools
import os
import re

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RC_WAIT, RD, SCAN, VTS_NONE, WD_GONE, WD_RUN, WR, XP, _abi
from helpers import make_batch
from mvcc_ref import rows_of, trim, versions_of
import mvcc_live_ref as ref
from mvcc_live_cases import KATS, admit, five_outcomes, history, hot_batch, make_ts, new_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constant(name, file):
    src = open(os.path.join(ROOT, "deneva_amd", "csrc", file)).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


TILE = kernel_constant("TS_T", "mvcc_live.hip") * kernel_constant("TS_ITEMS", "mvcc_live.hip")  # accesses per scan tile
RING = kernel_constant("SEG_RING", "seg_rounds.h")  # undecided-count ring


@pytest.fixture(autouse=True)
def clean_rows(request):
    if "engine" in request.fixturenames:
        request.getfixturevalue("engine").mvcc_clear()
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
    w, r = eng.mvcc_rows_get(keys)
    return {int(k): (int(a), int(b)) for k, a, b in zip(keys, w, r) if (a, b) != (0, 0)}


def engine_versions(eng):
    k, t = eng.mvcc_versions()
    return list(zip(k.tolist(), t.tolist()))


class Run:
    """The engine next to the closed form over one batch: every call is made on
    both and everything they leave is compared."""

    def __init__(self, eng, b, ts, run_batch=None, clear=True):
        if clear:
            eng.mvcc_clear()
        self.eng, self.b, self.ts = eng, b, np.asarray(ts, np.uint64)
        self.run_batch = run_batch if run_batch is not None else b
        self.state = {}
        self.vts = ref.new_vts(b)   # the replay's
        self.gvts = ref.new_vts(b)  # the engine's

    def same_store(self, exp=None):
        rows, vers = exp if exp is not None else (rows_of(self.state), versions_of(self.state))
        assert engine_rows(self.eng, self.b.keys) == rows
        assert engine_versions(self.eng) == vers
        assert self.eng.mvcc_versions_size == len(vers)

    def call(self, dev, rc, pos, leave, fn):
        """fn(batch, ts, rc, pos[, leave], vts) on host arrays or device
        tensors; returns rc, pos as numpy and what fn returned."""
        if dev:
            args = [to_dev(self.ts, np.uint64), to_dev(rc, np.uint8), to_dev(pos, np.uint32)]
            if leave is not None:
                args.append(to_dev(leave, np.uint8))
            v = to_dev(self.gvts, np.uint64)
            out = fn(self.run_batch.to_torch("cuda:0"), *args, v)
            self.gvts = from_dev(v, np.uint64)[:len(self.gvts)].copy()
            return from_dev(args[1], np.uint8), from_dev(args[2], np.uint32), out
        r, p = np.array(rc, np.uint8), np.array(pos, np.uint32)
        args = [self.ts, r, p] + ([np.asarray(leave, np.uint8)] if leave is not None else [])
        v = self.gvts if len(self.gvts) else np.zeros(1, np.uint64)
        return r, p, fn(self.run_batch, *args, v)

    def epoch(self, rc, pos, dev=False, exp=None, want_conflict=True):
        """exp: (replay's result, vts, rows, versions) computed before."""
        if exp is None:
            exp = (ref.epoch(self.b, self.ts, rc, pos, self.vts, self.state), self.vts,
                   rows_of(self.state), versions_of(self.state))
        e = exp[0]
        r, p, out = self.call(dev, rc, pos, None,
                              lambda b, t, r, p, v: self.eng.mvcc_access_epoch(b, t, r, p, v, want_conflict))
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
        differ("vts", self.gvts, exp[1])
        self.same_store(exp[2:])
        n, m = self.b.n_txn, self.b.nnz
        if n:
            assert st["alg_bytes"] == d.mvcc_access_alg_bytes(n, m, want_conflict, True)
            assert d.mvcc_access_alg_bytes(n, m, True, True) == d.waitdie_alg_bytes(n, m, True) + 8 * m
        return r, p, cf, st

    def finish(self, rc, pos, leave, dev=False, exp=None):
        if exp is None:
            exp = (ref.finish(self.b, self.ts, rc, pos, leave, self.vts, self.state), self.vts,
                   rows_of(self.state), versions_of(self.state))
        e = exp[0]
        r, p, out = self.call(dev, rc, pos, leave,
                              lambda b, t, r, p, lv, v: self.eng.mvcc_finish(b, t, r, p, lv, v))
        left, prom, st = out
        differ("rc", r, e[0])
        differ("pos", p, e[1])
        assert (left, prom) == (e[2], e[3])
        assert st["n_commit"] == e[2] and st["n_survivors"] == e[3]
        differ("vts", self.gvts, exp[1])
        self.same_store(exp[2:])
        return r, p, left, prom

    def trim(self, floor):
        assert self.eng.mvcc_trim(floor) == trim(self.state, floor)
        self.same_store()


def leave_of(rc, states):
    return np.isin(rc, states).astype(np.uint8)


def outcomes(st):
    return st["n_commit"], st["n_abort"], st["n_survivors"]


# ------------------------------------------------------------ the hand cases
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_hand_cases(engine, case, dev):
    _, txns, ts, rc0, steps = case
    run = Run(engine, make_batch(txns), ts)
    rc, pos = np.asarray(rc0, np.uint8), np.zeros(len(txns), np.uint32)
    for s in steps:
        if s[0] == "admit":
            admit(rc, pos, s[1])
        elif s[0] == "epoch":
            rc, pos, cf, _ = run.epoch(rc, pos, dev=dev)
            assert (rc.tolist(), pos.tolist(), cf.tolist(), run.gvts.tolist()) == (s[1], s[2], s[3], s[4])
        else:
            leave = np.zeros(len(txns), np.uint8)
            leave[s[1]] = 1
            rc, pos, left, prom = run.finish(rc, pos, leave, dev=dev)
            assert (rc.tolist(), pos.tolist(), left, prom, run.gvts.tolist()) == (s[2], s[3], len(s[1]), s[4], s[5])


# ---------------------------------------------------------------- the edges
def test_empty_zero_length_gone_and_run_at_len(engine):
    e = make_batch([])
    z = np.zeros(0, np.uint64)
    rc, pos, cf, st = engine.mvcc_access_epoch(e, z, np.zeros(0, np.uint8), np.zeros(0, np.uint32))
    assert len(rc) == 0 and len(pos) == 0 and len(cf) == 0 and st["n_commit"] == 0
    assert engine.mvcc_finish(e, z, np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint8))[:2] == (0, 0)
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


def test_lanes_per_txn_and_the_length_limit(engine):
    """Txn lengths 1, 2, 16, 17 and 64 in one batch (64 lanes per txn), then a
    txn of 65: DCC_EINVAL with rc / pos as they were."""
    rng = np.random.default_rng(5)
    lens = [1, 2, 16, 17, 64] * 40
    txns = [[(int(k), int(t)) for k, t in zip(rng.integers(0, 600, size=L), rng.choice([RD, WR, XP, SCAN], size=L,
                                                                                        p=[.6, .2, .1, .1]))]
            for L in lens]
    b = make_batch(txns)
    ts = make_ts(rng, b.n_txn, "permuted")
    run = Run(engine, b, ts)
    e1 = run.epoch(*new_state(b.n_txn))
    assert min(outcomes(e1[3])) > 0
    assert int(((e1[0] != RC_RCOK) & (e1[2] > 32)).sum()) > 0  # stops in the upper lanes too
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=True)
    assert f1[3] > 0
    run.epoch(f1[0], f1[1], dev=True)
    long = make_batch([[(1, RD)], [(100 + q, WR) for q in range(65)], [(2, WR)]])
    t3 = np.asarray([9, 8, 7], np.uint64)
    for dev in (False, True):
        rc, pos = new_state(3)
        if dev:
            bb = long.to_torch("cuda:0")
            args = [to_dev(t3, np.uint64), to_dev(rc, np.uint8), to_dev(pos, np.uint32), to_dev(np.ones(3), np.uint8)]
        else:
            bb, args = long, [t3, rc, pos, np.ones(3, np.uint8)]
        for call in (lambda: engine.mvcc_access_epoch(bb, *args[:3]), lambda: engine.mvcc_finish(bb, *args)):
            with pytest.raises(d.DccError) as e:
                call()
            assert e.value.code == _abi.DCC_EINVAL
            r, p = (from_dev(args[1], np.uint8), from_dev(args[2], np.uint32)) if dev else (args[1], args[2])
            assert np.all(r == WD_RUN) and np.all(p == 0)
    run.same_store()


# ------------------------------------------------------------- tile seams
@pytest.mark.parametrize("n", [TILE + 1, 2 * TILE + 3])
@pytest.mark.parametrize("shape", ["low_prewrite", "all_wr"])
def test_one_row_across_tiles(engine, n, shape):
    """One row named by n one-access RUN txns, its segment across the tile
    seams: one low prewrite in front of readers that all wait, or writers
    only, whose aborts and waits depend on all that ran before."""
    rng = np.random.default_rng(n)
    if shape == "low_prewrite":
        at = np.full(n, RD, np.uint8)
        at[0] = WR
        ts = np.uint64(1) + np.concatenate([[0], 1 + rng.permutation(n - 1)]).astype(np.uint64)
    else:
        at = np.full(n, WR, np.uint8)
        ts = make_ts(rng, n, "permuted")
    b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, 77, np.uint64), at)
    run = Run(engine, b, ts)
    e1 = run.epoch(*new_state(n))
    if shape == "low_prewrite":
        assert outcomes(e1[3]) == (1, 0, n - 1)
    else:
        assert min(outcomes(e1[3])) > 0
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=True)
    assert f1[3] > 0
    run.epoch(f1[0], f1[1], dev=True)


@pytest.mark.parametrize("m", [TILE - 1, TILE, TILE + 1])
def test_batch_of_a_tile(engine, m):
    """m accesses in all, one per txn, on three hot rows."""
    rng = np.random.default_rng(m)
    keys = rng.choice(np.asarray([3, 9, 1 << 40], np.uint64), size=m, p=[0.5, 0.3, 0.2])
    at = rng.choice(np.asarray([RD, WR, SCAN], np.uint8), size=m, p=[0.7, 0.2, 0.1])
    b = d.EpochBatch(np.arange(m + 1, dtype=np.uint32), keys, at)
    # the first third in random order (aborts), the rest rising above it (waits)
    ts = np.arange(1, m + 1).astype(np.uint64)
    ts[:m // 3] = rng.permutation(ts[:m // 3])
    run = Run(engine, b, ts)
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
    end, and its dynamic accesses begin, on either side of a tile seam."""
    rng = np.random.default_rng(n_static + n_dyn)
    b, ts, is_dyn = one_row(rng, n_static, n_dyn)
    run = Run(engine, b, ts)
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
        assert np.all(run.gvts[2:][rts <= ts[1]] == 1)
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
    state, vts = {}, ref.new_vts(b)
    snap = lambda r: (r, vts.copy(), rows_of(state), versions_of(state))
    e1 = snap(ref.epoch(b, ts, rc, pos, vts, state))
    leave = leave_of(e1[0][0], [RC_RCOK, RC_ABORT])
    f1 = snap(ref.finish(b, ts, e1[0][0], e1[0][1], leave, vts, state))
    e2 = snap(ref.epoch(b, ts, f1[0][0], f1[0][1], vts, state))
    return b, ts, e1, leave, f1, e2


@pytest.mark.parametrize("form", ["host", "device", "compact"])
def test_ycsb_epoch_finish_epoch(engine, form):
    """8,192 x 16 at theta 0.9: an epoch, the finish of every RCOK and ABORT
    txn, a second epoch; host, device and compact batches."""
    b, ts, e1, leave, f1, e2 = ycsb(8192)
    # behind rising ts nothing aborts at first; the promoted txns then meet larger rts
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


@pytest.mark.parametrize("family", ["permuted", "tied", "wrap"])
def test_six_epoch_histories(engine, family):
    """2,000 txns over 400 rows admitted over six epochs, two finishes after
    each (the second has RUN leavers) and a dcc_mvcc_trim between: compared
    after every call."""
    b, ts, steps, tot = history(len(family), family, epochs=6, per_epoch=334, n_rows=400, max_len=8, trim_after=3)
    five_outcomes(tot)
    assert tot["run_leavers"] > 0
    run = Run(engine, b, ts)
    for q, s in enumerate(steps):
        dev = q % 4 >= 2
        if s[0] == "epoch":
            run.epoch(s[1], s[2], exp=(s[4], s[5], s[6], s[7]), dev=dev)
        elif s[0] == "finish":
            run.finish(s[1], s[2], s[3], exp=(s[5], s[6], s[7], s[8]), dev=dev)
        else:
            assert engine.mvcc_trim(s[1]) == s[2]
            run.same_store(s[3:])


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
    run = Run(engine, b, make_ts(rng, n, "permuted"))
    e1 = run.epoch(*new_state(n))
    assert min(outcomes(e1[3])) > 0
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=True)
    run.epoch(f1[0], f1[1], dev=True)
    keys = np.asarray(b.keys).copy()
    keys[0] ^= np.uint64(1 << 20)
    b64 = d.EpochBatch(b.offsets, keys, b.acctype)
    rc, pos = new_state(n)
    with pytest.raises(d.DccError) as e:
        engine.mvcc_access_epoch(b64, run.ts, rc, pos)
    assert e.value.code == _abi.DCC_ENOTSUP and np.all(rc == WD_RUN) and np.all(pos == 0)
    run.same_store()
    engine.mvcc_clear()
    run = Run(engine, b64, run.ts)
    st0 = np.where(np.arange(n) % 2 == 0, RC_RCOK, WD_GONE).astype(np.uint8)
    lens = np.diff(np.asarray(b64.offsets).astype(np.int64)).astype(np.uint32)
    run.ts = np.sort(run.ts)
    run.finish(st0, lens, leave_of(st0, [RC_RCOK]))


# ----------------------------------------------- interplay with other calls
def test_one_at_a_time_equals_validate_epoch(engine):
    """64 txns run one at a time as (an epoch with one RUN txn, its finish) give
    dcc_mvcc_validate_epoch's rc, conflict ordinals, versions read, rows and
    exported store."""
    rng = np.random.default_rng(64)
    n = 64
    b = hot_batch(rng, n, 6, 12)
    ts = make_ts(rng, n, "permuted")
    engine.mvcc_clear()
    rc, pos = new_state(n, WD_GONE)
    vts = ref.new_vts(b)
    out_rc, out_cf = np.empty(n, np.uint8), np.empty(n, np.uint32)
    for i in range(n):
        rc[i], pos[i] = WD_RUN, 0
        _, _, cf, st = engine.mvcc_access_epoch(b, ts, rc, pos, vts)
        assert rc[i] in (RC_RCOK, RC_ABORT) and st["n_survivors"] == 0
        out_rc[i], out_cf[i] = rc[i], cf[i]
        leave = np.zeros(n, np.uint8)
        leave[i] = 1
        assert engine.mvcc_finish(b, ts, rc, pos, leave, vts)[:2] == (1, 0)
        assert rc[i] == WD_GONE
    rows, vers = engine_rows(engine, b.keys), engine_versions(engine)
    engine.mvcc_clear()
    vrc, vcf, vvts, _ = engine.mvcc_validate_epoch(b, ts)
    assert 0 < int((vrc == RC_ABORT).sum()) < n
    differ("rc", out_rc, vrc)
    differ("conflict", out_cf, vcf)
    differ("vts", vts, vvts)
    assert engine_rows(engine, b.keys) == rows and engine_versions(engine) == vers


def test_a_carried_population_decides_the_same(engine):
    """dcc_waitdie_carry moves an MVCC population unchanged: the carried batch
    decides, through src, what the uncompacted one decides."""
    rng = np.random.default_rng(3)
    n = 1500
    b = hot_batch(rng, n, 6, 200)
    ts = make_ts(rng, n, "jitter")
    run = Run(engine, b, ts)
    e1 = run.epoch(*new_state(n))
    f1 = run.finish(e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]))
    assert f1[3] > 0
    rc, pos = f1[0], f1[1]
    exp = ref.epoch(b, ts, rc, pos, None, run.state)
    got, cts, crc, cpos, src, kept, _ = engine.waitdie_carry(b, ts, rc, pos)
    assert kept == int((rc != WD_GONE).sum()) == got.n_txn and 0 < kept < n
    r, p, cf, _ = engine.mvcc_access_epoch(got, cts, crc, cpos)
    differ("rc", r, exp[0][src])
    differ("pos", p, exp[1][src])
    differ("conflict", cf, exp[2][src])
    run.same_store()


# ---------------------------------------------------------------- rejections
def test_rejections_leave_everything(engine):
    b = make_batch([[(1, RD), (2, WR)], [(3, WR)], [(2, RD)]])
    ts = np.asarray([1, 2, 3], np.uint64)
    # something in the rows and the store first
    run = Run(engine, b, ts)
    e1 = run.epoch(*new_state(3))
    assert e1[0].tolist() == [RC_RCOK, RC_RCOK, RC_WAIT]
    run.finish(e1[0], e1[1], np.asarray([0, 1, 0], np.uint8))
    leave = np.asarray([1, 0, 0], np.uint8)
    off = b.offsets.copy()
    off[1] = 4  # [0, 4, 3, 4]: decreases
    keys = b.keys.copy()
    keys[1] = d.KEY_RESERVED
    ok_rc, ok_pos = [WD_RUN, WD_RUN, WD_RUN], [0, 0, 0]
    U = (1 << 64) - 1
    bad = [(b, ts, [WD_RUN, 0x12, WD_RUN], [0, 0, 0]),        # rc bytes outside the five states
           (b, ts, [WD_RUN, 1, WD_RUN], [0, 0, 0]),
           (b, ts, [WD_RUN, 0xFF, WD_RUN], [0, 0, 0]),
           (b, ts, [WD_RUN, WD_RUN, WD_RUN], [3, 0, 0]),      # pos > len
           (b, ts, [RC_ABORT, WD_RUN, WD_RUN], [3, 0, 0]),
           (b, ts, [RC_RCOK, WD_RUN, WD_RUN], [1, 0, 0]),     # RCOK with pos != len
           (b, ts, [RC_WAIT, WD_RUN, WD_RUN], [2, 0, 0]),     # WAIT with pos >= len
           (b, [1, 0, 3], ok_rc, ok_pos),                     # a ts of 0 or UINT64_MAX
           (b, [1, 2, U], ok_rc, ok_pos),
           (d.EpochBatch(off, b.keys, b.acctype), ts, ok_rc, ok_pos),
           (d.EpochBatch(b.offsets, keys, b.acctype), ts, ok_rc, ok_pos)]
    calls = [(bb, t, r, p, leave, True) for bb, t, r, p in bad]
    calls.append((b, ts, [RC_WAIT, WD_RUN, WD_RUN], [1, 0, 0], leave, False))  # a WAIT leaver: the finish only
    for bb, t, rc0, pos0, lv, both in calls:
        t = np.asarray(t, np.uint64)
        for dev in (False, True):
            v0 = np.asarray([7, 8, 9, 10], np.uint64)
            if dev:
                run_b = bb.to_torch("cuda:0")
                args = [to_dev(t, np.uint64), to_dev(rc0, np.uint8), to_dev(pos0, np.uint32), to_dev(lv, np.uint8)]
                v = to_dev(v0, np.uint64)
            else:
                run_b = bb
                args = [t, np.asarray(rc0, np.uint8), np.asarray(pos0, np.uint32), lv]
                v = v0.copy()
            fns = [lambda: engine.mvcc_finish(run_b, *args, v)]
            if both:
                fns.append(lambda: engine.mvcc_access_epoch(run_b, *args[:3], v))
            for call in fns:
                with pytest.raises(d.DccError) as e:
                    call()
                assert e.value.code == _abi.DCC_EINVAL
                r, p = (from_dev(args[1], np.uint8), from_dev(args[2], np.uint32)) if dev else (args[1], args[2])
                assert r.tolist() == rc0 and p.tolist() == pos0
                assert (from_dev(v, np.uint64) if dev else v).tolist() == v0.tolist()
                run.same_store()
    # NULL ts / rc / pos / leave
    rc, pos = new_state(3)
    for args in ((None, rc, pos), (ts, None, pos), (ts, rc, None)):
        with pytest.raises(d.DccError) as e:
            engine.mvcc_access_epoch(b, *args)
        assert e.value.code == _abi.DCC_EINVAL
        with pytest.raises(d.DccError) as e:
            engine.mvcc_finish(b, *args, leave)
        assert e.value.code == _abi.DCC_EINVAL
    with pytest.raises(d.DccError) as e:
        engine.mvcc_finish(b, ts, rc, pos, None)
    assert e.value.code == _abi.DCC_EINVAL
    assert np.all(rc == WD_RUN) and np.all(pos == 0)
    run.same_store()
    # a GONE txn's pos and ts are ignored, and the context still works
    run.ts = np.asarray([0, 2, 3], np.uint64)
    run.epoch(np.asarray([WD_GONE, WD_RUN, WD_RUN], np.uint8), np.asarray([99, 0, 0], np.uint32))


def test_reserve_and_repeat(engine):
    b, ts, e1, leave, f1, e2 = ycsb(8192)
    engine.reserve(b.n_txn, b.nnz)
    for _ in range(2):
        run = Run(engine, b, ts)
        run.epoch(*new_state(b.n_txn), exp=e1, dev=True)
        run.finish(e1[0][0], e1[0][1], leave, exp=f1, dev=True)
        run.epoch(f1[0][0], f1[0][1], exp=e2)


# ----------------------------------------------------------------- multi-GPU
def test_multi_context_runs_on_rank0():
    b, ts, e1, leave, f1, e2 = ycsb(8192)
    with d.Engine(devices=[0, 0]) as m:
        run = Run(m, b, ts)
        run.epoch(*new_state(b.n_txn), exp=e1)
        run.finish(e1[0][0], e1[0][1], leave, exp=f1, dev=True)
        run.epoch(f1[0][0], f1[0][1], exp=e2, dev=True)


def test_two_rank_communicator_not_supported():
    b, ts, e1, leave, _, _ = ycsb(8192)
    rc, pos = new_state(b.n_txn)
    with d.Engine(0) as eng:
        eng.comm_init_host(0, 2, lambda buf: None)
        with pytest.raises(d.DccError) as e:
            eng.mvcc_access_epoch(b, ts, rc, pos)
        assert e.value.code == _abi.DCC_ENOTSUP
        with pytest.raises(d.DccError) as e:
            eng.mvcc_finish(b, ts, rc, pos, leave)
        assert e.value.code == _abi.DCC_ENOTSUP
        assert np.all(rc == WD_RUN) and np.all(pos == 0)
        eng.comm_destroy()
