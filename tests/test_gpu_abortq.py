"""GPU parity of the device-resident abort queue (abortq.hip, dcc_abortq_*,
Engine.abort_queue) with the reference's restatement (abortq_ref.py),
bit-exact.  A device queue and a reference queue are driven in lockstep; every
output array of a pop sits inside a sentinel-filled one: whatever lies before
the bases and behind base + count must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RD, SCAN, WR, XP, _abi
from abortq_ref import (BACKOFF_EXP, BACKOFF_NONE, BACKOFF_REFERENCE, EINVAL, ERANGE, OK, AbortQueue,
                        pop_alg_bytes, push_alg_bytes)
from helpers import make_batch, random_batch

pytestmark = pytest.mark.gpu

GUARD = 37  # elements behind every output array (odd: the arrays end unaligned)
DTYPES = {"offsets": np.uint32, "keys": np.uint64, "acctype": np.uint8, "src": np.uint32, "cnt": np.uint32,
          "due": np.uint64}
SIGNED = {np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}
POLICIES = (BACKOFF_REFERENCE, BACKOFF_NONE, BACKOFF_EXP)
FAR = 1 << 62  # a clock at which everything parked with small penalties is due


def sentinel(dtype, k):
    return np.frombuffer(bytes([0xA5]) * (k * np.dtype(dtype).itemsize), dtype).copy()


def to_dev(a):
    """numpy -> cuda:0, unsigned arrays as the signed dtype of the same width."""
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(SIGNED.get(a.dtype.type, a.dtype.type))).to("cuda:0")
    torch.cuda.synchronize()  # the engine runs on a stream of its own
    return t


def to_host(t, dtype):
    return t.cpu().numpy().view(dtype) if not isinstance(t, np.ndarray) else t


def batch_to_dev(b):
    return d.EpochBatch(to_dev(b.offsets), to_dev(b.keys), to_dev(b.acctype), None, None, None, dict(b.meta))


class Pair:
    """A device queue and its reference, driven in lockstep."""

    def __init__(self, eng, cap_txn, cap_nnz, pen, pen_max, policy, flags=0):
        self.eng = eng
        self.g = eng.abort_queue(cap_txn, cap_nnz, pen, pen_max, policy, flags)
        self.r = AbortQueue(cap_txn, cap_nnz, pen, pen_max, policy)

    def close(self):
        self.g.close()

    def push(self, b, rc, now, want=RC_ABORT, src=None, cnt=None, dev=False, run_batch=None):
        rc = np.asarray(rc, np.uint8)
        src = None if src is None else np.asarray(src, np.uint32)
        cnt = None if cnt is None else np.asarray(cnt, np.uint32)
        before = self.r.size()
        code, n, m = self.r.push(b, rc, want, src, cnt, now)
        bb = run_batch if run_batch is not None else b
        args = (batch_to_dev(bb), to_dev(rc), now, want, to_dev(src), to_dev(cnt)) if dev else \
            (bb, rc, now, want, src, cnt)
        if code != OK:
            with pytest.raises(d.DccError) as e:
                self.g.push(*args)
            assert e.value.code == (_abi.DCC_ERANGE if code == ERANGE else _abi.DCC_EINVAL)
            if code == ERANGE:
                assert e.value.needed == (n, m)
            assert self.g.size() == before
        else:
            gn, gm, st = self.g.push(*args)
            assert (gn, gm) == (n, m)
            assert st["n_commit"] == n and st["n_abort"] == b.n_txn - n
            assert st["alg_bytes"] == push_alg_bytes(b.n_txn, n, m)
        assert self.g.size() == self.r.size()
        return code, n, m

    def pop(self, now, dev=False, txn_base=0, nnz_base=0, cap_txn=None, cap_nnz=None, want_cnt=True,
            want_due=True):
        qn, qm = self.r.size()
        ct = qn if cap_txn is None else cap_txn
        cm = qm if cap_nnz is None else cap_nnz
        code, n, m, rows = self.r.pop(now, txn_base, nnz_base, ct, cm)
        lens = {"offsets": txn_base + ct + 1, "keys": nnz_base + cm, "acctype": nnz_base + cm,
                "src": txn_base + ct}
        if want_cnt:
            lens["cnt"] = txn_base + ct
        if want_due:
            lens["due"] = txn_base + ct
        big = {k: sentinel(DTYPES[k], v + GUARD) for k, v in lens.items()}
        arr = {k: (to_dev(v) if dev else v) for k, v in big.items()}
        view = {k: arr[k][:lens[k]] for k in arr}
        out = d.EpochBatch(view["offsets"], view["keys"], view["acctype"],
                           meta={k: view[k] for k in ("src", "cnt", "due") if k in view})
        expect = {k: v.copy() for k, v in big.items()}
        kw = dict(out=out, txn_base=txn_base, nnz_base=nnz_base, want_cnt=want_cnt, want_due=want_due)
        if code == ERANGE:
            with pytest.raises(d.DccError) as e:
                self.g.pop(now, **kw)
            assert e.value.code == _abi.DCC_ERANGE and e.value.needed == (n, m)
            assert self.g.size() == (qn, qm)
        else:
            got, st = self.g.pop(now, **kw)
            assert got.n_txn == txn_base + n and got.nnz == nnz_base + m
            assert set(got.meta) == {k for k in ("src", "cnt", "due") if k in view}
            assert all(v.shape[0] == txn_base + n for v in got.meta.values())
            assert st["n_commit"] == n and st["n_abort"] == qn - n
            assert st["alg_bytes"] == pop_alg_bytes(qn, qm, n, m)
            for k in expect:
                base = nnz_base if k in ("keys", "acctype") else txn_base
                expect[k][base:base + rows[k].size] = rows[k]
        for k in expect:
            got_k = to_host(arr[k], DTYPES[k])
            bad = np.nonzero(got_k != expect[k])[0]
            assert bad.size == 0, f"{k}: differs at {bad[:8]} (gpu {got_k[bad[:8]]} ref {expect[k][bad[:8]]})"
        assert self.g.size() == self.r.size()
        return code, n, m, rows


@pytest.fixture
def pair(engine):
    made = []

    def make(cap_txn=4096, cap_nnz=65536, pen=10, pen_max=1000, policy=BACKOFF_EXP, eng=None, flags=0):
        p = Pair(eng or engine, cap_txn, cap_nnz, pen, pen_max, policy, flags)
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


def seam_batch(rng, n):
    """Ragged lengths, all four access types, empty txns at the tile ends
    (indices 255, 256, 511, 512) and one 5,000-access txn."""
    lens = rng.integers(0, 9, size=n)
    for i in (0, 255, 256, 511, 512):
        if i < n:
            lens[i] = 0
    if n > 3:
        lens[n // 2] = 5000
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(off[-1])
    return d.EpochBatch(off, rng.integers(0, 1 << 62, size=nnz).astype(np.uint64),
                        rng.choice(np.array([RD, WR, XP, SCAN], np.uint8), size=nnz))


@pytest.mark.parametrize("n_txn", [0, 1, 255, 256, 257, 513])
def test_push_seams(pair, n_txn):
    rng = np.random.default_rng(100 + n_txn)
    b = seam_batch(rng, n_txn)
    rc = rng.choice(np.array([RC_RCOK, RC_ABORT], np.uint8), size=n_txn)
    if n_txn > 3:
        rc[n_txn // 2] = RC_ABORT  # the long txn is parked
    for dev in (False, True):
        p = pair()
        assert p.push(b, rc, 3, want=RC_ABORT, dev=dev)[0] == OK
        assert p.push(b, rc, 4, want=RC_RCOK, dev=dev)[0] == OK
        assert p.push(b, rc, 5, want=77, dev=dev)[:2] == (OK, 0)  # a byte nobody has
        assert p.push(b, np.full(n_txn, RC_ABORT, np.uint8), 6, dev=dev)[0] == OK
        p.pop(FAR, dev=dev, txn_base=2, nnz_base=3)
        assert p.g.size() == (0, 0)
        p.close()


def test_pop_nothing_everything_and_the_strict_edge(pair):
    rng = np.random.default_rng(7)
    b = random_batch(rng, 700, 12, 1 << 20, unique=False)
    rc = np.full(b.n_txn, RC_ABORT, np.uint8)
    for dev in (False, True):
        p = pair(policy=BACKOFF_NONE, pen=10)
        p.push(b, rc[:b.n_txn], 5, dev=dev)       # due 15
        p.push(b, rc, 6, dev=dev)                 # due 16
        assert p.pop(0, dev=dev)[1] == 0          # before anything was pushed
        assert p.pop(15, dev=dev, txn_base=1, nnz_base=1)[1] == 0   # 15 < 15 is false
        assert p.pop(16, dev=dev)[1] == b.n_txn   # exactly the entries with due == now - 1
        assert p.pop(16, dev=dev)[1] == 0         # due == now stays
        assert p.pop(17, dev=dev)[1] == b.n_txn   # and leaves at now + 1
        assert p.pop(FAR, dev=dev)[1] == 0        # an empty queue
        p.push(b, rc, 1, dev=dev)
        assert p.pop(FAR, dev=dev)[1] == b.n_txn  # everything due
        p.close()


def test_release_order_is_not_pool_order(pair):
    rng = np.random.default_rng(11)
    b = random_batch(rng, 300, 6, 1 << 20, unique=False)
    rc = np.full(b.n_txn, RC_ABORT, np.uint8)
    for dev in (False, True):
        p = pair(policy=BACKOFF_EXP, pen=10, pen_max=1000)
        p.push(b, rc, 0, cnt=np.full(b.n_txn, 2, np.uint32), dev=dev)   # cnt 3: due 80
        p.push(b, rc, 10, cnt=np.zeros(b.n_txn, np.uint32), dev=dev)    # cnt 1: due 30
        p.push(b, rc, 60, src=np.arange(1000, 1000 + b.n_txn), dev=dev)  # cnt 1: due 80, ties keep push order
        _, n, _, rows = p.pop(81, dev=dev)
        assert n == 3 * b.n_txn and rows["due"][0] == 30 and rows["due"][-1] == 80
        assert list(rows["src"][b.n_txn:b.n_txn + 2]) == [0, 1] and rows["src"][-1] == 1000 + b.n_txn - 1
        p.close()
    # interleaved dues within one push, part of them released: the kept ones stay in push order
    p = pair(policy=BACKOFF_EXP, pen=1, pen_max=1 << 40)
    cnt = rng.integers(0, 20, size=b.n_txn).astype(np.uint32)
    p.push(b, rc, 0, cnt=cnt, dev=True)
    p.push(b, rc, 100, cnt=cnt[::-1].copy(), dev=True)
    for now in (1 << 6, 1 << 12, 1 << 12, 1 << 19, FAR):
        p.pop(now, dev=True)
    assert p.g.size() == (0, 0)


@pytest.mark.parametrize("n_due", [2047, 2048, 2049])
@pytest.mark.parametrize("flags", [0, _abi.ABORTQ_SORT_FULL])
def test_sort_tile_seams(pair, n_due, flags):
    """Due counts around the radix sort's small tile, the pool exactly that long
    and longer, dues in a scrambled order."""
    rng = np.random.default_rng(n_due)
    b = random_batch(rng, n_due + 300, 3, 1 << 20, unique=False)
    rc = np.full(b.n_txn, RC_ABORT, np.uint8)
    cnt = rng.integers(0, 9, size=b.n_txn).astype(np.uint32)   # due = 2 ** (cnt + 1): 2 .. 512
    cnt[n_due:] = 20                                           # the 300 that stay
    p = pair(policy=BACKOFF_EXP, pen=1, pen_max=1 << 40, flags=flags)
    p.push(b, rc, 0, cnt=cnt, dev=True)
    assert p.pop(1000, dev=True)[1] == n_due
    q = pair(policy=BACKOFF_EXP, pen=1, pen_max=1 << 40, flags=flags)
    sub = d.EpochBatch(b.offsets[:n_due + 1], b.keys[:int(b.offsets[n_due])], b.acctype[:int(b.offsets[n_due])])
    q.push(sub, rc, 0, cnt=cnt[:n_due], dev=True)
    assert q.pop(1000, dev=True)[1] == n_due and q.g.size() == (0, 0)


def test_chaining_in_front_of_fresh_txns(pair):
    """pop into the front of the next epoch behind odd bases, the fresh txns
    copied in behind the counts: one CSR."""
    import torch
    rng = np.random.default_rng(13)
    b = seam_batch(rng, 600)
    fresh = random_batch(rng, 100, 5, 1 << 20, unique=False)
    p = pair()
    p.push(b, np.full(b.n_txn, RC_ABORT, np.uint8), 0, dev=True)
    for nnz_base in (1, 3):  # the access-type stores start unaligned
        p.pop(0, dev=True, txn_base=5, nnz_base=nnz_base)
    qn, qm = p.g.size()
    out = d.EpochBatch(torch.zeros(qn + fresh.n_txn + 1, dtype=torch.int32, device="cuda:0"),
                       torch.zeros(qm + fresh.nnz, dtype=torch.int64, device="cuda:0"),
                       torch.zeros(qm + fresh.nnz, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    got, _ = p.g.pop(FAR, out=out)
    _, n, m, rows = p.r.pop(FAR)
    assert (got.n_txn, got.nnz) == (n, m) == (qn, qm)
    df = batch_to_dev(fresh)
    out.offsets[n + 1:] = df.offsets[1:] + m
    out.keys[m:] = df.keys
    out.acctype[m:] = df.acctype
    off = to_host(out.offsets, np.uint32)
    assert np.array_equal(off, np.concatenate([rows["offsets"], fresh.offsets[1:] + np.uint32(m)]))
    assert np.array_equal(to_host(out.keys, np.uint64), np.concatenate([rows["keys"], fresh.keys]))
    assert np.array_equal(to_host(out.acctype, np.uint8), np.concatenate([rows["acctype"], fresh.acctype]))
    assert np.array_equal(to_host(got.meta["src"], np.uint32), rows["src"])


def test_optional_outputs_and_allocating_pop(pair):
    rng = np.random.default_rng(17)
    b = random_batch(rng, 500, 8, 1 << 20, unique=False)
    rc = np.full(b.n_txn, RC_ABORT, np.uint8)
    for dev in (False, True):
        p = pair()
        p.push(b, rc, 0, dev=dev)
        p.push(b, rc, 0, dev=dev)
        p.push(b, rc, 50, dev=dev)
        p.pop(21, dev=dev, want_cnt=False, want_due=False, cap_txn=b.n_txn * 2 + 3)   # both NULL
        # out=None: arrays of the queue's size, numpy or torch
        got, st = p.g.pop(FAR, device="cuda:0" if dev else None)
        _, n, m, rows = p.r.pop(FAR)
        assert dev == got.on_device and (got.n_txn, got.nnz) == (n, m) == (b.n_txn, b.nnz)
        for k in ("offsets", "keys", "acctype"):
            assert np.array_equal(to_host(getattr(got, k), DTYPES[k]), rows[k])
        for k in ("src", "cnt", "due"):
            assert np.array_equal(to_host(got.meta[k], DTYPES[k]), rows[k])
        p.close()


def test_src_and_cnt_compose_over_retries(pair):
    rng = np.random.default_rng(19)
    b = random_batch(rng, 400, 8, 1 << 20, unique=False)
    p = pair(policy=BACKOFF_EXP, pen=1, pen_max=1 << 30)
    cur, src, cnt = b, np.arange(5000, 5000 + b.n_txn, dtype=np.uint32), None
    for r in range(3):
        rc = np.where(rng.random(cur.n_txn) < 0.7, RC_ABORT, RC_RCOK).astype(np.uint8)
        rc[0] = RC_ABORT
        p.push(cur, rc, r * 100, src=src, cnt=cnt, dev=r != 1)
        _, n, _, rows = p.pop(FAR, dev=r != 1)
        assert np.all(rows["cnt"] == r + 1) and np.all(rows["src"] >= 5000)
        assert np.all(rows["due"] == r * 100 + (2 << r))
        j = int(rows["src"][0]) - 5000   # the txn is the one it was at the start
        assert np.array_equal(rows["keys"][:int(rows["offsets"][1])], b.keys[b.offsets[j]:b.offsets[j + 1]])
        cur, src, cnt = d.EpochBatch(rows["offsets"], rows["keys"], rows["acctype"]), rows["src"], rows["cnt"]
    assert cur.n_txn > 0


@pytest.mark.parametrize("dev", [True, False])
def test_erange(pair, dev):
    rng = np.random.default_rng(23)
    b = random_batch(rng, 600, 8, 1 << 20, unique=False)
    rc = np.where(rng.random(b.n_txn) < 0.5, RC_ABORT, RC_RCOK).astype(np.uint8)
    lens = np.diff(b.offsets.astype(np.int64))
    n, m = int((rc == RC_ABORT).sum()), int(lens[rc == RC_ABORT].sum())
    # push: txn room, access room; then exactly enough
    p = pair(cap_txn=2 * n - 1, cap_nnz=2 * m)
    assert p.push(b, rc, 0, dev=dev)[0] == OK
    assert p.push(b, rc, 1, dev=dev) == (ERANGE, n, m)
    p.pop(FAR, dev=dev)  # the parked half is intact
    p = pair(cap_txn=2 * n, cap_nnz=2 * m - 1)
    assert p.push(b, rc, 0, dev=dev)[0] == OK
    assert p.push(b, rc, 1, dev=dev) == (ERANGE, n, m)
    p.pop(FAR, dev=dev)
    p = pair(cap_txn=2 * n, cap_nnz=2 * m)
    assert p.push(b, rc, 0, dev=dev)[0] == OK and p.push(b, rc, 1, dev=dev)[0] == OK
    # pop: cap_txn, cap_nnz; the next call with room gives the reference's result
    assert p.pop(FAR, dev=dev, cap_txn=2 * n - 1, txn_base=3, nnz_base=5)[0] == ERANGE
    assert p.pop(FAR, dev=dev, cap_nnz=2 * m - 1, txn_base=3, nnz_base=5)[0] == ERANGE
    # pushed at 0 and 1 under EXP 10: due 20 and 21; a partial release that does not fit, then fits
    assert p.pop(21, dev=dev, cap_txn=n - 1)[:3] == (ERANGE, n, m)
    assert p.pop(21, dev=dev, cap_txn=n, cap_nnz=m, txn_base=3, nnz_base=5)[:3] == (OK, n, m)
    assert p.pop(FAR, dev=dev)[:3] == (OK, n, m)


def test_erange_nnz_base_near_2_32(pair):
    """nnz_base + accesses past 2^32 - 1, straight through the C ABI: nothing is
    written, so the arrays need not reach the base."""
    rng = np.random.default_rng(29)
    b = random_batch(rng, 300, 8, 1 << 20, unique=False)
    rc = np.full(b.n_txn, RC_ABORT, np.uint8)
    p = pair()
    p.push(b, rc, 0)
    lib, ns, ms = _abi.lib, C.c_uint64(0), C.c_uint64(0)
    big = {k: sentinel(DTYPES[k], 16) for k in ("offsets", "keys", "acctype")}
    for base, flags in ((0xFFFFFFFF - b.nnz + 1, 0), (1 << 32, 0)):
        so = _abi.SelectOut(b.n_txn, b.nnz, 0, base, big["offsets"].ctypes.data, big["keys"].ctypes.data,
                            big["acctype"].ctypes.data, None, None, None, None)
        assert lib.dcc_abortq_pop(p.g._q, FAR, C.byref(so), None, None, flags, C.byref(ns), C.byref(ms),
                                  None) == _abi.DCC_ERANGE
        if base < (1 << 32):
            assert (ns.value, ms.value) == (b.n_txn, b.nnz)
        assert p.g.size() == (b.n_txn, b.nnz)
    for k, v in big.items():
        assert np.array_equal(v, sentinel(DTYPES[k], 16))
    # null out / null rc
    assert lib.dcc_abortq_pop(p.g._q, FAR, None, None, None, 0, None, None, None) == _abi.DCC_EINVAL
    cb = b.to_c()
    assert lib.dcc_abortq_push(p.g._q, C.byref(cb), None, RC_ABORT, None, None, 0, None, None,
                               None) == _abi.DCC_EINVAL
    assert p.pop(FAR, dev=True, nnz_base=7)[:3] == (OK, b.n_txn, b.nnz)


def test_malformed_offsets(pair):
    good = make_batch([[(1, RD)], [(2, WR), (3, RD)], [(4, RD)]])
    rc = np.array([2, 2, 2], np.uint8)
    p = pair()
    p.push(good, rc, 0)
    for bad_off in ([0, 4, 3, 4], [1, 1, 3, 4], [0, 1, 3, 5]):
        bad = d.EpochBatch(np.array(bad_off, np.uint32), good.keys, good.acctype)
        for dev in (False, True):
            assert p.push(bad, rc, 1, dev=dev)[0] == EINVAL
    p.push(good, rc, 2, dev=True)
    assert p.pop(FAR, dev=True)[1] == 6


@pytest.mark.parametrize("policy", POLICIES)
def test_random_cycles(pair, policy):
    rng = np.random.default_rng(31 + policy)
    p = pair(cap_txn=3000, cap_nnz=30000, pen=3, pen_max=40 if policy == BACKOFF_EXP else 5, policy=policy)
    now = 0
    for cycle in range(12):
        dev = bool(cycle & 1)
        n = int(rng.integers(0, 601))
        b = random_batch(rng, n, 8, 1 << 20, unique=False)
        rc = rng.choice(np.array([RC_RCOK, RC_ABORT, 3], np.uint8), size=n)
        cnt = rng.integers(0, 6, size=n).astype(np.uint32)
        src = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        p.push(b, rc, now, src=src, cnt=cnt, dev=dev)   # may be ERANGE: both sides agree and go on
        now += int(rng.choice([0, 0, 1, 3, 9, 30]))
        p.pop(now, dev=dev, txn_base=cycle, nnz_base=cycle)
    p.g.clear()
    p.r.clear()
    assert p.g.size() == (0, 0)
    b = random_batch(rng, 300, 8, 1 << 20, unique=False)
    p.push(b, np.full(300, RC_ABORT, np.uint8), now, dev=True)
    assert p.pop(FAR, dev=True)[1] == 300


def test_compact_host_batch(engine, pair):
    rng = np.random.default_rng(37)
    b = random_batch(rng, 900, 12, 1 << 20, unique=False)
    rc = np.where(rng.random(b.n_txn) < 0.5, RC_ABORT, RC_RCOK).astype(np.uint8)
    c = engine.compact_host_batch(b)
    assert c.keys.dtype == np.uint32 and c.meta.get("acctype_2bit")
    p = pair()
    p.push(b, rc, 0, run_batch=c)
    p.push(b, rc, 0, run_batch=c, dev=True)
    p.pop(FAR)


@pytest.mark.parametrize("shards", [1, 2])
def test_multi_context_runs_on_rank0(engine, shards):
    rng = np.random.default_rng(41)
    b = random_batch(rng, 900, 12, 1 << 20, unique=False)
    rc = np.where(rng.random(b.n_txn) < 0.5, RC_ABORT, RC_RCOK).astype(np.uint8)
    with d.Engine(devices=[0] * shards) as m:
        p = Pair(m, 4096, 65536, 10, 1000, BACKOFF_EXP)
        for dev in (False, True):
            p.push(b, rc, 0, dev=dev)
            p.push(b, rc, 7, cnt=np.full(b.n_txn, 1, np.uint32), dev=dev)
            p.pop(30, dev=dev)
            p.pop(FAR, dev=dev)
        p.close()


def test_create_destroy_and_queue_alive_at_close(engine):
    rng = np.random.default_rng(43)
    b = random_batch(rng, 300, 8, 1 << 20, unique=False)
    rc = np.full(b.n_txn, RC_ABORT, np.uint8)
    eng = d.Engine(0)
    for i in range(20):
        q = eng.abort_queue(1000 + i, 10000, 1, 1, BACKOFF_NONE)
        q.push(b, rc, 0)
        assert q.size() == (b.n_txn, b.nnz)
        q.close()
        q.close()  # idempotent
    with pytest.raises(d.DccError) as e:
        eng.abort_queue(1 << 32, 10, 1, 1)
    assert e.value.code == _abi.DCC_ERANGE
    with pytest.raises(d.DccError):
        eng.abort_queue(10, 10, 1, 1, policy=9)
    left = eng.abort_queue(1000, 10000, 1, 1)
    left.push(b, rc, 0)
    eng.close()   # frees the queue with the context
    left.close()  # and closing it afterwards touches nothing
    with pytest.raises(ValueError):
        left.size()


def test_reserve_and_repeat(engine, pair):
    rng = np.random.default_rng(47)
    b = random_batch(rng, 3000, 12, 1 << 20, unique=False)
    rc = np.where(rng.random(b.n_txn) < 0.5, RC_ABORT, RC_RCOK).astype(np.uint8)
    engine.reserve(b.n_txn, b.nnz)
    p = pair(cap_txn=8192, cap_nnz=1 << 17)
    db, drc = batch_to_dev(b), to_dev(rc)
    outs = []
    for it in range(3):  # the first call warms up
        p.g.push(db, drc, 0)
        p.g.push(db, drc, 5, cnt=to_dev(np.full(b.n_txn, 1, np.uint32)))
        got, _ = p.g.pop(1 << 20, device="cuda:0")
        outs.append([to_host(a, t) for a, t in ((got.offsets, np.uint32), (got.keys, np.uint64),
                                                (got.acctype, np.uint8), (got.meta["src"], np.uint32),
                                                (got.meta["cnt"], np.uint32), (got.meta["due"], np.uint64))])
        assert p.g.size() == (0, 0)
    assert all(np.array_equal(x, y) for x, y in zip(outs[0], outs[1]))
    assert all(np.array_equal(x, y) for x, y in zip(outs[1], outs[2]))
    p.push(b, rc, 0, dev=True)
    p.pop(FAR, dev=True)


def test_closed_loop_nowait(engine):
    """Four NO_WAIT epochs of 2,000 fresh txns at theta 0.9, the clock the epoch
    index: epoch e = pop(e) ++ fresh(e), its aborted txns parked with their
    src / cnt.  The device queue on device batches against abortq_ref on host
    batches: the same rc per epoch."""
    import torch
    F, E = 2000, 4
    fresh = [d.gen_ycsb(n_txn=F, zipf_theta=0.9, table_size=1 << 16, seed=900 + e) for e in range(E)]
    gq = engine.abort_queue(E * F, E * F * 16, 1, 4, BACKOFF_EXP)
    rq = AbortQueue(E * F, E * F * 16, 1, 4, BACKOFF_EXP)
    parked = 0
    for e in range(E):
        nf = fresh[e]
        ids = np.arange(e * F, (e + 1) * F, dtype=np.uint32)
        # host: the reference queue
        _, n0, m0, r = rq.pop(e)
        h_cur = d.EpochBatch(np.concatenate([r["offsets"], nf.offsets[1:] + np.uint32(m0)]).astype(np.uint32),
                             np.concatenate([r["keys"], nf.keys]), np.concatenate([r["acctype"], nf.acctype]))
        h_src = np.concatenate([r["src"], ids])
        h_cnt = np.concatenate([r["cnt"], np.zeros(F, np.uint32)])
        # device: pop into the front of the epoch's arrays, the fresh txns behind
        qn, qm = gq.size()
        out = d.EpochBatch(torch.empty(qn + F + 1, dtype=torch.int32, device="cuda:0"),
                           torch.empty(qm + nf.nnz, dtype=torch.int64, device="cuda:0"),
                           torch.empty(qm + nf.nnz, dtype=torch.uint8, device="cuda:0"),
                           meta={"src": torch.empty(qn + F, dtype=torch.int32, device="cuda:0"),
                                 "cnt": torch.zeros(qn + F, dtype=torch.int32, device="cuda:0")})
        torch.cuda.synchronize()
        got, st = gq.pop(e, out=out, want_due=False)
        assert (got.n_txn, got.nnz) == (n0, m0)
        dn = batch_to_dev(nf)
        out.offsets[n0 + 1:n0 + 1 + F] = dn.offsets[1:] + m0
        out.keys[m0:m0 + nf.nnz] = dn.keys
        out.acctype[m0:m0 + nf.nnz] = dn.acctype
        out.meta["src"][n0:n0 + F] = to_dev(ids)
        out.meta["cnt"][n0:n0 + F] = 0
        torch.cuda.synchronize()
        cur = d.EpochBatch(out.offsets[:n0 + F + 1], out.keys[:m0 + nf.nnz], out.acctype[:m0 + nf.nnz])
        d_src, d_cnt = out.meta["src"][:n0 + F], out.meta["cnt"][:n0 + F]
        assert np.array_equal(to_host(d_src, np.uint32), h_src) and np.array_equal(to_host(d_cnt, np.uint32), h_cnt)
        rc, _, _ = engine.nowait_lock_epoch(cur, want_conflict=False)
        hrc, _, _ = engine.nowait_lock_epoch(h_cur, want_conflict=False)
        assert np.array_equal(rc.cpu().numpy(), hrc), f"epoch {e}: rc differs between the two paths"
        assert 0 < int((hrc == RC_ABORT).sum()) < hrc.size
        code, n, m = rq.push(h_cur, hrc, RC_ABORT, h_src, h_cnt, e)
        assert code == OK and gq.push(cur, rc, e, src=d_src, cnt=d_cnt)[:2] == (n, m)
        assert gq.size() == rq.size()
        parked += n
    assert parked > 0 and any(x[3] > 1 for x in rq.heap), "no txn was retried and aborted again"
    gq.close()
