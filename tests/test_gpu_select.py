"""GPU parity of dcc_batch_select (select.hip, Engine.select_batch) with its
numpy restatement (select_ref.py), bit-exact.  Every output array sits inside
a sentinel-filled one: whatever lies before the bases and behind base + count
must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RC_WAIT, RD, WR, _abi
from helpers import make_batch, random_batch
from nowait_ref import replay
from select_ref import ERANGE, OK, select

pytestmark = pytest.mark.gpu

GUARD = 37  # elements behind every output array (odd: the arrays end unaligned)
TILE = 256  # txns per workgroup tile of select.hip
DTYPES = {"offsets": np.uint32, "keys": np.uint64, "acctype": np.uint8, "start_tn": np.uint64,
          "finish_tn": np.uint64, "order": np.uint64, "src": np.uint32}
SIGNED = {np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}
PER_TXN = ("start_tn", "finish_tn", "order")


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
    return d.EpochBatch(to_dev(b.offsets), to_dev(b.keys), to_dev(b.acctype), to_dev(b.start_tn),
                        to_dev(b.finish_tn), to_dev(b.order), dict(b.meta))


def run(eng, b, rc, want, dev=False, src_in=None, txn_base=0, nnz_base=0, cap_txn=None, cap_nnz=None,
        tn_out=True, run_batch=None):
    """Select from `b` (or run_batch, another form of the same epoch) into
    guarded arrays and compare everything with select_ref.  Returns the
    reference's (code, n_sel, nnz_sel, rows)."""
    rc = np.asarray(rc, np.uint8)
    ref = select(b, rc, want, src_in, txn_base, nnz_base, cap_txn, cap_nnz)
    code, ns, ms, rows = ref
    ct = b.n_txn if cap_txn is None else cap_txn
    cm = b.nnz if cap_nnz is None else cap_nnz
    lens = {"offsets": txn_base + ct + 1, "keys": nnz_base + cm, "acctype": nnz_base + cm, "src": txn_base + ct}
    if tn_out:
        lens.update({k: txn_base + ct for k in PER_TXN})
    big = {k: sentinel(DTYPES[k], v + GUARD) for k, v in lens.items()}
    arr = {k: (to_dev(v) if dev else v) for k, v in big.items()}
    view = {k: arr[k][:lens[k]] for k in arr}
    out = d.EpochBatch(view["offsets"], view["keys"], view["acctype"], view.get("start_tn"),
                       view.get("finish_tn"), view.get("order"), {"src": view["src"]})
    bb = run_batch if run_batch is not None else b
    src_x = None if src_in is None else np.asarray(src_in, np.uint32)
    rc_x = rc
    if dev:
        bb, rc_x, src_x = batch_to_dev(bb), to_dev(rc), to_dev(src_x)
    expect = {k: v.copy() for k, v in big.items()}
    if code == ERANGE:
        with pytest.raises(d.DccError) as e:
            eng.select_batch(bb, rc_x, want, src=src_x, out=out, txn_base=txn_base, nnz_base=nnz_base)
        assert e.value.code == _abi.DCC_ERANGE and e.value.needed == (ns, ms)
    else:
        sel, src, st = eng.select_batch(bb, rc_x, want, src=src_x, out=out, txn_base=txn_base,
                                        nnz_base=nnz_base)
        assert sel.n_txn == txn_base + ns and sel.nnz == nnz_base + ms and src.shape[0] == txn_base + ns
        assert st["n_commit"] == ns and st["n_abort"] == b.n_txn - ns
        carried = 1 + sum(1 for k in PER_TXN if tn_out and getattr(b, k) is not None)
        assert st["alg_bytes"] == d.select_alg_bytes(b.n_txn, ns, ms, carried if b.n_txn else 0)
        for k in expect:
            if k in rows:
                base = nnz_base if k in ("keys", "acctype") else txn_base
                expect[k][base:base + rows[k].size] = rows[k]
    for k in expect:
        got = to_host(arr[k], DTYPES[k])
        bad = np.nonzero(got != expect[k])[0]
        assert bad.size == 0, f"{k}: differs at {bad[:8]} (gpu {got[bad[:8]]} ref {expect[k][bad[:8]]})"
    return ref


PATTERNS = ("none", "all", "alternating", "last", "first", "random")


def pattern_rc(name, n, rng):
    rc = np.zeros(n, np.uint8)
    if name == "all":
        rc[:] = RC_ABORT
    elif name == "alternating":
        rc[::2] = RC_ABORT
    elif name == "last":
        rc[n - 1:] = RC_ABORT
    elif name == "first":
        rc[:1] = RC_ABORT
    elif name == "random":
        rc[rng.random(n) < 0.5] = RC_ABORT
    return rc


@pytest.mark.parametrize("n_txn", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_seams(engine, n_txn):
    rng = np.random.default_rng(1000 + n_txn)
    b = random_batch(rng, n_txn, 12, 1 << 20, unique=False)
    for i, name in enumerate(PATTERNS):
        rc = pattern_rc(name, n_txn, rng)
        run(engine, b, rc, RC_ABORT, dev=True)
        run(engine, b, rc, RC_ABORT, dev=False, txn_base=i, nnz_base=i)


def long_batch():
    """Zero-length txns, txns of 1, 64, 65, 300 and 5,000 accesses, and runs of
    600 unselected txns: rc 2 selects, rc 0 does not."""
    lens, rc = [], []

    def add(ls, r):
        lens.extend(ls)
        rc.extend([r] * len(ls))

    add([3] * 10 + [5000] + [0] * 5 + [1, 64, 65, 300], 2)
    add([2] * 600, 0)
    add([0, 5000, 7, 0, 0, 300], 2)
    add([1] * 300 + [5000] + [0] * 299, 0)  # an unselected long txn too
    add([300, 65, 0, 64, 1, 5000], 2)
    add([4] * 100, 0)
    add([9], 2)
    lens = np.asarray(lens, np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(off[-1])
    rng = np.random.default_rng(3)
    b = d.EpochBatch(off, rng.integers(0, 1 << 62, size=nnz).astype(np.uint64),
                     rng.integers(0, 4, size=nnz).astype(np.uint8))
    return b, np.asarray(rc, np.uint8)


def test_long_and_empty_txns(engine):
    b, rc = long_batch()
    lens = np.diff(b.offsets.astype(np.int64))
    per_tile = np.add.reduceat(np.where(rc == 2, lens, 0), np.arange(0, b.n_txn, TILE))
    empty = np.nonzero(per_tile == 0)[0]
    assert empty.size and per_tile[:empty[0]].sum() > 0 and per_tile[empty[0]:].sum() > 0, \
        "no tile with an empty output range between two others"
    assert per_tile.max() > 5000  # a long txn shares its tile's output range with its neighbours
    for dev in (True, False):
        for nnz_base in (0, 1, 2, 3):  # every alignment of the access-type output
            run(engine, b, rc, 2, dev=dev, nnz_base=nnz_base, txn_base=nnz_base)
        run(engine, b, rc, 0, dev=dev)  # the unselected side, its long txn included


def test_other_want_values(engine):
    rng = np.random.default_rng(17)
    b = random_batch(rng, 3000, 12, 1 << 20, unique=False)
    rc = rng.choice(np.array([0, 2, 3, 7], np.uint8), size=b.n_txn)
    for want in (RC_RCOK, RC_ABORT, RC_WAIT, 7, 5, 255):
        code, ns, _, _ = run(engine, b, rc, want, dev=True)
        assert code == OK and ns == int((rc == want).sum())
    run(engine, b, rc, RC_WAIT, dev=False)


def test_bases_and_chaining(engine):
    """Aborted into [0, ..), committed behind them in the same arrays: one CSR."""
    import torch
    rng = np.random.default_rng(23)
    b = random_batch(rng, 3000, 12, 1 << 20, unique=False)
    rc = np.where(rng.random(b.n_txn) < 0.4, RC_ABORT, RC_RCOK).astype(np.uint8)
    db, drc = batch_to_dev(b), to_dev(rc)
    out = d.EpochBatch(torch.empty(b.n_txn + 1, dtype=torch.int32, device="cuda:0"),
                       torch.empty(b.nnz, dtype=torch.int64, device="cuda:0"),
                       torch.empty(b.nnz, dtype=torch.uint8, device="cuda:0"))
    s0, _, _ = engine.select_batch(db, drc, RC_ABORT, out=out)
    n0, m0 = s0.n_txn, s0.nnz
    s1, src, _ = engine.select_batch(db, drc, RC_RCOK, out=out, txn_base=n0, nnz_base=m0)
    assert s1.n_txn == b.n_txn and s1.nnz == b.nnz  # every txn is in one of the two
    _, _, _, r0 = select(b, rc, RC_ABORT)
    _, _, _, r1 = select(b, rc, RC_RCOK, txn_base=n0, nnz_base=m0)
    off = to_host(s1.offsets, np.uint32)
    assert off[0] == 0 and np.all(np.diff(off.astype(np.int64)) >= 0) and off[-1] == b.nnz
    assert np.array_equal(off, np.concatenate([r0["offsets"], r1["offsets"][1:]]))
    assert np.array_equal(to_host(s1.keys, np.uint64), np.concatenate([r0["keys"], r1["keys"]]))
    assert np.array_equal(to_host(s1.acctype, np.uint8), np.concatenate([r0["acctype"], r1["acctype"]]))
    assert np.array_equal(to_host(src, np.uint32), np.concatenate([r0["src"], r1["src"]]))


def tn_batch(rng, n):
    b = random_batch(rng, n, 12, 1 << 20, unique=False)
    b.start_tn = rng.integers(0, 1 << 30, size=n).astype(np.uint64)
    b.finish_tn = b.start_tn + rng.integers(0, 1 << 10, size=n).astype(np.uint64)
    b.order = rng.permutation(n).astype(np.uint64) << np.uint64(33)
    return b


def test_per_txn_arrays_and_src(engine):
    rng = np.random.default_rng(29)
    b = tn_batch(rng, 2500)
    rc = pattern_rc("random", b.n_txn, rng)
    for dev in (True, False):
        run(engine, b, rc, RC_ABORT, dev=dev, tn_out=True)
        run(engine, b, rc, RC_ABORT, dev=dev, tn_out=False)
    # three successive selects, each carrying the src of the one before
    cur, src, ref_b, ref_src = batch_to_dev(b), None, b, None
    for step in range(3):
        rc = pattern_rc("random", ref_b.n_txn, rng)
        cur, src, _ = engine.select_batch(cur, to_dev(rc), RC_ABORT, src=src)
        _, _, _, rows = select(ref_b, rc, RC_ABORT, src_in=ref_src)
        ref_b = d.EpochBatch(rows["offsets"], rows["keys"], rows["acctype"], rows["start_tn"],
                             rows["finish_tn"], rows["order"])
        ref_src = rows["src"]
        assert np.array_equal(to_host(src, np.uint32), ref_src)
    assert 0 < cur.n_txn < b.n_txn
    src = to_host(src, np.uint32).astype(np.int64)
    off, o0 = to_host(cur.offsets, np.uint32).astype(np.int64), b.offsets.astype(np.int64)
    keys = to_host(cur.keys, np.uint64)
    for q in range(cur.n_txn):  # the final src indexes the original batch
        assert np.array_equal(keys[off[q]:off[q + 1]], b.keys[o0[src[q]]:o0[src[q] + 1]])
    assert np.array_equal(to_host(cur.start_tn, np.uint64), b.start_tn[src])
    assert np.array_equal(to_host(cur.order, np.uint64), b.order[src])


def test_forms(engine):
    """Host, device and the compact transfer forms of one epoch: one wide output."""
    rng = np.random.default_rng(31)
    b = tn_batch(rng, 3000)
    rc = pattern_rc("random", b.n_txn, rng)
    c = engine.compact_host_batch(b)
    assert c.keys.dtype == np.uint32 and c.meta.get("acctype_2bit") and c.start_tn.dtype == np.uint32
    run(engine, b, rc, RC_ABORT, dev=False)
    run(engine, b, rc, RC_ABORT, dev=True)
    run(engine, b, rc, RC_ABORT, dev=False, run_batch=c)
    run(engine, b, rc, RC_ABORT, dev=True, run_batch=c)
    plain = d.EpochBatch(b.offsets, b.keys, b.acctype)  # no timestamps: nothing gathered
    run(engine, plain, rc, RC_ABORT, dev=True, run_batch=engine.compact_host_batch(plain))


@pytest.mark.parametrize("dev", [True, False])
def test_capacity(engine, dev):
    rng = np.random.default_rng(37)
    b = random_batch(rng, 2000, 12, 1 << 20, unique=False)
    rc = pattern_rc("random", b.n_txn, rng)
    _, ns, ms, _ = select(b, rc, RC_ABORT)
    assert run(engine, b, rc, RC_ABORT, dev=dev, cap_txn=ns, cap_nnz=ms, txn_base=5, nnz_base=9)[0] == OK
    assert run(engine, b, rc, RC_ABORT, dev=dev, cap_txn=ns - 1, cap_nnz=ms, txn_base=5, nnz_base=9)[0] == ERANGE
    assert run(engine, b, rc, RC_ABORT, dev=dev, cap_txn=ns, cap_nnz=ms - 1, txn_base=5, nnz_base=9)[0] == ERANGE
    assert run(engine, b, rc, RC_ABORT, dev=dev, cap_txn=0, cap_nnz=0)[0] == ERANGE
    assert run(engine, b, rc, RC_ABORT, dev=dev)[0] == OK  # the context still works


def test_malformed(engine):
    good = make_batch([[(1, RD)], [(2, WR), (3, RD)], [(4, RD)]])
    rc = np.array([2, 2, 2], np.uint8)
    for bad_off in ([0, 4, 3, 4], [1, 1, 3, 4], [0, 1, 3, 5]):
        bad = d.EpochBatch(np.array(bad_off, np.uint32), good.keys, good.acctype)
        for bb, r in ((bad, rc), (batch_to_dev(bad), to_dev(rc))):
            with pytest.raises(d.DccError) as e:
                engine.select_batch(bb, r, RC_ABORT)
            assert e.value.code == _abi.DCC_EINVAL
    # null rc / null out, straight through the C ABI
    big = {k: sentinel(DTYPES[k], 16) for k in ("offsets", "keys", "acctype")}
    so = _abi.SelectOut(3, 4, 0, 0, big["offsets"].ctypes.data, big["keys"].ctypes.data,
                        big["acctype"].ctypes.data, None, None, None, None)
    cb = good.to_c()
    ns, ms = C.c_uint64(0), C.c_uint64(0)
    lib = _abi.lib
    assert lib.dcc_batch_select(engine.handle, C.byref(cb), None, RC_ABORT, None, C.byref(so),
                                C.byref(ns), C.byref(ms), None) == _abi.DCC_EINVAL
    assert lib.dcc_batch_select(engine.handle, C.byref(cb), rc.ctypes.data, RC_ABORT, None, None,
                                C.byref(ns), C.byref(ms), None) == _abi.DCC_EINVAL
    for k, v in big.items():
        assert np.array_equal(v, sentinel(DTYPES[k], 16))
    assert lib.dcc_batch_select(engine.handle, C.byref(cb), rc.ctypes.data, RC_ABORT, None, C.byref(so),
                                C.byref(ns), C.byref(ms), None) == _abi.DCC_OK
    assert (ns.value, ms.value) == (3, 4) and big["offsets"][:4].tolist() == [0, 1, 3, 4]
    run(engine, good, rc, RC_ABORT, dev=True)  # the context still works


def test_multi_context_runs_on_rank0(engine):
    rng = np.random.default_rng(41)
    b = tn_batch(rng, 3000)
    rc = pattern_rc("random", b.n_txn, rng)
    with d.Engine(devices=[0, 0]) as m:
        run(m, b, rc, RC_ABORT, dev=False)
        run(m, b, rc, RC_ABORT, dev=True)


def test_with_communicator_attached(engine):
    """A local call: a two-rank communicator is attached and never used."""
    rng = np.random.default_rng(43)
    b = random_batch(rng, 3000, 12, 1 << 20, unique=False)
    rc = pattern_rc("random", b.n_txn, rng)
    called = []
    with d.Engine(0) as eng:
        eng.comm_init_host(0, 2, lambda buf: called.append(1))
        run(eng, b, rc, RC_ABORT, dev=False)
        run(eng, b, rc, RC_ABORT, dev=True)
        assert not called and eng.comm_calls == 0
        eng.comm_destroy()


def test_reserve_and_repeat(engine):
    rng = np.random.default_rng(47)
    b = random_batch(rng, 3000, 12, 1 << 20, unique=False)
    rc = pattern_rc("random", b.n_txn, rng)
    engine.reserve(b.n_txn, b.nnz)
    for dev in (True, False):
        bb, r = (batch_to_dev(b), to_dev(rc)) if dev else (b, rc)
        outs = []
        for _ in range(2):
            sel, src, _ = engine.select_batch(bb, r, RC_ABORT)
            outs.append([to_host(a, t) for a, t in ((sel.offsets, np.uint32), (sel.keys, np.uint64),
                                                    (sel.acctype, np.uint8), (src, np.uint32))])
        assert all(np.array_equal(x, y) for x, y in zip(*outs))
        run(engine, b, rc, RC_ABORT, dev=dev)


def test_external_stream(engine):
    import torch
    rng = np.random.default_rng(53)
    b = random_batch(rng, 3000, 12, 1 << 20, unique=False)
    rc = pattern_rc("random", b.n_txn, rng)
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()  # the inputs were uploaded on torch's stream
    engine.set_stream(s.cuda_stream)
    try:
        run(engine, b, rc, RC_ABORT, dev=True)
        run(engine, b, rc, RC_ABORT, dev=False)
    finally:
        engine.set_stream(None)


def test_closed_loop_nowait(engine):
    """Four NO_WAIT epochs, epoch e + 1 = aborted(e) ++ fresh, held(e + 1) =
    the requests of committed(e), every carry on the device; each epoch against
    the Row_lock replay of the same epoch built on the host."""
    import torch
    F, E = 2000, 4
    rng = np.random.default_rng(59)
    fresh = [random_batch(rng, F, 12, 20000, p_write=0.3, unique=True) for _ in range(E)]
    # host mirror of the loop
    h_cur, h_ids, h_held = fresh[0], np.arange(F, dtype=np.uint32), None
    # the device's
    cur, ids, held = batch_to_dev(fresh[0]), to_dev(h_ids), None
    retried_commits = 0
    for e in range(E):
        erc, ecf = replay(h_cur, h_held)
        assert 0 < int((erc == RC_RCOK).sum()) < erc.size, "the replay yields one outcome only"
        rc, cf, _ = engine.nowait_lock_epoch(cur, held=held)
        assert np.array_equal(rc.cpu().numpy(), erc), f"epoch {e}: rc differs from the replay"
        assert np.array_equal(cf.cpu().numpy().view(np.uint32), ecf), f"epoch {e}: conflict ordinal"
        n_retry = h_cur.n_txn - F
        retried_commits += int((erc[:n_retry] == RC_RCOK).sum())
        # src maps every txn of the epoch to its first appearance
        got = to_host(ids, np.uint32).astype(np.int64)
        assert np.array_equal(got, h_ids)
        assert np.all(got[:n_retry] < e * F) and np.array_equal(got[n_retry:], np.arange(e * F, (e + 1) * F))
        off = h_cur.offsets.astype(np.int64)
        for q in range(n_retry):
            f, j = fresh[got[q] // F], got[q] % F
            assert np.array_equal(h_cur.keys[off[q]:off[q + 1]], f.keys[f.offsets[j]:f.offsets[j + 1]])
        if e + 1 == E:
            break
        nf = fresh[e + 1]
        # host: numpy
        _, n0, m0, r = select(h_cur, erc, RC_ABORT, src_in=h_ids)
        per_req = np.repeat(erc == RC_RCOK, np.diff(off))
        h_held = (h_cur.keys[per_req].copy(), h_cur.acctype[per_req].copy())
        h_cur = d.EpochBatch(np.concatenate([r["offsets"], nf.offsets[1:] + np.uint32(m0)]).astype(np.uint32),
                             np.concatenate([r["keys"], nf.keys]), np.concatenate([r["acctype"], nf.acctype]))
        h_ids = np.concatenate([r["src"], np.arange((e + 1) * F, (e + 2) * F, dtype=np.uint32)])
        # device: select the aborted into the front, the fresh txns behind them
        held = engine.held_from(cur, rc)
        assert np.array_equal(to_host(held[0], np.uint64), h_held[0])
        assert np.array_equal(to_host(held[1], np.uint8), h_held[1])
        out = d.EpochBatch(torch.empty(cur.n_txn + F + 1, dtype=torch.int32, device="cuda:0"),
                           torch.empty(cur.nnz + nf.nnz, dtype=torch.int64, device="cuda:0"),
                           torch.empty(cur.nnz + nf.nnz, dtype=torch.uint8, device="cuda:0"),
                           meta={"src": torch.empty(cur.n_txn + F, dtype=torch.int32, device="cuda:0")})
        sel, _, st = engine.select_batch(cur, rc, RC_ABORT, src=ids, out=out)
        assert (sel.n_txn, sel.nnz) == (n0, m0) == (st["n_commit"], int(r["keys"].size))
        dn = batch_to_dev(nf)
        out.offsets[n0 + 1:n0 + 1 + F] = dn.offsets[1:] + m0
        out.keys[m0:m0 + nf.nnz] = dn.keys
        out.acctype[m0:m0 + nf.nnz] = dn.acctype
        out.meta["src"][n0:n0 + F] = torch.arange((e + 1) * F, (e + 2) * F, dtype=torch.int32, device="cuda:0")
        cur = d.EpochBatch(out.offsets[:n0 + F + 1], out.keys[:m0 + nf.nnz], out.acctype[:m0 + nf.nnz])
        ids = out.meta["src"][:n0 + F]
        torch.cuda.synchronize()  # torch's copies above, before the engine's stream reads them
        assert np.array_equal(to_host(cur.offsets, np.uint32), h_cur.offsets)
        assert np.array_equal(to_host(cur.keys, np.uint64), h_cur.keys)
    assert retried_commits > 0, "no retried txn committed in four epochs"
