"""GPU parity of the shared stable LSD radix sort (radix_sort.hip) at both of
its tilings, and of the key packing in front of it, on the cases of
sort_cases.py (test_sort_cases.py proves on the CPU that they are what they
claim).  Everything is bit-exact; nothing is derived from the GPU's output.

A  the sort itself through dcc_calvin_dispatch -- a stable u64 sort of `order`,
   then a stable u32 sort of `wave` -- against two numpy stable argsorts: the
   seams of the 2,048-pair tile, the threshold RS_SMALL between the tilings,
   the seams of the 8,192-pair tile with a partial last tile, odd counts (the
   unaligned, scalar loads of k_rs_hist), and order / wave patterns with one
   live digit, two digits, long tied runs and every pass count of the wave sort.
B  every engine that sorts, once above RS_SMALL with a partial last tile, each
   on a context of its own: the scratch (rs_scratch_words) is then what that
   engine's own reservation asked for, not what an earlier, larger test left.
C  key shapes at small size through every engine that packs or hashes keys: 32
   one-bit runs, bit 63, keys next to KEY_RESERVED, and exactly 31 / 32 / 33 /
   63 / 64 varying bits; WAIT_DIE refuses 64 with rc / pos untouched.

Which sort instantiation (key type, items per thread) meets a partial last
tile where:
  u64, 4   A at 1 .. 2 T4 + 1 (order); C (TIMESTAMP, WAIT_DIE, Calvin 33+ bits)
  u32, 4   A at the same sizes (wave); C (Calvin up to 32 bits)
  u64, 16  A at RS_SMALL + 1 .. RS_SMALL + T16 + 1 (order); B (TIMESTAMP, MVCC,
           WAIT_DIE epoch and release, Calvin wide keys, Calvin 63-bit order,
           the history builds)
  u32, 16  A at the same sizes (wave); B (the key sort of the Calvin order case)
"""
import numpy as np
import pytest

import _oracle as orc
import deneva_amd as d
import sort_cases as sc
from deneva_amd import RC_ABORT, RC_RCOK, _abi
from locktab_ref import LockTable
from test_gpu_locktab import epoch as locktab_epoch
from test_gpu_locktab import release as locktab_release
from test_gpu_locktab import state_of
from test_gpu_nowait import check as nowait_check
from test_gpu_tso import check as tso_check
from test_gpu_waitdie import check_epoch, check_release, differ, from_dev, leave_of, three_outcomes, to_dev
from waitdie_cases import new_state

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAPS = list(sc.KEY_MAPS)


def dispatch_id(c):
    n, pattern, wmax = c
    rel = n - sc.RS_SMALL
    size = str(n) if rel < 0 else "RS_SMALL" + (f"+{rel}" if rel else "")
    return f"{size}-{pattern}-w{wmax}"


def check_dispatch(eng, wave, order, dev=False):
    eoff, etxn = sc.dispatch_expected(wave, order)
    if dev:
        import torch
        w = torch.from_numpy(wave.view(np.int32)).to(DEV)
        o = None if order is None else torch.from_numpy(order.view(np.int64)).to(DEV)
        off, txn = eng.calvin_dispatch(w, o)
        off, txn = off.cpu().numpy().view(np.uint32), txn.cpu().numpy().view(np.uint32)
    else:
        off, txn = eng.calvin_dispatch(wave, order)
    differ("txn", np.asarray(txn), etxn)
    assert np.asarray(off).size == eoff.size
    differ("wave_off", np.asarray(off), eoff)


# ---------------------------------------------------------- A: the sort itself
@pytest.mark.parametrize("case", [c for c in sc.DISPATCH_CASES if c[0] < sc.RS_SMALL], ids=dispatch_id)
def test_sort_small_tile(engine, case):
    check_dispatch(engine, *sc.dispatch_arrays(*case))


@pytest.mark.parametrize("case", [c for c in sc.DISPATCH_CASES if c[0] >= sc.RS_SMALL], ids=dispatch_id)
def test_sort_threshold_and_large_tile(case):
    """On a context of its own: the workspace and the sort scratch are sized by
    this call alone."""
    wave, order = sc.dispatch_arrays(*case)
    with d.Engine(0) as eng:
        check_dispatch(eng, wave, order)


def test_sort_large_tile_device_arrays():
    wave, order = sc.dispatch_arrays(sc.LARGE_ALL, "random", sc.WAVE_MAX[-1])
    with d.Engine(0) as eng:
        check_dispatch(eng, wave, order, dev=True)


def test_sort_large_tile_without_order():
    """order = None: the wave sort alone, its values the index."""
    wave, _ = sc.dispatch_arrays(sc.LARGE_ALL, "random", 65536)
    with d.Engine(0) as eng:
        check_dispatch(eng, wave, None)
        check_dispatch(eng, wave[:sc.SMALL_ALL], None, dev=True)


# ------------------------------ B: the engines above the threshold, fresh contexts
def test_tso_above_threshold():
    b, ts, erc, ecf, k, ewts, erts = sc.big_tso()
    assert sc.above_threshold(b.nnz)
    with d.Engine(0) as eng:
        rc, cf, st = eng.tso_validate_epoch(b, ts)
        differ("rc", rc, erc)
        differ("conflict", cf, ecf)
        assert st["n_commit"] == int((erc == RC_RCOK).sum()) and st["n_abort"] == int((erc == RC_ABORT).sum())
        assert eng.tso_rows_size == k.size
        w, r = eng.tso_rows_get(k)
        differ("wts", w, ewts)
        differ("rts", r, erts)


def test_mvcc_above_threshold():
    b, ts, erc, ecf, evts, k, elatest, erts, evk, evt = sc.big_mvcc()
    assert sc.above_threshold(b.nnz)
    with d.Engine(0) as eng:
        rc, cf, vts, st = eng.mvcc_validate_epoch(b, ts)
        differ("rc", rc, erc)
        differ("conflict", cf, ecf)
        differ("vts", vts, evts)
        assert st["n_commit"] == int((erc == RC_RCOK).sum()) and st["n_abort"] == int((erc == RC_ABORT).sum())
        latest, rts = eng.mvcc_rows_get(k)
        differ("latest version", latest, elatest)
        differ("rts", rts, erts)
        vk, vt = eng.mvcc_versions()
        assert eng.mvcc_versions_size == evk.size == vk.size
        differ("version keys", vk, evk)
        differ("version ts", vt, evt)


def test_waitdie_above_threshold():
    """An epoch, the release of every RCOK and ABORT txn (two sorts: by
    timestamp, then by key), a second epoch."""
    b, ts, e1, leave, r1, e2 = sc.big_waitdie()
    assert sc.above_threshold(b.nnz)
    three_outcomes(e1)
    rc, pos = new_state(b.n_txn)
    with d.Engine(0) as eng:
        check_epoch(eng, b, ts, rc, pos, exp=e1)
        check_release(eng, b, ts, e1[0], e1[1], leave, exp=r1)
        check_epoch(eng, b, ts, r1[0], r1[1], exp=e2, dev=True)


def check_calvin(eng, b, ref, dev=False, waves=False):
    """The epoch on the sort path (the caller selects it) against the oracle's
    (group, rc, wave) of the host batch b."""
    eg, erc, ew = ref
    g, rc, w, st = eng.calvin_order_epoch(b.to_torch(DEV) if dev else b, want_group=True, want_wave=waves)
    if dev:
        g, rc = g.cpu().numpy(), rc.cpu().numpy()
        w = w.cpu().numpy() if waves else None
    assert st["fallback"] == 0, "the epoch took the bucket path"
    differ("group", np.asarray(g).view(np.uint32), eg)
    differ("rc", np.asarray(rc), erc)
    if waves:
        differ("wave", np.asarray(w).view(np.uint32), ew)
    assert st["n_commit"] == int((erc == 0).sum())


def test_calvin_wide_keys_above_threshold():
    """More than 32 varying key bits: the u64 key sort of 2,097,168 requests."""
    b, ref = sc.big_calvin_keys()
    assert sc.above_threshold(b.nnz) and sc.varying_bits(b.keys) > 32
    with d.Engine(0) as eng:
        eng.set_option(_abi.OPT_CALVIN_PATH, 1)  # the global sort + scan at every size
        check_calvin(eng, b, ref)


def test_calvin_wide_order_above_threshold():
    """RS_SMALL + 1 txns under a 63-bit order: the u64 order sort, then the u32
    key sort of as many requests, both with a last tile of one pair."""
    b, ref = sc.big_calvin_order()
    assert sc.above_threshold(b.n_txn) and sc.varying_bits(b.order) > 32 and sc.varying_bits(b.keys) <= 32
    with d.Engine(0) as eng:
        eng.set_option(_abi.OPT_CALVIN_PATH, 1)  # the global sort + scan at every size
        check_calvin(eng, b, ref)


@pytest.mark.parametrize("two_sorts", [False, True], ids=["one_sort", "two_sorts"])
def test_history_above_threshold(two_sorts):
    """The level build sorts RS_SMALL + 16 pairs (+ 16 for the two-sort build)
    by (key, tn); an epoch's windows then read the runs it made."""
    appends, b, (erc, etn, etnc), (hk, ht) = sc.big_history(two_sorts)
    assert sc.above_threshold(hk.size)
    with d.Engine(0) as eng:
        for k, t in appends:
            eng.history_append(k, t)
        assert eng.history_size == hk.size
        eng.tnc = sc.HIST_TNC
        rc, tn, _ = eng.occ_validate_epoch(b, want_tn=True)
        differ("rc", np.asarray(rc), erc)
        differ("tn", np.asarray(tn, np.uint64), etn)
        assert eng.tnc == etnc
        # the export is of the flat pairs: none was lost (the epoch above read the sorted runs)
        gk, gt = eng.history_export()
        o = np.lexsort((ht, hk))
        differ("history keys", gk, hk[o])
        differ("history tn", gt, ht[o])


# ------------------------------------------------- C: key shapes at small size
@pytest.fixture
def sort_path(engine):
    engine.set_option(_abi.OPT_CALVIN_PATH, 1)
    yield engine
    engine.set_option(_abi.OPT_CALVIN_PATH, 0)


def case_of(name):
    """(mapped batch, ts, device batch?): host and device batches alternate."""
    b, ts = sc.hot_base()
    return sc.mapped(b, name), ts, MAPS.index(name) % 2 == 1


@pytest.mark.parametrize("name", MAPS)
def test_key_shapes_tso(engine, name):
    b, ts, dev = case_of(name)
    tso_check(engine, b, ts, dev=dev)
    engine.tso_rows_clear()


def waitdie_three_calls(eng, b, ts, dev):
    rc, pos = new_state(b.n_txn)
    e1 = check_epoch(eng, b, ts, rc, pos, dev=dev)
    assert min(e1[3]["n_commit"], e1[3]["n_abort"], e1[3]["n_survivors"]) > 0
    r1 = check_release(eng, b, ts, e1[0], e1[1], leave_of(e1[0], [RC_RCOK, RC_ABORT]), dev=not dev)
    assert r1[3] > 0
    check_epoch(eng, b, ts, r1[0], r1[1], dev=dev)
    return e1


@pytest.mark.parametrize("name", [m for m in MAPS if m != "varying64"])
def test_key_shapes_waitdie(engine, name):
    """At varying63 the epoch and the release sort kp.bits + 1 == 64 bits."""
    b, ts, dev = case_of(name)
    waitdie_three_calls(engine, b, ts, dev)


def test_waitdie_refuses_64_varying_bits():
    """DCC_ENOTSUP from both calls, rc / pos byte for byte as passed, host and
    device; the same context then runs 63 varying bits."""
    base, ts = sc.hot_base()
    b64, b63 = sc.mapped(base, "varying64"), sc.mapped(base, "varying63")
    assert sc.varying_bits(b64.keys) == 64 and sc.varying_bits(b63.keys) == 63
    with d.Engine(0) as eng:
        # a state with every value of rc in it: the one an epoch leaves
        e1 = waitdie_three_calls(eng, base, ts, False)
        rc0, pos0 = e1[0].copy(), e1[1].copy()
        leave = leave_of(rc0, [RC_RCOK])
        assert np.unique(rc0).size >= 3 and np.unique(pos0).size > 3
        for dev in (False, True):
            if dev:
                bb = b64.to_torch(DEV)
                args = to_dev(ts, rc0, pos0, leave)
            else:
                bb, args = b64, [ts, rc0.copy(), pos0.copy(), leave]
            for call in (lambda: eng.waitdie_lock_epoch(bb, *args[:3]), lambda: eng.waitdie_release(bb, *args)):
                with pytest.raises(d.DccError) as e:
                    call()
                assert e.value.code == _abi.DCC_ENOTSUP
                r, p = from_dev(args[1], args[2]) if dev else (args[1], args[2])
                assert r.tobytes() == rc0.tobytes() and p.tobytes() == pos0.tobytes()
        waitdie_three_calls(eng, b63, ts, True)


@pytest.mark.parametrize("name", MAPS)
def test_key_shapes_nowait(engine, name):
    b, _, dev = case_of(name)
    rc, _, _ = nowait_check(engine, b, dev=dev)
    assert 0 < int((rc == RC_RCOK).sum()) < rc.size


@pytest.mark.parametrize("name", MAPS)
def test_key_shapes_locktab(engine, name):
    """Lock epoch, release of half the committed txns, a second epoch on what
    stays held, release; the export after every call."""
    b, _, dev = case_of(name)
    ref = LockTable()
    with engine.locktab(1 << 16) as lt:
        rc, _, _ = locktab_epoch(lt, ref, b, dev=dev)
        assert 0 < int((rc == RC_RCOK).sum()) < rc.size
        assert state_of(lt, dev) == ref.export()
        half = np.where(np.arange(b.n_txn) % 2 == 0, rc, RC_ABORT).astype(np.uint8)
        locktab_release(lt, ref, b, half, dev=not dev)
        assert state_of(lt) == ref.export() and len(ref.export()) > 0
        rc2, _, _ = locktab_epoch(lt, ref, b, dev=dev)
        assert state_of(lt, not dev) == ref.export()
        locktab_release(lt, ref, b, rc2, dev=dev)
        locktab_release(lt, ref, b, np.where(np.arange(b.n_txn) % 2 == 1, rc, RC_ABORT).astype(np.uint8))
        assert state_of(lt) == ref.export() == {}


@pytest.mark.parametrize("name", MAPS)
def test_key_shapes_calvin(sort_path, name):
    """Grant groups, readiness and wave levels on the sort path: the u32 key
    sort up to 32 varying bits, the u64 one from 33."""
    b, _, dev = case_of(name)
    ref = orc.calvin(b)
    assert 0 < int((ref[1] == 0).sum()) < b.n_txn and int(ref[0].max()) > 3
    check_calvin(sort_path, b, ref, dev=dev, waves=True)


@pytest.mark.parametrize("name", ["varying32", "varying33"])
def test_calvin_at_the_u32_u64_boundary(sort_path, name):
    """Exactly 32 packed bits (the last u32 key sort) against 33 (the first u64
    one), groups wanted, host and device batches, under a sequencer order."""
    base, ts = sc.hot_base()
    b = sc.mapped(base, name)
    assert sc.varying_bits(b.keys) == int(name[7:])
    b.order = ts  # distinct, permuted
    ref = orc.calvin(b)
    assert int(ref[0].max()) > 3
    for dev in (False, True):
        check_calvin(sort_path, b, ref, dev=dev)
