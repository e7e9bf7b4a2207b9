"""GPU: the one-CU Calvin wave walk at its chunk seams (calvin_wave_cases.py;
the facts of every case are proved on the CPU by test_calvin_wave_cases.py).
Grant groups, readiness and wave levels equal the oracle's bit for bit, the
number of rounds is the deepest wave + 1, and every probe's reader sits at
D + 1: its carrier's wave reached it over the path its classes name."""
import numpy as np
import pytest

import _oracle as orc
import calvin_wave_cases as cw

pytestmark = pytest.mark.gpu

_want = {}


def oracle(name):
    """(case, groups, rc, waves) of a case, computed once and left unchanged."""
    if name not in _want:
        c = cw.build(name)
        g, rc, w = orc.calvin(c.batch)
        for a in (g, rc, w):
            a.setflags(write=False)
        _want[name] = (c, g, rc, w)
    return _want[name]


def host(a, n):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a[:n]


def check(engine, name, dev=False):
    c, eg, erc, ew = oracle(name)
    b = c.batch
    g, rc, w, st = engine.calvin_order_epoch(b.to_torch("cuda:0") if dev else b, want_group=True,
                                             want_wave=True)
    if dev:
        import torch
        torch.cuda.synchronize()
    g, rc, w = host(g, b.nnz).astype(np.uint32), host(rc, b.n_txn), host(w, b.n_txn).astype(np.uint32)
    bad = np.nonzero(g != eg)[0]
    assert bad.size == 0, f"{name}: group mismatch at requests {bad[:10]} (gpu {g[bad[:10]]} oracle {eg[bad[:10]]})"
    bad = np.nonzero(rc != erc)[0]
    assert bad.size == 0, f"{name}: rc mismatch at txns {bad[:10]}"
    lost = [f"'{p.name}' (own {p.own} +{p.own_dist}, previous {p.prev} -{p.prev_dist}): carrier {w[p.m]} "
            f"(D = {p.D}), reader {w[p.t]} (D + 1 = {p.D + 1})"
            for p in c.probes if w[p.t] != p.D + 1 or w[p.m] != p.D]
    assert not lost, f"{name}: {len(lost)} of {len(c.probes)} probes lost their wave: " + "; ".join(lost[:8])
    bad = np.nonzero(w != ew)[0]
    assert bad.size == 0, f"{name}: wave mismatch at txns {bad[:10]} (gpu {w[bad[:10]]} oracle {ew[bad[:10]]})"
    assert st["rounds"] == int(ew.max()) + 1
    assert st["n_commit"] == int((erc == 0).sum())
    return w


@pytest.mark.parametrize("name", list(cw.CASES))
def test_case(engine, name):
    check(engine, name)


@pytest.mark.parametrize("name", cw.DEV_CASES)
def test_case_device_pointers(engine, name):
    check(engine, name, dev=True)


@pytest.mark.parametrize("lg", [4, 5])
def test_helper_threshold_back_to_back(engine, lg):
    """The last size of the walker's workgroup alone and the first with helper
    workgroups, each twice in a row, then again after a larger epoch: the helper
    counters, the two-chunk records and the maxima do not leak between calls."""
    lo, hi, big = f"sizes-lg{lg}-2C", f"sizes-lg{lg}-2C+1", f"grid-lg{lg}-index"
    assert not cw.plan(oracle(lo)[0].n, 1 << lg).helpers and cw.plan(oracle(hi)[0].n, 1 << lg).helpers
    first = {}
    for name in (lo, lo, hi, hi, big, hi, lo, big, lo, hi):
        w = check(engine, name)
        assert np.array_equal(first.setdefault(name, w), w), name


def test_dispatch_lists(engine):
    """The dispatch lists of a grid batch in sequencer order: txns by (wave,
    sequence position)."""
    c, _, _, ew = oracle("grid-lg4-seq")
    w = check(engine, "grid-lg4-seq")
    off, txn = engine.calvin_dispatch(w, c.batch.order)
    seq = np.argsort(c.batch.order, kind="stable")
    want = seq[np.argsort(ew[seq], kind="stable")]
    assert np.array_equal(np.asarray(txn), want.astype(np.uint32))
    counts = np.bincount(ew, minlength=int(ew.max()) + 1)
    assert np.array_equal(np.diff(np.asarray(off, np.int64)), counts)
