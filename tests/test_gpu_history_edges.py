"""Directed cases of the device OCC history on the GPU (csrc/occ_history.h,
occ_history.hip, the hist_* host code of dcc_ctx.hip): the scenarios of
history_cases.py -- window edges on every resolution path and level, chain
order, the walk bound and both overflow rebuilds, a cluster wrapping past the
last slot, the key bitmap, the merge threshold, out-of-order appends, trim
floors and the append kernels' workgroup seams -- run step by step, with host
and with device batches.  After every step the RCs, the commit tns, tnc,
history_size and history_export() are compared with the plain model;
test_history_cases.py proves that model equal to the literal oracle and the
cases' structural claims (which level and path answers, where a table
overflows) in numbers.  Everything is bit-exact."""
import numpy as np
import pytest

import _oracle as orc
import deneva_amd as d
import history_cases as hc
from deneva_amd import WR
from deneva_amd._abi import OPT_HIST_MERGE, RC_ABORT, RC_RCOK

pytestmark = pytest.mark.gpu


def to_np(x, dtype=None):
    if hasattr(x, "cpu"):
        import torch
        torch.cuda.synchronize()
        x = x.cpu().numpy()
    x = np.asarray(x)
    return x.view(dtype) if dtype is not None and x.dtype != dtype else x


def check_state(eng, m, where):
    assert eng.history_size == len(m.pairs), where
    gk, gt = eng.history_export()
    wk, wt = m.sorted_pairs()
    assert np.array_equal(gk, wk) and np.array_equal(gt, wt), f"{where}: the exported pairs differ"
    assert eng.tnc == m.tnc, where


def do_reads(eng, m, st, dev, where):
    reads = m.reads_of(st)
    b, top = hc.read_batch(reads)
    want = m.read_rc(reads)
    n = b.n_txn
    if st.snapshot:
        aoff, aidx = np.zeros(n + 1, np.uint32), np.zeros(1, np.uint32)
        hk = np.array([k for k, _ in m.pairs], np.uint64)
        ht = np.array([t for _, t in m.pairs], np.uint64)
        assert np.array_equal(orc.occ_snapshot(b, aoff, np.zeros(0, np.uint32), top, hk, ht), want), where
        if dev:
            import torch
            cv = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).cuda()
            rc, _ = eng.occ_validate_snapshot(b.to_torch("cuda:0"), cv(aoff), cv(aidx), cv(top))
        else:
            rc, _ = eng.occ_validate_snapshot(b, aoff, aidx, top)
        rc = to_np(rc)
    else:
        rc, tn, _ = eng.occ_validate_epoch(b.to_torch("cuda:0") if dev else b, want_tn=True)
        rc = to_np(rc)
        assert not to_np(tn, np.uint64).any(), f"{where}: a read-only txn took a commit tn"
    bad = np.nonzero(rc != want)[0]
    assert bad.size == 0, (f"{where}: {bad.size} of {n} windows decided wrongly, e.g. (key, lo, hi[, top]) "
                           f"{[reads[i] for i in bad[:4]]} got {rc[bad[:4]]}; the key's tns "
                           f"{[m.tns_of(reads[i][0]) for i in bad[:4]]}")


def do_write(eng, m, st, dev, where):
    b = hc.write_batch(st.txns)
    want_rc, want_tn, _ = m.write(st.txns)
    bb = b.to_torch("cuda:0") if dev else b
    if st.defer:
        rc, _, _ = eng.occ_validate_epoch(bb, defer_finish=True)
        assert np.array_equal(to_np(rc), want_rc), f"{where}: rc differs"
        tn = eng.occ_finish_epoch(rc)
    else:
        rc, tn, _ = eng.occ_validate_epoch(bb, want_tn=True, append_history=True)
        assert np.array_equal(to_np(rc), want_rc), f"{where}: rc differs"
    assert np.array_equal(to_np(tn, np.uint64), want_tn), f"{where}: commit tns differ"


def run_scenario(eng, sc, dev, fresh=False):
    m = hc.Model()
    try:
        if not fresh:
            eng.history_clear()
            eng.tnc = 0
            eng.set_option(OPT_HIST_MERGE, hc.DEFAULT_MERGE)
        for i, st in enumerate(sc.steps):
            where = f"{sc.name} step {i} ({type(st).__name__})"
            if isinstance(st, hc.Expect):
                continue
            if isinstance(st, hc.Reads):
                do_reads(eng, m, st, dev, where)
            elif isinstance(st, hc.Write):
                do_write(eng, m, st, dev, where)
            else:
                m.apply(st)
                if isinstance(st, hc.Opt):
                    eng.set_option(OPT_HIST_MERGE, st.merge_min)
                elif isinstance(st, hc.Tnc):
                    eng.tnc = st.value
                elif isinstance(st, hc.Append):
                    eng.history_append(np.array(st.keys, np.uint64), np.array(st.tns, np.uint64))
                elif isinstance(st, hc.Trim):
                    eng.history_trim(st.floor)
                elif isinstance(st, hc.Clear):
                    eng.history_clear()
            check_state(eng, m, where)
    finally:
        eng.set_option(OPT_HIST_MERGE, 65536)
        eng.history_clear()
        eng.tnc = 0


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", hc.NAMES)
def test_scenario(engine, name, dev):
    run_scenario(engine, hc.scenario(name), dev)


@pytest.mark.parametrize("name", ["edges_chain", "edges_run"])
def test_first_use_of_a_context(name):
    """The same on a context whose history was never cleared: its first epoch
    appends into a delta level that no call has emptied before, and the next
    epoch's windows must see those pairs."""
    with d.Engine(0) as eng:
        run_scenario(eng, hc.scenario(name), False, fresh=True)


def test_trim_to_nothing_then_decide_as_without_history(engine):
    """After a trim at or above every tn the history is empty: an epoch with
    wide windows over every former key commits as with no history at all, and
    its appends start a new history."""
    sc = hc.scenario("trim_above_all")
    m = hc.Model()
    try:
        engine.history_clear()
        engine.tnc = 0
        for st in sc.steps:
            if isinstance(st, hc.Trim):
                break
            if isinstance(st, hc.Reads):
                do_reads(engine, m, st, False, "setup")
            elif isinstance(st, hc.Write):
                do_write(engine, m, st, False, "setup")
            elif not isinstance(st, hc.Expect):
                m.apply(st)
                if isinstance(st, hc.Opt):
                    engine.set_option(OPT_HIST_MERGE, st.merge_min)
                elif isinstance(st, hc.Tnc):
                    engine.tnc = st.value
                else:
                    engine.history_append(np.array(st.keys, np.uint64), np.array(st.tns, np.uint64))
        keys = sorted({k for k, _ in m.pairs})
        assert len(m.pairs) == 7 and engine.history_size == 7
        engine.history_trim(max(t for _, t in m.pairs))
        assert engine.history_size == 0 and engine.history_export()[0].size == 0
        # RD old key + WR new key, windows over everything that was there
        from helpers import make_batch
        b = make_batch([[(k, d.RD), (k ^ 0x5555, WR)] for k in keys], [0] * len(keys), [1000] * len(keys))
        rc, tn, _ = engine.occ_validate_epoch(b, want_tn=True, append_history=True)
        assert (np.asarray(rc) == RC_RCOK).all()
        t0 = m.tnc
        assert list(np.asarray(tn, np.uint64)) == list(range(t0 + 1, t0 + 1 + len(keys)))
        gk, gt = engine.history_export()
        assert sorted(zip(gk.tolist(), gt.tolist())) == sorted((k ^ 0x5555, t0 + 1 + i) for i, k in enumerate(keys))
        rc, _, _ = engine.occ_validate_epoch(b, want_tn=True)   # now the new pairs are seen
        assert (np.asarray(rc) == RC_RCOK).all()
        b2 = make_batch([[(k ^ 0x5555, d.RD)] for k in keys], [0] * len(keys), [1000] * len(keys))
        rc, _, _ = engine.occ_validate_epoch(b2, want_tn=True)
        assert (np.asarray(rc) == RC_ABORT).all()
    finally:
        engine.set_option(OPT_HIST_MERGE, 65536)
        engine.history_clear()
        engine.tnc = 0
