"""Closed loop over resident device batches: epoch e + 1 = aborted(e) ++ fresh
txns, and for NO_WAIT held(e + 1) = the requests of committed(e).  Reports
goodput: commits per second with the retries in the loop.

    python tools/retry_loop.py [--alg nowait|occ] [--epochs 8] [--fresh 65536] [--theta 0.9]
                               [--loop-warmup 1] [--loop-reps 3]
                               [--select-shapes both|c2|headline|none] [--warmup 5] [--steps 20]
                               [--backoff none|reference|exp --penalty P --penalty-max M]
                               [--queue-shapes both|c2|headline|none] [--json PATH]
                               [--hold D] [--table-shapes both|c2|headline|none]

The loop runs twice in one process on the same pre-generated fresh txns
(gen_ycsb, already on the device, so the loop times the engine and the carry,
not the generator):
  path A  carries with dcc_batch_select (Engine.select_batch / held_from):
          nothing but the two counts crosses to the host;
  path B  carries on the host: rc to the host, a numpy build of the next epoch
          and of the held rows, EpochBatch.to_torch back to the device.
Per path: wall ms per epoch as median [min, max] over the timed passes, the
goodput, and for path A the select's own device_ms and alg_bytes / device_ms.
Both paths must produce the same rc sequence.

--select-shapes times dcc_batch_select alone on the C2 (65,536 x 16) and the
headline (1,048,576 x 16) YCSB epoch at theta 0.9 with that epoch's NO_WAIT rc,
want = ABORT and want = RCOK, next to dcc_copy_bandwidth over the same byte
count (alternately, same process), and the per-pass times of a profiled call.

--backoff parks the aborted txns in an abort queue instead of retrying them at
once (system/abort_queue.cpp), the clock being the epoch index: epoch e + 1 =
pop(e + 1) ++ fresh txns.  Path A uses the device queue (Engine.abort_queue)
and carries the epoch's src / cnt arrays on the device, the fresh txns getting
0; path B does the same on the host with tests/abortq_ref.py.  Without
--backoff the loop is the one above.

--queue-shapes times the queue's push and pop alone on the same two epochs:
the push of the aborted txns next to dcc_batch_select of the same selection
and dcc_copy_bandwidth over the same bytes, a pop that releases all of them
and one that releases about half (EXP, cnt 0 or 1 at random), the pop's
phases, and the pop of all with the sort over all 64 bits.

--hold D (--alg nowait): the committed txns of epoch e keep their rows until
epoch e + D, as the reference's do while they execute.  Path A keeps the lock
state in a device lock table (Engine.locktab): lock_epoch, then
release(batch of epoch e - D, its rc, RCOK).  Path B is the way without one,
on the device: dcc_batch_select(RCOK) of each of the last D epochs, chained
through txn_base / nnz_base into one held list that is passed to
dcc_nowait_lock_epoch.  Both carry the aborted txns with dcc_batch_select.

--table-shapes times the table epoch against dcc_nowait_lock_epoch with the
equivalent held list, alternately, on the C2 and the headline epoch with the
commits of the previous one and of the previous four epochs held; the release
alone next to dcc_copy_bandwidth over its byte count; and the seed / grant /
rebuild passes and the release's phases from profiled calls."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deneva_amd as d  # noqa: E402
from deneva_amd import RC_ABORT, RC_RCOK, _abi  # noqa: E402

DEV = "cuda:0"


def mmm(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def fmt(m):
    return f"{m['median']:.3f} [{m['min']:.3f}, {m['max']:.3f}]"


def dev_batch(b):
    """Device batch with torch's signed dtypes (i32 offsets, i64 keys)."""
    return d.EpochBatch(torch.from_numpy(b.offsets.view(np.int32)).to(DEV),
                        torch.from_numpy(b.keys.view(np.int64)).to(DEV), torch.from_numpy(b.acctype).to(DEV))


def copy_ms(eng, traffic_bytes):
    """The engine's device copy moving `traffic_bytes` in all (read + written)."""
    g = C.c_double(0)
    code = _abi.lib.dcc_copy_bandwidth(eng.handle, max(traffic_bytes // 2, 16), 1, C.byref(g))
    assert code == 0
    return traffic_bytes / (g.value * 1e9) * 1e3


# ------------------------------------------------------------ select alone
def time_select(eng, n, a):
    b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
    db = dev_batch(b)
    eng.reserve(b.n_txn, b.nnz)
    rc = eng.nowait_lock_epoch(db, want_conflict=False)[0]
    out = d.EpochBatch(torch.empty(n + 1, dtype=torch.int32, device=DEV),
                       torch.empty(b.nnz, dtype=torch.int64, device=DEV),
                       torch.empty(b.nnz, dtype=torch.uint8, device=DEV))
    res = {}
    for name, want in (("abort", RC_ABORT), ("rcok", RC_RCOK)):
        def sel():
            return eng.select_batch(db, rc, want, out=out)[2]
        for _ in range(a.warmup):
            st = sel()
            copy_ms(eng, st["alg_bytes"])
        ms, cp = [], []
        for _ in range(a.steps):  # alternately: both see the same machine state
            st = sel()
            ms.append(st["device_ms"])
            cp.append(copy_ms(eng, st["alg_bytes"]))
        eng.set_profiling(True)
        ph = [sel()["phase_ms"] for _ in range(5)]
        eng.set_profiling(False)
        r = {"selected": st["n_commit"], "selected_frac": st["n_commit"] / n, "alg_bytes": st["alg_bytes"],
             "device_ms": mmm(ms), "copy_ms": mmm(cp),
             "alg_GBps": st["alg_bytes"] / (statistics.median(ms) * 1e-3) / 1e9,
             "select_over_copy": statistics.median(ms) / statistics.median(cp),
             "pass_ms": {k: statistics.median(p[q] for p in ph) for q, k in enumerate(("count", "scan", "scatter"))}}
        res[name] = r
        print(f"  want={name:5s} selected {r['selected']} ({100 * r['selected_frac']:.1f} %)  device_ms "
              f"{fmt(r['device_ms'])}  {r['alg_GBps']:.0f} GB/s  copy_ms {fmt(r['copy_ms'])}  select/copy "
              f"{r['select_over_copy']:.2f}  passes {({k: round(v, 4) for k, v in r['pass_ms'].items()})}")
    return res


# ------------------------------------------------------------- queue alone
def time_queue(eng, n, a):
    b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
    db = dev_batch(b)
    eng.reserve(b.n_txn, b.nnz)
    rc = eng.nowait_lock_epoch(db, want_conflict=False)[0]
    out = d.EpochBatch(torch.empty(n + 1, dtype=torch.int32, device=DEV),
                       torch.empty(b.nnz, dtype=torch.int64, device=DEV),
                       torch.empty(b.nnz, dtype=torch.uint8, device=DEV),
                       meta={"src": torch.empty(n, dtype=torch.int32, device=DEV),
                             "cnt": torch.empty(n, dtype=torch.int32, device=DEV),
                             "due": torch.empty(n, dtype=torch.int64, device=DEV)})
    cnt_in = torch.from_numpy(np.random.default_rng(5).integers(0, 2, size=n).astype(np.int32)).to(DEV)
    torch.cuda.synchronize()
    # EXP, penalty 1: cnt_in 0 -> due 2, cnt_in 1 -> due 4 (pushed at 0)
    qs = {"varying": eng.abort_queue(n, b.nnz, 1, 1 << 40, _abi.BACKOFF_EXP),
          "full": eng.abort_queue(n, b.nnz, 1, 1 << 40, _abi.BACKOFF_EXP, _abi.ABORTQ_SORT_FULL)}
    q = qs["varying"]

    def cycle(qq, now):
        qq.clear()
        pst = qq.push(db, rc, 0, cnt=cnt_in)[2]
        return pst, qq.pop(now, out=out)[1]

    def sel():
        return eng.select_batch(db, rc, RC_ABORT, out=out)[2]
    for _ in range(a.warmup):
        pst, _ = cycle(q, 5)
        cycle(q, 3)
        cycle(qs["full"], 5)
        sel()
        copy_ms(eng, pst["alg_bytes"])
    push, selm, cp, pop_all, pop_half, pop_full = [], [], [], [], [], []
    for _ in range(a.steps):  # alternately: all see the same machine state
        pst, ost = cycle(q, 5)
        push.append(pst["device_ms"])
        pop_all.append(ost["device_ms"])
        selm.append(sel()["device_ms"])
        cp.append(copy_ms(eng, pst["alg_bytes"]))
        hst = cycle(q, 3)[1]
        pop_half.append(hst["device_ms"])
        pop_full.append(cycle(qs["full"], 5)[1]["device_ms"])
    eng.set_profiling(True)
    names = ("flags", "sort", "gather", "keep")
    ph = {k: [cycle(qq, now)[1]["phase_ms"] for _ in range(5)]
          for k, qq, now in (("all", q, 5), ("half", q, 3), ("all_sort64", qs["full"], 5))}
    eng.set_profiling(False)
    for qq in qs.values():
        qq.close()
    r = {"parked": pst["n_commit"], "parked_frac": pst["n_commit"] / n, "push_alg_bytes": pst["alg_bytes"],
         "push_ms": mmm(push), "select_ms": mmm(selm), "copy_ms": mmm(cp),
         "push_over_select": statistics.median(push) / statistics.median(selm),
         "pop_all": {"released": ost["n_commit"], "alg_bytes": ost["alg_bytes"], "device_ms": mmm(pop_all)},
         "pop_half": {"released": hst["n_commit"], "alg_bytes": hst["alg_bytes"], "device_ms": mmm(pop_half)},
         "pop_all_sort64": {"device_ms": mmm(pop_full)},
         "phase_ms": {k: {nm: statistics.median(p[i] for p in v) for i, nm in enumerate(names)}
                      for k, v in ph.items()}}
    print(f"  parked {r['parked']} ({100 * r['parked_frac']:.1f} %)  push {fmt(r['push_ms'])}  select "
          f"{fmt(r['select_ms'])}  copy {fmt(r['copy_ms'])}  push/select {r['push_over_select']:.2f}")
    print(f"  pop all ({r['pop_all']['released']}) {fmt(r['pop_all']['device_ms'])}  half "
          f"({r['pop_half']['released']}) {fmt(r['pop_half']['device_ms'])}  all, 64-bit sort "
          f"{fmt(r['pop_all_sort64']['device_ms'])}")
    for k, v in r["phase_ms"].items():
        print(f"    phases {k}: {({nm: round(x, 4) for nm, x in v.items()})}")
    return r


# ------------------------------------------------------------- table alone
def time_table(eng, n, K, a):
    """Epoch K against the commits of epochs 0 .. K-1: in a lock table, and as
    a held list."""
    bs = [d.gen_ycsb(n_txn=n, zipf_theta=0.9, seed=2000 + e) for e in range(K + 1)]
    dbs = [dev_batch(b) for b in bs]
    m = sum(b.nnz for b in bs)
    eng.reserve(n, bs[0].nnz)
    lt = eng.locktab(m)
    held = d.EpochBatch(torch.empty(K * n + 1, dtype=torch.int32, device=DEV),
                        torch.empty(m, dtype=torch.int64, device=DEV), torch.empty(m, dtype=torch.uint8, device=DEV))
    tn = tm = 0
    for e in range(K):  # epoch e meets the commits of the epochs before it, and adds its own
        rc = lt.lock_epoch(dbs[e], want_conflict=False)[0]
        sel = eng.select_batch(dbs[e], rc, RC_RCOK, out=held, txn_base=tn, nnz_base=tm, want_src=False)[0]
        tn, tm = sel.n_txn, sel.nnz
    hk, ha = held.keys[:tm], held.acctype[:tm]
    rows, slots, _ = lt.size()
    cur = dbs[K]
    rc_t = torch.empty(n, dtype=torch.uint8, device=DEV)
    rc_h = torch.empty(n, dtype=torch.uint8, device=DEV)

    def table():
        est = lt.lock_epoch(cur, want_conflict=False, out_rc=rc_t)[2]
        return est, lt.release(cur, rc_t, RC_RCOK)[2]  # the table is as before

    def heldlist():
        return eng.nowait_lock_epoch(cur, held=(hk, ha), want_conflict=False, out_rc=rc_h)[2]
    for _ in range(a.warmup):
        est, rst = table()
        heldlist()
        copy_ms(eng, rst["alg_bytes"])
    same = bool(torch.equal(rc_t, rc_h))
    te, tr, th, cp = [], [], [], []
    for _ in range(a.steps):  # alternately: all see the same machine state
        est, rst = table()
        te.append(est["device_ms"])
        tr.append(rst["device_ms"])
        th.append(heldlist()["device_ms"])
        cp.append(copy_ms(eng, rst["alg_bytes"]))
    eng.set_profiling(True)
    prof = []
    for _ in range(5):
        est, rst = table()
        prof.append((lt.pass_ms(), est["phase_ms"], rst["phase_ms"], heldlist()["phase_ms"]))
    # a rebuild: a table with room for the held rows and the epoch, its other
    # slots taken by rows that were held once
    rebuild = []
    cap = max(rows + cur.nnz, tm) + 1024
    small = eng.locktab(cap)
    once = torch.arange(cap - rows - 512, dtype=torch.int64, device=DEV) + (1 << 40)
    once_at = torch.zeros(once.shape[0], dtype=torch.uint8, device=DEV)
    for _ in range(3):
        small.clear()
        small.acquire_rows(hk, ha)
        small.acquire_rows(once, once_at)
        small.release_rows(once)
        before = small.size()
        small.lock_epoch(cur, want_conflict=False, out_rc=rc_t)
        if small.size()[2] > before[2]:
            rebuild.append(small.pass_ms()["rebuild"])
    eng.set_profiling(False)
    small.close()
    lt.close()
    med = statistics.median
    r = {"n_txn": n, "held_epochs": K, "held_requests": tm, "held_rows": rows, "slots_used": slots,
         "rc_identical": same, "commits": est["n_commit"],
         "table_epoch_ms": mmm(te), "heldlist_epoch_ms": mmm(th), "release_ms": mmm(tr), "copy_ms": mmm(cp),
         "table_over_heldlist": med(te) / med(th),
         "release_alg_bytes": rst["alg_bytes"], "release_alg_GBps": rst["alg_bytes"] / (med(tr) * 1e-3) / 1e9,
         "release_over_copy": med(tr) / med(cp),
         "pass_ms": {k: med(p[0][k] for p in prof) for k in ("seed", "grant")},
         "table_phase_ms": [med(p[1][q] for p in prof) for q in range(4)],
         "release_phase_ms": [med(p[2][q] for p in prof) for q in range(4)],
         "heldlist_phase_ms": [med(p[3][q] for p in prof) for q in range(4)],
         "rebuild_ms": rebuild}
    print(f"  held {K} epoch(s): {tm} requests on {rows} rows; table epoch {fmt(r['table_epoch_ms'])}  held-list epoch "
          f"{fmt(r['heldlist_epoch_ms'])}  table/held-list {r['table_over_heldlist']:.2f}  rc identical {same}")
    print(f"    release {fmt(r['release_ms'])}  {r['release_alg_GBps']:.0f} GB/s  copy {fmt(r['copy_ms'])}  "
          f"release/copy {r['release_over_copy']:.2f}  seed {r['pass_ms']['seed']:.4f}  grant "
          f"{r['pass_ms']['grant']:.4f}  release phases {[round(x, 4) for x in r['release_phase_ms']]}  "
          f"rebuild {[round(x, 4) for x in rebuild]}")
    return r


# ------------------------------------------------------------- closed loop
def decide(eng, alg, cur, held):
    if alg == "nowait":
        rc, _, st = eng.nowait_lock_epoch(cur, held=held, want_conflict=False)
    else:
        rc, _, st = eng.occ_validate_epoch(cur)
    return rc, st


def loop_device(eng, alg, fresh_dev, E, bufs, timed):
    """Path A.  bufs: two sets of arrays the epochs alternate between."""
    F = fresh_dev[0].n_txn
    cur, held = fresh_dev[0], None
    wall, rcs, commits, sel_stats = [], [], 0, []
    for e in range(E):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, st = decide(eng, alg, cur, held)
        commits += st["n_commit"]
        if e + 1 < E:
            nf = fresh_dev[e + 1]
            if alg == "nowait":
                held = eng.held_from(cur, rc)
            out = bufs[e & 1]
            sel, _, sst = eng.select_batch(cur, rc, RC_ABORT, out=out, want_src=False)
            n0, m0 = sel.n_txn, sel.nnz
            torch.add(nf.offsets[1:], m0, out=out.offsets[n0 + 1:n0 + 1 + F])
            out.keys[m0:m0 + nf.nnz].copy_(nf.keys)
            out.acctype[m0:m0 + nf.nnz].copy_(nf.acctype)
            cur = d.EpochBatch(out.offsets[:n0 + F + 1], out.keys[:m0 + nf.nnz], out.acctype[:m0 + nf.nnz])
            sel_stats.append(sst)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        if not timed:
            rcs.append(rc.cpu().numpy().copy())
    return wall, rcs, commits, sel_stats


def loop_host(eng, alg, fresh, E, timed):
    """Path B: the carry of tests/test_gpu_nowait.py::test_held_rows_carried_over_epochs."""
    h = fresh[0]
    cur, held = h.to_torch(DEV), None
    wall, rcs, commits = [], [], 0
    for e in range(E):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, st = decide(eng, alg, cur, held)
        commits += st["n_commit"]
        hrc = rc.cpu().numpy()
        if e + 1 < E:
            nf = fresh[e + 1]
            lens = np.diff(h.offsets.astype(np.int64))
            ab = hrc == RC_ABORT
            per_req = np.repeat(ab, lens)
            if alg == "nowait":
                ok = np.repeat(hrc == RC_RCOK, lens)
                held = (torch.from_numpy(h.keys[ok].view(np.int64)).to(DEV), torch.from_numpy(h.acctype[ok]).to(DEV))
            off = np.concatenate([[0], np.cumsum(lens[ab])])
            m0 = int(off[-1])
            h = d.EpochBatch(np.concatenate([off, nf.offsets[1:].astype(np.int64) + m0]).astype(np.uint32),
                             np.concatenate([h.keys[per_req], nf.keys]),
                             np.concatenate([h.acctype[per_req], nf.acctype]))
            cur = h.to_torch(DEV)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        if not timed:
            rcs.append(hrc.copy())
    return wall, rcs, commits


def loop_device_backoff(eng, alg, fresh_dev, E, bufs, q, timed):
    """Path A with the device abort queue; the clock is the epoch index."""
    F = fresh_dev[0].n_txn
    q.clear()
    ids = [torch.arange(e * F, (e + 1) * F, dtype=torch.int32, device=DEV) for e in range(E)]
    cur, held = fresh_dev[0], None
    src, cnt = ids[0], torch.zeros(F, dtype=torch.int32, device=DEV)
    wall, rcs, commits, q_stats = [], [], 0, []
    for e in range(E):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, st = decide(eng, alg, cur, held)
        commits += st["n_commit"]
        if e + 1 < E:
            nf = fresh_dev[e + 1]
            if alg == "nowait":
                held = eng.held_from(cur, rc)
            pst = q.push(cur, rc, e, src=src, cnt=cnt)[2]
            out = bufs[e & 1]
            got, ost = q.pop(e + 1, out=out, want_due=False)
            n0, m0 = got.n_txn, got.nnz
            torch.add(nf.offsets[1:], m0, out=out.offsets[n0 + 1:n0 + 1 + F])
            out.keys[m0:m0 + nf.nnz].copy_(nf.keys)
            out.acctype[m0:m0 + nf.nnz].copy_(nf.acctype)
            out.meta["src"][n0:n0 + F].copy_(ids[e + 1])
            out.meta["cnt"][n0:n0 + F].zero_()
            cur = d.EpochBatch(out.offsets[:n0 + F + 1], out.keys[:m0 + nf.nnz], out.acctype[:m0 + nf.nnz])
            src, cnt = out.meta["src"][:n0 + F], out.meta["cnt"][:n0 + F]
            q_stats.append((pst, ost))
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        if not timed:
            rcs.append(rc.cpu().numpy().copy())
    return wall, rcs, commits, q_stats


def loop_host_backoff(eng, alg, fresh, E, rq, timed):
    """Path B with the reference queue (tests/abortq_ref.py) on the host."""
    F = fresh[0].n_txn
    rq.clear()
    h = fresh[0]
    h_src, h_cnt = np.arange(F, dtype=np.uint32), np.zeros(F, np.uint32)
    cur, held = h.to_torch(DEV), None
    wall, rcs, commits = [], [], 0
    for e in range(E):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, st = decide(eng, alg, cur, held)
        commits += st["n_commit"]
        hrc = rc.cpu().numpy()
        if e + 1 < E:
            nf = fresh[e + 1]
            if alg == "nowait":
                ok = np.repeat(hrc == RC_RCOK, np.diff(h.offsets.astype(np.int64)))
                held = (torch.from_numpy(h.keys[ok].view(np.int64)).to(DEV), torch.from_numpy(h.acctype[ok]).to(DEV))
            code, _, _ = rq.push(h, hrc, RC_ABORT, h_src, h_cnt, e)
            assert code == 0
            _, n0, m0, r = rq.pop(e + 1)
            h = d.EpochBatch(np.concatenate([r["offsets"], nf.offsets[1:] + np.uint32(m0)]).astype(np.uint32),
                             np.concatenate([r["keys"], nf.keys]), np.concatenate([r["acctype"], nf.acctype]))
            h_src = np.concatenate([r["src"], np.arange((e + 1) * F, (e + 2) * F, dtype=np.uint32)])
            h_cnt = np.concatenate([r["cnt"], np.zeros(F, np.uint32)])
            cur = h.to_torch(DEV)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        if not timed:
            rcs.append(hrc.copy())
    return wall, rcs, commits


def closed_loop_backoff(eng, a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import abortq_ref
    E, F = a.epochs, a.fresh
    policy = {"none": _abi.BACKOFF_NONE, "reference": _abi.BACKOFF_REFERENCE, "exp": _abi.BACKOFF_EXP}[a.backoff]
    fresh = [d.gen_ycsb(n_txn=F, zipf_theta=a.theta, seed=1000 + e) for e in range(E)]
    fresh_dev = [dev_batch(b) for b in fresh]
    cap_n, cap_m = E * F, sum(b.nnz for b in fresh)
    eng.reserve(cap_n, cap_m)
    bufs = [d.EpochBatch(torch.empty(cap_n + 1, dtype=torch.int32, device=DEV),
                         torch.empty(cap_m, dtype=torch.int64, device=DEV),
                         torch.empty(cap_m, dtype=torch.uint8, device=DEV),
                         meta={"src": torch.empty(cap_n, dtype=torch.int32, device=DEV),
                               "cnt": torch.empty(cap_n, dtype=torch.int32, device=DEV)}) for _ in range(2)]
    q = eng.abort_queue(cap_n, cap_m, a.penalty, a.penalty_max, policy)
    rq = abortq_ref.AbortQueue(cap_n, cap_m, a.penalty, a.penalty_max, policy)
    _, rc_a, _, _ = loop_device_backoff(eng, a.alg, fresh_dev, E, bufs, q, timed=False)
    _, rc_b, _ = loop_host_backoff(eng, a.alg, fresh, E, rq, timed=False)
    same = len(rc_a) == len(rc_b) and all(np.array_equal(x, y) for x, y in zip(rc_a, rc_b))
    for _ in range(max(a.loop_warmup - 1, 0)):
        loop_device_backoff(eng, a.alg, fresh_dev, E, bufs, q, timed=True)
        loop_host_backoff(eng, a.alg, fresh, E, rq, timed=True)
    wa, wb, ca, cb, qst = [], [], 0, 0, []
    for _ in range(a.loop_reps):  # alternately
        w, _, c, s = loop_device_backoff(eng, a.alg, fresh_dev, E, bufs, q, timed=True)
        wa += w
        ca += c
        qst += s
        w, _, c = loop_host_backoff(eng, a.alg, fresh, E, rq, timed=True)
        wb += w
        cb += c
    left = q.size()
    q.close()
    res = {"alg": a.alg, "epochs": E, "fresh": F, "theta": a.theta, "backoff": a.backoff, "penalty": a.penalty,
           "penalty_max": a.penalty_max, "rc_identical": bool(same),
           "txns_per_epoch": [int(r.size) for r in rc_a],
           "commits_per_epoch": [int((r == RC_RCOK).sum()) for r in rc_a],
           "parked_at_end": left,
           "A_queue": {"wall_ms_per_epoch": mmm(wa), "goodput_commits_per_s": ca / (sum(wa) * 1e-3),
                       "push_device_ms": mmm([s[0]["device_ms"] for s in qst]),
                       "pop_device_ms": mmm([s[1]["device_ms"] for s in qst])},
           "B_host": {"wall_ms_per_epoch": mmm(wb), "goodput_commits_per_s": cb / (sum(wb) * 1e-3)}}
    res["wall_B_over_A"] = res["B_host"]["wall_ms_per_epoch"]["median"] / res["A_queue"]["wall_ms_per_epoch"]["median"]
    res["goodput_A_over_B"] = res["A_queue"]["goodput_commits_per_s"] / res["B_host"]["goodput_commits_per_s"]
    print(f"closed loop {a.alg}, back-off {a.backoff} (penalty {a.penalty}, max {a.penalty_max}): {E} epochs of "
          f"{F} fresh txns, theta {a.theta}; txns per epoch {res['txns_per_epoch']}, commits "
          f"{res['commits_per_epoch']}, parked at the end {left}")
    for k in ("A_queue", "B_host"):
        r = res[k]
        print(f"  {k:9s} wall ms/epoch {fmt(r['wall_ms_per_epoch'])}  goodput {r['goodput_commits_per_s'] / 1e6:.2f} M commits/s"
              + (f"  push device_ms {fmt(r['push_device_ms'])}  pop device_ms {fmt(r['pop_device_ms'])}"
                 if "push_device_ms" in r else ""))
    print(f"  wall B / A = {res['wall_B_over_A']:.2f}  goodput A / B = {res['goodput_A_over_B']:.2f}  "
          f"rc identical {res['rc_identical']}")
    return res


def next_epoch(eng, cur, rc, nf, out):
    """aborted(cur) ++ the fresh txns nf, in the arrays of `out`."""
    F = nf.n_txn
    sel, _, sst = eng.select_batch(cur, rc, RC_ABORT, out=out, want_src=False)
    n0, m0 = sel.n_txn, sel.nnz
    torch.add(nf.offsets[1:], m0, out=out.offsets[n0 + 1:n0 + 1 + F])
    out.keys[m0:m0 + nf.nnz].copy_(nf.keys)
    out.acctype[m0:m0 + nf.nnz].copy_(nf.acctype)
    return d.EpochBatch(out.offsets[:n0 + F + 1], out.keys[:m0 + nf.nnz], out.acctype[:m0 + nf.nnz]), sst


def loop_hold_table(eng, fresh_dev, E, D, bufs, lt, timed):
    """Path A: the lock table holds the commits of the last D epochs."""
    lt.clear()
    cur = fresh_dev[0]
    wall, rcs, commits, stats, done = [], [], 0, [], []
    for e in range(E):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, _, st = lt.lock_epoch(cur, want_conflict=False)
        commits += st["n_commit"]
        done.append((cur, rc))
        rst = lt.release(*done[e - D], RC_RCOK)[2] if e >= D else None
        stats.append((st, rst))
        if e + 1 < E:
            cur, _ = next_epoch(eng, cur, rc, fresh_dev[e + 1], bufs[e % len(bufs)])
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        if not timed:
            rcs.append(rc.cpu().numpy().copy())
    return wall, rcs, commits, stats


def loop_hold_list(eng, fresh_dev, E, D, bufs, held, timed):
    """Path B: the held list is selected again from the last D epochs."""
    cur = fresh_dev[0]
    wall, rcs, commits, stats, done = [], [], 0, [], []
    for e in range(E):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tn = tm = 0
        for b, r in done[-D:]:
            sel = eng.select_batch(b, r, RC_RCOK, out=held, txn_base=tn, nnz_base=tm, want_src=False)[0]
            tn, tm = sel.n_txn, sel.nnz
        rc, _, st = eng.nowait_lock_epoch(cur, held=(held.keys[:tm], held.acctype[:tm]) if tm else None,
                                          want_conflict=False)
        commits += st["n_commit"]
        done.append((cur, rc))
        stats.append(st)
        if e + 1 < E:
            cur, _ = next_epoch(eng, cur, rc, fresh_dev[e + 1], bufs[e % len(bufs)])
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        if not timed:
            rcs.append(rc.cpu().numpy().copy())
    return wall, rcs, commits, stats


def closed_loop_hold(eng, a):
    E, F, D = a.epochs, a.fresh, a.hold
    fresh = [d.gen_ycsb(n_txn=F, zipf_theta=a.theta, seed=1000 + e) for e in range(E)]
    fresh_dev = [dev_batch(b) for b in fresh]
    cap_n, cap_m = E * F, sum(b.nnz for b in fresh)
    eng.reserve(cap_n, cap_m)
    # an epoch's arrays stay until its commits are released: D + 2 sets
    bufs = [d.EpochBatch(torch.empty(cap_n + 1, dtype=torch.int32, device=DEV),
                         torch.empty(cap_m, dtype=torch.int64, device=DEV),
                         torch.empty(cap_m, dtype=torch.uint8, device=DEV)) for _ in range(D + 2)]
    held = d.EpochBatch(torch.empty(cap_n + 1, dtype=torch.int32, device=DEV),
                        torch.empty(cap_m, dtype=torch.int64, device=DEV),
                        torch.empty(cap_m, dtype=torch.uint8, device=DEV))
    lt = eng.locktab(cap_m)  # every request of the run fits: no DCC_ERANGE whatever commits
    _, rc_a, _, _ = loop_hold_table(eng, fresh_dev, E, D, bufs, lt, timed=False)
    _, rc_b, _, _ = loop_hold_list(eng, fresh_dev, E, D, bufs, held, timed=False)
    same = len(rc_a) == len(rc_b) and all(np.array_equal(x, y) for x, y in zip(rc_a, rc_b))
    for _ in range(max(a.loop_warmup - 1, 0)):
        loop_hold_table(eng, fresh_dev, E, D, bufs, lt, timed=True)
        loop_hold_list(eng, fresh_dev, E, D, bufs, held, timed=True)
    wa, wb, ca, cb, sa, sb = [], [], 0, 0, [], []
    for _ in range(a.loop_reps):  # alternately
        w, _, c, s = loop_hold_table(eng, fresh_dev, E, D, bufs, lt, timed=True)
        wa += w
        ca += c
        sa += s
        w, _, c, s = loop_hold_list(eng, fresh_dev, E, D, bufs, held, timed=True)
        wb += w
        cb += c
        sb += s
    size = lt.size()
    lt.close()
    res = {"alg": "nowait", "epochs": E, "fresh": F, "theta": a.theta, "hold": D, "rc_identical": bool(same),
           "txns_per_epoch": [int(r.size) for r in rc_a],
           "commits_per_epoch": [int((r == RC_RCOK).sum()) for r in rc_a],
           "table_at_end": {"rows_held": size[0], "slots_used": size[1], "rebuilds": size[2]},
           "A_table": {"wall_ms_per_epoch": mmm(wa), "goodput_commits_per_s": ca / (sum(wa) * 1e-3),
                       "epoch_device_ms": mmm([s[0]["device_ms"] for s in sa]),
                       "release_device_ms": mmm([s[1]["device_ms"] for s in sa if s[1] is not None] or [0.0])},
           "B_heldlist": {"wall_ms_per_epoch": mmm(wb), "goodput_commits_per_s": cb / (sum(wb) * 1e-3),
                          "epoch_device_ms": mmm([s["device_ms"] for s in sb])}}
    res["wall_B_over_A"] = res["B_heldlist"]["wall_ms_per_epoch"]["median"] / res["A_table"]["wall_ms_per_epoch"]["median"]
    res["goodput_A_over_B"] = res["A_table"]["goodput_commits_per_s"] / res["B_heldlist"]["goodput_commits_per_s"]
    print(f"closed loop nowait, commits held for {D} epoch(s): {E} epochs of {F} fresh txns, theta {a.theta}; txns "
          f"per epoch {res['txns_per_epoch']}, commits {res['commits_per_epoch']}, table at the end "
          f"{res['table_at_end']}")
    for k in ("A_table", "B_heldlist"):
        r = res[k]
        print(f"  {k:10s} wall ms/epoch {fmt(r['wall_ms_per_epoch'])}  goodput {r['goodput_commits_per_s'] / 1e6:.2f} "
              f"M commits/s  epoch device_ms {fmt(r['epoch_device_ms'])}"
              + (f"  release device_ms {fmt(r['release_device_ms'])}" if "release_device_ms" in r else ""))
    print(f"  wall B / A = {res['wall_B_over_A']:.2f}  goodput A / B = {res['goodput_A_over_B']:.2f}  "
          f"rc identical {res['rc_identical']}")
    return res


def closed_loop(eng, a):
    E, F = a.epochs, a.fresh
    fresh = [d.gen_ycsb(n_txn=F, zipf_theta=a.theta, seed=1000 + e) for e in range(E)]
    fresh_dev = [dev_batch(b) for b in fresh]
    cap_n, cap_m = E * F, sum(b.nnz for b in fresh)
    eng.reserve(cap_n, cap_m)
    bufs = [d.EpochBatch(torch.empty(cap_n + 1, dtype=torch.int32, device=DEV),
                         torch.empty(cap_m, dtype=torch.int64, device=DEV),
                         torch.empty(cap_m, dtype=torch.uint8, device=DEV)) for _ in range(2)]
    # one untimed pass per path records the rc sequences
    _, rc_a, _, _ = loop_device(eng, a.alg, fresh_dev, E, bufs, timed=False)
    _, rc_b, _ = loop_host(eng, a.alg, fresh, E, timed=False)
    same = len(rc_a) == len(rc_b) and all(np.array_equal(x, y) for x, y in zip(rc_a, rc_b))
    for _ in range(max(a.loop_warmup - 1, 0)):
        loop_device(eng, a.alg, fresh_dev, E, bufs, timed=True)
        loop_host(eng, a.alg, fresh, E, timed=True)
    wa, wb, ca, cb, sst = [], [], 0, 0, []
    for _ in range(a.loop_reps):  # alternately
        w, _, c, s = loop_device(eng, a.alg, fresh_dev, E, bufs, timed=True)
        wa += w
        ca += c
        sst += s
        w, _, c = loop_host(eng, a.alg, fresh, E, timed=True)
        wb += w
        cb += c
    res = {"alg": a.alg, "epochs": E, "fresh": F, "theta": a.theta, "rc_identical": bool(same),
           "txns_per_epoch": [int(r.size) for r in rc_a],
           "commits_per_epoch": [int((r == RC_RCOK).sum()) for r in rc_a],
           "A_select": {"wall_ms_per_epoch": mmm(wa), "goodput_commits_per_s": ca / (sum(wa) * 1e-3),
                        "select_device_ms": mmm([s["device_ms"] for s in sst]),
                        "select_alg_GBps": statistics.median(s["alg_bytes"] / (s["device_ms"] * 1e-3) / 1e9
                                                             for s in sst)},
           "B_host": {"wall_ms_per_epoch": mmm(wb), "goodput_commits_per_s": cb / (sum(wb) * 1e-3)}}
    res["wall_B_over_A"] = res["B_host"]["wall_ms_per_epoch"]["median"] / res["A_select"]["wall_ms_per_epoch"]["median"]
    res["goodput_A_over_B"] = res["A_select"]["goodput_commits_per_s"] / res["B_host"]["goodput_commits_per_s"]
    print(f"closed loop {a.alg}: {E} epochs of {F} fresh txns, theta {a.theta}; txns per epoch "
          f"{res['txns_per_epoch']}, commits {res['commits_per_epoch']}")
    for k in ("A_select", "B_host"):
        r = res[k]
        print(f"  {k:9s} wall ms/epoch {fmt(r['wall_ms_per_epoch'])}  goodput {r['goodput_commits_per_s'] / 1e6:.2f} M commits/s"
              + (f"  select device_ms {fmt(r['select_device_ms'])}  {r['select_alg_GBps']:.0f} GB/s"
                 if "select_device_ms" in r else ""))
    print(f"  wall B / A = {res['wall_B_over_A']:.2f}  goodput A / B = {res['goodput_A_over_B']:.2f}  "
          f"rc identical {res['rc_identical']}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alg", choices=("nowait", "occ"), default="nowait")
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--fresh", type=int, default=65536)
    ap.add_argument("--theta", type=float, default=0.9)
    ap.add_argument("--loop-warmup", type=int, default=1)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--select-shapes", choices=("both", "c2", "headline", "none"), default="both")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--backoff", choices=("none", "reference", "exp"), default=None)
    ap.add_argument("--penalty", type=int, default=1)
    ap.add_argument("--penalty-max", type=int, default=4)
    ap.add_argument("--queue-shapes", choices=("both", "c2", "headline", "none"), default="none")
    ap.add_argument("--json", default=None)
    ap.add_argument("--hold", type=int, default=0, metavar="D")
    ap.add_argument("--table-shapes", choices=("both", "c2", "headline", "none"), default="none")
    a = ap.parse_args()
    if a.hold and (a.alg != "nowait" or a.backoff):
        ap.error("--hold goes with --alg nowait and without --backoff")
    assert torch.cuda.is_available(), "retry_loop needs cuda:0"
    out = {}
    with d.Engine(0) as eng:
        for name, n, key in (("C2 65,536 x 16", 65536, "c2"), ("headline 1,048,576 x 16", 1 << 20, "headline")):
            if a.select_shapes in ("both", key):
                print(f"select alone, {name}:")
                out[f"select {name}"] = time_select(eng, n, a)
            if a.queue_shapes in ("both", key):
                print(f"abort queue alone, {name}:")
                out[f"queue {name}"] = time_queue(eng, n, a)
            if a.table_shapes in ("both", key):
                print(f"lock table alone, {name}:")
                out[f"table {name}"] = {f"held_{K}": time_table(eng, n, K, a) for K in (1, 4)}
    with d.Engine(0) as eng:
        if a.epochs > 0:
            out["closed_loop"] = closed_loop_hold(eng, a) if a.hold else \
                closed_loop_backoff(eng, a) if a.backoff else closed_loop(eng, a)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    assert out.get("closed_loop", {}).get("rc_identical", True), "the two carries gave different rc sequences"


if __name__ == "__main__":
    main()
