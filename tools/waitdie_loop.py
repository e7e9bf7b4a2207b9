"""The closed WAIT_DIE loop on a device-resident population, and the call that
closes it (dcc_waitdie_carry) alone.

    python tools/waitdie_loop.py [--epochs 8] [--fresh 65536] [--theta 0.9]
                                 [--loop-warmup 1] [--loop-reps 3]
                                 [--shapes both|c2|headline|none] [--warmup 5] [--steps 20]
                                 [--json PATH]

Per epoch the loop runs
  1. dcc_waitdie_lock_epoch on the population,
  2. dcc_waitdie_release of every RCOK and ABORT txn,
  3. the next population: the waiters and the promoted txns stay, the died txns
     are revived at once with the ts they keep, `--fresh` new YCSB txns arrive
     with ts from a global arrival counter.
Steps 1 and 2 are the same device calls on both paths; step 3 runs two ways:
  device  dcc_waitdie_carry on device arrays, ping-ponged between two buffers
  host    rc and pos are copied to the host, the population (whose CSR, ts and
          src the host mirrors) is compacted with numpy and copied back: the
          loop without the carry call
Both paths alternate, after one untimed pass each that records the states: the
tool reports per-epoch device ms of epoch / release / carry, wall ms per epoch
of both paths, goodput (RCOK txns per second over the run), the population per
epoch and rc_identical (both paths reach the same rc / pos after every epoch).
The first three epochs are then replayed through tests/waitdie_ref.py (parity).

--shapes times the carry alone on a population of 65,536 x 16 (C2) and
1,048,576 x 16 (headline) txns in the state one epoch and one release leave,
the died txns revived: without fresh txns, beside a dcc_batch_select of the
same kept set into the same arrays (the comparable existing call: the same
tile bodies, one per-txn array instead of four), and with as many fresh txns
again, beside the engine's device copy moving the same bytes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deneva_amd as d  # noqa: E402
from deneva_amd import RC_ABORT, RC_RCOK, WD_GONE, WD_RUN, _abi  # noqa: E402
from waitdie_ref import replay_epoch, replay_release  # noqa: E402  (checker only)

DEV = "cuda:0"


def mmm(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def fmt(m):
    return f"{m['median']:.3f} [{m['min']:.3f}, {m['max']:.3f}]"


def dev(a):
    a = np.ascontiguousarray(a)
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return torch.from_numpy(a.view(view)).to(DEV)


def dev_batch(b):
    return d.EpochBatch(dev(b.offsets), dev(b.keys), dev(b.acctype))


def copy_ms(eng, traffic_bytes):
    """The engine's device copy moving `traffic_bytes` in all (read + written)."""
    g = C.c_double(0)
    code = _abi.lib.dcc_copy_bandwidth(eng.handle, max(traffic_bytes // 2, 16), 1, C.byref(g))
    assert code == 0
    return traffic_bytes / (g.value * 1e9) * 1e3


def out_buffers(cap_n, cap_m):
    o = d.EpochBatch(torch.empty(cap_n + 1, dtype=torch.int32, device=DEV),
                     torch.empty(cap_m, dtype=torch.int64, device=DEV),
                     torch.empty(cap_m, dtype=torch.uint8, device=DEV))
    o.meta["cap"] = (cap_n, cap_m)
    return o


# ------------------------------------------------------------- the carry alone
def time_carry(eng, n, a):
    b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
    f = d.gen_ycsb(n_txn=n, zipf_theta=0.9, seed=77)
    db, df = dev_batch(b), dev_batch(f)
    eng.reserve(n, b.nnz)
    ts = dev(np.arange(n, dtype=np.uint64) + np.random.default_rng(7).integers(0, 257, size=n).astype(np.uint64))
    fts = dev(np.arange(n, 2 * n, dtype=np.uint64))
    rc = torch.full((n,), WD_RUN, dtype=torch.uint8, device=DEV)
    pos = torch.zeros(n, dtype=torch.int32, device=DEV)
    eng.waitdie_lock_epoch(db, ts, rc, pos, want_conflict=False)
    died = (rc == RC_ABORT).to(torch.uint8)
    eng.waitdie_release(db, ts, rc, pos, ((rc == RC_RCOK) | (rc == RC_ABORT)).to(torch.uint8))
    stay = ((rc != WD_GONE) | (died != 0)).to(torch.uint8)  # the kept set as a decision byte
    out = out_buffers(2 * n, b.nnz + f.nnz)
    calls = {
        "carry": lambda: eng.waitdie_carry(db, ts, rc, pos, revive=died, out=out)[6],
        "select": lambda: eng.select_batch(db, stay, 1, out=out)[2],
        "carry_fresh": lambda: eng.waitdie_carry(db, ts, rc, pos, revive=died, fresh=df, fresh_ts=fts,
                                                 fresh_src_base=n, out=out)[6],
    }
    for _ in range(a.warmup):
        for fn in calls.values():
            copy_ms(eng, fn()["alg_bytes"])
    ms = {k: [] for k in calls}
    cp = {k: [] for k in calls}
    for _ in range(a.steps):  # alternately: all see the same machine state
        for k, fn in calls.items():
            st = fn()
            ms[k].append(st["device_ms"])
            cp[k].append(copy_ms(eng, st["alg_bytes"]))
    eng.set_profiling(True)
    res = {"n_txn": n, "nnz": b.nnz, "n_fresh": n, "nnz_fresh": f.nnz}
    for k, fn in calls.items():
        ph = [fn()["phase_ms"] for _ in range(5)]
        st = fn()
        med = statistics.median(ms[k])
        res[k] = {"kept": st["n_commit"], "kept_frac": st["n_commit"] / n, "revived": st["n_survivors"],
                  "alg_bytes": st["alg_bytes"], "device_ms": mmm(ms[k]), "copy_ms": mmm(cp[k]),
                  "alg_GBps": st["alg_bytes"] / (med * 1e-3) / 1e9, "over_copy": med / statistics.median(cp[k]),
                  "phase_ms": [statistics.median(p[q] for p in ph) for q in range(4)]}
    eng.set_profiling(False)
    res["carry_over_select"] = res["carry"]["device_ms"]["median"] / res["select"]["device_ms"]["median"]
    for k in calls:
        r = res[k]
        print(f"  {k:11s} kept {r['kept']} ({100 * r['kept_frac']:.1f} %)  device_ms {fmt(r['device_ms'])}  "
              f"{r['alg_GBps']:.0f} GB/s  copy_ms {fmt(r['copy_ms'])}  / copy {r['over_copy']:.2f}  "
              f"phases {[round(x, 4) for x in r['phase_ms']]}")
    print(f"  carry / select of the same kept set = {res['carry_over_select']:.2f}", flush=True)
    return res


# ------------------------------------------------------------------- the loop
def run_epoch(eng, cur, ts, rc, pos):
    """Steps 1 and 2 on device arrays; rc / pos are updated in place."""
    est = eng.waitdie_lock_epoch(cur, ts, rc, pos, want_conflict=False)[3]
    died = (rc == RC_ABORT).to(torch.uint8)
    after_epoch = rc.clone()
    leave = ((rc == RC_RCOK) | (rc == RC_ABORT)).to(torch.uint8)
    rst = eng.waitdie_release(cur, ts, rc, pos, leave)[2]
    return est, rst, died, after_epoch


def first_state(n):
    return (torch.full((n,), WD_RUN, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV))


def loop_device(eng, fresh_dev, fresh_ts, E, bufs, timed):
    F = fresh_dev[0].n_txn
    cur, ts = fresh_dev[0], fresh_ts[0]
    rc, pos = first_state(F)
    src = torch.arange(F, dtype=torch.int32, device=DEV)
    wall, states, commits, ms, pop = [], [], 0, {"epoch": [], "release": [], "carry": []}, []
    for e in range(E):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pop.append(cur.n_txn)
        est, rst, died, after_epoch = run_epoch(eng, cur, ts, rc, pos)
        commits += est["n_commit"]
        ms["epoch"].append(est["device_ms"])
        ms["release"].append(rst["device_ms"])
        if not timed:
            states.append((src.clone(), after_epoch, rc.clone(), pos.clone()))
        if e + 1 < E:
            cur, ts, rc, pos, src, _, cst = eng.waitdie_carry(cur, ts, rc, pos, revive=died, src_in=src,
                                                              fresh=fresh_dev[e + 1], fresh_ts=fresh_ts[e + 1],
                                                              fresh_src_base=(e + 1) * F, out=bufs[e & 1])
            ms["carry"].append(cst["device_ms"])
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall, states, commits, ms, pop


def loop_host(eng, fresh, fresh_ts_h, E, timed):
    F = fresh[0].n_txn
    h, hts = fresh[0], fresh_ts_h[0]
    hsrc = np.arange(F, dtype=np.uint32)
    cur, ts = dev_batch(h), dev(hts)
    rc, pos = first_state(F)
    wall, states, commits, pops = [], [], 0, []
    for e in range(E):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if not timed and e < 3:
            pops.append((h, hts))
        est, rst, died, after_epoch = run_epoch(eng, cur, ts, rc, pos)
        commits += est["n_commit"]
        if not timed:
            states.append((dev(hsrc), after_epoch, rc.clone(), pos.clone()))
        if e + 1 < E:
            hrc, hpos, hdied = rc.cpu().numpy(), pos.cpu().numpy().view(np.uint32), died.cpu().numpy() != 0
            nf = fresh[e + 1]
            lens = np.diff(h.offsets.astype(np.int64))
            stay = (hrc != WD_GONE) | hdied
            per_req = np.repeat(stay, lens)
            off = np.concatenate([[0], np.cumsum(lens[stay])])
            m0 = int(off[-1])
            h = d.EpochBatch(np.concatenate([off, nf.offsets[1:].astype(np.int64) + m0]).astype(np.uint32),
                             np.concatenate([h.keys[per_req], nf.keys]),
                             np.concatenate([h.acctype[per_req], nf.acctype]))
            hts = np.concatenate([hts[stay], fresh_ts_h[e + 1]])
            hsrc = np.concatenate([hsrc[stay], np.arange((e + 1) * F, (e + 2) * F, dtype=np.uint32)])
            nrc = np.concatenate([np.where(hdied[stay], WD_RUN, hrc[stay]), np.full(F, WD_RUN)]).astype(np.uint8)
            npos = np.concatenate([np.where(hdied[stay], 0, hpos[stay]), np.zeros(F)]).astype(np.uint32)
            cur, ts, rc, pos = dev_batch(h), dev(hts), dev(nrc), dev(npos)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall, states, commits, pops


def closed_loop(eng, a):
    E, F = a.epochs, a.fresh
    fresh = [d.gen_ycsb(n_txn=F, zipf_theta=a.theta, seed=1000 + e) for e in range(E)]
    fresh_ts_h = [np.arange(e * F, (e + 1) * F, dtype=np.uint64) + np.uint64(1) for e in range(E)]  # arrival counter
    fresh_dev = [dev_batch(b) for b in fresh]
    fresh_ts = [dev(t) for t in fresh_ts_h]
    cap_n, cap_m = E * F, sum(b.nnz for b in fresh)
    eng.reserve(cap_n, cap_m)
    bufs = [out_buffers(cap_n, cap_m) for _ in range(2)]
    # one untimed pass per path records the states
    _, sa, _, _, pop = loop_device(eng, fresh_dev, fresh_ts, E, bufs, timed=False)
    _, sb, _, pops = loop_host(eng, fresh, fresh_ts_h, E, timed=False)
    same = len(sa) == len(sb) and all(torch.equal(x, y) for p, q in zip(sa, sb) for x, y in zip(p, q))
    for _ in range(max(a.loop_warmup - 1, 0)):
        loop_device(eng, fresh_dev, fresh_ts, E, bufs, timed=True)
        loop_host(eng, fresh, fresh_ts_h, E, timed=True)
    wa, wb, ca, cb = [], [], 0, 0
    ms = {"epoch": [], "release": [], "carry": []}
    for _ in range(a.loop_reps):  # alternately
        w, _, c, m, _ = loop_device(eng, fresh_dev, fresh_ts, E, bufs, timed=True)
        wa.append(w)
        ca += c
        for k in ms:
            ms[k].append(m[k])
        w, _, c, _ = loop_host(eng, fresh, fresh_ts_h, E, timed=True)
        wb.append(w)
        cb += c
    per_epoch = lambda runs: [statistics.median(r[e] for r in runs) for e in range(len(runs[0]))]
    flat = lambda runs: [x for r in runs for x in r]
    # parity: the first epochs of the host path's populations through the replay
    parity = True
    for e, (h, hts) in enumerate(pops):
        n = h.n_txn
        prev = (np.full(n, WD_RUN, np.uint8), np.zeros(n, np.uint32)) if e == 0 else nxt
        ep = replay_epoch(h, hts, *prev)
        parity &= np.array_equal(sa[e][1].cpu().numpy(), ep[0])
        lv = np.isin(ep[0], [RC_RCOK, RC_ABORT]).astype(np.uint8)
        rl = replay_release(h, hts, ep[0], ep[1], lv)
        parity &= np.array_equal(sa[e][2].cpu().numpy(), rl[0])
        parity &= np.array_equal(sa[e][3].cpu().numpy().view(np.uint32), rl[1])
        if e + 1 < len(pops):  # the state the next population starts from, as loop_host builds it
            stay = (rl[0] != WD_GONE) | (ep[0] == RC_ABORT)
            died = (ep[0] == RC_ABORT)[stay]
            nxt = (np.concatenate([np.where(died, WD_RUN, rl[0][stay]), np.full(F, WD_RUN)]).astype(np.uint8),
                   np.concatenate([np.where(died, 0, rl[1][stay]), np.zeros(F)]).astype(np.uint32))
    res = {"epochs": E, "fresh": F, "theta": a.theta, "rc_identical": bool(same),
           "parity_vs_replay": bool(parity), "parity_epochs": len(pops), "population_per_epoch": pop,
           "commits_per_epoch": [int((s[1] == RC_RCOK).sum().item()) for s in sa],
           "device_ms_per_epoch": {k: per_epoch(v) for k, v in ms.items()},
           "device_ms": {k: mmm(flat(v)) for k, v in ms.items()},
           "A_carry": {"wall_ms_per_epoch": per_epoch(wa), "wall_ms": mmm(flat(wa)),
                       "goodput_commits_per_s": ca / (sum(flat(wa)) * 1e-3)},
           "B_host": {"wall_ms_per_epoch": per_epoch(wb), "wall_ms": mmm(flat(wb)),
                      "goodput_commits_per_s": cb / (sum(flat(wb)) * 1e-3)}}
    res["wall_B_over_A"] = res["B_host"]["wall_ms"]["median"] / res["A_carry"]["wall_ms"]["median"]
    res["goodput_A_over_B"] = res["A_carry"]["goodput_commits_per_s"] / res["B_host"]["goodput_commits_per_s"]
    print(f"closed loop waitdie: {E} epochs of {F} fresh txns, theta {a.theta}; population per epoch {pop}, "
          f"RCOK {res['commits_per_epoch']}")
    print("  device ms  " + "  ".join(f"{k} {fmt(v)}" for k, v in res["device_ms"].items()))
    for k in ("A_carry", "B_host"):
        r = res[k]
        print(f"  {k:8s} wall ms/epoch {fmt(r['wall_ms'])}  per epoch {[round(x, 2) for x in r['wall_ms_per_epoch']]}  "
              f"goodput {r['goodput_commits_per_s'] / 1e6:.2f} M RCOK/s")
    print(f"  wall B / A = {res['wall_B_over_A']:.2f}  goodput A / B = {res['goodput_A_over_B']:.2f}  "
          f"rc identical {res['rc_identical']}  parity with the replay ({len(pops)} epochs) {res['parity_vs_replay']}",
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--fresh", type=int, default=65536)
    ap.add_argument("--theta", type=float, default=0.9)
    ap.add_argument("--loop-warmup", type=int, default=1)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--shapes", choices=("both", "c2", "headline", "none"), default="both")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "waitdie_loop needs cuda:0"
    out = {}
    with d.Engine(0) as eng:
        for name, n, key in (("C2 65,536 x 16", 65536, "c2"), ("headline 1,048,576 x 16", 1 << 20, "headline")):
            if a.shapes in ("both", key):
                print(f"carry alone, {name}:")
                out[f"carry {name}"] = time_carry(eng, n, a)
    with d.Engine(0) as eng:
        if a.epochs > 0:
            out["closed_loop"] = closed_loop(eng, a)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    loop = out.get("closed_loop", {})
    assert loop.get("rc_identical", True), "the two paths reached different states"
    assert loop.get("parity_vs_replay", True), "the loop differs from the replay"


if __name__ == "__main__":
    main()
