"""Times the TIMESTAMP epoch (dcc_tso_validate_epoch) on resident device batches
next to the NO_WAIT lock epoch (dcc_nowait_lock_epoch), in one process on the
same batches: the C2 shape (65,536 x 16, theta 0.9) and the headline shape
(1,048,576 x 16, theta 0.9), with three timestamp patterns: index order, index
order with a jitter of up to 256, a random permutation.

    python tools/tso_bench.py [--warmup 5] [--steps 20] [--shape both|c2|headline]
                              [--pattern all|index|jitter|permuted] [--json PATH]

Every call's timestamps lie above those of the call before (ts + call * (n +
4096), as a timestamp allocator hands them out), so every epoch meets the row
table the epochs before it left: the rows exist, none of their wts / rts is
ahead of the epoch.  device_ms is the engine's own device time of the decision
(HIP events on its stream around the kernels of one call, batch resident); the
table reports the median of the timed calls with the minimum and maximum, the
rounds, and alg_bytes / device_ms.  Phase times come from separate profiled
calls.  Parity with the replay (tests/tso_ref.py) is checked on the C2 shape
after timing, from an empty row table."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deneva_amd as d  # noqa: E402
from tso_ref import replay  # noqa: E402  (checker only)

PATTERNS = ("index", "jitter", "permuted")


def pattern_ts(rng, n, pattern):
    idx = np.arange(n, dtype=np.uint64)
    if pattern == "index":
        return idx
    if pattern == "jitter":
        return idx + rng.integers(0, 257, size=n).astype(np.uint64)
    return rng.permutation(n).astype(np.uint64)


def summary(stats):
    ms = [s["device_ms"] for s in stats]
    med = statistics.median(ms)
    rounds = [s["rounds"] for s in stats]
    return {"device_ms": med, "device_ms_min": min(ms), "device_ms_max": max(ms),
            "rounds": int(statistics.median(rounds)), "rounds_max": max(rounds),
            "alg_bytes": stats[-1]["alg_bytes"],
            "alg_GBps": stats[-1]["alg_bytes"] / (med * 1e-3) / 1e9,
            "n_commit": stats[-1]["n_commit"], "n_abort": stats[-1]["n_abort"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=("both", "c2", "headline"), default="both",
                    help="one shape only (for a kernel trace of that shape)")
    ap.add_argument("--pattern", choices=("all",) + PATTERNS, default="all")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tso_bench needs cuda:0"
    out = {}
    with d.Engine(0) as eng:
        for name, n in (("C2 65,536 x 16", 65536), ("headline 1,048,576 x 16", 1 << 20)):
            if a.shape != "both" and (a.shape == "c2") != (n == 65536):
                continue
            b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
            db = b.to_torch("cuda:0")
            rc = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            cf = torch.empty(n, dtype=torch.int32, device="cuda:0")
            nrc = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            ncf = torch.empty(n, dtype=torch.int32, device="cuda:0")
            eng.reserve(b.n_txn, b.nnz)
            out[name] = {}
            for pattern in PATTERNS:
                if a.pattern not in ("all", pattern):
                    continue
                ts0 = pattern_ts(np.random.default_rng(7), n, pattern)
                dts0 = torch.from_numpy(ts0.view(np.int64)).to("cuda:0")
                eng.tso_rows_clear()
                call = [0]

                def tso():
                    call[0] += 1
                    dts = dts0 + call[0] * (n + 4096)
                    return eng.tso_validate_epoch(db, dts, out_rc=rc, out_conflict=cf)[2]

                def nowait():
                    return eng.nowait_lock_epoch(db, out_rc=nrc, out_conflict=ncf)[2]

                res = {}
                for _ in range(a.warmup):
                    tso()
                    nowait()
                # alternate the two so that both see the same machine state
                st_t, st_n = [], []
                for _ in range(a.steps):
                    st_t.append(tso())
                    st_n.append(nowait())
                torch.cuda.synchronize()
                res["tso"] = summary(st_t)
                res["nowait"] = summary(st_n)
                res["ratio"] = res["tso"]["device_ms"] / res["nowait"]["device_ms"]
                eng.set_profiling(True)
                for key, fn in (("tso", tso), ("nowait", nowait)):
                    ph = [fn()["phase_ms"] for _ in range(5)]
                    res[key]["phase_ms"] = [statistics.median(p[q] for p in ph) for q in range(4)]
                eng.set_profiling(False)
                res["rows"] = eng.tso_rows_size
                if n == 65536:
                    eng.tso_rows_clear()
                    rows = {}
                    erc, ecf = replay(b, ts0, rows)
                    eng.tso_validate_epoch(db, dts0, out_rc=rc, out_conflict=cf)
                    k = np.unique(b.keys)
                    w, r = eng.tso_rows_get(k)
                    ew = np.asarray([rows.get(int(x), (0, 0))[0] for x in k], np.uint64)
                    er = np.asarray([rows.get(int(x), (0, 0))[1] for x in k], np.uint64)
                    res["parity_vs_replay"] = bool(
                        np.array_equal(rc.cpu().numpy(), erc)
                        and np.array_equal(cf.cpu().numpy().view(np.uint32), ecf)
                        and np.array_equal(w, ew) and np.array_equal(r, er))
                out[name][pattern] = res
                print(f"{name}, ts {pattern}:")
                for key in ("tso", "nowait"):
                    r = res[key]
                    print(f"  {key:7s} device_ms {r['device_ms']:.3f} (min {r['device_ms_min']:.3f}, "
                          f"max {r['device_ms_max']:.3f})  rounds {r['rounds']}  "
                          f"alg {r['alg_GBps']:.1f} GB/s  commits {r['n_commit']}  "
                          f"phase_ms {[round(x, 3) for x in r['phase_ms']]}")
                print(f"  TIMESTAMP / NO_WAIT = {res['ratio']:.2f}"
                      + (f"  parity_vs_replay {res['parity_vs_replay']}" if "parity_vs_replay" in res else ""),
                      flush=True)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    assert all(r.get("parity_vs_replay", True) for s in out.values() for r in s.values()), \
        "TIMESTAMP differs from the replay"


if __name__ == "__main__":
    main()
