"""Times the MVCC epoch (dcc_mvcc_validate_epoch) on resident device batches next
to the TIMESTAMP epoch (dcc_tso_validate_epoch), alternating in one process on
the same batches and the same timestamps: the C2 shape (65,536 x 16, theta
0.9) and the headline shape (1,048,576 x 16, theta 0.9), with three timestamp
patterns: index order, index order with a jitter of up to 256, a random
permutation.

    python tools/mvcc_bench.py [--warmup 5] [--steps 20] [--shape both|c2|headline]
                               [--pattern all|index|jitter|permuted] [--growth] [--json PATH]

Every call's timestamps lie above those of the call before (ts + call * (n +
4096)), so every epoch meets the rows and the versions the epochs before it
left.  Before every MVCC call the store is trimmed with the call's lowest
timestamp as the floor (outside the timed region): it then holds one version
per written row, and the epoch's merge moves that plus its own commits.
device_ms is the engine's own device time (HIP events on its stream, batch
resident): median of the timed calls with minimum and maximum, rounds, commits,
late lookups (n_survivors), the store's size before and after the call, and
the phases from separate profiled calls.  --growth: the final pass + lookups +
merge time (phase 3) as a function of the store's size, eight epochs without a
trim and eight with one between the epochs.  Parity with the replay
(tests/mvcc_ref.py) is checked on the C2 shape after timing, from empty state."""
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
from mvcc_ref import replay, rows_of, versions_of  # noqa: E402  (checker only)

PATTERNS = ("index", "jitter", "permuted")


def pattern_ts(rng, n, pattern):
    idx = np.arange(n, dtype=np.uint64) + np.uint64(1)  # MVCC: ts >= 1
    if pattern == "index":
        return idx
    if pattern == "jitter":
        return idx + rng.integers(0, 257, size=n).astype(np.uint64)
    return np.uint64(1) + rng.permutation(n).astype(np.uint64)


def summary(stats):
    ms = [s["device_ms"] for s in stats]
    med = statistics.median(ms)
    return {"device_ms": med, "device_ms_min": min(ms), "device_ms_max": max(ms),
            "rounds": int(statistics.median(s["rounds"] for s in stats)),
            "n_commit": stats[-1]["n_commit"], "n_abort": stats[-1]["n_abort"],
            "late": stats[-1]["n_survivors"], "alg_bytes": stats[-1]["alg_bytes"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=("both", "c2", "headline"), default="both")
    ap.add_argument("--pattern", choices=("all",) + PATTERNS, default="all")
    ap.add_argument("--growth", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mvcc_bench needs cuda:0"
    out = {}
    with d.Engine(0) as eng:
        for name, n in (("C2 65,536 x 16", 65536), ("headline 1,048,576 x 16", 1 << 20)):
            if a.shape != "both" and (a.shape == "c2") != (n == 65536):
                continue
            b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
            db = b.to_torch("cuda:0")
            bufs = {e: (torch.empty(n, dtype=torch.uint8, device="cuda:0"),
                        torch.empty(n, dtype=torch.int32, device="cuda:0")) for e in ("mvcc", "tso")}
            vts = torch.empty(b.nnz, dtype=torch.int64, device="cuda:0")
            eng.reserve(b.n_txn, b.nnz)
            out[name] = {}
            for pattern in PATTERNS:
                if a.pattern not in ("all", pattern):
                    continue
                ts0 = pattern_ts(np.random.default_rng(7), n, pattern)
                dts0 = torch.from_numpy(ts0.view(np.int64)).to("cuda:0")
                eng.tso_rows_clear()
                eng.mvcc_clear()
                call = [0]
                sizes = []

                def pair(do_trim=True):
                    """One MVCC and one TIMESTAMP epoch at the same timestamps."""
                    call[0] += 1
                    base = call[0] * (n + 4096)
                    dts = dts0 + base
                    if do_trim:
                        eng.mvcc_trim(base)
                    before = eng.mvcc_versions_size
                    m = eng.mvcc_validate_epoch(db, dts, out_rc=bufs["mvcc"][0], out_conflict=bufs["mvcc"][1],
                                                out_vts=vts)[3]
                    sizes.append((before, eng.mvcc_versions_size))
                    t = eng.tso_validate_epoch(db, dts, out_rc=bufs["tso"][0], out_conflict=bufs["tso"][1])[2]
                    return m, t

                for _ in range(a.warmup):
                    pair()
                st = [pair() for _ in range(a.steps)]
                torch.cuda.synchronize()
                res = {"mvcc": summary([s[0] for s in st]), "tso": summary([s[1] for s in st])}
                res["mvcc"]["store_before"], res["mvcc"]["store_after"] = sizes[-1]
                res["ratio"] = res["mvcc"]["device_ms"] / res["tso"]["device_ms"]
                eng.set_profiling(True)
                ph = [pair() for _ in range(5)]
                for q, key in enumerate(("mvcc", "tso")):
                    res[key]["phase_ms"] = [statistics.median(p[q]["phase_ms"][x] for p in ph) for x in range(4)]
                if a.growth:
                    for mode, do_trim in (("untrimmed", False), ("trimmed", True)):
                        eng.mvcc_clear()
                        rows = []
                        for _ in range(8):
                            m, _ = pair(do_trim)
                            rows.append({"store_before": sizes[-1][0], "store_after": sizes[-1][1],
                                         "phase3_ms": m["phase_ms"][3], "device_ms": m["device_ms"]})
                        res["growth_" + mode] = rows
                eng.set_profiling(False)
                if n == 65536:
                    eng.mvcc_clear()
                    state = {}
                    erc, ecf, ev = replay(b, ts0, state)
                    eng.mvcc_validate_epoch(db, dts0, out_rc=bufs["mvcc"][0], out_conflict=bufs["mvcc"][1],
                                            out_vts=vts)
                    k = np.unique(b.keys)
                    w, r = eng.mvcc_rows_get(k)
                    rows = rows_of(state)
                    vk, vt = eng.mvcc_versions()
                    res["parity_vs_replay"] = bool(
                        np.array_equal(bufs["mvcc"][0].cpu().numpy(), erc)
                        and np.array_equal(bufs["mvcc"][1].cpu().numpy().view(np.uint32), ecf)
                        and np.array_equal(vts.cpu().numpy().view(np.uint64), ev)
                        and w.tolist() == [rows.get(int(x), (0, 0))[0] for x in k]
                        and r.tolist() == [rows.get(int(x), (0, 0))[1] for x in k]
                        and list(zip(vk.tolist(), vt.tolist())) == versions_of(state))
                out[name][pattern] = res
                print(f"{name}, ts {pattern}:")
                for key in ("mvcc", "tso"):
                    r = res[key]
                    print(f"  {key:5s} device_ms {r['device_ms']:.3f} (min {r['device_ms_min']:.3f}, "
                          f"max {r['device_ms_max']:.3f})  rounds {r['rounds']}  commits {r['n_commit']}  "
                          f"late {r['late']}  phase_ms {[round(x, 3) for x in r['phase_ms']]}"
                          + (f"  store {r['store_before']} -> {r['store_after']}" if key == "mvcc" else ""))
                for mode in ("untrimmed", "trimmed"):
                    for row in res.get("growth_" + mode, []):
                        print(f"  {mode}: store {row['store_before']} -> {row['store_after']}  "
                              f"phase 3 {row['phase3_ms']:.3f} ms  device_ms {row['device_ms']:.3f}")
                print(f"  MVCC / TIMESTAMP = {res['ratio']:.2f}"
                      + (f"  parity_vs_replay {res['parity_vs_replay']}" if "parity_vs_replay" in res else ""),
                      flush=True)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    assert all(r.get("parity_vs_replay", True) for s in out.values() for r in s.values()), \
        "MVCC differs from the replay"


if __name__ == "__main__":
    main()
