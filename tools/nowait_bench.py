"""Times the NO_WAIT lock epoch (dcc_nowait_lock_epoch) on resident device
batches next to the OCC round solver (dcc_occ_validate_epoch with
DCC_OPT_SOLVER = 1, the design it parallels), in one process on the same
batches: the C2 shape (65,536 x 16, theta 0.9) and the headline shape
(1,048,576 x 16, theta 0.9).

    python tools/nowait_bench.py [--warmup 5] [--steps 20] [--shape both|c2|headline]
                                 [--check-1m] [--json PATH] [--shards R]
                                 [--isolation ser|rc|ru|all]

device_ms is the engine's own device time of the decision (HIP events on its
stream around the kernels of one call, batch resident); the table reports the
median of the timed calls with the minimum and maximum, the rounds, and
alg_bytes / device_ms.  Parity with the Row_lock replay (tests/nowait_ref.py)
is checked on the C2 shape after timing; --check-1m also replays the headline
shape (~30 s of Python).  Phase times come from a separate profiled call.

--shards R times the key-sharded epoch (DCC_SHARD_SELF) alone,
on Engine(devices=[0] * R): R ranks that share cuda:0 and exchange through the
host, so the figures show what sharding costs and how much smaller a rank's
lock table is, not how it scales.  R = 1 is the unflagged epoch on one
context.  device_ms is the maximum over the ranks; the collectives come from
dcc_comm_calls, the table bytes from the sizing rule (16-byte slots, the next
power of two above 1.25 x the rank's own requests, at least 1,024).

--isolation times the epoch at the isolation levels (DCC_ISO_*, DESIGN.md
§8q): the levels chosen and the OCC round solver alternate call by call in one
process on the same resident batches; parity with the levels' replay
(tests/nowait_iso_ref.py) is checked on the C2 shape after timing, and every
result carries its level."""
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
from deneva_amd import _abi  # noqa: E402
from nowait_ref import replay  # noqa: E402  (checker only)

ISO = {"ser": d.ISO_SERIALIZABLE, "rc": d.ISO_READ_COMMITTED, "ru": d.ISO_READ_UNCOMMITTED}


def summary(stats):
    ms = [s["device_ms"] for s in stats]
    med = statistics.median(ms)
    return {"device_ms": med, "device_ms_min": min(ms), "device_ms_max": max(ms),
            "rounds": stats[-1]["rounds"], "alg_bytes": stats[-1]["alg_bytes"],
            "alg_GBps": stats[-1]["alg_bytes"] / (med * 1e-3) / 1e9,
            "n_commit": stats[-1]["n_commit"], "n_abort": stats[-1]["n_abort"]}


def table_bytes(requests):
    cap = 1024
    while cap < requests + requests // 4 + 1:
        cap *= 2
    return 16 * cap


def run_shards(a):
    R = a.shards
    out = {}
    with (d.Engine(0) if R == 1 else d.Engine(devices=[0] * R)) as eng:
        for name, n in (("C2 65,536 x 16", 65536), ("headline 1,048,576 x 16", 1 << 20)):
            if a.shape != "both" and (a.shape == "c2") != (n == 65536):
                continue
            b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
            db = b.to_torch("cuda:0")
            rc = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            cf = torch.empty(n, dtype=torch.int32, device="cuda:0")
            eng.reserve(b.n_txn, b.nnz)

            def nowait():
                return eng.nowait_lock_epoch(db, out_rc=rc, out_conflict=cf, shard=R > 1)[2]

            for _ in range(a.warmup):
                nowait()
            c0 = eng.comm_calls
            st = [nowait() for _ in range(a.steps)]
            torch.cuda.synchronize()
            res = summary(st)
            assert st[-1]["n_shards"] == R
            res["shards"] = R
            res["collectives_per_epoch"] = (eng.comm_calls - c0) / (R * a.steps)
            res["bytes_exchanged_per_rank"] = int(res["collectives_per_epoch"] * n)
            own = np.bincount(d.shard_of_keys(np.asarray(b.keys), R), minlength=R)
            res["own_requests"] = own.tolist()
            res["table_bytes_per_rank"] = [table_bytes(int(c)) for c in own]
            res["table_bytes_one_gpu"] = table_bytes(b.nnz)
            if n == 65536 or a.check_1m:
                erc, ecf = replay(b)
                res["parity_vs_replay"] = bool(
                    np.array_equal(rc.cpu().numpy(), erc)
                    and np.array_equal(cf.cpu().numpy().view(np.uint32), ecf))
            out[name] = res
            print(f"{name}: shards {R}  device_ms {res['device_ms']:.3f} (min {res['device_ms_min']:.3f}, "
                  f"max {res['device_ms_max']:.3f})  rounds {res['rounds']}  "
                  f"collectives {res['collectives_per_epoch']:.1f}  "
                  f"exchanged {res['bytes_exchanged_per_rank']} B  "
                  f"table {max(res['table_bytes_per_rank'])} B of {res['table_bytes_one_gpu']} B"
                  + (f"  parity_vs_replay {res['parity_vs_replay']}" if "parity_vs_replay" in res else ""))
    return out


def run_isolation(a):
    from nowait_iso_ref import replay as iso_replay  # checker only
    levels = list(ISO) if a.isolation == "all" else [a.isolation]
    out = {}
    with d.Engine(0) as eng:
        for name, n in (("C2 65,536 x 16", 65536), ("headline 1,048,576 x 16", 1 << 20)):
            if a.shape != "both" and (a.shape == "c2") != (n == 65536):
                continue
            b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
            db = b.to_torch("cuda:0")
            rc = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            cf = torch.empty(n, dtype=torch.int32, device="cuda:0")
            orc = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            eng.reserve(b.n_txn, b.nnz)

            def nowait(lv):
                return eng.nowait_lock_epoch(db, out_rc=rc, out_conflict=cf, isolation=ISO[lv])[2]

            def occ():
                return eng.occ_validate_epoch(db, out_rc=orc)[2]

            eng.set_option(_abi.OPT_SOLVER, 1)
            for _ in range(a.warmup):
                for lv in levels:
                    nowait(lv)
                occ()
            st = {lv: [] for lv in levels}
            st_o = []
            for _ in range(a.steps):  # alternate, so that all see the same machine state
                for lv in levels:
                    st[lv].append(nowait(lv))
                st_o.append(occ())
            torch.cuda.synchronize()
            res = {lv: dict(summary(st[lv]), isolation=lv) for lv in levels}
            res["occ_rounds"] = summary(st_o)
            eng.set_profiling(True)
            for lv in levels:
                ph = [nowait(lv)["phase_ms"] for _ in range(5)]
                res[lv]["phase_ms"] = [statistics.median(p[q] for p in ph) for q in range(4)]
            eng.set_profiling(False)
            eng.set_option(_abi.OPT_SOLVER, 0)
            for lv in levels:
                res[lv]["ratio_to_occ_rounds"] = res[lv]["device_ms"] / res["occ_rounds"]["device_ms"]
                if "ser" in res:
                    res[lv]["ratio_to_ser"] = res[lv]["device_ms"] / res["ser"]["device_ms"]
                if n == 65536 or a.check_1m:
                    erc, ecf = iso_replay(b, None, ISO[lv])
                    nowait(lv)
                    res[lv]["parity_vs_replay"] = bool(
                        np.array_equal(rc.cpu().numpy(), erc)
                        and np.array_equal(cf.cpu().numpy().view(np.uint32), ecf))
            out[name] = res
            print(f"{name}:")
            for lv in levels:
                r = res[lv]
                print(f"  {lv:10s} device_ms {r['device_ms']:.3f} (min {r['device_ms_min']:.3f}, "
                      f"max {r['device_ms_max']:.3f})  rounds {r['rounds']}  "
                      f"commits {r['n_commit']}  aborts {r['n_abort']}  "
                      f"phase_ms {[round(x, 3) for x in r['phase_ms']]}  x OCC rounds {r['ratio_to_occ_rounds']:.2f}"
                      + (f"  parity_vs_replay {r['parity_vs_replay']}" if "parity_vs_replay" in r else ""))
            r = res["occ_rounds"]
            print(f"  occ_rounds device_ms {r['device_ms']:.3f} (min {r['device_ms_min']:.3f}, "
                  f"max {r['device_ms_max']:.3f})  rounds {r['rounds']}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=("both", "c2", "headline"), default="both",
                    help="one shape only (for a kernel trace of that shape)")
    ap.add_argument("--check-1m", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--shards", type=int, default=0,
                    help="time the key-sharded epoch on R ranks sharing cuda:0 (1: the unflagged epoch)")
    ap.add_argument("--isolation", choices=("ser", "rc", "ru", "all"), default=None,
                    help="time the epoch at these isolation levels, alternating in one process")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nowait_bench needs cuda:0"
    assert not (a.shards and a.isolation), "a key-sharded epoch is SERIALIZABLE only"
    out = {}
    if a.shards:
        out = run_shards(a)
    if a.isolation:
        out = run_isolation(a)
    with d.Engine(0) as eng:
        for name, n in (("C2 65,536 x 16", 65536), ("headline 1,048,576 x 16", 1 << 20)):
            if a.shards or a.isolation or (a.shape != "both" and (a.shape == "c2") != (n == 65536)):
                continue
            b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
            db = b.to_torch("cuda:0")
            rc = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            cf = torch.empty(n, dtype=torch.int32, device="cuda:0")
            orc = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            eng.reserve(b.n_txn, b.nnz)

            def nowait():
                return eng.nowait_lock_epoch(db, out_rc=rc, out_conflict=cf)[2]

            def occ():
                return eng.occ_validate_epoch(db, out_rc=orc)[2]

            eng.set_option(_abi.OPT_SOLVER, 1)
            res = {}
            for _ in range(a.warmup):
                nowait()
                occ()
            # alternate the two so that both see the same machine state
            st_n, st_o = [], []
            for _ in range(a.steps):
                st_n.append(nowait())
                st_o.append(occ())
            torch.cuda.synchronize()
            res["nowait"] = summary(st_n)
            res["occ_rounds"] = summary(st_o)
            res["ratio"] = res["nowait"]["device_ms"] / res["occ_rounds"]["device_ms"]
            eng.set_profiling(True)
            for key, fn in (("nowait", nowait), ("occ_rounds", occ)):
                ph = [fn()["phase_ms"] for _ in range(5)]
                res[key]["phase_ms"] = [statistics.median(p[q] for p in ph) for q in range(4)]
            eng.set_profiling(False)
            eng.set_option(_abi.OPT_SOLVER, 0)
            if n == 65536 or a.check_1m:
                erc, ecf = replay(b)
                nowait()
                res["parity_vs_replay"] = bool(
                    np.array_equal(rc.cpu().numpy(), erc)
                    and np.array_equal(cf.cpu().numpy().view(np.uint32), ecf))
            out[name] = res
            print(f"{name}:")
            for key in ("nowait", "occ_rounds"):
                r = res[key]
                print(f"  {key:10s} device_ms {r['device_ms']:.3f} (min {r['device_ms_min']:.3f}, "
                      f"max {r['device_ms_max']:.3f})  rounds {r['rounds']}  "
                      f"alg {r['alg_GBps']:.1f} GB/s  commits {r['n_commit']}  "
                      f"phase_ms {[round(x, 3) for x in r['phase_ms']]}")
            print(f"  NO_WAIT / OCC rounds = {res['ratio']:.2f}"
                  + (f"  parity_vs_replay {res['parity_vs_replay']}" if "parity_vs_replay" in res else ""))
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    flat = [x for r in out.values() for x in [r] + [v for v in r.values() if isinstance(v, dict)]]
    assert all(x.get("parity_vs_replay", True) for x in flat), "NO_WAIT differs from the replay"


if __name__ == "__main__":
    main()
