"""Times TIMESTAMP with txns in flight (dcc_tso_access_epoch, dcc_tso_finish) on
resident device batches next to its two neighbours, the one-txn-in-flight
TIMESTAMP epoch (dcc_tso_validate_epoch) and the in-flight MVCC access epoch
(dcc_mvcc_access_epoch), in one process on the same batches: the C2 shape
(65,536 x 16, theta 0.9) and the headline shape (1,048,576 x 16, theta 0.9),
ts = index with a jitter of up to 256.

    python tools/tso_live_bench.py [--warmup 5] [--steps 20] [--shape both|c2|headline]
                                   [--json PATH]

A step clears the context's TIMESTAMP rows and then makes, in this order,
  epoch     every txn (RUN, 0): a first access epoch on empty rows
  finish    all RCOK + ABORT txns of that epoch leave
  epoch2    the epoch after that finish: promoted txns resume against the
            prewrites the others kept and the wts the leavers left
  validate  dcc_tso_validate_epoch on cleared rows
  mvcc      dcc_mvcc_access_epoch on cleared MVCC rows, every txn (RUN, 0)
so every call starts from the same state in every step and all see the same
machine state.  device_ms is the engine's own device time of the call (HIP
events on its stream around the kernels, batch resident); the table reports
the median of the timed calls with the minimum and maximum, the rounds,
device_ms per round and alg_bytes / device_ms.  Phase times come from separate
profiled steps.  Parity with the replay (tests/tso_live_ref.py) is checked on
the C2 shape after timing."""
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
import tso_live_ref as ref  # noqa: E402  (checker only)


def summary(stats):
    ms = [s["device_ms"] for s in stats]
    med = statistics.median(ms)
    out = {"device_ms": med, "device_ms_min": min(ms), "device_ms_max": max(ms), "device_ms_all": ms}
    last = stats[-1]
    if last["alg_bytes"]:
        rounds = [s["rounds"] for s in stats]
        per = [s["device_ms"] / max(s["rounds"], 1) for s in stats]
        out.update(rounds=int(statistics.median(rounds)), rounds_max=max(rounds), alg_bytes=last["alg_bytes"],
                   alg_GBps=last["alg_bytes"] / (med * 1e-3) / 1e9, ms_per_round=statistics.median(per),
                   ms_per_round_min=min(per), ms_per_round_max=max(per))
    out.update(n_commit=last["n_commit"], n_abort=last["n_abort"], n_survivors=last["n_survivors"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=("both", "c2", "headline"), default="both")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tso_live_bench needs cuda:0"
    out = {}
    dev = "cuda:0"
    with d.Engine(0) as eng:
        for name, n in (("C2 65,536 x 16", 65536), ("headline 1,048,576 x 16", 1 << 20)):
            if a.shape != "both" and (a.shape == "c2") != (n == 65536):
                continue
            b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
            db = b.to_torch(dev)
            ts = np.arange(1, n + 1, dtype=np.uint64) + np.random.default_rng(7).integers(0, 257, size=n).astype(np.uint64)
            dts = torch.from_numpy(ts.view(np.int64)).to(dev)
            eng.reserve(b.n_txn, b.nnz)
            rc = torch.empty(n, dtype=torch.uint8, device=dev)
            pos = torch.empty(n, dtype=torch.int32, device=dev)
            mrc, mpos = torch.empty_like(rc), torch.empty_like(pos)
            vrc = torch.empty(n, dtype=torch.uint8, device=dev)
            vcf = torch.empty(n, dtype=torch.int32, device=dev)
            seen = {}

            def step():
                """One step; returns the stats of its three calls."""
                st = {}
                eng.tso_rows_clear()
                rc.fill_(d.WD_RUN)
                pos.zero_()
                st["epoch"] = eng.tso_access_epoch(db, dts, rc, pos)[3]
                seen["s1"] = (rc.clone(), pos.clone())
                leave = ((rc == d.RC_RCOK) | (rc == d.RC_ABORT)).to(torch.uint8)
                seen["leave"] = leave
                left, prom, st["finish"] = eng.tso_finish(db, dts, rc, pos, leave)
                st["finish"]["n_commit"], st["finish"]["n_survivors"] = left, prom
                seen["s2"] = (rc.clone(), pos.clone())
                st["epoch2"] = eng.tso_access_epoch(db, dts, rc, pos)[3]
                return st

            def neighbours(st):
                eng.tso_rows_clear()
                st["validate"] = eng.tso_validate_epoch(db, dts, out_rc=vrc, out_conflict=vcf)[2]
                eng.mvcc_clear()
                mrc.fill_(d.WD_RUN)
                mpos.zero_()
                st["mvcc"] = eng.mvcc_access_epoch(db, dts, mrc, mpos)[3]
                return st

            for _ in range(a.warmup):
                neighbours(step())
            names = ("epoch", "finish", "epoch2", "validate", "mvcc")
            runs = {k: [] for k in names}
            for _ in range(a.steps):
                st = neighbours(step())
                for k in names:
                    runs[k].append(st[k])
            torch.cuda.synchronize()
            res = {k: summary(v) for k, v in runs.items()}
            res["epoch_over_validate"] = res["epoch"]["device_ms"] / res["validate"]["device_ms"]
            res["epoch_over_mvcc"] = res["epoch"]["device_ms"] / res["mvcc"]["device_ms"]
            res["leavers"] = int(seen["leave"].sum().item())
            eng.set_profiling(True)
            ph = [neighbours(step()) for _ in range(5)]
            for key in ("epoch", "epoch2", "validate", "mvcc"):
                res[key]["phase_ms"] = [statistics.median(p[key]["phase_ms"][q] for p in ph) for q in range(4)]
            eng.set_profiling(False)
            if n == 65536:
                step()  # the context and the arrays as the three calls leave them
                state = {}
                h0 = (np.full(n, d.WD_RUN, np.uint8), np.zeros(n, np.uint32))
                e1 = ref.epoch(b, ts, *h0, state)
                lv = np.isin(e1[0], [d.RC_RCOK, d.RC_ABORT]).astype(np.uint8)
                f1 = ref.finish(b, ts, e1[0], e1[1], lv, state)
                e2 = ref.epoch(b, ts, f1[0], f1[1], state)
                same = lambda s, e: (np.array_equal(s[0].cpu().numpy(), e[0]) and
                                     np.array_equal(s[1].cpu().numpy().view(np.uint32), e[1]))
                uk = np.unique(b.keys)
                w, r = eng.tso_rows_get(uk)
                rows = {int(k): (int(x), int(y)) for k, x, y in zip(uk, w, r) if (x, y) != (0, 0)}
                res["parity_vs_replay"] = bool(
                    same(seen["s1"], e1) and same(seen["s2"], f1) and same((rc, pos), e2) and
                    np.array_equal(seen["leave"].cpu().numpy(), lv) and rows == ref.rows_of(state))
            out[name] = res
            print(f"{name}:")
            for key in names:
                r = res[key]
                extra = (f"  rounds {r['rounds']}  ms/round {r['ms_per_round']:.4f} [{r['ms_per_round_min']:.4f}, "
                         f"{r['ms_per_round_max']:.4f}]  alg {r['alg_GBps']:.1f} GB/s" if "rounds" in r else "")
                phase = f"  phase_ms {[round(x, 3) for x in r['phase_ms']]}" if "phase_ms" in r else ""
                print(f"  {key:8s} device_ms {r['device_ms']:.3f} [{r['device_ms_min']:.3f}, "
                      f"{r['device_ms_max']:.3f}]{extra}  RCOK / leavers {r['n_commit']} ABORT {r['n_abort']} "
                      f"WAIT / promoted {r['n_survivors']}{phase}")
            print(f"  access epoch / validate epoch = {res['epoch_over_validate']:.2f}, / MVCC access epoch = "
                  f"{res['epoch_over_mvcc']:.2f}"
                  + (f"  parity_vs_replay {res['parity_vs_replay']}" if "parity_vs_replay" in res else ""),
                  flush=True)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    assert all(r.get("parity_vs_replay", True) for r in out.values()), "TIMESTAMP with txns in flight differs from the replay"


if __name__ == "__main__":
    main()
