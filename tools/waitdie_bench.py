"""Times the WAIT_DIE calls (dcc_waitdie_lock_epoch, dcc_waitdie_release) on
resident device batches next to the NO_WAIT lock epoch (dcc_nowait_lock_epoch),
in one process on the same batches: the C2 shape (65,536 x 16, theta 0.9) and
the headline shape (1,048,576 x 16, theta 0.9), ts = index with a jitter of up
to 256.

    python tools/waitdie_bench.py [--warmup 5] [--steps 20] [--shape both|c2|headline]
                                  [--json PATH]

Three WAIT_DIE calls are timed, each from the same state every time (the state
arrays are restored on the device outside the timed region):
  epoch    every txn (RUN, 0): a first acquisition epoch
  release  all RCOK + ABORT txns of that epoch leave
  epoch2   the epoch after that release: promoted waiters resume against the
           entries the waiters kept
device_ms is the engine's own device time of the call (HIP events on its stream
around the kernels, batch resident); the table reports the median of the timed
calls with the minimum and maximum, the rounds, and alg_bytes / device_ms.  The
epoch and the NO_WAIT epoch alternate, so both see the same machine state.
Phase times come from separate profiled calls.  Parity with the replay
(tests/waitdie_ref.py) is checked on the C2 shape after timing."""
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
from waitdie_ref import replay_epoch, replay_release  # noqa: E402  (checker only)


def summary(stats):
    ms = [s["device_ms"] for s in stats]
    med = statistics.median(ms)
    out = {"device_ms": med, "device_ms_min": min(ms), "device_ms_max": max(ms)}
    last = stats[-1]
    if last["alg_bytes"]:
        rounds = [s["rounds"] for s in stats]
        out.update(rounds=int(statistics.median(rounds)), rounds_max=max(rounds), alg_bytes=last["alg_bytes"],
                   alg_GBps=last["alg_bytes"] / (med * 1e-3) / 1e9)
    out.update(n_commit=last["n_commit"], n_abort=last["n_abort"], n_survivors=last["n_survivors"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=("both", "c2", "headline"), default="both")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "waitdie_bench needs cuda:0"
    out = {}
    with d.Engine(0) as eng:
        for name, n in (("C2 65,536 x 16", 65536), ("headline 1,048,576 x 16", 1 << 20)):
            if a.shape != "both" and (a.shape == "c2") != (n == 65536):
                continue
            b = d.gen_ycsb(n_txn=n, zipf_theta=0.9)
            db = b.to_torch("cuda:0")
            ts = np.arange(n, dtype=np.uint64) + np.random.default_rng(7).integers(0, 257, size=n).astype(np.uint64)
            dts = torch.from_numpy(ts.view(np.int64)).to("cuda:0")
            eng.reserve(b.n_txn, b.nnz)
            rc = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            pos = torch.empty(n, dtype=torch.int32, device="cuda:0")
            nrc = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            ncf = torch.empty(n, dtype=torch.int32, device="cuda:0")

            def epoch(state):
                rc.copy_(state[0])
                pos.copy_(state[1])
                return eng.waitdie_lock_epoch(db, dts, rc, pos)[3]

            def release(state, leave):
                rc.copy_(state[0])
                pos.copy_(state[1])
                return eng.waitdie_release(db, dts, rc, pos, leave)[2]

            def nowait():
                return eng.nowait_lock_epoch(db, out_rc=nrc, out_conflict=ncf)[2]

            s0 = (torch.full((n,), d.WD_RUN, dtype=torch.uint8, device="cuda:0"),
                  torch.zeros(n, dtype=torch.int32, device="cuda:0"))
            epoch(s0)
            s1 = (rc.clone(), pos.clone())
            leave = ((s1[0] == d.RC_RCOK) | (s1[0] == d.RC_ABORT)).to(torch.uint8)
            release(s1, leave)
            s2 = (rc.clone(), pos.clone())
            calls = {"epoch": lambda: epoch(s0), "release": lambda: release(s1, leave), "epoch2": lambda: epoch(s2)}
            for _ in range(a.warmup):
                for fn in calls.values():
                    fn()
                nowait()
            st = {k: [] for k in list(calls) + ["nowait"]}
            for _ in range(a.steps):  # alternate, so that all see the same machine state
                for k, fn in calls.items():
                    st[k].append(fn())
                st["nowait"].append(nowait())
            torch.cuda.synchronize()
            res = {k: summary(v) for k, v in st.items()}
            res["ratio"] = res["epoch"]["device_ms"] / res["nowait"]["device_ms"]
            res["leavers"] = int(leave.sum().item())
            eng.set_profiling(True)
            for key, fn in (("epoch", calls["epoch"]), ("epoch2", calls["epoch2"]), ("nowait", nowait)):
                ph = [fn()["phase_ms"] for _ in range(5)]
                res[key]["phase_ms"] = [statistics.median(p[q] for p in ph) for q in range(4)]
            eng.set_profiling(False)
            if n == 65536:
                h0 = (np.full(n, d.WD_RUN, np.uint8), np.zeros(n, np.uint32))
                e1 = replay_epoch(b, ts, *h0)
                lv = np.isin(e1[0], [d.RC_RCOK, d.RC_ABORT]).astype(np.uint8)
                r1 = replay_release(b, ts, e1[0], e1[1], lv)
                e2 = replay_epoch(b, ts, r1[0], r1[1])
                same = lambda s, e: (np.array_equal(s[0].cpu().numpy(), e[0]) and
                                     np.array_equal(s[1].cpu().numpy().view(np.uint32), e[1]))
                epoch(s2)
                res["parity_vs_replay"] = bool(same(s1, e1) and same(s2, r1) and same((rc, pos), e2) and
                                               np.array_equal(leave.cpu().numpy(), lv))
            out[name] = res
            print(f"{name}:")
            for key in ("epoch", "epoch2", "release", "nowait"):
                r = res[key]
                extra = (f"  rounds {r['rounds']}  alg {r['alg_GBps']:.1f} GB/s" if "rounds" in r else "")
                phase = f"  phase_ms {[round(x, 3) for x in r['phase_ms']]}" if "phase_ms" in r else ""
                print(f"  {key:8s} device_ms {r['device_ms']:.3f} (min {r['device_ms_min']:.3f}, "
                      f"max {r['device_ms_max']:.3f}){extra}  RCOK {r['n_commit']} ABORT {r['n_abort']} "
                      f"WAIT / promoted {r['n_survivors']}{phase}")
            print(f"  WAIT_DIE epoch / NO_WAIT epoch = {res['ratio']:.2f}"
                  + (f"  parity_vs_replay {res['parity_vs_replay']}" if "parity_vs_replay" in res else ""),
                  flush=True)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    assert all(r.get("parity_vs_replay", True) for r in out.values()), "WAIT_DIE differs from the replay"


if __name__ == "__main__":
    main()
