"""Call sequences on the NO_WAIT lock table with their expected results from
locktab_ref.LockTable, shared by the CPU test of the reference
(test_locktab_ref.py) and the GPU parity test (test_gpu_locktab.py).

A sequence is a list of steps, each a dict:
  kind "epoch":    batch, rc, conflict (the reference's), state (export after)
  kind "release":  batch, sel (rc bytes to select with), want, n, nnz, state
The references are computed once per process and never changed."""
import functools

import numpy as np

from deneva_amd import ACCESS_NONE as N
from deneva_amd import RC_ABORT as AB
from deneva_amd import RC_RCOK as OK
from deneva_amd import RD, SCAN, WR, XP
from helpers import make_batch, random_batch
from locktab_ref import LockTable
from nowait_ref import LOCK_EX as EX
from nowait_ref import LOCK_SH as SH

# The hand-worked sequence: (kind, txns, ...) with
#   ("epoch", txns, rc, conflict, state after)
#   ("release", txns, selecting rc bytes, state after)     want = RC_RCOK
_E1 = [[(1, WR), (2, RD)], [(2, RD), (3, RD)], [(1, RD)]]
KAT = [
    # T0 takes 1 EX and 2 SH; T1 shares 2 and takes 3; T2's read of 1 meets T0's EX
    ("epoch", _E1, [OK, OK, AB], [N, N, 0], {1: (EX, 1), 2: (SH, 2), 3: (SH, 1)}),
    # 2 is SH-held by two owners of epoch 1: a writer aborts; a reader of 3 joins
    ("epoch", [[(2, WR)], [(3, RD)]], [AB, OK], [0, N], {1: (EX, 1), 2: (SH, 2), 3: (SH, 2)}),
    # T0 of epoch 1 finishes: 1 goes 1 -> 0 (LOCK_NONE), 2 goes 2 -> 1
    ("release", _E1, [OK, AB, AB], {2: (SH, 1), 3: (SH, 2)}),
    # 1 is free again: its writer commits; 2 still has T1's share: its writer aborts
    ("epoch", [[(1, WR)], [(2, WR)]], [OK, AB], [N, 0], {1: (EX, 1), 2: (SH, 1), 3: (SH, 2)}),
    # T1 of epoch 1 finishes: 2 goes 1 -> 0, 3 goes 2 -> 1
    ("release", _E1, [AB, OK, AB], {1: (EX, 1), 3: (SH, 1)}),
    ("epoch", [[(2, WR)]], [OK], [N], {1: (EX, 1), 2: (EX, 1), 3: (SH, 1)}),
]


def kat_steps():
    steps = []
    for c in KAT:
        if c[0] == "epoch":
            steps.append({"kind": "epoch", "batch": make_batch(c[1]), "rc": np.asarray(c[2], np.uint8),
                          "conflict": np.asarray(c[3], np.uint32), "state": c[4]})
        else:
            b = make_batch(c[1])
            sel = np.asarray(c[2], np.uint8)
            lens = np.diff(b.offsets.astype(np.int64))
            steps.append({"kind": "release", "batch": b, "sel": sel, "want": OK, "n": int((sel == OK).sum()),
                          "nnz": int(lens[sel == OK].sum()), "state": c[3]})
    return steps


N_SEQ, N_EPOCH, SEED = 8, 6, 21


@functools.lru_cache(maxsize=None)
def random_sequences():
    """N_SEQ sequences of N_EPOCH epochs; the commits of epoch e - D are
    released after epoch e, D = 1 + s % 3.  Returns a tuple of (steps, facts),
    facts = {"commits", "aborts", "changed", "regrants"}: decisions that differ
    from the same epoch on an empty table, and granted requests on rows that
    were held earlier and freed by a release."""
    rng = np.random.default_rng(SEED)
    out = []
    for s in range(N_SEQ):
        nk = int(rng.integers(50, 4000))
        D = 1 + s % 3
        types = (RD, WR, XP, SCAN) if s % 3 == 0 else (RD, WR)
        ref = LockTable()
        steps, done = [], []
        facts = {"commits": 0, "aborts": 0, "changed": 0, "regrants": 0}
        freed = set()  # rows a release took to LOCK_NONE
        for e in range(N_EPOCH):
            b = random_batch(rng, int(rng.integers(1, 3000)), int(rng.integers(1, 17)), nk,
                             p_write=0.5 * float(rng.random()), types=types, unique=bool(s % 2))
            rc, cf = ref.lock_epoch(b)
            erc, _ = LockTable().lock_epoch(b)
            facts["commits"] += int((rc == OK).sum())
            facts["aborts"] += int((rc == AB).sum())
            facts["changed"] += int((rc != erc).sum())
            granted = b.keys[np.repeat(rc == OK, np.diff(b.offsets.astype(np.int64)))]
            facts["regrants"] += sum(1 for k in granted.tolist() if k in freed)
            steps.append({"kind": "epoch", "batch": b, "rc": rc, "conflict": cf, "state": ref.export()})
            done.append((b, rc))
            if e - D >= 0:
                rb, rrc = done[e - D]
                before = ref.export()
                n, nnz = ref.release(rb, rrc, OK)
                after = ref.export()
                freed |= {k for k in before if k not in after}
                steps.append({"kind": "release", "batch": rb, "sel": rrc, "want": OK, "n": n, "nnz": nnz,
                              "state": after})
        out.append((steps, facts))
    return tuple(out)
