"""Known answers of the TIMESTAMP epoch (dcc_tso_validate_epoch), derived by
hand from concurrency_control/row_ts.cpp, storage/row.cpp:239-282 / 371-390
and system/txn.cpp:700-761.  Txns run one at a time in index order.

  R_REQ (RD, SCAN, and the second request of a WR): Abort if ts < wts
        (row_ts.cpp:176), else rts = max(rts, ts) (:188-189)
  P_REQ (the first request of a WR): Abort if ts < rts (:193) or ts < wts (:200)
  W_REQ (a WR of a committed txn): wts = max(wts, ts) (:237-239)
  XP_REQ (a WR of an aborted txn): drops the prewrite, nothing else (:249-253)

A case is (name, txns, ts, seed, rc, conflict, rows): txns a list of lists of
(key, access type), seed and rows dicts key -> (wts, rts) before and after.
"""
from deneva_amd import ACCESS_NONE as NONE
from deneva_amd import RC_ABORT as AB
from deneva_amd import RC_RCOK as OK
from deneva_amd import RD, SCAN, WR, XP

import numpy as np

M = (1 << 64) - 1
H = 1 << 63

TS_FAMILIES = ("permuted", "jitter", "tied", "span63")


def make_ts(rng, n, family, base=1000):
    """u64[n] timestamps: a random permutation of base .. base + n - 1; index
    order with a jitter of up to 64; a few values many txns share; values on
    both sides of 2^63 (an unsigned compare and a signed one disagree)."""
    idx = np.arange(n, dtype=np.uint64)
    if family == "permuted":
        return np.uint64(base) + rng.permutation(n).astype(np.uint64)
    if family == "jitter":
        return np.uint64(base) + idx + rng.integers(0, 65, size=n).astype(np.uint64)
    if family == "tied":
        return np.uint64(base) + rng.integers(0, max(2, n // 8), size=n).astype(np.uint64)
    if family == "span63":
        return np.uint64(H - n // 2) + rng.permutation(n).astype(np.uint64)
    if family == "index":
        return np.uint64(base) + idx
    raise ValueError(family)


def seed_rows(rng, n_keys, ts, frac=0.2):
    """A random seed: some of the keys with wts / rts drawn from the range of ts."""
    k = rng.choice(n_keys, size=max(1, int(n_keys * frac)), replace=False).astype(np.uint64)
    lo, hi = int(ts.min()), int(ts.max())
    pick = lambda: np.asarray([lo + int(v) for v in rng.integers(0, hi - lo + 1, size=k.size)], np.uint64)
    return {int(a): (int(w), int(r)) for a, w, r in zip(k, pick(), pick())}

KATS = [
    # T0 ts 10 WR: 10 < rts 0, 10 < wts 0 both false: rts = 10, commit, wts = 10.
    # T1 ts 7 RD: 7 < wts 10 (:176): Abort at 0.
    # T2 ts 12 RD: passes, rts = 12.
    # T3 ts 11 WR: 11 < rts 12 (:193): Abort at 0.
    # T4 ts 12 WR: 12 < 12 is false for rts and wts: commit, wts = 12.
    ("one_row_ties",
     [[(5, WR)], [(5, RD)], [(5, RD)], [(5, WR)], [(5, WR)]], [10, 7, 12, 11, 12], {},
     [OK, AB, OK, AB, OK], [NONE, 0, NONE, 0, NONE], {5: (12, 12)}),
    # T0 ts 20 reads row 1 (rts = 20), then its WR of row 2 meets rts 30 (:193):
    # Abort at 1.  Nothing undoes the read's bump (cleanup sends nothing for a
    # RD, row.cpp:375-379), so T1 ts 15 WR row 1: 15 < rts 20: Abort at 0.
    ("aborted_read_bump_stays",
     [[(1, RD), (2, WR)], [(1, WR)]], [20, 15], {2: (0, 30)},
     [AB, AB], [1, 0], {1: (0, 20), 2: (0, 30)}),
    # T0 ts 20 WR row 1: P_REQ passes, R_REQ sets rts = 20; WR row 2 aborts at
    # 1; XP_REQ on row 1 drops the prewrite, wts stays 0 (txn.cpp:700-704,
    # row.cpp:380-384).  T1 ts 15 RD row 1: 15 < wts 0 false: commit (rts stays
    # 20).  T2 ts 15 WR row 1: 15 < rts 20: Abort at 0.
    ("aborted_write_leaves_wts",
     [[(1, WR), (2, WR)], [(1, RD)], [(1, WR)]], [20, 15, 15], {2: (0, 30)},
     [AB, OK, AB], [1, NONE, 0], {1: (0, 20), 2: (0, 30)}),
    # XP makes no request: T0 ts 5 leaves row 3 at (0, 0) and writes row 4
    # (5, 5).  T1 ts 3 WR row 3 passes (3, 3); its XP of row 4 does not meet
    # wts 5.  T2 ts 1 XP row 4 commits.  T3 ts 4 RD row 4: 4 < wts 5: Abort at 0.
    ("xp_makes_no_request",
     [[(3, XP), (4, WR)], [(3, WR), (4, XP)], [(4, XP)], [(4, RD)]], [5, 3, 1, 4], {},
     [OK, OK, OK, AB], [NONE, NONE, NONE, 0], {3: (3, 3), 4: (5, 5)}),
    # A txn meets its own bumps with ts < ts, which is false.  T0 ts 9 RD then
    # WR of row 7: rts = 9, P_REQ 9 < 9 false: commit (9, 9).  T1 ts 9 WR twice:
    # ties pass.  T2 ts 8 WR: 8 < rts 9: Abort at 0.  T3 ts 10 WR row 8 twice
    # (10, 10) and SCAN row 7: 10 < wts 9 false, rts 7 = 10.
    ("same_row_twice_in_a_txn",
     [[(7, RD), (7, WR)], [(7, WR), (7, WR)], [(7, WR), (7, WR)], [(8, WR), (8, WR), (7, SCAN)]],
     [9, 9, 8, 10], {},
     [OK, OK, AB, OK], [NONE, NONE, 0, NONE], {7: (9, 10), 8: (10, 10)}),
    # ts 0 never fails against a fresh row (0 < 0 false) and fails against any
    # positive wts / rts.  T3: RD row 3 passes (0 < wts 0 false), its WR meets
    # rts 1: Abort at 1.
    ("ts_zero",
     [[(1, WR)], [(1, RD)], [(2, RD)], [(3, RD), (3, WR)]], [0, 0, 0, 0], {2: (1, 0), 3: (0, 1)},
     [OK, OK, AB, AB], [NONE, NONE, 0, 1], {1: (0, 0), 2: (1, 0), 3: (0, 1)}),
    # Unsigned comparisons at the top of the range.  T0 ts 2^64-1 WR row 1:
    # (M, M).  T1 ts M-1 RD: M-1 < wts M: Abort at 0.  T2 ts M WR row 1 (tie)
    # and RD row 2: commit, row 2 rts = M.  T3 ts 2^63 WR row 2: 2^63 < rts M:
    # Abort at 0.  T4 ts 2^63 WR row 4 against rts 2^63-1: passes as unsigned
    # (a signed compare would abort it): (2^63, 2^63).
    ("ts_top_of_range",
     [[(1, WR)], [(1, RD)], [(1, WR), (2, RD)], [(2, WR)], [(4, WR)]], [M, M - 1, M, H, H],
     {4: (0, H - 1)},
     [OK, AB, OK, AB, OK], [NONE, 0, NONE, 0, NONE], {1: (M, M), 2: (0, M), 4: (H, H)}),
]
