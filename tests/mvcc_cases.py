"""Known answers of the MVCC epoch (dcc_mvcc_validate_epoch), derived by hand
from concurrency_control/row_mvcc.cpp, storage/row.cpp:239-282 / 371-390 and
system/txn.cpp:700-761.  Txns run one at a time in index order.

  R_REQ (RD, SCAN, and the second request of a WR): never aborts; returns the
        newest-inserted version with wts <= ts, else the base row (:266-270),
        and enters ts into the read history
  P_REQ (the first request of a WR): Abort iff a read above ts exists with no
        write between (:218-239); every write ts is also a read ts, so: iff
        ts < the row's largest read ts
  W_REQ (a WR of a committed txn): installs the version ts
  XP_REQ (a WR of an aborted txn): drops the prewrite, nothing else

A case is (name, txns, ts, rc, conflict, vts, rows, versions) from empty
state: txns a list of lists of (key, access type), vts per access in batch
order (B: the base row, N: none), rows key -> (latest version, rts) after,
versions the sorted (key, ts) list after.
"""
import numpy as np

from deneva_amd import ACCESS_NONE as NONE
from deneva_amd import RC_ABORT as AB
from deneva_amd import RC_RCOK as OK
from deneva_amd import RD, SCAN, VTS_BASE as B, VTS_NONE as N, WR, XP

H = 1 << 63

TS_FAMILIES = ("index", "jitter", "permuted", "tied", "span63")


def make_ts(rng, n, family, base=1000):
    """u64[n] timestamps in [1, 2^64-2]: index order; index order with a jitter
    of up to 64; a random permutation of base .. base + n - 1; ties in 1..4;
    a permutation on both sides of 2^63 (an unsigned compare and a signed one
    disagree)."""
    idx = np.arange(n, dtype=np.uint64)
    if family == "index":
        return np.uint64(base) + idx
    if family == "jitter":
        return np.uint64(base) + idx + rng.integers(0, 65, size=n).astype(np.uint64)
    if family == "permuted":
        return np.uint64(base) + rng.permutation(n).astype(np.uint64)
    if family == "tied":
        return rng.integers(1, 5, size=n).astype(np.uint64)
    if family == "span63":
        return np.uint64(H - n // 2) + rng.permutation(n).astype(np.uint64)
    raise ValueError(family)


def epoch_base(family, e, n):
    """The base of epoch e of a chain: the epochs overlap by half, so that a
    later epoch has txns below the rts and the versions the earlier ones left
    (aborts and late reads in index order too)."""
    return 1000 + e * (n // 2)


KATS = [
    # T0 ts 10 and T1 ts 20 write row 5 (each reads what was there: base, 10).
    # T2 ts 15 RD: versions (10, 20), the newest with wts <= 15 is 10, not the
    # latest.  T3 ts 5 RD: none is <= 5: the base row.  rts = 20.
    ("late_read_sees_the_older_of_two",
     [[(5, WR)], [(5, WR)], [(5, RD)], [(5, RD)]], [10, 20, 15, 5],
     [OK, OK, OK, OK], [NONE] * 4, [B, 10, 10, B], {5: (20, 20)}, [(5, 10), (5, 20)]),
    # W_REQ runs at commit (row.cpp:385-390): T0's RD behind its own WR of row 7
    # sees the base row.  T1 at the same ts sees T0's version (wts <= ts).
    ("own_write_is_not_visible",
     [[(7, WR), (7, RD)], [(7, SCAN)]], [9, 9],
     [OK, OK], [NONE] * 2, [B, B, 9], {7: (9, 9)}, [(7, 9)]),
    # T0 and T1 both write row 3 at ts 8 (8 < rts 8 is false); T1's read copies
    # T0's version.  T2 ts 8 sees a version 8, T3 ts 7 the base row.
    ("two_writers_with_an_equal_ts",
     [[(3, WR)], [(3, WR)], [(3, RD)], [(3, RD)]], [8, 8, 8, 7],
     [OK, OK, OK, OK], [NONE] * 4, [B, 8, 8, B], {3: (8, 8)}, [(3, 8), (3, 8)]),
    # T0 ts 20 reads row 1.  T1 ts 15 WR row 1: the read 20 lies above 15 with
    # no write between (:218-239): Abort at 0.
    ("write_below_an_earlier_reader",
     [[(1, RD)], [(1, WR)]], [20, 15],
     [OK, AB], [NONE, 0], [B, N], {1: (0, 20)}, []),
    # The same with the reader inside a txn that aborts later: T1 ts 20 reads
    # row 1 (ordinal 0), then its WR of row 2 meets T0's read at 30: Abort at 1.
    # Nothing undoes the read (cleanup sends nothing for a RD): T2 ts 15 WR row
    # 1 aborts at 0.
    ("reader_before_its_txns_abort_ordinal_counts",
     [[(2, WR)], [(1, RD), (2, WR)], [(1, WR)]], [30, 20, 15],
     [OK, AB, AB], [NONE, 1, 0], [B, B, N, N], {1: (0, 20), 2: (30, 30)}, [(2, 30)]),
    # T1 aborts at ordinal 0: its RD of row 1 at ordinal 1 is never made, so T2
    # ts 15 may write row 1.
    ("reader_after_the_abort_ordinal_does_not_count",
     [[(2, WR)], [(2, WR), (1, RD)], [(1, WR)]], [30, 20, 15],
     [OK, AB, OK], [NONE, 0, NONE], [B, N, N, B], {1: (15, 15), 2: (30, 30)}, [(1, 15), (2, 30)]),
    # T1 ts 40 writes row 5 (P_REQ and R_REQ pass, rts 5 = 40) and aborts at its
    # WR of row 4 (read at 50): XP_REQ drops the prewrite of row 5, no version.
    # T2 ts 45 RD row 5: the base row; rts 5 = 45.
    ("aborted_writer_installs_no_version",
     [[(4, RD)], [(5, WR), (4, WR)], [(5, RD)]], [50, 40, 45],
     [OK, AB, OK], [NONE, 1, NONE], [B, B, N, B], {4: (0, 50), 5: (0, 45)}, []),
    # XP makes no request; an empty txn makes none either: all commit, nothing changes.
    ("xp_only_and_empty_txns",
     [[], [(1, XP)], [(1, XP), (2, XP)], []], [4, 3, 2, 1],
     [OK, OK, OK, OK], [NONE] * 4, [N, N, N], {}, []),
    # ts == rts passes (the conflict needs a read strictly above ts); one below aborts.
    ("a_tie_with_rts_passes",
     [[(6, RD)], [(6, WR)], [(6, WR)]], [12, 12, 11],
     [OK, OK, AB], [NONE, NONE, 0], [B, B, N], {6: (12, 12)}, [(6, 12)]),
    # Unsigned compares across 2^63: T0 ts 2^63 writes row 1; T1 ts 2^63 - 1 RD
    # sees the base row (a signed compare would show it T0's version); T2 ts
    # 2^63 - 1 WR aborts (rts 2^63); T3 ts 2^64 - 2 RD sees 2^63.
    ("across_2_63",
     [[(1, WR)], [(1, RD)], [(1, WR)], [(1, RD)]], [H, H - 1, H - 1, (1 << 64) - 2],
     [OK, OK, AB, OK], [NONE, NONE, 0, NONE], [B, B, N, H], {1: (H, (1 << 64) - 2)}, [(1, H)]),
]
