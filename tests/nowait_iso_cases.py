"""Known answers of the NO_WAIT lock epoch at the three isolation levels:
(name, txns, held, {level: (rc, conflict)}).  None as a level's entry: every
txn commits."""
from deneva_amd import (ACCESS_NONE, ISO_READ_COMMITTED, ISO_READ_UNCOMMITTED, ISO_SERIALIZABLE, RC_ABORT,
                        RC_RCOK, RD, SCAN, WR)

OK, AB, N = RC_RCOK, RC_ABORT, ACCESS_NONE
SER, RCL, RUL = ISO_SERIALIZABLE, ISO_READ_COMMITTED, ISO_READ_UNCOMMITTED


def _same(rc, cf):
    return {SER: (rc, cf), RCL: (rc, cf), RUL: (rc, cf)}


KATS = [
    # a reader never blocks a later writer; the writer then kills the next reader
    ("read_write_read", [[(7, RD)], [(7, WR)], [(7, RD)]], None,
     {SER: ([OK, AB, OK], [N, 0, N]), RCL: ([OK, OK, AB], [N, N, 0]), RUL: None}),
    ("write_read", [[(7, WR)], [(7, RD)]], None,
     {SER: ([OK, AB], [N, 0]), RCL: ([OK, AB], [N, 0]), RUL: None}),
    # the txn's own read is released before its write
    ("self_rd_wr", [[(5, RD), (5, WR)]], None, {SER: ([AB], [1]), RCL: None, RUL: None}),
    ("self_wr_rd", [[(5, WR), (9, RD), (5, RD)]], None, {SER: ([AB], [2]), RCL: ([AB], [2]), RUL: None}),
    ("self_wr_wr", [[(5, WR), (5, WR)], [(5, WR)]], None,
     {SER: ([AB, OK], [1, N]), RCL: ([AB, OK], [1, N]), RUL: None}),
    # an abort releases its EX rows
    ("abort_releases", [[(1, WR)], [(2, WR), (1, WR)], [(2, RD)]], None,
     {SER: ([OK, AB, OK], [N, 1, N]), RCL: ([OK, AB, OK], [N, 1, N]), RUL: None}),
    ("first_of_two", [[(1, WR), (2, WR)], [(1, RD), (3, WR)], [(3, RD), (2, RD)]], None,
     {SER: ([OK, AB, AB], [N, 0, 1]), RCL: ([OK, AB, AB], [N, 0, 1]), RUL: None}),
    ("held_sh", [[(8, RD)], [(1, RD), (8, WR)], [(8, SCAN)]], [(8, RD)], _same([OK, AB, OK], [N, 1, N])),
    ("held_ex", [[(8, RD)], [(8, WR)], [(9, WR)]], [(8, WR)], _same([AB, AB, OK], [0, 0, N])),
    # reads of rows nobody writes or holds
    ("absent_rows", [[(3, RD), (4, RD)], [(5, WR)]], None, {SER: None, RCL: None, RUL: None}),
]


def answer(case, level):
    _, txns, _, ans = case
    if ans[level] is None:
        return [OK] * len(txns), [N] * len(txns)
    return ans[level]


# ---- the inputs of the GPU tests, built here so that the CPU tests can check
# the conditions on them (test_nowait_iso_ref.py)
def length_batch(L, n=200, seed=0):
    """n txns of L accesses over few rows; txn t reads a row nobody writes or
    holds in its first (t % 3 == 0), a middle (1) or its last (2) lane; every
    fourth txn has none (at L = 1 those are the ones that can conflict)."""
    import numpy as np
    from helpers import make_batch
    rng = np.random.default_rng(100 + L + seed)
    txns = []
    for t in range(n):
        ks = rng.integers(0, 40 * L, size=L).tolist()
        ts = np.where(rng.random(L) < 0.15, WR, RD).tolist()
        q = (0, L // 2, L - 1)[t % 3]
        if t % 4 != 3:
            ks[q], ts[q] = (1 << 40) + t, RD
        txns.append(list(zip(ks, ts)))
    return make_batch(txns)


N_TXN_EDGES = (1, 63, 64, 65, 15, 16, 17)  # and NW_T / P - 1, NW_T / P, NW_T / P + 1 at P = 16


def ntxn_batch(n):
    """n txns of 16 accesses (P = 16) on a few rows: txn t reads rows and
    writes one; txn 0 reads then writes one row, which SERIALIZABLE alone
    aborts, so the levels differ from n = 1 on."""
    import numpy as np
    from helpers import make_batch
    rng = np.random.default_rng(300 + n)
    txns = []
    for t in range(n):
        ks = rng.integers(0, 24, size=16).tolist()
        ts = [RD] * 16
        ts[int(rng.integers(0, 16))] = WR
        if t == 0:
            ks[:2], ts[:2] = [1000, 1000], [RD, WR]
        txns.append(list(zip(ks, ts)))
    return make_batch(txns)


def hot_row(n, readers):
    """n one-access txns on one row: all write it, or every third (txn 0
    first) only reads it."""
    import numpy as np
    import deneva_amd as d
    at = np.full(n, WR, np.uint8)
    if readers:
        at[0::3] = RD
    return d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, 77, np.uint64), at)


def random_draws():
    """12 draws as test_gpu_nowait.py::test_random's: (draw, batch, held).  The
    held prefixes cover at most an eighth of the rows, so that the epoch's own
    requests still decide (a larger one leaves the levels nothing to differ in)."""
    import numpy as np
    from deneva_amd import XP
    from helpers import random_batch
    rng = np.random.default_rng(RANDOM_SEED)
    for it in range(12):
        nk = int(rng.integers(1, 2000))
        types = (RD, WR) if it % 3 else (RD, WR, XP, SCAN)
        b = random_batch(rng, int(rng.integers(1, 5000)), int(rng.integers(1, 64)), nk,
                         p_write=float(rng.random()), types=types, unique=bool(it % 2))
        held = None
        if it >= 6:  # a random held prefix over distinct keys
            hk = rng.choice(nk, size=int(rng.integers(0, nk // 8 + 1)), replace=False).astype(np.uint64)
            held = (hk, rng.integers(0, 4, size=hk.size).astype(np.uint8))
        yield it, b, held


RANDOM_SEED = 11
YCSB_THETAS = (0.6, 0.9)
CARRY_SEEDS = (70, 71, 72, 73)


def chain_variant(n):
    """chain_batch with txn 0 reading its row before writing it: SERIALIZABLE
    aborts txn 0 and every decision of the chain flips."""
    import numpy as np
    import deneva_amd as d
    from helpers import chain_batch
    b = chain_batch(n)
    off = np.concatenate([[0], b.offsets[1:].astype(np.int64) + 1]).astype(np.uint32)
    return d.EpochBatch(off, np.concatenate([[0], b.keys]).astype(np.uint64),
                        np.concatenate([[RD], b.acctype]).astype(np.uint8))


def carry(b, rc):
    """The next READ_COMMITTED epoch's held list: the EX rows of the committed txns."""
    import numpy as np
    per_req = np.repeat(rc == RC_RCOK, np.diff(b.offsets.astype(np.int64)))
    per_req &= (b.acctype != RD) & (b.acctype != SCAN)
    return b.keys[per_req].copy(), b.acctype[per_req].copy()
