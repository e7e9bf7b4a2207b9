"""CPU: the numpy reference of dcc_batch_select (select_ref.py) on cases worked
by hand, and the alg-bytes formula of the library."""
import numpy as np

import deneva_amd as d
from deneva_amd import RD, WR
from helpers import make_batch
from select_ref import ERANGE, OK, alg_bytes, select

# five txns of lengths 2, 0, 3, 1, 0; keys 10.., types alternate
TXNS = [[(10, RD), (11, WR)], [], [(12, RD), (13, WR), (14, RD)], [(15, WR)], []]
RC = [2, 0, 2, 2, 0]


def test_hand_worked():
    b = make_batch(TXNS)
    assert b.offsets.tolist() == [0, 2, 2, 5, 6, 6]
    code, n, m, r = select(b, RC, 2)
    assert (code, n, m) == (OK, 3, 6)
    assert r["offsets"].tolist() == [0, 2, 5, 6]
    assert r["keys"].tolist() == [10, 11, 12, 13, 14, 15]
    assert r["acctype"].tolist() == [RD, WR, RD, WR, RD, WR]
    assert r["src"].tolist() == [0, 2, 3]
    # the others: two empty txns, kept
    code, n, m, r = select(b, RC, 0)
    assert (code, n, m) == (OK, 2, 0)
    assert r["offsets"].tolist() == [0, 0, 0] and r["keys"].size == 0 and r["src"].tolist() == [1, 4]
    # a value no txn has
    code, n, m, r = select(b, RC, 3)
    assert (code, n, m) == (OK, 0, 0) and r["offsets"].tolist() == [0]


def test_bases():
    b = make_batch(TXNS)
    code, n, m, r = select(b, RC, 2, txn_base=2, nnz_base=7)
    assert (code, n, m) == (OK, 3, 6)
    assert r["offsets"].tolist() == [7, 9, 12, 13]  # offsets[txn_base] = nnz_base
    assert r["keys"].tolist() == [10, 11, 12, 13, 14, 15] and r["src"].tolist() == [0, 2, 3]


def test_src_composes():
    b = make_batch(TXNS)
    code, n, m, r = select(b, RC, 2, src_in=[100, 101, 102, 103, 104])
    assert r["src"].tolist() == [100, 102, 103]
    # a second select over the first's output, carrying the first's src
    b2 = d.EpochBatch(r["offsets"], r["keys"], r["acctype"])
    code, n, m, r2 = select(b2, [0, 2, 2], 2, src_in=r["src"])
    assert (n, m) == (2, 4) and r2["src"].tolist() == [102, 103]
    assert r2["keys"].tolist() == [12, 13, 14, 15] and r2["offsets"].tolist() == [0, 3, 4]


def test_per_txn_arrays():
    b = make_batch(TXNS, start_tn=[1, 2, 3, 4, 5], finish_tn=[6, 7, 8, 9, 10], order=[50, 40, 30, 20, 10])
    _, _, _, r = select(b, RC, 2)
    assert r["start_tn"].tolist() == [1, 3, 4] and r["finish_tn"].tolist() == [6, 8, 9]
    assert r["order"].tolist() == [50, 30, 20]


def test_capacity_conditions():
    b = make_batch(TXNS)
    assert select(b, RC, 2, cap_txn=3, cap_nnz=6)[0] == OK
    assert select(b, RC, 2, cap_txn=2, cap_nnz=6) == (ERANGE, 3, 6, None)
    assert select(b, RC, 2, cap_txn=3, cap_nnz=5) == (ERANGE, 3, 6, None)
    assert select(b, RC, 2, nnz_base=0xFFFFFFFF - 6)[0] == OK
    assert select(b, RC, 2, nnz_base=0xFFFFFFFF - 5) == (ERANGE, 3, 6, None)


def test_alg_bytes_formula():
    for args in ((0, 0, 0, 0), (5, 3, 6, 0), (65536, 53106, 53106 * 16, 1), (1 << 20, 1 << 19, 9 << 20, 4)):
        assert d.select_alg_bytes(*args) == alg_bytes(*args)
    assert d.select_alg_bytes(5, 3, 6, 2) == 24 + 5 + 108 + 16 + 96
