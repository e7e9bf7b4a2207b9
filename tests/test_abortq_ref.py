"""CPU: the abort queue's reference restatement (abortq_ref.py) against values
worked by hand from system/abort_queue.cpp:26-82, and the alg_bytes formulas
of dcc.h against the library's."""
import numpy as np

import deneva_amd as d
from abortq_ref import (BACKOFF_EXP, BACKOFF_NONE, BACKOFF_REFERENCE, ERANGE, OK, AbortQueue, penalty,
                        pop_alg_bytes, push_alg_bytes)
from helpers import make_batch

U64 = (1 << 64) - 1
ABORT, RCOK = d.RC_ABORT, d.RC_RCOK


def test_policy_constants_match_the_header():
    assert (BACKOFF_REFERENCE, BACKOFF_NONE, BACKOFF_EXP) == \
        (d.BACKOFF_REFERENCE, d.BACKOFF_NONE, d.BACKOFF_EXP)


def test_reference_penalty_kats():
    # line 30: max(penalty * 2 ^ abort_cnt, max) = max((10 * 2) ^ cnt, 5) = max(20 ^ cnt, 5)
    # 20 = 0b10100
    assert penalty(BACKOFF_REFERENCE, 10, 5, 1) == 21    # 10100 ^ 00001 = 10101
    assert penalty(BACKOFF_REFERENCE, 10, 5, 2) == 22    # 10100 ^ 00010 = 10110
    assert penalty(BACKOFF_REFERENCE, 10, 5, 3) == 23    # 10100 ^ 00011 = 10111
    assert penalty(BACKOFF_REFERENCE, 10, 5, 4) == 16    # 10100 ^ 00100 = 10000
    assert penalty(BACKOFF_REFERENCE, 10, 5, 5) == 17    # 10100 ^ 00101 = 10001
    assert penalty(BACKOFF_REFERENCE, 10, 5, 20) == 5    # 10100 ^ 10100 = 0, max(0, 5)
    # config.h:112-114: 10 ms and 500 ms in ns: (2e7 ^ cnt) < 5e8 for every cnt < 2^28
    for cnt in (1, 2, 7, 1000, (1 << 28) - 1):
        assert penalty(BACKOFF_REFERENCE, 10 * 1000000, 5 * 100 * 1000000, cnt) == 500000000
    # u64: penalty * 2 wraps before the XOR
    assert penalty(BACKOFF_REFERENCE, 1 << 63, 0, 1) == 1


def test_none_is_the_flat_penalty():
    for cnt in (1, 5, 100):
        assert penalty(BACKOFF_NONE, 10, 5, cnt) == 10   # line 28 alone (BACKOFF false)


def test_exp_penalty_and_saturation():
    assert [penalty(BACKOFF_EXP, 10, 1000, c) for c in (1, 2, 3, 6, 7)] == [20, 40, 80, 640, 1000]
    big = 1 << 62
    assert penalty(BACKOFF_EXP, 1, U64, 63) == 1 << 63           # the last exact shift
    assert penalty(BACKOFF_EXP, 1, big, 63) == big               # min
    assert penalty(BACKOFF_EXP, 1, U64, 64) == U64               # cnt >= 64: penalty_max
    assert penalty(BACKOFF_EXP, 1, 77, 70) == 77
    assert penalty(BACKOFF_EXP, 3, U64, 63) == U64               # 3 << 63 loses a bit: penalty_max
    assert penalty(BACKOFF_EXP, 3, 99, 63) == 99
    assert penalty(BACKOFF_EXP, 0, 5, 70) == 5 and penalty(BACKOFF_EXP, 0, 5, 3) == 0


def one_txn_batch(k=1):
    return make_batch([[(7, d.WR)]] * k)


def test_first_abort_has_cnt_1_and_counts_compose():
    q = AbortQueue(8, 8, 10, 1000, BACKOFF_EXP)
    assert q.push(one_txn_batch(), [ABORT], ABORT, None, None, 0) == (OK, 1, 1)
    _, _, _, rows = q.pop(1 << 40)
    assert list(rows["cnt"]) == [1] and list(rows["due"]) == [20]
    q.push(one_txn_batch(), [ABORT], ABORT, [9], rows["cnt"], 5)
    _, _, _, rows = q.pop(1 << 40)
    assert list(rows["cnt"]) == [2] and list(rows["due"]) == [45] and list(rows["src"]) == [9]
    q.push(one_txn_batch(), [ABORT], ABORT, None, [0xFFFFFFFF], 0)   # the count saturates
    assert list(q.pop(1 << 40)[3]["cnt"]) == [0xFFFFFFFF]


def test_strict_compare():
    q = AbortQueue(8, 8, 10, 10, BACKOFF_NONE)
    q.push(one_txn_batch(), [ABORT], ABORT, None, None, 5)       # due 15
    assert q.pop(15)[:3] == (OK, 0, 0) and q.size() == (1, 1)    # line 62: 15 < 15 is false
    assert q.pop(16)[:3] == (OK, 1, 1) and q.size() == (0, 0)


def test_release_order_due_then_push_order():
    q = AbortQueue(16, 16, 10, 1000, BACKOFF_EXP)
    b = one_txn_batch(3)
    q.push(b, [ABORT] * 3, ABORT, [10, 11, 12], [2, 0, 2], 0)    # due 80, 20, 80
    q.push(b, [ABORT] * 3, ABORT, [20, 21, 22], [0, 2, 1], 40)   # due 60, 120, 80
    _, n, _, rows = q.pop(81)
    assert n == 5
    assert list(rows["due"]) == [20, 60, 80, 80, 80]
    assert list(rows["src"]) == [11, 20, 10, 12, 22]             # equal due: push order
    assert q.size() == (1, 1) and list(q.pop(121)[3]["src"]) == [21]


def test_due_saturates():
    q = AbortQueue(4, 4, 10, 10, BACKOFF_NONE)
    q.push(one_txn_batch(), [ABORT], ABORT, None, None, U64 - 3)
    assert q.pop(U64)[:3] == (OK, 0, 0)                          # due = 2^64 - 1 is never < now
    assert q.heap[0][0] == U64


def test_erange_leaves_the_queue_unchanged():
    q = AbortQueue(2, 100, 1, 1, BACKOFF_NONE)
    b = make_batch([[(1, d.RD)], [(2, d.WR), (3, d.RD)], []])
    assert q.push(b, [ABORT] * 3, ABORT, None, None, 0) == (ERANGE, 3, 3) and q.size() == (0, 0)
    assert q.push(b, [ABORT, RCOK, ABORT], ABORT, None, None, 0) == (OK, 2, 1)
    assert q.pop(10, cap_txn=1)[:3] == (ERANGE, 2, 1) and q.size() == (2, 1)
    assert q.pop(10, nnz_base=0xFFFFFFFF)[:3] == (ERANGE, 2, 1)
    code, n, m, rows = q.pop(10, txn_base=3, nnz_base=5)
    assert (code, n, m) == (OK, 2, 1) and list(rows["offsets"]) == [5, 6, 6] and list(rows["src"]) == [0, 2]


def test_three_epoch_trace():
    """Clock = epoch index, EXP with penalty 1, max 4: cnt 1 -> 2, cnt 2 -> 4,
    cnt 3 -> 4.  Txns A, B, C abort in epoch 0."""
    q = AbortQueue(16, 64, 1, 4, BACKOFF_EXP)
    e0 = make_batch([[(1, d.WR)], [(2, d.WR), (3, d.RD)], [(4, d.RD)], [(5, d.WR)]])
    # epoch 0: A (0), B (1), C (2) abort, txn 3 commits; due = 0 + 2
    assert q.push(e0, [ABORT, ABORT, ABORT, RCOK], ABORT, None, None, 0) == (OK, 3, 4)
    # epoch 1: pop(1), pop(2): 2 < 2 is false, nothing leaves
    assert q.pop(1)[1] == 0 and q.pop(2)[1] == 0
    # epoch 3: all three leave, in push order
    code, n, m, r = q.pop(3)
    assert (n, m) == (3, 4) and list(r["src"]) == [0, 1, 2] and list(r["cnt"]) == [1, 1, 1]
    assert list(r["offsets"]) == [0, 1, 3, 4] and list(r["keys"]) == [1, 2, 3, 4]
    e3 = d.EpochBatch(r["offsets"], r["keys"], r["acctype"])
    # epoch 3: B aborts again (cnt 2: due 3 + 4 = 7), A and C commit; a fresh D (src 9) aborts: due 5
    q.push(e3, [RCOK, ABORT, RCOK], ABORT, r["src"], r["cnt"], 3)
    q.push(one_txn_batch(), [ABORT], ABORT, [9], None, 3)
    assert q.size() == (2, 3)
    code, n, m, r = q.pop(6)                                      # D only
    assert list(r["src"]) == [9] and list(r["due"]) == [5]
    code, n, m, r = q.pop(8)                                      # B, its second retry
    assert list(r["src"]) == [1] and list(r["cnt"]) == [2] and list(r["keys"]) == [2, 3]
    assert q.size() == (0, 0)


def test_alg_bytes_formulas():
    for a in ((0, 0, 0), (1000, 300, 4800), (65536, 65536, 1 << 20)):
        assert d.abortq_push_alg_bytes(*a) == push_alg_bytes(*a) == d.select_alg_bytes(*a, 1) + 12 * a[1]
    for a in ((0, 0, 0, 0), (1000, 16000, 0, 0), (1000, 16000, 400, 6400), (5, 80, 5, 80)):
        assert d.abortq_pop_alg_bytes(*a) == pop_alg_bytes(*a)
    assert pop_alg_bytes(10, 100, 4, 40) == 80 + 44 + 240 + 1800 + 20 + 28 + 320
