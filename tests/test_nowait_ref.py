"""CPU: the NO_WAIT replay (nowait_ref.py, the parity reference of
dcc_nowait_lock_epoch) against hand-worked answers, and the parts of the
entry point that need no GPU."""
import ctypes as C
import time

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import ACCESS_NONE, RC_ABORT, RC_RCOK, RD, WR, _abi
from helpers import make_batch
from nowait_cases import KATS
from nowait_ref import replay


def held_arrays(held):
    if held is None:
        return None
    return (np.array([k for k, _ in held], np.uint64), np.array([t for _, t in held], np.uint8))


@pytest.mark.parametrize("case", KATS, ids=[c[0] for c in KATS])
def test_known_answers(case):
    _, txns, held, rc, conflict = case
    grc, gcf = replay(make_batch(txns), held_arrays(held))
    assert grc.tolist() == rc
    assert gcf.tolist() == conflict


def test_constants():
    assert ACCESS_NONE == 0xFFFFFFFF and RC_RCOK == 0 and RC_ABORT == 2


def test_release_order_and_counts():
    """Three SH owners, one aborts later and releases: the row stays SH-held by
    the other two, so an EX request still aborts."""
    b = make_batch([[(1, RD)], [(1, RD)], [(9, WR)], [(1, RD), (9, RD)], [(1, WR)], [(9, RD)]])
    rc, cf = replay(b)
    assert rc.tolist() == [0, 0, 0, 2, 2, 2]
    assert cf.tolist() == [ACCESS_NONE, ACCESS_NONE, ACCESS_NONE, 1, 0, 0]


def test_alg_bytes_formula():
    # 4(N+1) + 9 nnz + 16 nnz (one lock-table slot per request) + N [+ 4N]
    n, nnz = 1 << 20, 16 << 20
    base = 4 * (n + 1) + 9 * nnz + 16 * nnz + n
    assert d.nowait_alg_bytes(n, nnz, False) == base
    assert d.nowait_alg_bytes(n, nnz, True) == base + 4 * n
    assert d.nowait_alg_bytes(0, 0, True) == 4


def test_null_arguments_are_einval():
    """No context, no batch or no out_rc: DCC_EINVAL, without touching a GPU."""
    b = make_batch([[(1, WR)]]).to_c()
    rc = np.zeros(1, np.uint8)
    f = _abi.lib.dcc_nowait_lock_epoch
    assert f(None, C.byref(b), None, rc.ctypes.data, None, None) == _abi.DCC_EINVAL
    assert f(None, None, None, None, None, None) == _abi.DCC_EINVAL


def test_replay_speed():
    """The C2 shape (65,536 x 16) replays fast enough to serve the GPU tests."""
    b = d.gen_ycsb(n_txn=65536, zipf_theta=0.9)
    for _ in range(2):  # a second try only if the machine was busy during the first
        t0 = time.perf_counter()
        rc, cf = replay(b)
        dt = time.perf_counter() - t0
        if dt < 2.0:
            break
    assert dt < 2.0, f"replay took {dt:.2f} s"
    assert 0 < int((rc == RC_RCOK).sum()) < b.n_txn
    assert np.array_equal(cf == ACCESS_NONE, rc == RC_RCOK)
    assert int(((rc == RC_ABORT) & (cf > 0)).sum()) > 0
