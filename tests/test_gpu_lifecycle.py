"""Destroying a context returns its device memory: every buffer of a context
is owned by it (DevBuf, dcc_ctx.h) and goes when dcc_destroy returns."""
import numpy as np
import pytest
import torch

import deneva_amd as d
from deneva_amd import RC_ABORT, WR

pytestmark = pytest.mark.gpu

CYCLES = 16


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def one_context(b, held, rows):
    """Open a context, run one host-batch epoch of every engine and an index
    insert, return the free device memory with all of it allocated, close."""
    with d.Engine(0) as eng:
        eng.reserve(4096, 65536)
        rc, _, _ = eng.occ_validate_epoch(b, want_tn=True, append_history=True)
        eng.calvin_order_epoch(b, want_group=True, held=held)
        eng.nowait_lock_epoch(b, held=held)
        eng.maat_validate_epoch(b)
        eng.select_batch(b, rc, want=RC_ABORT)
        eng.index_insert(rows, rows + 7)
        return free_bytes()


def test_destroy_returns_device_memory():
    """Cycles 3..16 of open / work / close must cost less than half of one
    context's own footprint (f0 - f_in, measured here): a context that leaks
    a tenth of its buffers per cycle fails, allocator granularity does not."""
    b = d.gen_ycsb(n_txn=1024, req_per_query=16, zipf_theta=0.6)
    held = (np.arange(64, dtype=np.uint64) * 3 + 1, np.full(64, WR, np.uint8))
    rows = np.arange(1, 1001, dtype=np.uint64)
    torch.zeros(1, device="cuda:0")  # the runtime's own start-up allocations come first
    f0 = free_bytes()
    f_in = f2 = None
    for c in range(1, CYCLES + 1):
        f = one_context(b, held, rows)
        if c == 1:
            f_in = f
        if c == 2:
            f2 = free_bytes()
    f16 = free_bytes()
    print(f"f0 {f0} f_in {f_in} f2 {f2} f16 {f16}: footprint {f0 - f_in}, 14 cycles cost {f2 - f16}")
    assert f0 - f_in > 0, "the context's work allocated nothing"
    assert f2 - f16 < (f0 - f_in) / 2
