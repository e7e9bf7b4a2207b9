"""numpy restatement of dcc_batch_select: the parity reference of the device
select (select.hip) and of Engine.select_batch.

The txns with rc[i] == want, in index order, each with its accesses in list
order, go to rows txn_base.. and accesses nnz_base.. of the output arrays.
"""
from __future__ import annotations

import numpy as np

OK, ERANGE = 0, -34


def select(batch, rc, want, src_in=None, txn_base=0, nnz_base=0, cap_txn=None, cap_nnz=None):
    """Returns (code, n_sel, nnz_sel, rows).  rows is None unless code == OK,
    else a dict of the values written: offsets u32[n_sel + 1] (at txn_base..),
    keys u64 / acctype u8 [nnz_sel] (at nnz_base..), src u32[n_sel] and, where
    the batch has them, start_tn / finish_tn / order u64[n_sel] (at
    txn_base..).  cap_* None: unlimited."""
    off = np.asarray(batch.offsets).astype(np.int64)
    n = off.size - 1
    rc = np.asarray(rc, np.uint8)[:n]
    sel = np.nonzero(rc == np.uint8(want))[0]
    lens = (off[1:] - off[:-1])[sel]
    n_sel, nnz_sel = int(sel.size), int(lens.sum())
    if (cap_txn is not None and n_sel > cap_txn) or (cap_nnz is not None and nnz_sel > cap_nnz) \
            or nnz_base + nnz_sel > 0xFFFFFFFF:
        return ERANGE, n_sel, nnz_sel, None
    # the accesses of selected txn q: off[sel[q]] + 0 .. lens[q] - 1
    starts = np.concatenate([[0], np.cumsum(lens)])
    idx = np.repeat(off[sel] - starts[:-1], lens) + np.arange(nnz_sel, dtype=np.int64)
    keys = np.asarray(batch.keys).astype(np.uint64)
    rows = {
        "offsets": (nnz_base + starts).astype(np.uint32),
        "keys": keys[idx],
        "acctype": np.asarray(batch.acctype, np.uint8)[idx],
        "src": (sel if src_in is None else np.asarray(src_in)[sel]).astype(np.uint32),
    }
    for name in ("start_tn", "finish_tn", "order"):
        a = getattr(batch, name)
        if a is not None:
            rows[name] = np.asarray(a).astype(np.uint64)[sel]
    return OK, n_sel, nnz_sel, rows


def alg_bytes(n_txn, n_sel, nnz_sel, n_txn_arrays):
    """dcc_select_alg_bytes as documented in dcc.h."""
    return 4 * (n_txn + 1) + n_txn + 18 * nnz_sel + 4 * (n_sel + 1) + 16 * n_sel * n_txn_arrays
