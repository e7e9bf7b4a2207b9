"""The GPU index (csrc/index.hip) restated: the dict oracle of its answers and
the sizing rule of its table.  Pure Python / numpy: no GPU."""
from __future__ import annotations

import numpy as np

from deneva_amd._abi import ROW_NONE

IX_MIN_BITS = 12  # dcc_ctx::index_reserve: std::max(ix_bits, 12)


def index_oracle(inserts, probe):
    """BucketHeader::insert_item / read_item: the newest item of a key."""
    m = {}
    for keys, rows in inserts:
        for k, r in zip(keys.tolist(), rows.tolist()):
            m[k] = r
    return np.array([m.get(k, ROW_NONE) for k in probe.tolist()], np.uint64)


def bits_after_insert(bits, nkeys, n):
    """Table size (log2 slots) after an insert of n keys (duplicates counted)
    into an index of `nkeys` distinct keys and 2^bits slots (0: no table yet):
    index_reserve(nkeys + n) keeps the table while 2 * want <= capacity, else
    takes the smallest size >= 2^12 with 2 * want <= 2^bits (never shrinks)."""
    want = nkeys + n
    if n == 0 or (bits and 2 * want <= (1 << bits)):
        return bits
    bits = max(bits, IX_MIN_BITS)
    while (1 << bits) < 2 * want:
        bits += 1
    return bits
