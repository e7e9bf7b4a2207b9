"""deneva_amd — MI355X-native batched concurrency control for Deneva's hot path.

The engine decides commit/abort (OCC) and lock-grant order (Calvin) for a whole
epoch of transactions on gfx950 (libdcc.so, C ABI in include/dcc.h).  This
package is the thin Python view of that ABI used by tests and bench.py.
"""
from ._abi import (ACCESS_NONE, BACKOFF_EXP, BACKOFF_NONE, BACKOFF_REFERENCE, DEVICE_PTRS, GROUP_NONE, ISO_READ_COMMITTED, ISO_READ_UNCOMMITTED, ISO_SERIALIZABLE, KEY_RESERVED, LOCK_EX, LOCK_SH, OCC_APPEND_HISTORY, OCC_DEFER_FINISH, RC_ABORT, RC_RCOK,
                   RC_WAIT, RD, SCAN, VTS_BASE, VTS_NONE, WD_GONE, WD_RUN, WR, XP, DccError, EXPORTED, LIB_PATH)
from .engine import (AbortQueue, Engine, EpochBatch, LockTable, locktab_epoch_alg_bytes, locktab_release_alg_bytes, abortq_pop_alg_bytes, abortq_push_alg_bytes, alg_bytes, calvin_alg_bytes, comm_unique_id, gen_tpcc, gen_ycsb,
                     key_shard, mvcc_access_alg_bytes, mvcc_alg_bytes, nowait_alg_bytes, nowait_iso_alg_bytes, read_batch_file, select_alg_bytes, shard_filter, shard_of_keys, tpcc_params, tso_access_alg_bytes, tso_alg_bytes, waitdie_alg_bytes, waitdie_carry_alg_bytes, write_batch_file,
                     ycsb_params)

__all__ = [
    "Engine", "EpochBatch", "AbortQueue", "LockTable", "LOCK_EX", "LOCK_SH", "locktab_epoch_alg_bytes",
    "locktab_release_alg_bytes", "BACKOFF_NONE", "BACKOFF_REFERENCE", "BACKOFF_EXP",
    "abortq_push_alg_bytes", "abortq_pop_alg_bytes", "DccError", "gen_ycsb", "gen_tpcc", "ycsb_params", "tpcc_params",
    "shard_filter", "shard_of_keys", "key_shard", "comm_unique_id", "alg_bytes", "calvin_alg_bytes", "nowait_alg_bytes", "tso_alg_bytes", "mvcc_alg_bytes", "select_alg_bytes", "RD", "WR", "XP", "SCAN",
    "waitdie_alg_bytes", "waitdie_carry_alg_bytes", "mvcc_access_alg_bytes", "tso_access_alg_bytes", "WD_RUN", "WD_GONE",
    "RC_RCOK", "RC_ABORT", "RC_WAIT", "KEY_RESERVED", "GROUP_NONE", "ACCESS_NONE", "VTS_BASE", "VTS_NONE", "DEVICE_PTRS",
    "ISO_SERIALIZABLE", "ISO_READ_COMMITTED", "ISO_READ_UNCOMMITTED", "nowait_iso_alg_bytes",
    "OCC_APPEND_HISTORY", "OCC_DEFER_FINISH", "EXPORTED", "LIB_PATH", "read_batch_file", "write_batch_file",
]
