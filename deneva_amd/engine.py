"""Python mirror of the engine's C ABI for tests, bench and tooling.

The product is libdcc.so (HIP kernels + C ABI) and its C++ host shim
(deneva_amd/csrc/host/); this module is plumbing over ``include/dcc.h``:
numpy (host) or torch (device) arrays in, per-transaction RC codes out.

Names follow the reference's plugin surface:
``Engine.occ_validate_epoch`` is ``TxnManager::validate`` / ``OptCC::validate``
(concurrency_control/occ.cpp:42) for a whole epoch; ``Engine.calvin_order_epoch``
is the ``Sequencer::send_next_batch`` -> ``acquire_locks`` hand-off
(system/sequencer.cpp:283, benchmarks/ycsb_txn.cpp:49).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _abi
from ._abi import DccError, lib


def _ptr(a) -> Optional[int]:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"], "arrays must be contiguous"
        return a.ctypes.data
    return int(a.data_ptr())  # torch tensor


def _itemsize(a) -> int:
    return int(a.itemsize) if isinstance(a, np.ndarray) else int(a.element_size())


def pack_acctype(at) -> np.ndarray:
    """access_t bytes -> 2-bit codes, four per byte (DCC_ACCTYPE_2BIT)."""
    at = np.asarray(at, np.uint8)
    pad = np.zeros((-at.size) % 4, np.uint8)
    q = np.concatenate([at, pad]).reshape(-1, 4) & 3
    return (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8)


def _is_signed(a) -> bool:
    """A signed numpy array.  Device (torch) tensors are exempt: torch holds
    u32 row ids as int32 tensors, read bit for bit as DCC_KEYS_U32."""
    return isinstance(a, np.ndarray) and a.dtype.kind == "i"


def _is_device(a) -> bool:
    return a is not None and not isinstance(a, np.ndarray) and bool(getattr(a, "is_cuda", False))


@dataclass
class EpochBatch:
    """One epoch as a CSR of per-transaction access lists (dcc_batch)."""

    offsets: object            # u32 [n_txn+1]
    keys: object               # u64 [nnz]
    acctype: object            # u8  [nnz] access_t
    start_tn: object = None    # u64 [n_txn] or None
    finish_tn: object = None   # u64 [n_txn] or None
    order: object = None       # u64 [n_txn] (Calvin sequence key) or None
    meta: dict = field(default_factory=dict)

    @property
    def n_txn(self) -> int:
        return int(self.offsets.shape[0]) - 1

    @property
    def nnz(self) -> int:
        return int(self.keys.shape[0])

    @property
    def on_device(self) -> bool:
        return _is_device(self.offsets)

    def to_c(self, flags: int = 0) -> _abi.Batch:
        b = _abi.Batch()
        b.n_txn = self.n_txn
        b.nnz = self.nnz
        b.offsets = _ptr(self.offsets)
        b.keys = _ptr(self.keys)
        b.acctype = _ptr(self.acctype)
        b.start_tn = _ptr(self.start_tn)
        b.finish_tn = _ptr(self.finish_tn)
        b.order = _ptr(self.order)
        b.flags = flags | (_abi.DEVICE_PTRS if self.on_device else 0)
        # compact transfer forms (dcc.h): 4-byte keys / timestamps, packed types
        if _itemsize(self.keys) == 4:
            if _is_signed(self.keys):
                raise TypeError("4-byte keys must be an unsigned dtype (DCC_KEYS_U32 row ids)")
            b.flags |= _abi.KEYS_U32
        if self.meta.get("acctype_2bit"):
            b.flags |= _abi.ACCTYPE_2BIT
        if self.start_tn is not None:
            if self.finish_tn is None or _itemsize(self.start_tn) != _itemsize(self.finish_tn):
                raise TypeError("start_tn and finish_tn must both be set, with the same dtype size")
            if _itemsize(self.start_tn) == 4:
                b.flags |= _abi.TN_U32
        return b

    def to_torch(self, device="cuda"):
        import torch

        def cv(a):
            if a is None:
                return None
            return torch.from_numpy(np.ascontiguousarray(a)).to(device)

        return EpochBatch(cv(self.offsets), cv(self.keys), cv(self.acctype), cv(self.start_tn),
                          cv(self.finish_tn), cv(self.order), dict(self.meta))


def _check(code: int, ctx=None) -> None:
    if code != _abi.DCC_OK:
        detail = lib.dcc_last_error(ctx).decode() if ctx else ""
        raise DccError(code, f"{_abi.strerror(code)}{': ' + detail if detail else ''}")


class Engine:
    """One engine context per process and device (OptCC::init / occ_man).
    devices=[...]: one process drives several GPUs (dcc_init_multi): every
    epoch is key-sharded over them inside the context."""

    def __init__(self, device: int = 0, devices=None):
        h = C.c_void_p()
        if devices is not None:
            ids = (C.c_int * len(devices))(*devices)
            code = lib.dcc_init_multi(C.byref(h), len(devices), ids)
        else:
            code = lib.dcc_init(C.byref(h), device)
        if code != _abi.DCC_OK:
            detail = lib.dcc_last_error(h).decode() if h.value else ""
            raise DccError(code, f"dcc_init(device={device}, devices={devices}): "
                                 f"{_abi.strerror(code)} {detail}")
        self._h = h
        self._queues = []  # AbortQueue objects alive on this context

    def close(self) -> None:
        if getattr(self, "_h", None):
            for q in list(getattr(self, "_queues", [])):
                q._q = None  # dcc_destroy frees the queues and lock tables still alive
            self._queues = []
            lib.dcc_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr: Optional[int]) -> None:
        _check(lib.dcc_set_stream(self._h, stream_ptr), self._h)

    def set_profiling(self, enable: bool) -> None:
        _check(lib.dcc_set_profiling(self._h, 1 if enable else 0), self._h)

    def set_option(self, option: int, value: int) -> None:
        _check(lib.dcc_set_option(self._h, option, value), self._h)

    def reserve(self, max_txn: int, max_nnz: int) -> None:
        _check(lib.dcc_reserve(self._h, max_txn, max_nnz), self._h)

    def host_empty(self, n: int, dtype) -> np.ndarray:
        """A numpy array in pinned host memory (dcc_host_alloc): host batches
        and outputs in it move at DMA speed with no staging copy.  Freed with
        the array."""
        import weakref
        dt = np.dtype(dtype)
        nbytes = max(int(n), 1) * dt.itemsize
        p = C.c_void_p()
        _check(lib.dcc_host_alloc(self._h, nbytes, C.byref(p)), self._h)
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dt, count=max(int(n), 1))[:int(n)]
        # freed with the buffer (no context needed: the engine may be gone)
        weakref.finalize(buf, lib.dcc_host_free, None, p.value)
        return arr

    def compact_host_batch(self, b: "EpochBatch") -> "EpochBatch":
        """The batch in pinned host memory and its compact transfer form:
        u32 keys when every key fits, 2-bit access types, u32 timestamps when
        they fit (dcc.h DCC_KEYS_U32 / DCC_ACCTYPE_2BIT / DCC_TN_U32) -- what a
        host shim builds directly (OccEpoch) to cut the PCIe bytes."""
        def pin(a, dtype):
            a = np.asarray(a)
            out = self.host_empty(a.size, dtype)
            out[...] = a
            return out
        keys = np.asarray(b.keys, np.uint64)
        k = pin(keys, np.uint32) if (keys.size == 0 or int(keys.max()) < (1 << 32)) else pin(keys, np.uint64)
        at = pin(pack_acctype(b.acctype), np.uint8)
        st = ft = None
        if b.start_tn is not None:
            big = max(int(np.max(b.start_tn, initial=0)), int(np.max(b.finish_tn, initial=0)))
            dt = np.uint32 if big < (1 << 32) else np.uint64
            st, ft = pin(b.start_tn, dt), pin(b.finish_tn, dt)
        od = None if b.order is None else pin(b.order, np.uint64)
        meta = dict(b.meta)
        meta["acctype_2bit"] = True
        meta["nnz"] = int(keys.size)
        return EpochBatch(pin(b.offsets, np.uint32), k, at, st, ft, od, meta)

    # ------------------------------------------------------------ OCC
    def occ_validate_epoch(self, batch: EpochBatch, want_tn: bool = False,
                           append_history: bool = False, out_rc=None, out_tn=None,
                           defer_finish: bool = False, shard_self: bool = False):
        """Decide every txn of the epoch; returns (rc u8[n], tn u64[n] | None, stats).
        defer_finish: 2PC participant -- rc is the local vote; commit tn and
        history wait for ``occ_finish_epoch(global_rc)``.  shard_self: a
        key-sharded rank given the WHOLE epoch keeps its own key shard
        (DCC_SHARD_SELF)."""
        n = batch.n_txn
        dev = batch.on_device
        if out_rc is None:
            if dev:
                import torch
                out_rc = torch.empty(max(n, 1), dtype=torch.uint8, device=batch.offsets.device)
            else:
                out_rc = np.empty(max(n, 1), np.uint8)
        if want_tn and out_tn is None:
            if dev:
                import torch
                out_tn = torch.empty(max(n, 1), dtype=torch.int64, device=batch.offsets.device)
            else:
                out_tn = np.empty(max(n, 1), np.uint64)
        st = _abi.Stats()
        flags = _abi.OCC_APPEND_HISTORY if append_history else 0
        if defer_finish:
            flags |= _abi.OCC_DEFER_FINISH
        if shard_self:
            flags |= _abi.SHARD_SELF
        b = batch.to_c(flags)
        _check(lib.dcc_occ_validate_epoch(self._h, C.byref(b), _ptr(out_rc), _ptr(out_tn),
                                          C.byref(st)), self._h)
        if defer_finish:
            self._fin_n = n
        return out_rc[:n], (out_tn[:n] if want_tn else None), st.as_dict()

    def occ_submit_epoch(self, batch: EpochBatch, out_rc, out_tn=None,
                         append_history: bool = False) -> int:
        """Enqueue an epoch on the pipeline (dcc_occ_submit_epoch) and return
        its ticket; the batch arrays and outputs must stay alive and unchanged
        until ``occ_wait_epoch(ticket)``.  Results equal dcc_occ_validate_epoch
        on the epochs in submit order (commit tn and the history append
        included: each epoch's central_finish runs on its lane right behind its
        decision once the epoch before it finished, DCC_OPT_PIPE_CHAIN, or the
        context runs it as the epoch completes)."""
        b = batch.to_c(_abi.OCC_APPEND_HISTORY if append_history else 0)
        t = C.c_uint64(0)
        _check(lib.dcc_occ_submit_epoch(self._h, C.byref(b), _ptr(out_rc), _ptr(out_tn),
                                        C.byref(t)), self._h)
        return int(t.value)

    def occ_wait_epoch(self, ticket: int) -> dict:
        """Complete every epoch up to `ticket` (submit order); that epoch's stats."""
        st = _abi.Stats()
        _check(lib.dcc_occ_wait_epoch(self._h, ticket, C.byref(st)), self._h)
        return st.as_dict()

    @property
    def pending_finish(self) -> Optional[int]:
        """n_txn of the epoch awaiting occ_finish_epoch, or None."""
        return getattr(self, "_fin_n", None)

    def occ_finish_epoch(self, final_rc, want_tn: bool = True, out_tn=None):
        """central_finish with the global RC of a deferred epoch
        (dcc_occ_finish_epoch; OptCC::finish after RFIN, occ.cpp:248-294):
        globally committed writers take tn = tnc+1.. and join the history.
        Returns tn u64[n] | None."""
        dev = _is_device(final_rc)
        n = int(final_rc.shape[0])
        if self.pending_finish is not None and n != self.pending_finish:
            raise ValueError(f"final_rc holds {n} txns, the pending epoch {self.pending_finish}")
        if not dev:
            final_rc = np.ascontiguousarray(final_rc, dtype=np.uint8)
        if want_tn and out_tn is None:
            if dev:
                import torch
                out_tn = torch.empty(max(n, 1), dtype=torch.int64, device=final_rc.device)
            else:
                out_tn = np.empty(max(n, 1), np.uint64)
        _check(lib.dcc_occ_finish_epoch(self._h, _ptr(final_rc), _ptr(out_tn),
                                        _abi.DEVICE_PTRS if dev else 0), self._h)
        self._fin_n = None
        return out_tn[:n] if want_tn else None

    # ----------------------------------------------------------------- MaaT
    def maat_validate_epoch(self, batch: EpochBatch, want_cts: bool = True,
                            read_and_prewrite: bool = False, out_rc=None, out_cts=None):
        """MaaT epoch (dcc_maat_validate_epoch): returns (rc u8[n],
        commit_ts u64[n] | None, stats).  read_and_prewrite: the TPC-C path."""
        n = batch.n_txn
        dev = batch.on_device
        if out_rc is None:
            if dev:
                import torch
                out_rc = torch.empty(max(n, 1), dtype=torch.uint8, device=batch.offsets.device)
            else:
                out_rc = np.empty(max(n, 1), np.uint8)
        if want_cts and out_cts is None:
            if dev:
                import torch
                out_cts = torch.empty(max(n, 1), dtype=torch.int64, device=batch.offsets.device)
            else:
                out_cts = np.empty(max(n, 1), np.uint64)
        st = _abi.Stats()
        b = batch.to_c(_abi.MAAT_READ_AND_PREWRITE if read_and_prewrite else 0)
        _check(lib.dcc_maat_validate_epoch(self._h, C.byref(b), _ptr(out_rc), _ptr(out_cts),
                                           C.byref(st)), self._h)
        return out_rc[:n], (out_cts[:n] if want_cts else None), st.as_dict()

    # the persistent row tables (MaaT's, TIMESTAMP's): a row's two u64 values
    def _rows_set(self, fn, what, keys, a, b) -> None:
        keys = np.ascontiguousarray(keys, np.uint64)
        a = np.ascontiguousarray(a, np.uint64)
        b = np.ascontiguousarray(b, np.uint64)
        if a.shape[0] != keys.shape[0] or b.shape[0] != keys.shape[0]:
            raise ValueError(f"{what} must have one length")
        _check(fn(self._h, _ptr(keys), _ptr(a), _ptr(b), keys.shape[0]), self._h)

    def _rows_get(self, fn, keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        a = np.empty(keys.shape[0], np.uint64)
        b = np.empty(keys.shape[0], np.uint64)
        _check(fn(self._h, _ptr(keys), _ptr(a), _ptr(b), keys.shape[0]), self._h)
        return a, b

    def maat_rows_set(self, keys, last_read, last_write) -> None:
        self._rows_set(lib.dcc_maat_rows_set, "maat_rows_set: keys, last_read and last_write",
                       keys, last_read, last_write)

    def maat_rows_get(self, keys):
        """(last_read u64[n], last_write u64[n]) of the rows; (0, 0) for rows never seen."""
        return self._rows_get(lib.dcc_maat_rows_get, keys)

    def maat_rows_clear(self) -> None:
        _check(lib.dcc_maat_rows_clear(self._h), self._h)

    @property
    def maat_rows_size(self) -> int:
        return int(lib.dcc_maat_rows_size(self._h))

    def occ_validate_snapshot(self, batch: EpochBatch, active_off, active_idx,
                              hist_top=None, out_rc=None):
        """Captured-snapshot validation (dcc_occ_validate_snapshot): every txn
        against its own captured history head and active list
        (occ.cpp:137-158); returns (rc u8[n], stats).  Arrays live where the
        batch lives (numpy on the host, torch on the device)."""
        n = batch.n_txn
        dev = batch.on_device
        if not dev:
            active_off = np.ascontiguousarray(active_off, np.uint32)
            active_idx = np.ascontiguousarray(active_idx, np.uint32)
            if hist_top is not None:
                hist_top = np.ascontiguousarray(hist_top, np.uint64)
        if out_rc is None:
            if dev:
                import torch
                out_rc = torch.empty(max(n, 1), dtype=torch.uint8, device=batch.offsets.device)
            else:
                out_rc = np.empty(max(n, 1), np.uint8)
        sn = _abi.Snapshot()
        sn.hist_top = _ptr(hist_top)
        sn.active_off = _ptr(active_off)
        sn.active_idx = _ptr(active_idx) if len(active_idx) else None
        st = _abi.Stats()
        b = batch.to_c(0)
        _check(lib.dcc_occ_validate_snapshot(self._h, C.byref(b), C.byref(sn), _ptr(out_rc),
                                             C.byref(st)), self._h)
        return out_rc[:n], st.as_dict()

    def history_append(self, keys: np.ndarray, tn: np.ndarray) -> None:
        keys = np.ascontiguousarray(keys, np.uint64)
        tn = np.ascontiguousarray(tn, np.uint64)
        _check(lib.dcc_occ_history_append(self._h, _ptr(keys), _ptr(tn), keys.shape[0]), self._h)

    def history_trim(self, tn_floor: int) -> None:
        """Drop history entries with tn <= tn_floor (dcc_occ_history_trim)."""
        _check(lib.dcc_occ_history_trim(self._h, tn_floor), self._h)

    def history_export(self):
        """The history's (key, tn) pairs, sorted by (key, tn)."""
        n = C.c_uint64(0)
        _check(lib.dcc_occ_history_export(self._h, None, None, 0, C.byref(n)), self._h)
        k = np.empty(n.value, np.uint64)
        t = np.empty(n.value, np.uint64)
        if n.value:
            _check(lib.dcc_occ_history_export(self._h, _ptr(k), _ptr(t), n.value, C.byref(n)),
                   self._h)
        o = np.lexsort((t, k))
        return k[o], t[o]

    def history_clear(self) -> None:
        _check(lib.dcc_occ_history_clear(self._h), self._h)

    @property
    def history_size(self) -> int:
        return int(lib.dcc_occ_history_size(self._h))

    @property
    def tnc(self) -> int:
        return int(lib.dcc_occ_get_tnc(self._h))

    @tnc.setter
    def tnc(self, v: int) -> None:
        _check(lib.dcc_occ_set_tnc(self._h, v), self._h)

    # ------------------------------------------------------------ Calvin
    def calvin_order_epoch(self, batch: EpochBatch, want_group: bool = True,
                           want_wave: bool = False, held=None, out_group=None, out_rc=None):
        """Returns (group u32[nnz] | None, rc u8[n], wave u32[n] | None, stats).
        held = (keys u64[h], acctype u8[h]): rows still locked at the epoch's
        start, per row owners first then waiters (dcc_calvin_order_epoch_held).
        out_group / out_rc: caller-owned output buffers (reused across epochs,
        the engine then replays the epoch's captured launches)."""
        n, nnz = batch.n_txn, batch.nnz
        dev = batch.on_device
        if dev:
            import torch
            d = batch.offsets.device
            rc = out_rc if out_rc is not None else torch.empty(max(n, 1), dtype=torch.uint8, device=d)
            grp = None
            if want_group:
                grp = out_group if out_group is not None else torch.empty(max(nnz, 1), dtype=torch.int32,
                                                                          device=d)
            wav = torch.empty(max(n, 1), dtype=torch.int32, device=d) if want_wave else None
        else:
            rc = out_rc if out_rc is not None else np.empty(max(n, 1), np.uint8)
            grp = None
            if want_group:
                grp = out_group if out_group is not None else np.empty(max(nnz, 1), np.uint32)
            wav = np.empty(max(n, 1), np.uint32) if want_wave else None
        if rc.shape[0] < n or (grp is not None and grp.shape[0] < nnz):
            raise ValueError("calvin_order_epoch: output buffer shorter than the epoch")
        st = _abi.Stats()
        b = batch.to_c()
        if held is None:
            _check(lib.dcc_calvin_order_epoch(self._h, C.byref(b), _ptr(grp), _ptr(rc), _ptr(wav),
                                              C.byref(st)), self._h)
        else:
            hk, ha = held
            if not dev:
                hk = np.ascontiguousarray(hk, np.uint64)
                ha = np.ascontiguousarray(ha, np.uint8)
            h = _abi.CalvinHeld(int(hk.shape[0]), _ptr(hk), _ptr(ha))
            _check(lib.dcc_calvin_order_epoch_held(self._h, C.byref(b), C.byref(h), _ptr(grp),
                                                   _ptr(rc), _ptr(wav), C.byref(st)), self._h)
        return (grp[:nnz] if want_group else None, rc[:n],
                (wav[:n] if want_wave else None), st.as_dict())

    # ------------------------------------------------------ NO_WAIT (2PL)
    def nowait_lock_epoch(self, batch: EpochBatch, held=None, want_conflict: bool = True,
                          out_rc=None, out_conflict=None, shard: bool = False,
                          isolation: int = _abi.ISO_SERIALIZABLE):
        """NO_WAIT lock acquisition of an epoch (dcc_nowait_lock_epoch): returns
        (rc u8[n], conflict u32[n] | None, stats).  held = (keys u64[h],
        acctype u8[h]): rows still locked by txns of earlier epochs.
        conflict[i] is the ordinal of the request an aborted txn aborted at,
        ACCESS_NONE for a committed one.  shard: on a multi-GPU engine or one
        with a communicator the epoch is key-sharded across the ranks
        (DCC_SHARD_SELF): every rank passes this whole batch and held list and
        gets the whole outputs.  isolation: ISO_SERIALIZABLE, ISO_READ_COMMITTED
        (a read lock is released right after the read) or ISO_READ_UNCOMMITTED
        (every lock is released right after its access)."""
        n = batch.n_txn
        dev = batch.on_device
        if dev:
            import torch
            d = batch.offsets.device
            if out_rc is None:
                out_rc = torch.empty(max(n, 1), dtype=torch.uint8, device=d)
            if want_conflict and out_conflict is None:
                out_conflict = torch.empty(max(n, 1), dtype=torch.int32, device=d)
        else:
            if out_rc is None:
                out_rc = np.empty(max(n, 1), np.uint8)
            if want_conflict and out_conflict is None:
                out_conflict = np.empty(max(n, 1), np.uint32)
        if not want_conflict:
            out_conflict = None
        if out_rc.shape[0] < n or (out_conflict is not None and out_conflict.shape[0] < n):
            raise ValueError("nowait_lock_epoch: output buffer shorter than the epoch")
        st = _abi.Stats()
        b = batch.to_c((_abi.SHARD_SELF if shard else 0) | int(isolation))
        h = None
        if held is not None:
            hk, ha = held
            if not dev:
                hk = np.ascontiguousarray(hk, np.uint64)
                ha = np.ascontiguousarray(ha, np.uint8)
            h = C.byref(_abi.CalvinHeld(int(hk.shape[0]), _ptr(hk), _ptr(ha)))
        _check(lib.dcc_nowait_lock_epoch(self._h, C.byref(b), h, _ptr(out_rc), _ptr(out_conflict),
                                         C.byref(st)), self._h)
        return out_rc[:n], (out_conflict[:n] if want_conflict else None), st.as_dict()

    # ------------------------------------------------ TIMESTAMP (basic T/O)
    def tso_validate_epoch(self, batch: EpochBatch, ts, want_conflict: bool = True,
                           out_rc=None, out_conflict=None):
        """TIMESTAMP epoch (dcc_tso_validate_epoch): returns (rc u8[n],
        conflict u32[n] | None, stats).  ts: u64[n] timestamps, a host array
        for a host batch, a device tensor (int64 read bit for bit) for a device
        batch.  conflict[i] is the ordinal of the access an aborted txn aborted
        at, ACCESS_NONE for a committed one.  The rows' wts / rts persist in the
        context (tso_rows_*)."""
        n = batch.n_txn
        dev = batch.on_device
        if ts is None:
            ts_ptr = None
        elif dev:
            if not _is_device(ts):
                raise TypeError("tso_validate_epoch: a device batch takes a device ts tensor")
            ts_ptr = _ptr(ts) if n else _ptr(batch.offsets)
        else:
            ts = np.ascontiguousarray(ts, np.uint64)
            ts_ptr = _ptr(ts) if n else _ptr(np.zeros(1, np.uint64))
        if ts is not None and (_itemsize(ts) != 8 or ts.shape[0] < n):
            raise ValueError("tso_validate_epoch: ts must hold n_txn 8-byte timestamps")
        if dev:
            import torch
            d = batch.offsets.device
            if out_rc is None:
                out_rc = torch.empty(max(n, 1), dtype=torch.uint8, device=d)
            if want_conflict and out_conflict is None:
                out_conflict = torch.empty(max(n, 1), dtype=torch.int32, device=d)
        else:
            if out_rc is None:
                out_rc = np.empty(max(n, 1), np.uint8)
            if want_conflict and out_conflict is None:
                out_conflict = np.empty(max(n, 1), np.uint32)
        if not want_conflict:
            out_conflict = None
        if out_rc.shape[0] < n or (out_conflict is not None and out_conflict.shape[0] < n):
            raise ValueError("tso_validate_epoch: output buffer shorter than the epoch")
        st = _abi.Stats()
        b = batch.to_c()
        _check(lib.dcc_tso_validate_epoch(self._h, C.byref(b), ts_ptr, _ptr(out_rc),
                                          _ptr(out_conflict), C.byref(st)), self._h)
        return out_rc[:n], (out_conflict[:n] if want_conflict else None), st.as_dict()

    def tso_rows_set(self, keys, wts, rts) -> None:
        self._rows_set(lib.dcc_tso_rows_set, "tso_rows_set: keys, wts and rts", keys, wts, rts)

    def tso_rows_get(self, keys):
        """(wts u64[n], rts u64[n]) of the rows; (0, 0) for rows never seen."""
        return self._rows_get(lib.dcc_tso_rows_get, keys)

    def tso_rows_clear(self) -> None:
        _check(lib.dcc_tso_rows_clear(self._h), self._h)

    @property
    def tso_rows_size(self) -> int:
        return int(lib.dcc_tso_rows_size(self._h))

    # --------------------------------------------------------- WAIT_DIE
    def _waitdie_state(self, what, batch, ts, rc, pos, leave=False):
        """Pointers of the per-txn arrays of a WAIT_DIE call, which are of the
        batch's kind: device tensors (8 / 1 / 4-byte items, read bit for bit)
        for a device batch, host arrays otherwise.  rc (uint8) and pos
        (uint32) are updated in place, so a host call takes them as numpy
        arrays of exactly those types."""
        n = batch.n_txn
        dev = batch.on_device
        arrs = [("ts", ts, 8, np.uint64), ("rc", rc, 1, np.uint8), ("pos", pos, 4, np.uint32)]
        if leave is not False:
            arrs.append(("leave", leave, 1, np.uint8))
        keep, ptrs = [], []
        for name, a, size, dt in arrs:
            if a is None:
                ptrs.append(None)
                continue
            if dev:
                if not _is_device(a):
                    raise TypeError(f"{what}: a device batch takes a device {name} tensor")
                if not a.is_contiguous():
                    raise ValueError(f"{what}: {name} must be contiguous")
            elif name in ("rc", "pos"):
                if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags["C_CONTIGUOUS"] and
                        a.flags["WRITEABLE"]):
                    raise TypeError(f"{what}: {name} is updated in place: a writable contiguous {dt.__name__} array")
            else:
                a = np.ascontiguousarray(a, dt)
            if _itemsize(a) != size or a.shape[0] < n:
                raise ValueError(f"{what}: {name} must hold n_txn {size}-byte items")
            keep.append(a)
            ptrs.append(_ptr(a) if a.shape[0] else _ptr(batch.offsets))
        return keep, ptrs

    def waitdie_lock_epoch(self, batch: EpochBatch, ts, rc, pos, want_conflict: bool = True):
        """WAIT_DIE acquisition epoch (dcc_waitdie_lock_epoch): the WD_RUN
        txns request their locks from pos on.  rc and pos are updated in
        place.  Returns (rc[:n], pos[:n], conflict u32[n] | None, stats);
        conflict[i] is the ordinal of the request a txn waits or died at,
        ACCESS_NONE otherwise.  Arrays are numpy for a host batch, device
        tensors for a device batch."""
        n = batch.n_txn
        keep, ptrs = self._waitdie_state("waitdie_lock_epoch", batch, ts, rc, pos)
        conf = None
        if want_conflict:
            if batch.on_device:
                import torch
                conf = torch.empty(max(n, 1), dtype=torch.int32, device=batch.offsets.device)
            else:
                conf = np.empty(max(n, 1), np.uint32)
        st = _abi.Stats()
        b = batch.to_c()
        _check(lib.dcc_waitdie_lock_epoch(self._h, C.byref(b), *ptrs, _ptr(conf), C.byref(st)), self._h)
        return rc[:n], pos[:n], (conf[:n] if want_conflict else None), st.as_dict()

    def waitdie_release(self, batch: EpochBatch, ts, rc, pos, leave):
        """dcc_waitdie_release: the txns with leave[i] != 0 go (WD_GONE) and
        waiters are promoted to (WD_RUN, pos + 1); rc and pos are updated in
        place.  Returns (n_left, n_promoted, stats)."""
        keep, ptrs = self._waitdie_state("waitdie_release", batch, ts, rc, pos, leave)
        st = _abi.Stats()
        b = batch.to_c()
        left, prom = C.c_uint64(0), C.c_uint64(0)
        _check(lib.dcc_waitdie_release(self._h, C.byref(b), *ptrs, C.byref(left), C.byref(prom), C.byref(st)),
               self._h)
        return int(left.value), int(prom.value), st.as_dict()

    def waitdie_carry(self, batch: EpochBatch, ts, rc, pos, revive=None, src_in=None, fresh=None, fresh_ts=None,
                      fresh_src_base: int = 0, cap_txn=None, cap_nnz=None, out=None):
        """The next WAIT_DIE population where the batch lives (dcc_waitdie_carry):
        the txns that are not WD_GONE, and the GONE ones with revive[i] != 0 as
        (WD_RUN, 0), in index order, then the txns of `fresh` as (WD_RUN, 0) with
        fresh_ts and src = fresh_src_base + j.  Returns (EpochBatch, ts, rc, pos,
        src, kept, stats), the arrays cut to the output's size, numpy for a host
        batch and device tensors for a device batch; kept = the stayers.  `out`
        is an EpochBatch with room (wide keys), its per-txn arrays in
        out.meta["ts" / "rc" / "pos" / "src"] (allocated when absent); out=None
        allocates room for cap_txn txns / cap_nnz accesses (default: both
        batches whole).  A result that does not fit raises DccError(DCC_ERANGE)
        with (n, nnz, kept) it needed in .needed."""
        what = "waitdie_carry"
        n, m = batch.n_txn, batch.nnz
        dev = batch.on_device
        nf = fresh.n_txn if fresh is not None else 0
        mf = fresh.nnz if fresh is not None else 0
        if fresh is not None and fresh.on_device != dev:
            raise TypeError(f"{what}: batch and fresh must both be host or both be device batches")
        if dev:
            import torch
            d = batch.offsets.device

            def empty(k, wide):
                return torch.empty(max(k, 1), dtype={8: torch.int64, 4: torch.int32, 1: torch.uint8}[wide], device=d)
        else:
            def empty(k, wide):
                return np.empty(max(k, 1), {8: np.uint64, 4: np.uint32, 1: np.uint8}[wide])
        keep = []

        def arr(name, a, size, dt, need):
            if a is None:
                return None
            if dev:
                if not _is_device(a):
                    raise TypeError(f"{what}: a device batch takes a device {name} tensor")
                if not a.is_contiguous():
                    raise ValueError(f"{what}: {name} must be contiguous")
            else:
                a = np.ascontiguousarray(a, dt)
            if _itemsize(a) != size or a.shape[0] < need:
                raise ValueError(f"{what}: {name} must hold {need} {size}-byte items")
            keep.append(a)
            # an empty array has no address: any non-null pointer stands for it
            return _ptr(a) if a.shape[0] else _ptr(batch.offsets)

        p_ts, p_rc, p_pos = (arr("ts", ts, 8, np.uint64, n), arr("rc", rc, 1, np.uint8, n),
                             arr("pos", pos, 4, np.uint32, n))
        p_rev, p_src = arr("revive", revive, 1, np.uint8, n), arr("src_in", src_in, 4, np.uint32, n)
        p_fts = arr("fresh_ts", fresh_ts, 8, np.uint64, nf)
        if out is None:
            ct = n + nf if cap_txn is None else int(cap_txn)
            cm = m + mf if cap_nnz is None else int(cap_nnz)
            out = EpochBatch(empty(ct + 1, 4), empty(cm, 8), empty(cm, 1))
            out.meta["cap"] = (ct, cm)
        if _itemsize(out.offsets) != 4 or _itemsize(out.keys) != 8 or _itemsize(out.acctype) != 1:
            raise TypeError(f"{what}: out holds u32 offsets, u64 keys and u8 access types")
        ct, cm = out.meta.get("cap", (int(out.offsets.shape[0]) - 1,
                                      min(int(out.keys.shape[0]), int(out.acctype.shape[0]))))
        per = {}
        for name, wide in (("ts", 8), ("rc", 1), ("pos", 4), ("src", 4)):
            a = out.meta.get(name)
            if a is None:
                a = out.meta[name] = empty(ct, wide)
            if _itemsize(a) != wide or a.shape[0] < ct:
                raise ValueError(f"{what}: out.meta[{name!r}] must hold cap_txn {wide}-byte items")
            per[name] = a
        so = _abi.SelectOut(ct, cm, 0, 0, _ptr(out.offsets), _ptr(out.keys), _ptr(out.acctype), None, None, None,
                            _ptr(per["src"]))
        b = batch.to_c()
        fb = fresh.to_c() if fresh is not None else None
        a = _abi.WaitdieCarryArgs(C.pointer(b), p_ts, p_rc, p_pos, p_rev, p_src,
                                  C.pointer(fb) if fb is not None else None, p_fts, int(fresh_src_base),
                                  C.pointer(so), _ptr(per["ts"]), _ptr(per["rc"]), _ptr(per["pos"]))
        st = _abi.Stats()
        nt, mt, nk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        code = lib.dcc_waitdie_carry(self._h, C.byref(a), C.byref(nt), C.byref(mt), C.byref(nk), C.byref(st))
        try:
            _check(code, self._h)
        except DccError as e:
            e.needed = (int(nt.value), int(mt.value), int(nk.value))
            raise
        tn, tm = int(nt.value), int(mt.value)
        got = EpochBatch(out.offsets[:tn + 1], out.keys[:tm], out.acctype[:tm], None, None, None,
                         {k: v[:tn] for k, v in per.items()})
        return got, per["ts"][:tn], per["rc"][:tn], per["pos"][:tn], per["src"][:tn], int(nk.value), st.as_dict()

    # ------------------------------------------------------------- MVCC
    def mvcc_validate_epoch(self, batch: EpochBatch, ts, want_conflict: bool = True, want_vts: bool = True,
                            out_rc=None, out_conflict=None, out_vts=None):
        """MVCC epoch (dcc_mvcc_validate_epoch): returns (rc u8[n], conflict
        u32[n] | None, vts u64[nnz] | None, stats).  ts as in
        tso_validate_epoch, every value in [1, 2^64-2].  vts[a] is the
        timestamp of the version access a read: VTS_BASE for the base row,
        VTS_NONE for an XP access or one that was not executed (a device batch
        gets an int64 tensor, read bit for bit).  Rows and versions persist in
        the context (mvcc_rows_get, mvcc_versions, mvcc_trim, mvcc_clear)."""
        n, nnz = batch.n_txn, batch.nnz
        dev = batch.on_device
        if ts is None:
            ts_ptr = None
        elif dev:
            if not _is_device(ts):
                raise TypeError("mvcc_validate_epoch: a device batch takes a device ts tensor")
            ts_ptr = _ptr(ts) if n else _ptr(batch.offsets)
        else:
            ts = np.ascontiguousarray(ts, np.uint64)
            ts_ptr = _ptr(ts) if n else _ptr(np.zeros(1, np.uint64))
        if ts is not None and (_itemsize(ts) != 8 or ts.shape[0] < n):
            raise ValueError("mvcc_validate_epoch: ts must hold n_txn 8-byte timestamps")
        if dev:
            import torch
            d = batch.offsets.device
            if out_rc is None:
                out_rc = torch.empty(max(n, 1), dtype=torch.uint8, device=d)
            if want_conflict and out_conflict is None:
                out_conflict = torch.empty(max(n, 1), dtype=torch.int32, device=d)
            if want_vts and out_vts is None:
                out_vts = torch.empty(max(nnz, 1), dtype=torch.int64, device=d)
        else:
            if out_rc is None:
                out_rc = np.empty(max(n, 1), np.uint8)
            if want_conflict and out_conflict is None:
                out_conflict = np.empty(max(n, 1), np.uint32)
            if want_vts and out_vts is None:
                out_vts = np.empty(max(nnz, 1), np.uint64)
        if not want_conflict:
            out_conflict = None
        if not want_vts:
            out_vts = None
        if out_rc.shape[0] < n or (out_conflict is not None and out_conflict.shape[0] < n) or \
                (out_vts is not None and (out_vts.shape[0] < nnz or _itemsize(out_vts) != 8)):
            raise ValueError("mvcc_validate_epoch: output buffer shorter than the epoch")
        st = _abi.Stats()
        b = batch.to_c()
        _check(lib.dcc_mvcc_validate_epoch(self._h, C.byref(b), ts_ptr, _ptr(out_rc), _ptr(out_conflict),
                                           _ptr(out_vts), C.byref(st)), self._h)
        return (out_rc[:n], (out_conflict[:n] if want_conflict else None),
                (out_vts[:nnz] if want_vts else None), st.as_dict())

    def mvcc_rows_get(self, keys):
        """(latest version u64[n], rts u64[n]) of the rows; (0, 0) for rows never seen."""
        return self._rows_get(lib.dcc_mvcc_rows_get, keys)

    @property
    def mvcc_rows_size(self) -> int:
        return int(lib.dcc_mvcc_rows_size(self._h))

    @property
    def mvcc_versions_size(self) -> int:
        return int(lib.dcc_mvcc_versions_size(self._h))

    def mvcc_versions(self):
        """Every version in the store: (keys u64[v], ts u64[v]) sorted by (key, ts)."""
        v = self.mvcc_versions_size
        keys = np.empty(v, np.uint64)
        ts = np.empty(v, np.uint64)
        got = C.c_uint64(0)
        _check(lib.dcc_mvcc_versions_export(self._h, _ptr(keys) if v else None, _ptr(ts) if v else None, v,
                                            C.byref(got)), self._h)
        return keys[:got.value], ts[:got.value]

    def mvcc_trim(self, ts_floor: int) -> int:
        """Row_mvcc::clear_history(W_REQ, ts_floor) of every row; returns the
        number of versions dropped."""
        dropped = C.c_uint64(0)
        _check(lib.dcc_mvcc_trim(self._h, int(ts_floor), C.byref(dropped)), self._h)
        return int(dropped.value)

    def mvcc_clear(self) -> None:
        _check(lib.dcc_mvcc_clear(self._h), self._h)

    # ------------------------------------------ MVCC with txns in flight
    def _mvcc_vts(self, what, batch, vts):
        """The caller-kept versions array of an MVCC call with txns in flight:
        nnz 8-byte items of the batch's kind, updated in place."""
        if vts is None:
            return None
        if batch.on_device:
            if not _is_device(vts) or not vts.is_contiguous():
                raise TypeError(f"{what}: a device batch takes a contiguous device vts tensor")
        elif not (isinstance(vts, np.ndarray) and vts.dtype == np.uint64 and vts.flags["C_CONTIGUOUS"] and
                  vts.flags["WRITEABLE"]):
            raise TypeError(f"{what}: vts is updated in place: a writable contiguous uint64 array")
        if _itemsize(vts) != 8 or vts.shape[0] < batch.nnz:
            raise ValueError(f"{what}: vts must hold nnz 8-byte items")
        return _ptr(vts) if vts.shape[0] else None

    def mvcc_access_epoch(self, batch: EpochBatch, ts, rc, pos, vts=None, want_conflict: bool = True):
        """MVCC epoch with txns in flight (dcc_mvcc_access_epoch): the WD_RUN
        txns send their requests from pos on against the pending prewrites of
        the state and the context's MVCC rows and versions.  rc, pos and vts
        (the version every executed read returned, kept by the caller across
        calls; None: not wanted) are updated in place.  Returns (rc[:n],
        pos[:n], conflict u32[n] | None, stats); conflict[i] is the ordinal of
        the access a txn waits or aborted at, ACCESS_NONE otherwise.  Arrays
        are numpy for a host batch, device tensors for a device batch."""
        n = batch.n_txn
        keep, ptrs = self._waitdie_state("mvcc_access_epoch", batch, ts, rc, pos)
        vp = self._mvcc_vts("mvcc_access_epoch", batch, vts)
        conf = None
        if want_conflict:
            if batch.on_device:
                import torch
                conf = torch.empty(max(n, 1), dtype=torch.int32, device=batch.offsets.device)
            else:
                conf = np.empty(max(n, 1), np.uint32)
        st = _abi.Stats()
        b = batch.to_c()
        _check(lib.dcc_mvcc_access_epoch(self._h, C.byref(b), *ptrs, vp, _ptr(conf), C.byref(st)), self._h)
        return rc[:n], pos[:n], (conf[:n] if want_conflict else None), st.as_dict()

    def mvcc_finish(self, batch: EpochBatch, ts, rc, pos, leave, vts=None):
        """dcc_mvcc_finish: the txns with leave[i] != 0 commit (RC_RCOK) or
        abort (RC_ABORT, WD_RUN) and become WD_GONE; buffered reads that no
        remaining prewrite blocks are promoted to (WD_RUN, pos + 1) and their
        version goes to vts.  rc, pos and vts are updated in place.  Returns
        (n_left, n_promoted, stats)."""
        keep, ptrs = self._waitdie_state("mvcc_finish", batch, ts, rc, pos, leave)
        vp = self._mvcc_vts("mvcc_finish", batch, vts)
        st = _abi.Stats()
        b = batch.to_c()
        left, prom = C.c_uint64(0), C.c_uint64(0)
        _check(lib.dcc_mvcc_finish(self._h, C.byref(b), *ptrs, vp, C.byref(left), C.byref(prom), C.byref(st)),
               self._h)
        return int(left.value), int(prom.value), st.as_dict()

    # ------------------------------------- TIMESTAMP with txns in flight
    def tso_access_epoch(self, batch: EpochBatch, ts, rc, pos, want_conflict: bool = True):
        """TIMESTAMP epoch with txns in flight (dcc_tso_access_epoch): the
        WD_RUN txns send their requests from pos on against the pending
        prewrites of the state and the context's TIMESTAMP rows (tso_rows_*).
        rc and pos are updated in place.  Returns (rc[:n], pos[:n], conflict
        u32[n] | None, stats); conflict[i] is the ordinal of the access a txn
        waits or aborted at, ACCESS_NONE otherwise.  Arrays are numpy for a
        host batch, device tensors for a device batch."""
        n = batch.n_txn
        keep, ptrs = self._waitdie_state("tso_access_epoch", batch, ts, rc, pos)
        conf = None
        if want_conflict:
            if batch.on_device:
                import torch
                conf = torch.empty(max(n, 1), dtype=torch.int32, device=batch.offsets.device)
            else:
                conf = np.empty(max(n, 1), np.uint32)
        st = _abi.Stats()
        b = batch.to_c()
        _check(lib.dcc_tso_access_epoch(self._h, C.byref(b), *ptrs, _ptr(conf), C.byref(st)), self._h)
        return rc[:n], pos[:n], (conf[:n] if want_conflict else None), st.as_dict()

    def tso_finish(self, batch: EpochBatch, ts, rc, pos, leave):
        """dcc_tso_finish: the txns with leave[i] != 0 commit (RC_RCOK: wts =
        max(wts, ts) per WR access) or abort (RC_ABORT, WD_RUN) and become
        WD_GONE; buffered reads that no remaining prewrite blocks are promoted
        to (WD_RUN, pos + 1) and raise rts.  rc and pos are updated in place.
        Returns (n_left, n_promoted, stats)."""
        keep, ptrs = self._waitdie_state("tso_finish", batch, ts, rc, pos, leave)
        st = _abi.Stats()
        b = batch.to_c()
        left, prom = C.c_uint64(0), C.c_uint64(0)
        _check(lib.dcc_tso_finish(self._h, C.byref(b), *ptrs, C.byref(left), C.byref(prom), C.byref(st)), self._h)
        return int(left.value), int(prom.value), st.as_dict()

    # ------------------------------------------- select by decision (carry)
    def select_batch(self, batch: EpochBatch, rc, want: int = _abi.RC_ABORT, src=None, out=None,
                     txn_base: int = 0, nnz_base: int = 0, want_src: bool = True):
        """The txns with rc[i] == want as a CSR, where the batch lives
        (dcc_batch_select): returns (EpochBatch, src u32[txn_base + n] | None,
        stats).  The selection goes to rows txn_base.. / accesses nnz_base.. of
        `out`, an EpochBatch of arrays with room for it (its source indices to
        out.meta["src"], allocated when absent); the returned batch is `out`
        cut to [: txn_base + n + 1] / [: nnz_base + nnz], so whatever lies in
        front of the bases is part of it.  out=None allocates room for the whole
        batch behind the bases, numpy or torch to match the batch.  src:
        u32[n_txn], the identities the selected txns carry instead of their
        index.  A selection that does not fit raises DccError(DCC_ERANGE) with
        the counts it needed in .needed."""
        n, m = batch.n_txn, batch.nnz
        dev = batch.on_device
        has_tn = batch.start_tn is not None
        if dev:
            import torch
            d = batch.offsets.device

            def empty(k, like, wide):
                dt = like.dtype if like is not None and like.element_size() == wide else \
                    {8: torch.int64, 4: torch.int32, 1: torch.uint8}[wide]
                return torch.empty(max(k, 1), dtype=dt, device=d)
        else:
            def empty(k, like, wide):
                return np.empty(max(k, 1), {8: np.uint64, 4: np.uint32, 1: np.uint8}[wide])
            rc = np.ascontiguousarray(rc, np.uint8)
            src = None if src is None else np.ascontiguousarray(src, np.uint32)
        if rc.shape[0] < n or (src is not None and src.shape[0] < n):
            raise ValueError("select_batch: rc / src shorter than the epoch")
        if out is None:
            out = EpochBatch(empty(txn_base + n + 1, batch.offsets, 4), empty(nnz_base + m, batch.keys, 8),
                             empty(nnz_base + m, None, 1),
                             empty(txn_base + n, batch.start_tn, 8) if has_tn else None,
                             empty(txn_base + n, batch.finish_tn, 8) if has_tn else None,
                             empty(txn_base + n, batch.order, 8) if batch.order is not None else None)
        if _itemsize(out.offsets) != 4 or _itemsize(out.keys) != 8 or _itemsize(out.acctype) != 1:
            raise TypeError("select_batch: out holds u32 offsets, u64 keys and u8 access types")
        for a in (out.start_tn, out.finish_tn, out.order):
            if a is not None and _itemsize(a) != 8:
                raise TypeError("select_batch: out timestamps / order are u64")
        cap_txn = int(out.offsets.shape[0]) - 1 - txn_base
        cap_nnz = min(int(out.keys.shape[0]), int(out.acctype.shape[0])) - nnz_base
        per_txn = [out.start_tn if has_tn else None, out.finish_tn if has_tn else None,
                   out.order if batch.order is not None else None]
        o_src = None
        if want_src:
            o_src = out.meta.get("src")
            if o_src is None:
                o_src = out.meta["src"] = empty(txn_base + max(cap_txn, 0), None, 4)
            per_txn.append(o_src)
        for a in per_txn:
            if a is not None:
                cap_txn = min(cap_txn, int(a.shape[0]) - txn_base)
        if cap_txn < 0 or cap_nnz < 0:
            raise ValueError("select_batch: out ends before the bases")
        so = _abi.SelectOut(cap_txn, cap_nnz, txn_base, nnz_base, _ptr(out.offsets), _ptr(out.keys),
                            _ptr(out.acctype), _ptr(per_txn[0]), _ptr(per_txn[1]), _ptr(per_txn[2]),
                            _ptr(o_src))
        st = _abi.Stats()
        b = batch.to_c()
        ns, ms = C.c_uint64(0), C.c_uint64(0)
        code = lib.dcc_batch_select(self._h, C.byref(b), _ptr(rc), want, _ptr(src), C.byref(so),
                                    C.byref(ns), C.byref(ms), C.byref(st))
        try:
            _check(code, self._h)
        except DccError as e:
            e.needed = (int(ns.value), int(ms.value))
            raise
        tn, tm = txn_base + int(ns.value), nnz_base + int(ms.value)
        cut = [None if a is None else a[:tn] for a in per_txn[:3]]
        sel = EpochBatch(out.offsets[:tn + 1], out.keys[:tm], out.acctype[:tm], cut[0], cut[1], cut[2],
                         {"src": o_src[:tn]} if want_src else {})
        return sel, (o_src[:tn] if want_src else None), st.as_dict()

    # ------------------------------------ abort queue (back-off of the retries)
    def abort_queue(self, cap_txn: int, cap_nnz: int, penalty: int, penalty_max: int,
                    policy: int = _abi.BACKOFF_REFERENCE, flags: int = 0) -> "AbortQueue":
        """A device-resident abort queue with room for cap_txn parked txns /
        cap_nnz accesses (dcc_abortq_create): AbortQueue::enqueue / process of
        system/abort_queue.cpp on the caller's clock."""
        return AbortQueue(self, cap_txn, cap_nnz, penalty, penalty_max, policy, flags)

    # ------------------------------ NO_WAIT lock table that lives across epochs
    def locktab(self, cap_rows: int) -> "LockTable":
        """A device-resident NO_WAIT lock table with room for cap_rows rows
        (dcc_locktab_create): Row_lock's lock_type / owner_cnt across epochs."""
        return LockTable(self, cap_rows)

    def held_from(self, batch: EpochBatch, rc):
        """The requests of the txns that committed (rc == RC_RCOK) as (keys,
        acctype): the held prefix that nowait_lock_epoch(held=...) and
        calvin_order_epoch_held take for the next epoch."""
        sel, _, _ = self.select_batch(batch, rc, want=_abi.RC_RCOK, want_src=False)
        return sel.keys, sel.acctype

    def calvin_dispatch(self, wave, order=None):
        """Wave dispatch lists (dcc_calvin_dispatch): returns (wave_off u32[W+1],
        txn u32[n]) — txn[wave_off[w]:wave_off[w+1]] run in wave w."""
        dev = hasattr(wave, "device") and str(wave.device).startswith("cuda")
        n = int(wave.shape[0])
        nw = C.c_uint32(0)
        if dev:
            import torch
            txn = torch.empty(max(n, 1), dtype=torch.int32, device=wave.device)
            _check(lib.dcc_calvin_dispatch(self._h, _ptr(wave), _ptr(order), n, _abi.DEVICE_PTRS,
                                           None, 0, _ptr(txn), C.byref(nw)), self._h)
            off = torch.empty(nw.value + 1, dtype=torch.int32, device=wave.device)
            _check(lib.dcc_calvin_dispatch(self._h, _ptr(wave), _ptr(order), n, _abi.DEVICE_PTRS,
                                           _ptr(off), nw.value + 1, _ptr(txn), C.byref(nw)),
                   self._h)
            return off, txn[:n]
        wave = np.ascontiguousarray(wave, np.uint32)
        order = None if order is None else np.ascontiguousarray(order, np.uint64)
        txn = np.empty(max(n, 1), np.uint32)
        _check(lib.dcc_calvin_dispatch(self._h, _ptr(wave), _ptr(order), n, 0, None, 0,
                                       _ptr(txn), C.byref(nw)), self._h)
        off = np.empty(nw.value + 1, np.uint32)
        _check(lib.dcc_calvin_dispatch(self._h, _ptr(wave), _ptr(order), n, 0, _ptr(off),
                                       off.size, _ptr(txn), C.byref(nw)), self._h)
        return off, txn[:n]

    # ----------------------------------------------------------- GPU index
    def index_insert(self, keys, rows) -> None:
        keys = np.ascontiguousarray(keys, np.uint64)
        rows = np.ascontiguousarray(rows, np.uint64)
        _check(lib.dcc_index_insert(self._h, _ptr(keys), _ptr(rows), keys.shape[0]), self._h)

    def index_probe(self, keys):
        """Rows of keys (DCC_ROW_NONE when absent) and the missing count."""
        miss = C.c_uint64(0)
        if hasattr(keys, "device") and str(keys.device).startswith("cuda"):
            import torch
            out = torch.empty(keys.shape[0], dtype=torch.int64, device=keys.device)
            _check(lib.dcc_index_probe(self._h, _ptr(keys), keys.shape[0], _ptr(out),
                                       _abi.DEVICE_PTRS, C.byref(miss)), self._h)
            return out, miss.value
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.empty(keys.shape[0], np.uint64)
        _check(lib.dcc_index_probe(self._h, _ptr(keys), keys.shape[0], _ptr(out), 0, C.byref(miss)),
               self._h)
        return out, miss.value

    def index_clear(self) -> None:
        _check(lib.dcc_index_clear(self._h), self._h)

    @property
    def index_size(self) -> int:
        return int(lib.dcc_index_size(self._h))

    @property
    def index_last_ms(self) -> float:
        return float(lib.dcc_index_last_ms(self._h))

    # ------------------------------------------------------------ multi-GPU
    def comm_init(self, rank: int, nranks: int, unique_id: bytes) -> None:
        buf = C.create_string_buffer(bytes(unique_id), _abi.UNIQUE_ID_BYTES)
        _check(lib.dcc_comm_init(self._h, rank, nranks, buf), self._h)

    def comm_init_host(self, rank: int, nranks: int, allreduce_max) -> None:
        """Shard this engine with a host-side exchange: ``allreduce_max(buf)``
        must MAX-all-reduce the uint8 numpy array ``buf`` in place across the
        ranks (e.g. torch.distributed over gloo)."""
        def _cb(user, ptr, n):
            try:
                if n:
                    allreduce_max(np.ctypeslib.as_array(ptr, shape=(int(n),)))
                return 0
            except Exception:  # noqa: BLE001 - reported as DCC_ECOMM by the engine
                import traceback
                traceback.print_exc()
                return 1
        self._exchange = _abi.EXCHANGE_FN(_cb)  # keep alive as long as the engine
        _check(lib.dcc_comm_init_host(self._h, rank, nranks,
                                      C.cast(self._exchange, C.c_void_p), None), self._h)

    @property
    def comm_rank(self) -> int:
        return int(lib.dcc_comm_rank(self._h))

    @property
    def comm_size(self) -> int:
        return int(lib.dcc_comm_size(self._h))

    @property
    def comm_calls(self) -> int:
        """Collectives run by this engine's communicator (dcc_comm_calls)."""
        return int(lib.dcc_comm_calls(self._h))

    def comm_destroy(self) -> None:
        _check(lib.dcc_comm_destroy(self._h), self._h)


class AbortQueue:
    """dcc_abortq: parked aborted txns in device memory (Engine.abort_queue)."""

    def __init__(self, eng: "Engine", cap_txn: int, cap_nnz: int, penalty: int, penalty_max: int,
                 policy: int, flags: int = 0):
        self._eng = eng
        self._q = None
        self.cap_txn, self.cap_nnz = int(cap_txn), int(cap_nnz)
        p = _abi.AbortqParams(cap_txn, cap_nnz, penalty, penalty_max, policy, flags)
        h = C.c_void_p()
        _check(lib.dcc_abortq_create(eng._h, C.byref(p), C.byref(h)), eng._h)
        self._q = h
        eng._queues.append(self)

    def close(self) -> None:
        if self._q is not None:
            lib.dcc_abortq_destroy(self._q)
            self._q = None
            if self in self._eng._queues:
                self._eng._queues.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if self._q is None:
            raise ValueError("abort queue is closed")
        return self._q

    def push(self, batch: EpochBatch, rc, now: int, want: int = _abi.RC_ABORT, src=None, cnt=None):
        """Park the txns with rc[i] == want at clock `now` (dcc_abortq_push):
        returns (n, nnz, stats) of what was parked.  src / cnt: u32[n_txn], the
        identities and abort counts the txns carry (their index / 0 when
        None).  No room raises DccError(DCC_ERANGE) with .needed."""
        n = batch.n_txn
        if not batch.on_device:
            rc = np.ascontiguousarray(rc, np.uint8)
            src = None if src is None else np.ascontiguousarray(src, np.uint32)
            cnt = None if cnt is None else np.ascontiguousarray(cnt, np.uint32)
        for a in (rc, src, cnt):
            if a is not None and a.shape[0] < n:
                raise ValueError("push: rc / src / cnt shorter than the epoch")
        for a in (src, cnt):
            if a is not None and _itemsize(a) != 4:
                raise TypeError("push: src / cnt are u32")
        st = _abi.Stats()
        b = batch.to_c()
        ns, ms = C.c_uint64(0), C.c_uint64(0)
        code = lib.dcc_abortq_push(self._handle(), C.byref(b), _ptr(rc), want, _ptr(src), _ptr(cnt), now,
                                   C.byref(ns), C.byref(ms), C.byref(st))
        try:
            _check(code, self._eng._h)
        except DccError as e:
            e.needed = (int(ns.value), int(ms.value))
            raise
        return int(ns.value), int(ms.value), st.as_dict()

    def pop(self, now: int, out=None, txn_base: int = 0, nnz_base: int = 0, device=None,
            want_cnt: bool = True, want_due: bool = True):
        """Release the entries with due < now, in (due, push) order, to rows
        txn_base.. / accesses nnz_base.. of `out` (dcc_abortq_pop): returns
        (EpochBatch, stats).  The batch is `out` cut to the bases plus the
        counts; its meta carries "src", "cnt" and "due" (taken from out.meta,
        allocated when absent; cnt / due are left out with want_cnt / want_due
        False).  out=None allocates room for the whole queue behind the bases:
        torch on `device` when given, numpy otherwise.  A release that does not
        fit raises DccError(DCC_ERANGE) with .needed."""
        qn, qm = self.size()
        if out is not None:
            dev = out.on_device
            tdev = out.offsets.device if dev else None
        else:
            dev = device is not None
            tdev = device
        if dev:
            import torch

            def empty(k, wide):
                return torch.empty(max(k, 1), dtype={8: torch.int64, 4: torch.int32, 1: torch.uint8}[wide],
                                   device=tdev)
        else:
            def empty(k, wide):
                return np.empty(max(k, 1), {8: np.uint64, 4: np.uint32, 1: np.uint8}[wide])
        if out is None:
            out = EpochBatch(empty(txn_base + qn + 1, 4), empty(nnz_base + qm, 8), empty(nnz_base + qm, 1))
        if _itemsize(out.offsets) != 4 or _itemsize(out.keys) != 8 or _itemsize(out.acctype) != 1:
            raise TypeError("pop: out holds u32 offsets, u64 keys and u8 access types")
        cap_txn = int(out.offsets.shape[0]) - 1 - txn_base
        cap_nnz = min(int(out.keys.shape[0]), int(out.acctype.shape[0])) - nnz_base
        per = {}
        for name, wide, on in (("src", 4, True), ("cnt", 4, want_cnt), ("due", 8, want_due)):
            if not on:
                per[name] = None
                continue
            a = out.meta.get(name)
            if a is None:
                a = out.meta[name] = empty(txn_base + max(cap_txn, 0), wide)
            if _itemsize(a) != wide:
                raise TypeError(f"pop: out.meta[{name!r}] has the wrong item size")
            per[name] = a
            cap_txn = min(cap_txn, int(a.shape[0]) - txn_base)
        if cap_txn < 0 or cap_nnz < 0:
            raise ValueError("pop: out ends before the bases")
        so = _abi.SelectOut(cap_txn, cap_nnz, txn_base, nnz_base, _ptr(out.offsets), _ptr(out.keys),
                            _ptr(out.acctype), None, None, None, _ptr(per["src"]))
        st = _abi.Stats()
        ns, ms = C.c_uint64(0), C.c_uint64(0)
        code = lib.dcc_abortq_pop(self._handle(), now, C.byref(so), _ptr(per["cnt"]), _ptr(per["due"]),
                                  _abi.DEVICE_PTRS if dev else 0, C.byref(ns), C.byref(ms), C.byref(st))
        try:
            _check(code, self._eng._h)
        except DccError as e:
            e.needed = (int(ns.value), int(ms.value))
            raise
        tn, tm = txn_base + int(ns.value), nnz_base + int(ms.value)
        meta = {k: v[:tn] for k, v in per.items() if v is not None}
        return EpochBatch(out.offsets[:tn + 1], out.keys[:tm], out.acctype[:tm], None, None, None, meta), \
            st.as_dict()

    def size(self):
        """(parked txns, parked accesses): host state, no device work."""
        n, m = C.c_uint64(0), C.c_uint64(0)
        _check(lib.dcc_abortq_size(self._handle(), C.byref(n), C.byref(m)), self._eng._h)
        return int(n.value), int(m.value)

    def clear(self) -> None:
        _check(lib.dcc_abortq_clear(self._handle()), self._eng._h)


class LockTable:
    """dcc_locktab: the NO_WAIT lock state in device memory, acquired into by
    epochs and released from by finished txns (Engine.locktab)."""

    def __init__(self, eng: "Engine", cap_rows: int):
        self._eng = eng
        self._q = None
        self.cap_rows = int(cap_rows)
        p = _abi.LocktabParams(cap_rows, 0, 0)
        h = C.c_void_p()
        _check(lib.dcc_locktab_create(eng._h, C.byref(p), C.byref(h)), eng._h)
        self._q = h
        eng._queues.append(self)

    def close(self) -> None:
        if self._q is not None:
            lib.dcc_locktab_destroy(self._q)
            self._q = None
            if self in self._eng._queues:
                self._eng._queues.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if self._q is None:
            raise ValueError("lock table is closed")
        return self._q

    def lock_epoch(self, batch: EpochBatch, want_conflict: bool = True, out_rc=None, out_conflict=None,
                   isolation: int = _abi.ISO_SERIALIZABLE):
        """The epoch against the table's rows; the requests of its committed
        txns stay in the table (dcc_locktab_lock_epoch).  Returns (rc u8[n],
        conflict u32[n] | None, stats) as Engine.nowait_lock_epoch.  isolation:
        at ISO_READ_COMMITTED only the EX requests of the committed txns stay,
        at ISO_READ_UNCOMMITTED none."""
        n = batch.n_txn
        if batch.on_device:
            import torch
            dv = batch.offsets.device
            if out_rc is None:
                out_rc = torch.empty(max(n, 1), dtype=torch.uint8, device=dv)
            if want_conflict and out_conflict is None:
                out_conflict = torch.empty(max(n, 1), dtype=torch.int32, device=dv)
        else:
            if out_rc is None:
                out_rc = np.empty(max(n, 1), np.uint8)
            if want_conflict and out_conflict is None:
                out_conflict = np.empty(max(n, 1), np.uint32)
        if not want_conflict:
            out_conflict = None
        if out_rc.shape[0] < n or (out_conflict is not None and out_conflict.shape[0] < n):
            raise ValueError("lock_epoch: output buffer shorter than the epoch")
        st = _abi.Stats()
        b = batch.to_c(int(isolation))
        _check(lib.dcc_locktab_lock_epoch(self._handle(), C.byref(b), _ptr(out_rc), _ptr(out_conflict),
                                          C.byref(st)), self._eng._h)
        return out_rc[:n], (out_conflict[:n] if want_conflict else None), st.as_dict()

    def release(self, batch: EpochBatch, rc=None, want: int = _abi.RC_RCOK,
                isolation: int = _abi.ISO_SERIALIZABLE):
        """lock_release for every access of the txns with rc[i] == want (rc
        None: of every txn) (dcc_locktab_release): returns (n, nnz, stats) of
        what was released.  A row released more often than it is held raises
        DccError(DCC_EINVAL) and leaves the table unchanged.  isolation: the
        level the txns ran at: ISO_READ_COMMITTED releases their EX accesses
        only, ISO_READ_UNCOMMITTED nothing."""
        if rc is not None:
            if not batch.on_device:
                rc = np.ascontiguousarray(rc, np.uint8)
            if rc.shape[0] < batch.n_txn:
                raise ValueError("release: rc shorter than the epoch")
        st = _abi.Stats()
        b = batch.to_c(int(isolation))
        ns, ms = C.c_uint64(0), C.c_uint64(0)
        _check(lib.dcc_locktab_release(self._handle(), C.byref(b), _ptr(rc), want, C.byref(ns), C.byref(ms),
                                       C.byref(st)), self._eng._h)
        return int(ns.value), int(ms.value), st.as_dict()

    def acquire_rows(self, keys, acctype) -> None:
        """Take a plain (key, access type) list as a held prefix is taken: a
        row is EX if any of its entries is EX, its count goes up by one per
        entry (dcc_locktab_acquire_rows)."""
        dev = _is_device(keys)
        if not dev:
            keys = np.ascontiguousarray(keys, np.uint64)
            acctype = np.ascontiguousarray(acctype, np.uint8)
        if int(acctype.shape[0]) != int(keys.shape[0]) or _itemsize(keys) != 8 or _itemsize(acctype) != 1:
            raise ValueError("acquire_rows: u64 keys and u8 access types of one length")
        h = _abi.CalvinHeld(int(keys.shape[0]), _ptr(keys), _ptr(acctype))
        _check(lib.dcc_locktab_acquire_rows(self._handle(), C.byref(h), _abi.DEVICE_PTRS if dev else 0),
               self._eng._h)

    def release_rows(self, keys) -> None:
        """lock_release once per entry of a plain key list (dcc_locktab_release_rows)."""
        dev = _is_device(keys)
        if not dev:
            keys = np.ascontiguousarray(keys, np.uint64)
        if _itemsize(keys) != 8:
            raise TypeError("release_rows: u64 keys")
        _check(lib.dcc_locktab_release_rows(self._handle(), _ptr(keys), int(keys.shape[0]),
                                            _abi.DEVICE_PTRS if dev else 0), self._eng._h)

    def export(self, device=None):
        """(keys u64, lock_type u8, owner_cnt u32) of the rows with owner_cnt >
        0, in any order (dcc_locktab_export); lock_type is LOCK_EX / LOCK_SH.
        numpy arrays, or torch tensors on `device` when given."""
        rows = self.size()[0]
        n = C.c_uint64(0)
        if device is not None:
            import torch
            k = torch.empty(max(rows, 1), dtype=torch.int64, device=device)
            t = torch.empty(max(rows, 1), dtype=torch.uint8, device=device)
            c = torch.empty(max(rows, 1), dtype=torch.int32, device=device)
        else:
            k, t, c = np.empty(max(rows, 1), np.uint64), np.empty(max(rows, 1), np.uint8), \
                np.empty(max(rows, 1), np.uint32)
        _check(lib.dcc_locktab_export(self._handle(), _ptr(k), _ptr(t), _ptr(c), rows,
                                      _abi.DEVICE_PTRS if device is not None else 0, C.byref(n)), self._eng._h)
        m = int(n.value)
        return k[:m], t[:m], c[:m]

    def size(self):
        """(rows held, slots in use, rebuilds): host state, no device work."""
        r, s, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib.dcc_locktab_size(self._handle(), C.byref(r), C.byref(s), C.byref(b)), self._eng._h)
        return int(r.value), int(s.value), int(b.value)

    def pass_ms(self):
        """{"seed", "grant", "rebuild"}: device ms of the table's own passes in
        the last profiled lock epoch or acquire (dcc_locktab_pass_ms)."""
        out = (C.c_double * 3)()
        _check(lib.dcc_locktab_pass_ms(self._handle(), out), self._eng._h)
        return {"seed": out[0], "grant": out[1], "rebuild": out[2]}

    def clear(self) -> None:
        _check(lib.dcc_locktab_clear(self._handle()), self._eng._h)


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(_abi.UNIQUE_ID_BYTES)
    _check(lib.dcc_comm_unique_id(buf))
    return buf.raw


def key_shard(key: int, nranks: int) -> int:
    return int(lib.dcc_key_shard(key, nranks))


def shard_of_keys(keys, nranks: int) -> np.ndarray:
    """dcc_key_shard of every key (u32 array)."""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.empty(max(k.size, 1), np.uint32)
    _check(lib.dcc_key_shard_n(_ptr(k), k.size, nranks, _ptr(out)))
    return out[: k.size]


def shard_filter(batch: EpochBatch, rank: int, nranks: int) -> EpochBatch:
    n, nnz = batch.n_txn, batch.nnz
    off = np.empty(n + 1, np.uint32)
    keys = np.empty(max(nnz, 1), np.uint64)
    at = np.empty(max(nnz, 1), np.uint8)
    out = C.c_uint64()
    b = batch.to_c()
    _check(lib.dcc_shard_filter(C.byref(b), rank, nranks, _ptr(off), _ptr(keys), _ptr(at),
                                C.byref(out)))
    w = out.value
    return EpochBatch(off, keys[:w].copy(), at[:w].copy(), batch.start_tn, batch.finish_tn,
                      batch.order, dict(batch.meta, shard=(rank, nranks)))


def alg_bytes(n_txn: int, nnz: int, nnz_w: int) -> int:
    return int(lib.dcc_alg_bytes(n_txn, nnz, nnz_w))


def calvin_alg_bytes(n_txn: int, nnz: int, with_order: bool, with_wave: bool) -> int:
    return int(lib.dcc_calvin_alg_bytes(n_txn, nnz, int(with_order), int(with_wave)))


def nowait_alg_bytes(n_txn: int, nnz: int, with_conflict: bool = True) -> int:
    return int(lib.dcc_nowait_alg_bytes(n_txn, nnz, int(with_conflict)))


def nowait_iso_alg_bytes(n_txn: int, nnz: int, held_n: int = 0, with_conflict: bool = True,
                         isolation: int = _abi.ISO_SERIALIZABLE) -> int:
    return int(lib.dcc_nowait_iso_alg_bytes(n_txn, nnz, held_n, int(with_conflict), int(isolation)))


def tso_alg_bytes(n_txn: int, nnz: int, with_conflict: bool = True) -> int:
    return int(lib.dcc_tso_alg_bytes(n_txn, nnz, int(with_conflict)))


def waitdie_alg_bytes(n_txn: int, nnz: int, with_conflict: bool = True) -> int:
    return int(lib.dcc_waitdie_alg_bytes(n_txn, nnz, int(with_conflict)))


def waitdie_carry_alg_bytes(n_txn: int, n_kept: int, nnz_kept: int, n_fresh: int = 0, nnz_fresh: int = 0,
                            with_revive: bool = False, with_src: bool = True) -> int:
    return int(lib.dcc_waitdie_carry_alg_bytes(n_txn, n_kept, nnz_kept, n_fresh, nnz_fresh, int(with_revive),
                                               int(with_src)))


def tso_access_alg_bytes(n_txn: int, nnz: int, with_conflict: bool = True) -> int:
    return int(lib.dcc_tso_access_alg_bytes(n_txn, nnz, int(with_conflict)))


def mvcc_access_alg_bytes(n_txn: int, nnz: int, with_conflict: bool = True, with_vts: bool = True) -> int:
    return int(lib.dcc_mvcc_access_alg_bytes(n_txn, nnz, int(with_conflict), int(with_vts)))


def mvcc_alg_bytes(n_txn: int, nnz: int, with_conflict: bool = True, with_vts: bool = True) -> int:
    return int(lib.dcc_mvcc_alg_bytes(n_txn, nnz, int(with_conflict), int(with_vts)))


def select_alg_bytes(n_txn: int, n_sel: int, nnz_sel: int, n_txn_arrays: int = 0) -> int:
    return int(lib.dcc_select_alg_bytes(n_txn, n_sel, nnz_sel, n_txn_arrays))


# ---------------------------------------------------------------- producers
def abortq_push_alg_bytes(n_txn: int, n_sel: int, nnz_sel: int) -> int:
    return int(lib.dcc_abortq_push_alg_bytes(n_txn, n_sel, nnz_sel))


def abortq_pop_alg_bytes(n_q: int, nnz_q: int, n_due: int, nnz_due: int) -> int:
    return int(lib.dcc_abortq_pop_alg_bytes(n_q, nnz_q, n_due, nnz_due))


def locktab_epoch_alg_bytes(n_txn: int, nnz: int, nnz_granted: int, with_conflict: bool = True) -> int:
    return int(lib.dcc_locktab_epoch_alg_bytes(n_txn, nnz, nnz_granted, int(with_conflict)))


def locktab_release_alg_bytes(n_txn: int, n_sel: int, nnz_sel: int) -> int:
    return int(lib.dcc_locktab_release_alg_bytes(n_txn, n_sel, nnz_sel))


def ycsb_params(**kw) -> _abi.YcsbParams:
    p = _abi.YcsbParams()
    lib.dcc_ycsb_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown YCSB parameter {k!r}")
        setattr(p, k, v)
    return p


def gen_ycsb(want_home: bool = False, **kw) -> EpochBatch:
    """Deterministic YCSB batch (gen_requests_zipf, ycsb_query.cpp:303-376)."""
    p = ycsb_params(**kw)
    n, k = p.n_txn, p.req_per_query
    off = np.empty(n + 1, np.uint32)
    keys = np.empty(max(n * k, 1), np.uint64)
    at = np.empty(max(n * k, 1), np.uint8)
    home = np.empty(max(n, 1), np.uint32) if want_home else None
    _check(lib.dcc_gen_ycsb(C.byref(p), _ptr(off), _ptr(keys), _ptr(at), _ptr(home)))
    meta = {"workload": "ycsb", **{f: getattr(p, f) for f, _ in p._fields_ if f != "reserved"}}
    b = EpochBatch(off, keys[: n * k], at[: n * k], meta=meta)
    if want_home:
        b.meta["home"] = home[:n]
    return b


def tpcc_params(**kw) -> _abi.TpccParams:
    p = _abi.TpccParams()
    lib.dcc_tpcc_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown TPC-C parameter {k!r}")
        setattr(p, k, v)
    return p


def gen_tpcc(**kw) -> EpochBatch:
    """Deterministic TPC-C NewOrder/Payment batch (tpcc_query.cpp:149-263)."""
    p = tpcc_params(**kw)
    n = p.n_txn
    cap = n * lib.dcc_tpcc_max_access(C.byref(p))
    off = np.empty(n + 1, np.uint32)
    keys = np.empty(max(cap, 1), np.uint64)
    at = np.empty(max(cap, 1), np.uint8)
    tt = np.empty(max(n, 1), np.uint8)
    out = C.c_uint64()
    _check(lib.dcc_gen_tpcc(C.byref(p), _ptr(off), _ptr(keys), _ptr(at), _ptr(tt), C.byref(out)))
    w = out.value
    meta = {"workload": "tpcc", "txn_type": tt[:n].copy(),
            **{f: getattr(p, f) for f, _ in p._fields_ if f != "reserved"}}
    return EpochBatch(off, keys[:w].copy(), at[:w].copy(), meta=meta)


# ---------------------------------------------------------------- batch files
def write_batch_file(path: str, batch: EpochBatch, kind: int = _abi.FILE_OCC, rc=None,
                     commit_tn=None, group=None, wave=None, seed: int = 0, epoch: int = 0,
                     tnc_before: int = 0) -> None:
    """One epoch (and optionally its decisions) as a .dccb file (dcc_file_write)."""
    info = _abi.FileInfo(kind=kind, seed=seed, epoch=epoch, tnc_before=tnc_before)

    def c(a, dt):
        return None if a is None else np.ascontiguousarray(a, dt)
    at = np.asarray(batch.acctype)
    if batch.meta.get("acctype_2bit"):  # the compact transfer form: unpack to one byte per access
        nnz = int(np.asarray(batch.keys).shape[0])
        at = ((np.repeat(at.astype(np.uint8), 4) >> np.tile(np.array([0, 2, 4, 6], np.uint8), at.size)) & 3)[:nnz]
    host = EpochBatch(c(batch.offsets, np.uint32), c(batch.keys, np.uint64),
                      c(at, np.uint8), c(batch.start_tn, np.uint64),
                      c(batch.finish_tn, np.uint64), c(batch.order, np.uint64))
    arrs = [c(rc, np.uint8), c(commit_tn, np.uint64), c(group, np.uint32), c(wave, np.uint32)]
    b = host.to_c()
    _check(lib.dcc_file_write(path.encode(), C.byref(info), C.byref(b),
                              *[_ptr(a) for a in arrs]))


def read_batch_file(path: str):
    """Returns (EpochBatch, info dict, decisions dict) of a .dccb file."""
    info = _abi.FileInfo()
    _check(lib.dcc_file_read_info(path.encode(), C.byref(info)))
    n, nnz, sec = info.n_txn, info.nnz, info.sections
    off = np.empty(n + 1, np.uint32)
    keys = np.empty(max(nnz, 1), np.uint64)
    at = np.empty(max(nnz, 1), np.uint8)
    has = lambda bit: bool(sec & bit)  # noqa: E731
    st = np.empty(max(n, 1), np.uint64) if has(_abi.FILE_HAS_TN) else None
    ft = np.empty(max(n, 1), np.uint64) if has(_abi.FILE_HAS_TN) else None
    od = np.empty(max(n, 1), np.uint64) if has(_abi.FILE_HAS_ORDER) else None
    rc = np.empty(max(n, 1), np.uint8) if has(_abi.FILE_HAS_RC) else None
    tn = np.empty(max(n, 1), np.uint64) if has(_abi.FILE_HAS_COMMIT_TN) else None
    gr = np.empty(max(nnz, 1), np.uint32) if has(_abi.FILE_HAS_GROUP) else None
    wv = np.empty(max(n, 1), np.uint32) if has(_abi.FILE_HAS_WAVE) else None
    _check(lib.dcc_file_read(path.encode(), *[_ptr(a) for a in (off, keys, at, st, ft, od, rc,
                                                                   tn, gr, wv)]))
    cut = lambda a, k: None if a is None else a[:k]  # noqa: E731
    b = EpochBatch(off, keys[:nnz], at[:nnz], cut(st, n), cut(ft, n), cut(od, n))
    meta = {f: getattr(info, f) for f, _ in info._fields_ if f != "reserved"}
    dec = {"rc": cut(rc, n), "commit_tn": cut(tn, n), "group": cut(gr, nnz), "wave": cut(wv, n)}
    return b, meta, dec
