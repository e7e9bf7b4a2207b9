"""dcc_waitdie_carry restated in numpy as a pure function, and the history the
invariance tests run: a WAIT_DIE population carried over epochs next to the
same population never compacted.

carry() raises ValueError where the call returns DCC_EINVAL and CarryRange
(with the counts needed) where it returns DCC_ERANGE."""
import functools

import numpy as np

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RC_WAIT, WD_GONE, WD_RUN

STATES = (WD_RUN, RC_RCOK, RC_WAIT, RC_ABORT, WD_GONE)


class CarryRange(Exception):
    def __init__(self, n, nnz, kept):
        super().__init__(f"needs {n} txns / {nnz} accesses ({kept} stayers)")
        self.needed = (n, nnz, kept)


def _csr(b, what):
    off = np.asarray(b.offsets).astype(np.int64)
    keys = np.asarray(b.keys).astype(np.uint64)
    at = np.asarray(b.acctype).astype(np.uint8)
    n = off.size - 1
    if n and (off[0] != 0 or off[n] != keys.size or np.any(np.diff(off) < 0)):
        raise ValueError(f"{what}: malformed offsets")
    return off, keys, at, n


def carry(batch, ts, rc, pos, revive=None, src_in=None, fresh=None, fresh_ts=None, fresh_src_base=0,
          cap_txn=None, cap_nnz=None):
    """Returns a dict: offsets u32, keys u64, acctype u8, ts u64, rc u8, pos u32,
    src u32, kept.  The inputs are wide host arrays and are not written."""
    if batch is None or ts is None or rc is None or pos is None:
        raise ValueError("null batch / ts / rc / pos")
    if fresh is not None and fresh_ts is None:
        raise ValueError("fresh without fresh_ts")
    off, keys, at, n = _csr(batch, "batch")
    ts = np.asarray(ts, np.uint64)[:n]
    rc = np.asarray(rc, np.uint8)[:n]
    pos = np.asarray(pos, np.uint32)[:n]
    if min(ts.size, rc.size, pos.size) < n:
        raise ValueError("ts / rc / pos shorter than the population")
    rev = np.zeros(n, bool) if revive is None else np.asarray(revive)[:n] != 0
    src = np.arange(n, dtype=np.uint32) if src_in is None else np.asarray(src_in, np.uint32)[:n]
    if fresh is not None:
        foff, fkeys, fat, nf = _csr(fresh, "fresh")
        fts = np.asarray(fresh_ts, np.uint64)[:nf]
        if fts.size < nf:
            raise ValueError("fresh_ts shorter than the fresh batch")
    else:
        foff, fkeys, fat, nf = np.zeros(1, np.int64), np.zeros(0, np.uint64), np.zeros(0, np.uint8), 0
        fts = np.zeros(0, np.uint64)
    lens = np.diff(off)
    if np.any(~np.isin(rc, STATES)):
        raise ValueError("an rc byte outside the five states")
    live = rc != WD_GONE
    if np.any(live & ((pos > lens) | ((rc == RC_RCOK) & (pos != lens)) | ((rc == RC_WAIT) & (pos >= lens)))):
        raise ValueError("pos does not fit its txn's state")
    if np.any(live & rev):
        raise ValueError("revive set on a txn that is not GONE")
    stay = np.nonzero(live | rev)[0]
    kept = int(stay.size)
    kl = lens[stay]
    nnz_kept = int(kl.sum())
    n_out, nnz_out = kept + nf, nnz_kept + int(fkeys.size)
    if ((cap_txn is not None and n_out > cap_txn) or (cap_nnz is not None and nnz_out > cap_nnz) or
            nnz_out > 0xFFFFFFFF):
        raise CarryRange(n_out, nnz_out, kept)
    # the stayers' accesses: for each, its index in the source
    idx = (np.repeat(off[stay] - np.concatenate([[0], np.cumsum(kl)[:-1]]), kl) + np.arange(nnz_kept)
           if kept else np.zeros(0, np.int64)).astype(np.int64)
    o_off = np.concatenate([[0], np.cumsum(kl), nnz_kept + foff[1:]]).astype(np.uint32)
    revived = ~live[stay]
    return {
        "offsets": o_off,
        "keys": np.concatenate([keys[idx], fkeys]),
        "acctype": np.concatenate([at[idx], fat]),
        "ts": np.concatenate([ts[stay], fts]),
        "rc": np.concatenate([np.where(revived, WD_RUN, rc[stay]), np.full(nf, WD_RUN)]).astype(np.uint8),
        "pos": np.concatenate([np.where(revived, 0, pos[stay]), np.zeros(nf)]).astype(np.uint32),
        "src": np.concatenate([src[stay], (fresh_src_base + np.arange(nf)) & 0xFFFFFFFF]).astype(np.uint32),
        "kept": kept,
        "revived": int(revived.sum()),
    }


def as_batch(c):
    return d.EpochBatch(c["offsets"], c["keys"], c["acctype"])


def append(b, f):
    """The never-compacted population: f's txns behind b's."""
    return d.EpochBatch(np.concatenate([b.offsets, f.offsets[1:] + b.offsets[-1]]).astype(np.uint32),
                        np.concatenate([b.keys, f.keys]), np.concatenate([b.acctype, f.acctype]))


def alg_bytes(n_txn, n_kept, nnz_kept, n_fresh, nnz_fresh, with_revive, with_src):
    """The table of include/dcc.h."""
    return (4 * (n_txn + 1) + n_txn * (1 + int(bool(with_revive))) + 25 * n_kept + 18 * nnz_kept +
            4 * (n_fresh + 1) + 8 * n_fresh + 13 * n_fresh + 18 * nnz_fresh + 4 * (n_kept + n_fresh + 1) +
            (8 * n_kept + 4 * n_fresh if with_src else 0))


@functools.lru_cache(maxsize=None)
def carry_history(family, n0=600, n_fresh=200, epochs=6, max_len=6, n_keys=48, seed=7):
    """The loop epoch -> release of every RCOK and ABORT txn -> next population
    (the died txns revived at once, n_fresh arrivals), on the population U that
    is never compacted, by waitdie_ref's replays.  U's txn index is the src of
    every txn.  Returns (start, steps): start = (batch, ts) of the first
    population, steps a list of dicts per epoch:
      epoch     (rc, pos, conflict, stats) of U after the epoch
      leave     the release's leavers (over U)
      release   (rc, pos, n_left, n_promoted) of U after it
      revive    the txns revived (over U)
      fresh, fresh_ts, fresh_src_base   the arrivals
      batch, ts, rc, pos                U after the carry
    Computed once per family; nothing in it may be written."""
    from waitdie_cases import hot_batch, make_ts
    from waitdie_ref import replay_epoch, replay_release
    rng = np.random.default_rng(seed)
    b = hot_batch(rng, n0, max_len, n_keys)
    ts = make_ts(rng, n0, family)
    start = (b, ts)
    rc, pos = np.full(n0, WD_RUN, np.uint8), np.zeros(n0, np.uint32)
    steps = []
    for _ in range(epochs):
        s = {}
        e = replay_epoch(b, ts, rc, pos)
        s["epoch"] = e
        s["leave"] = np.isin(e[0], [RC_RCOK, RC_ABORT]).astype(np.uint8)
        r = replay_release(b, ts, e[0], e[1], s["leave"])
        s["release"] = r
        s["revive"] = (e[0] == RC_ABORT).astype(np.uint8)
        f = hot_batch(rng, n_fresh, max_len, n_keys)
        s["fresh"], s["fresh_src_base"] = f, b.n_txn
        s["fresh_ts"] = make_ts(rng, n_fresh, family, base=1000 + b.n_txn)
        rc, pos = r[0].copy(), r[1].copy()
        rc[s["revive"] != 0], pos[s["revive"] != 0] = WD_RUN, 0
        b = append(b, f)
        ts = np.concatenate([ts, s["fresh_ts"]])
        rc = np.concatenate([rc, np.full(n_fresh, WD_RUN, np.uint8)])
        pos = np.concatenate([pos, np.zeros(n_fresh, np.uint32)])
        s["batch"], s["ts"], s["rc"], s["pos"] = b, ts, rc, pos
        for v in s.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        steps.append(s)
    return start, steps
