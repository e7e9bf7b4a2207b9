"""GPU: the shared wave / workgroup scans (csrc/dcc_scan.h) at partial waves
and tile seams, through the public Engine API against the oracle.  A wrong
barrier or a swapped operand of a non-commutative scan (Calvin's grant state,
MaaT's round state) shows at sizes around the wave (63, 64, 65) and around
each path's workgroup tile T (T - 1, T, T + 1, 2T + 1), not at 1M.

Two kinds of batch per size: every scan element nonzero (each txn one write
to its own key: all commit, every counter is 1), and a ragged random one.
Where the tile counts requests (Calvin, MaaT) a third kind has one random key
per txn, so the request count hits the seam exactly under contention."""
import functools

import numpy as np
import pytest

import _oracle as orc
import deneva_amd as d
from deneva_amd import RD, WR
from helpers import random_batch

pytestmark = pytest.mark.gpu

WAVE = (1, 63, 64, 65)


def seams(*tiles):
    s = set(WAVE)
    for t in tiles:
        s |= {t - 1, t, t + 1, 2 * t + 1}
    return sorted(s)


@functools.lru_cache(maxsize=None)
def batch(kind, n):
    rng = np.random.default_rng(0x5CA9 + n)
    if kind == "ones":  # one write to the txn's own key
        b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint64),
                         np.full(n, WR, np.uint8))
    elif kind == "onekey":  # one random key per txn: nnz == n, contended
        b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32),
                         rng.integers(0, max(64, n // 8), size=n).astype(np.uint64),
                         np.where(rng.random(n) < 0.4, WR, RD).astype(np.uint8))
    else:
        b = random_batch(rng, n, 10, max(64, n // 8), p_write=0.4)
    return b


def committed_writes(b, etn):
    """(keys, tn) of the committed txns' writes, as the history holds them."""
    owner = np.repeat(np.arange(b.n_txn), np.diff(np.asarray(b.offsets, np.int64)))
    sel = (np.asarray(b.acctype) == WR) & (etn[owner] != 0)
    return np.asarray(b.keys)[sel], etn[owner[sel]]


@functools.lru_cache(maxsize=None)
def occ_case(kind, n):
    """Two epochs: the first appends to an empty history, the second has
    validation windows that read what the first appended."""
    rng = np.random.default_rng(0x0CC + n)
    b1 = batch(kind, n)
    e1 = orc.occ(b1)
    hk, ht = committed_writes(b1, e1[1])
    b2 = batch(kind, n)
    b2 = d.EpochBatch(b2.offsets, b2.keys, b2.acctype)
    b2.start_tn = rng.integers(0, e1[2] + 1, size=n).astype(np.uint64)
    b2.finish_tn = (b2.start_tn + rng.integers(0, 200, size=n)).astype(np.uint64)
    e2 = orc.occ(b2, hist_keys=hk, hist_tn=ht, tnc=e1[2])
    hk2, ht2 = committed_writes(b2, e2[1])
    hk, ht = np.concatenate([hk, hk2]), np.concatenate([ht, ht2])
    o = np.lexsort((ht, hk))
    return (b1, e1), (b2, e2), (hk[o], ht[o])


# k_fin: 2,048 txns per workgroup; k_hist_* / k_scan_*: 1,024
@pytest.mark.parametrize("kind", ["ones", "ragged"])
@pytest.mark.parametrize("n", seams(1024, 2048))
def test_occ_finish_and_history(engine, kind, n):
    (b1, e1), (b2, e2), (hk, ht) = occ_case(kind, n)
    engine.history_clear()
    engine.tnc = 0
    for b, (erc, etn, etnc) in ((b1, e1), (b2, e2)):
        rc, tn, _ = engine.occ_validate_epoch(b, want_tn=True, append_history=True)
        assert np.array_equal(np.asarray(rc), erc)
        assert np.array_equal(np.asarray(tn, np.uint64), etn)
        assert engine.tnc == etnc
    gk, gt = engine.history_export()
    assert np.array_equal(gk, hk) and np.array_equal(gt, ht)
    engine.history_clear()
    engine.tnc = 0


@functools.lru_cache(maxsize=None)
def calvin_case(kind, n):
    b = batch(kind, n)
    order = np.random.default_rng(0xCA1 + n).integers(0, max(2, n // 4), size=n)  # with ties
    b = d.EpochBatch(b.offsets, b.keys, b.acctype, order=order.astype(np.uint64))
    return b, orc.calvin(b)


# CV_TILE: 4,096 requests per workgroup; "ones" / "onekey" have nnz == n
@pytest.mark.parametrize("path", [1, 2], ids=["sort", "bucket"])
@pytest.mark.parametrize("kind", ["ones", "onekey", "ragged"])
@pytest.mark.parametrize("n", seams(4096))
def test_calvin_groups(engine, path, kind, n):
    b, (eg, erc, _) = calvin_case(kind, n)
    engine.set_option(d._abi.OPT_CALVIN_PATH, path)
    try:
        g, rc, _, _ = engine.calvin_order_epoch(b, want_group=True)
    finally:
        engine.set_option(d._abi.OPT_CALVIN_PATH, 0)
    assert np.array_equal(np.asarray(g).astype(np.uint32), eg)
    assert np.array_equal(np.asarray(rc), erc)


@functools.lru_cache(maxsize=None)
def maat_want(kind, n):
    return orc.maat(batch(kind, n))[:2]


# MT_TILE: 4,096 list positions per workgroup
@pytest.mark.parametrize("kind", ["ones", "onekey", "ragged"])
@pytest.mark.parametrize("n", seams(4096))
def test_maat_rounds(engine, kind, n):
    b = batch(kind, n)
    erc, ects = maat_want(kind, n)
    engine.maat_rows_clear()
    try:
        rc, cts, _ = engine.maat_validate_epoch(b)
    finally:
        engine.maat_rows_clear()
    assert np.array_equal(np.asarray(rc), erc)
    assert np.array_equal(np.asarray(cts, np.uint64), ects)


@pytest.fixture(scope="module")
def sharded():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with d.Engine(devices=[0, 0]) as eng:
        yield eng


@functools.lru_cache(maxsize=None)
def occ_want(kind, n):
    return orc.occ(batch(kind, n))


# SH_B: 256 txns per workgroup of the key-shard partition
@pytest.mark.parametrize("kind", ["ones", "ragged"])
@pytest.mark.parametrize("n", seams(256))
def test_key_shards(sharded, kind, n):
    b = batch(kind, n)
    erc, etn, etnc = occ_want(kind, n)
    sharded.tnc = 0
    rc, tn, _ = sharded.occ_validate_epoch(b, want_tn=True)
    assert np.array_equal(np.asarray(rc), erc)
    assert np.array_equal(np.asarray(tn, np.uint64), etn)
    assert sharded.tnc == etnc
