"""GPU: the key-sharded NO_WAIT lock epoch (dcc_nowait_lock_epoch with
DCC_SHARD_SELF, nowait.hip) against the literal Row_lock replay
of the whole batch (nowait_ref.py): RC, the request each aborted txn aborted
at and the counts bit-exact, on multi-GPU contexts whose R ranks share the
GPU over the in-process host exchange, on two rank processes over gloo and on
the one-rank RCCL clique."""
import functools
import os
import socket

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RD, SCAN, WR, XP, _abi
from helpers import chain_batch, make_batch, random_batch
from nowait_cases import KATS
from nowait_ref import replay
from nowait_shard_cases import directed

pytestmark = pytest.mark.gpu


def held_arrays(held):
    if held is None:
        return None
    return (np.array([k for k, _ in held], np.uint64), np.array([t for _, t in held], np.uint8))


@pytest.fixture(scope="module")
def multi():
    """Engine(devices=[0] * R), made once per R."""
    made = {}

    def get(R):
        if R not in made:
            made[R] = d.Engine(devices=[0] * R)
        return made[R]

    yield get
    for e in made.values():
        e.close()


def check(eng, R, b, held=None, ref=None, dev=False, run_batch=None, shard=True):
    """Run `b` (or run_batch, another form of the same epoch) key-sharded and
    compare with the replay of the whole `b`.  Returns (rc, conflict, stats)."""
    erc, ecf = ref if ref is not None else replay(b, held)
    bb = run_batch if run_batch is not None else b
    h = held
    if dev:
        import torch
        bb = bb.to_torch("cuda:0")
        if held is not None:
            h = (torch.from_numpy(np.ascontiguousarray(held[0], np.uint64).view(np.int64)).to("cuda:0"),
                 torch.from_numpy(np.ascontiguousarray(held[1], np.uint8)).to("cuda:0"))
    rc, cf, st = eng.nowait_lock_epoch(bb, held=h, shard=shard)
    if dev:
        rc, cf = rc.cpu().numpy(), cf.cpu().numpy().view(np.uint32)
    rc, cf = np.asarray(rc), np.asarray(cf)
    bad = np.nonzero(rc != erc)[0]
    assert bad.size == 0, f"rc mismatch at {bad[:10]} (gpu {rc[bad[:10]]} replay {erc[bad[:10]]})"
    bad = np.nonzero(cf != ecf)[0]
    assert bad.size == 0, f"conflict mismatch at {bad[:10]} (gpu {cf[bad[:10]]} replay {ecf[bad[:10]]})"
    assert st["n_shards"] == R
    assert st["n_commit"] == int((erc == RC_RCOK).sum())
    assert st["n_abort"] == int((erc == RC_ABORT).sum())
    if b.n_txn:
        at = np.asarray(b.acctype)
        ex = (at != RD) & (at != SCAN)
        assert st["nnz_w"] == int(ex.sum())
        exc = np.concatenate([[0], np.cumsum(ex)])
        off = np.asarray(b.offsets).astype(np.int64)
        assert st["n_readonly"] == int((exc[off[1:]] == exc[off[:-1]]).sum())
        assert st["alg_bytes"] == d.nowait_alg_bytes(b.n_txn, b.nnz, True)
    return rc, cf, st


@functools.lru_cache(maxsize=None)
def ycsb(n_txn, theta):
    b = d.gen_ycsb(n_txn=n_txn, zipf_theta=theta)
    return b, replay(b)


@functools.lru_cache(maxsize=None)
def tpcc():
    b = d.gen_tpcc(n_txn=16384, num_wh=128)
    return b, replay(b)


def both_outcomes(ref):
    erc, ecf = ref
    assert 0 < int((erc == RC_RCOK).sum()) < erc.size, "the replay yields one outcome only"
    assert int(((erc == RC_ABORT) & (ecf > 0)).sum()) > 0, "every abort is at request 0"


@pytest.mark.parametrize("R", [2, 3, 4])
def test_known_answers(multi, R):
    for _, txns, held, rc, conflict in KATS:
        for dev in (False, True):
            grc, gcf, _ = check(multi(R), R, make_batch(txns), held_arrays(held), dev=dev)
            assert grc.tolist() == rc and gcf.tolist() == conflict


@pytest.mark.parametrize("R", [2, 3, 4])
def test_directed(multi, R):
    """A self-conflict on one shard with live locks on another (without and
    with a held row); the first conflicting request on another rank, both
    ways; killed on one shard while only blocked at a lower ordinal on
    another; two ranks without any access; one txn; txns of length 0; the
    empty batch."""
    for name, txns, held in directed(d.key_shard, R):
        for dev in (False, True):
            if dev and not txns:
                continue
            check(multi(R), R, make_batch(txns), held_arrays(held), dev=dev)


@pytest.mark.parametrize("all_wr", [False, True])
def test_one_hot_row(multi, all_wr):
    """20,000 one-access txns on one row: one rank has every request."""
    n = 20000
    at = np.full(n, WR if all_wr else RD, np.uint8)
    at[10000] = WR
    b = d.EpochBatch(np.arange(n + 1, dtype=np.uint32), np.full(n, 77, np.uint64), at)
    rc, cf, _ = check(multi(2), 2, b)
    if all_wr:
        assert rc[0] == RC_RCOK and np.all(rc[1:] == RC_ABORT) and np.all(cf[1:] == 0)
    else:
        assert rc[10000] == RC_ABORT and cf[10000] == 0 and int((rc == RC_RCOK).sum()) == n - 1


@pytest.mark.parametrize("R", [2, 3])
def test_cross_shard_chain_past_the_tag_wrap(multi, R):
    sh = d.shard_of_keys(np.arange(300, dtype=np.uint64), R)
    assert int((sh[1:] != sh[:-1]).sum()) > 62  # every such round's decision crosses ranks
    _, _, st = check(multi(R), R, chain_batch(300))
    assert st["rounds"] > 62


def test_lengths_at_the_limit(multi):
    rng = np.random.default_rng(5)
    n = 300
    keys = rng.integers(0, 40000, size=(n, 64))
    at = np.where(rng.random((n, 64)) < 0.03, WR, RD)
    b = make_batch([list(zip(keys[i].tolist(), at[i].tolist())) for i in range(n)])
    assert np.all(np.diff(b.offsets) == 64)
    ref = replay(b)
    both_outcomes(ref)
    eng = multi(4)
    check(eng, 4, b, ref=ref)
    long = make_batch([[(1, RD)], [(100 + q, RD) for q in range(65)], [(2, WR)]])
    for bb in (long, long.to_torch("cuda:0")):
        with pytest.raises(d.DccError) as e:
            eng.nowait_lock_epoch(bb, shard=True)
        assert e.value.code == _abi.DCC_EINVAL
    check(eng, 4, b, ref=ref)  # the context still works


@functools.lru_cache(maxsize=None)
def random_draws():
    """The twelve draws of test_gpu_nowait.test_random with their replays."""
    rng = np.random.default_rng(11)
    out = []
    for it in range(12):
        nk = int(rng.integers(1, 2000))
        types = (RD, WR) if it % 3 else (RD, WR, XP, SCAN)
        b = random_batch(rng, int(rng.integers(1, 5000)), int(rng.integers(1, 64)), nk,
                         p_write=float(rng.random()), types=types, unique=bool(it % 2))
        held = None
        if it >= 6:  # a random held prefix over distinct keys, passed whole to every rank
            hk = rng.choice(nk, size=int(rng.integers(0, nk + 1)), replace=False).astype(np.uint64)
            held = (hk, rng.integers(0, 4, size=hk.size).astype(np.uint8))
        out.append((b, held, replay(b, held), it in (3, 8)))
    return out


@pytest.mark.parametrize("R", [2, 3, 4])
def test_random(multi, R):
    for b, held, ref, dev in random_draws():
        check(multi(R), R, b, held, ref=ref, dev=dev)


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("theta", [0.0, 0.6, 0.99])
def test_ycsb_8192_forms(multi, R, theta):
    b, ref = ycsb(8192, theta)
    both_outcomes(ref)
    eng = multi(R)
    check(eng, R, b, ref=ref)
    check(eng, R, b, ref=ref, dev=True)
    c = eng.compact_host_batch(b)
    assert c.keys.dtype == np.uint32 and c.meta.get("acctype_2bit")
    check(eng, R, b, ref=ref, run_batch=c)


@pytest.mark.parametrize("R", [2, 4])
def test_tpcc_forms(multi, R):
    b, ref = tpcc()
    both_outcomes(ref)
    eng = multi(R)
    check(eng, R, b, ref=ref)
    check(eng, R, b, ref=ref, dev=True)
    check(eng, R, b, ref=ref, run_batch=eng.compact_host_batch(b))


def test_held_rows_carried_over_epochs(multi):
    """Epoch e+1's held prefix is the requests of epoch e's committed txns."""
    held = None
    for e in range(4):
        b = d.gen_ycsb(n_txn=8192, zipf_theta=0.8, table_size=1 << 14, seed=70 + e)
        ref = replay(b, held)
        assert 0 < int((ref[0] == RC_RCOK).sum()) < b.n_txn
        rc, _, _ = check(multi(3), 3, b, held, ref=ref, dev=e == 2)
        per_req = np.repeat(rc == RC_RCOK, np.diff(b.offsets.astype(np.int64)))
        held = (b.keys[per_req].copy(), b.acctype[per_req].copy())
        assert held[0].size > 0


def test_malformed_batches(multi):
    eng = multi(3)
    good = make_batch([[(1, RD)], [(2, WR), (3, RD)]])
    off = good.offsets.copy()
    off[1] = 4  # [0, 4, 3]: decreases
    with pytest.raises(d.DccError) as e:
        eng.nowait_lock_epoch(d.EpochBatch(off, good.keys, good.acctype), shard=True)
    assert e.value.code == _abi.DCC_EINVAL
    keys = good.keys.copy()
    keys[1] = d.KEY_RESERVED
    with pytest.raises(d.DccError) as e:
        eng.nowait_lock_epoch(d.EpochBatch(good.offsets, keys, good.acctype), shard=True)
    assert e.value.code == _abi.DCC_EINVAL
    with pytest.raises(d.DccError) as e:
        eng.nowait_lock_epoch(good, held=(np.array([5, d.KEY_RESERVED], np.uint64), np.array([WR, WR], np.uint8)),
                              shard=True)
    assert e.value.code == _abi.DCC_EINVAL
    check(eng, 3, good)  # a good epoch follows


def test_reserve_and_repeat(multi):
    """After reserve, two identical flagged calls return identical outputs; a
    flagged call and an unflagged one on the same context do not disturb each
    other, in either order."""
    b, _ = ycsb(8192, 0.99)
    eng = multi(2)
    eng.reserve(b.n_txn, b.nnz)
    hk = np.unique(b.keys[:2000])
    held = (hk, np.where(hk % 3 == 0, WR, RD).astype(np.uint8))
    ref = replay(b, held)
    r1 = check(eng, 2, b, held, ref=ref)
    r2 = check(eng, 2, b, held, ref=ref)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    check(eng, 1, b, ref=ycsb(8192, 0.99)[1], shard=False)  # unflagged: rank 0 alone
    check(eng, 2, b, held, ref=ref)
    check(eng, 1, b, held, ref=ref, shard=False)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def allreduce_max(buf):
        t = torch.from_numpy(buf)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)

    eng = d.Engine(0)
    eng.comm_init_host(rank, world, allreduce_max)
    b = d.gen_ycsb(n_txn=8192, zipf_theta=0.9)
    rc, cf, st = eng.nowait_lock_epoch(b, shard=True)
    out[rank] = (np.asarray(rc).copy(), np.asarray(cf).copy(), st["n_shards"], st["n_commit"], st["rounds"],
                 eng.comm_calls)
    eng.close()
    dist.destroy_process_group()


def test_rank_processes():
    """Two rank processes sharing the GPU, the exchange over gloo: both return
    the replay's decisions."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    b = d.gen_ycsb(n_txn=8192, zipf_theta=0.9)
    erc, ecf = replay(b)
    for r in range(2):
        rc, cf, nsh, n_commit, rounds, calls = out[r]
        assert nsh == 2 and n_commit == int((erc == RC_RCOK).sum())
        assert np.array_equal(rc, erc), f"rank {r}: rc differs from the replay"
        assert np.array_equal(cf, ecf), f"rank {r}: conflict ordinals differ from the replay"
        assert calls >= rounds + 1
    assert out[0][4] == out[1][4] and out[0][5] == out[1][5]  # the same rounds, the same collectives


def test_solo_rccl_call_path():
    """The one-rank RCCL clique runs the flagged epoch's collectives on RCCL:
    one per round enqueued and one for the conflict ordinals."""
    b, ref = ycsb(8192, 0.6)
    with d.Engine(0) as solo:
        solo.set_option(_abi.OPT_COMM_SOLO, 1)
        solo.comm_init(0, 1, d.comm_unique_id())
        c0 = solo.comm_calls
        _, _, st = check(solo, 1, b, ref=ref)
        assert solo.comm_calls - c0 >= st["rounds"] + 1
        c1 = solo.comm_calls
        check(solo, 1, b, ref=ref, shard=False)  # unflagged: no collective
        assert solo.comm_calls == c1


@pytest.mark.parametrize("bad_rank", [0, 2])
def test_failing_rank_does_not_hang(bad_rank):
    """A rank fails before its first exchange (the host-side injection): the
    flagged epoch returns the error instead of waiting, and flagged epochs on
    this and on a fresh context are correct."""
    b, ref = ycsb(8192, 0.6)
    with d.Engine(devices=[0] * 3) as eng:
        eng.set_option(_abi.OPT_FAIL_RANK, bad_rank)
        with pytest.raises(d.DccError, match="injected"):
            eng.nowait_lock_epoch(b, shard=True)
        check(eng, 3, b, ref=ref)
    with d.Engine(devices=[0] * 3) as eng:
        check(eng, 3, b, ref=ref)


def test_unflagged_behaviour_unchanged(engine, multi):
    b, ref = ycsb(8192, 0.6)
    with d.Engine(0) as eng:
        eng.comm_init_host(0, 2, lambda buf: None)
        with pytest.raises(d.DccError) as e:
            eng.nowait_lock_epoch(b)
        assert e.value.code == _abi.DCC_ENOTSUP
        eng.comm_destroy()
    check(multi(2), 1, b, ref=ref, shard=False)  # the whole epoch on rank 0
    check(engine, 1, b, ref=ref, shard=True)  # no communicator: the flag is ignored
