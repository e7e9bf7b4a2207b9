"""GPU parity of dcc_waitdie_carry (waitdie_carry.hip) with its numpy
restatement (waitdie_carry_ref.carry): every output array bit-exact, on host
and on device arrays; the tile seams of the stayers' scatter and the alignment
seams of the fresh append; the rejections with nothing written; a six-epoch
history that stays on the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RC_WAIT, WD_GONE, WD_RUN, _abi
from deneva_amd.engine import pack_acctype
from waitdie_carry_ref import CarryRange, alg_bytes, as_batch, carry, carry_history

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def select_constant(name):
    src = open(os.path.join(ROOT, "deneva_amd", "csrc", "csr_select.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


SEL_T = select_constant("SEL_T")    # txns per tile of the stayers' scatter
SEL_KU = select_constant("SEL_KU")  # keys per lane and step of its gather
STATES = np.asarray([WD_RUN, RC_RCOK, RC_WAIT, RC_ABORT, WD_GONE], np.uint8)
NAMES = ("offsets", "keys", "acctype", "ts", "rc", "pos", "src")
BOTH = pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])


# ------------------------------------------------------------------ builders
def csr(rng, lens, wide_keys=False):
    lens = np.asarray(lens, np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    m = int(off[-1])
    keys = rng.integers(0, 1 << 32, size=m, dtype=np.uint64)
    if wide_keys:
        keys |= rng.integers(0, 1 << 31, size=m, dtype=np.uint64) << np.uint64(32)
    return d.EpochBatch(off, keys, rng.integers(0, 4, size=m).astype(np.uint8))


def state(rng, b, rc=None, p_gone=0.3):
    """A valid (ts, rc, pos) over b: rc given or random, pos drawn inside the
    range its state allows, anything for a GONE txn."""
    n = b.n_txn
    lens = np.diff(b.offsets.astype(np.int64))
    if rc is None:
        rc = np.where(rng.random(n) < p_gone, WD_GONE, STATES[rng.integers(0, 4, size=n)]).astype(np.uint8)
    rc = np.asarray(rc, np.uint8).copy()
    rc[(rc == RC_WAIT) & (lens == 0)] = WD_RUN  # a waiter waits at an access
    pos = np.floor(rng.random(n) * (lens + 1)).astype(np.uint32)
    pos[rc == RC_RCOK] = lens[rc == RC_RCOK]
    w = rc == RC_WAIT
    pos[w] = np.floor(rng.random(int(w.sum())) * lens[w]).astype(np.uint32)
    g = rc == WD_GONE
    pos[g] = rng.integers(0, 1 << 32, size=int(g.sum()), dtype=np.uint64).astype(np.uint32)
    ts = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    return ts, rc, pos


def random_pop(rng, n, max_len=6, **kw):
    b = csr(rng, rng.integers(0, max_len + 1, size=n))
    return (b,) + state(rng, b, **kw)


def compact(b):
    return d.EpochBatch(b.offsets, np.asarray(b.keys, np.uint32), pack_acctype(b.acctype), meta={"acctype_2bit": True})


def t_dev(a, dt):
    import torch
    a = np.array(a, dt)  # a writable copy
    view = {np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}[dt]
    return torch.from_numpy(a.view(view)).to("cuda:0")


def b_dev(b):
    """The batch on the device, wide or compact as it is."""
    kdt = np.uint32 if np.asarray(b.keys).dtype.itemsize == 4 else np.uint64
    return d.EpochBatch(t_dev(b.offsets, np.uint32), t_dev(b.keys, kdt), t_dev(b.acctype, np.uint8),
                        meta=dict(b.meta))


def to_np(a, dt):
    if isinstance(a, np.ndarray):
        return a.astype(dt, copy=True)
    return a.cpu().numpy().view(dt).copy()


DT = dict(offsets=np.uint32, keys=np.uint64, acctype=np.uint8, ts=np.uint64, rc=np.uint8, pos=np.uint32,
          src=np.uint32)


def result(got):
    o, ts, rc, pos, src, kept, st = got
    r = dict(offsets=o.offsets, keys=o.keys, acctype=o.acctype, ts=ts, rc=rc, pos=pos, src=src)
    r = {k: to_np(v, DT[k]) for k, v in r.items()}
    r["kept"], r["stats"] = kept, st
    return r


def run(eng, b, ts, rc, pos, revive=None, src_in=None, fresh=None, fresh_ts=None, base=0, dev=False, **kw):
    """The call on host or device copies of the arguments; the outputs as numpy."""
    if dev:
        got = eng.waitdie_carry(b if b.on_device else b_dev(b), t_dev(ts, np.uint64), t_dev(rc, np.uint8),
                                t_dev(pos, np.uint32),
                                None if revive is None else t_dev(revive, np.uint8),
                                None if src_in is None else t_dev(src_in, np.uint32),
                                None if fresh is None else (fresh if fresh.on_device else b_dev(fresh)),
                                None if fresh_ts is None else t_dev(fresh_ts, np.uint64), base, **kw)
    else:
        got = eng.waitdie_carry(b, ts, rc, pos, revive, src_in, fresh, fresh_ts, base, **kw)
    return result(got)


def same(exp, got, what=""):
    for k in NAMES:
        assert got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
        bad = np.nonzero(got[k] != exp[k])[0]
        assert bad.size == 0, f"{what}{k} differs at {bad[:8]}: gpu {got[k][bad[:8]]} ref {exp[k][bad[:8]]}"
    assert got["kept"] == exp["kept"]


def check(eng, b, ts, rc, pos, revive=None, src_in=None, fresh=None, fresh_ts=None, base=0, modes=(False, True),
          run_batch=None, run_fresh=None):
    """Host and device calls against the reference; run_batch / run_fresh: the
    forms of the two batches the engine gets (the reference takes the wide ones)."""
    exp = carry(b, ts, rc, pos, revive, src_in, fresh, fresh_ts, base)
    for dev in modes:
        got = run(eng, run_batch or b, ts, rc, pos, revive, src_in, run_fresh or fresh, fresh_ts, base, dev=dev)
        same(exp, got, "device: " if dev else "host: ")
        st = got["stats"]
        nf, mf = (fresh.n_txn, fresh.nnz) if fresh is not None else (0, 0)
        assert (st["n_commit"], st["n_abort"], st["n_survivors"]) == (exp["kept"], b.n_txn - exp["kept"],
                                                                      exp["revived"])
        assert st["alg_bytes"] == alg_bytes(b.n_txn, exp["kept"], int(exp["offsets"][exp["kept"]]), nf, mf,
                                            revive is not None, True)
    return exp


def fresh_of(rng, n, max_len=6, **kw):
    f = csr(rng, rng.integers(0, max_len + 1, size=n), **kw)
    return f, rng.integers(0, 1 << 64, size=n, dtype=np.uint64)


EMPTY = d.EpochBatch(np.zeros(1, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint8))
NO_STATE = (np.zeros(0, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint32))


# ------------------------------------------------------------ known answers
def test_empty_population_fresh_only(engine):
    rng = np.random.default_rng(1)
    f, fts = fresh_of(rng, 40)
    exp = check(engine, EMPTY, *NO_STATE, fresh=f, fresh_ts=fts, base=77)
    assert exp["kept"] == 0 and exp["src"].tolist() == list(range(77, 117))
    assert np.array_equal(exp["offsets"], f.offsets) and np.all(exp["rc"] == WD_RUN) and not exp["pos"].any()


def test_fresh_null_and_both_empty(engine):
    rng = np.random.default_rng(2)
    b, ts, rc, pos = random_pop(rng, 300)
    check(engine, b, ts, rc, pos)
    check(engine, b, ts, rc, pos, fresh=EMPTY, fresh_ts=np.zeros(0, np.uint64))
    exp = check(engine, EMPTY, *NO_STATE)
    assert exp["offsets"].tolist() == [0]
    check(engine, EMPTY, *NO_STATE, fresh=EMPTY, fresh_ts=np.zeros(0, np.uint64))


@pytest.mark.parametrize("pattern", ["all_gone", "none_gone", "alternating"])
def test_patterns(engine, pattern):
    rng = np.random.default_rng(3)
    n = 2 * SEL_T + 37
    b = csr(rng, rng.integers(0, 7, size=n), wide_keys=True)
    rc = STATES[rng.integers(0, 4, size=n)]
    if pattern == "all_gone":
        rc = np.full(n, WD_GONE, np.uint8)
    elif pattern == "alternating":
        rc[::2] = WD_GONE
    ts, rc, pos = state(rng, b, rc)
    f, fts = fresh_of(rng, 50, wide_keys=True)
    exp = check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, base=n)
    assert exp["kept"] == {"all_gone": 0, "none_gone": n, "alternating": n // 2}[pattern]


def test_zero_length_txns_kept(engine):
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 3, size=SEL_T + 9)
    lens[[0, 5, SEL_T - 1, SEL_T, SEL_T + 8]] = 0
    b = csr(rng, lens)
    ts, rc, pos = state(rng, b, np.full(lens.size, WD_RUN, np.uint8))
    flens = rng.integers(0, 3, size=70)
    flens[[0, 1, 69]] = 0
    f = csr(rng, flens)
    exp = check(engine, b, ts, rc, pos, fresh=f, fresh_ts=np.arange(70, dtype=np.uint64))
    assert exp["kept"] == lens.size and np.array_equal(np.diff(exp["offsets"].astype(np.int64)),
                                                       np.concatenate([lens, flens]))
    # a population of zero-length txns alone, and a fresh batch of them
    z = csr(rng, np.zeros(5, np.int64))
    check(engine, z, *state(rng, z, np.asarray([WD_RUN, RC_RCOK, RC_ABORT, WD_GONE, WD_RUN])), fresh=z,
          fresh_ts=np.arange(5, dtype=np.uint64))


def test_revive_every_gone_txn(engine):
    rng = np.random.default_rng(5)
    b, ts, rc, pos = random_pop(rng, 3 * SEL_T + 5, p_gone=0.5)
    exp = check(engine, b, ts, rc, pos, revive=(rc == WD_GONE).astype(np.uint8))
    assert exp["kept"] == b.n_txn and exp["revived"] == int((rc == WD_GONE).sum()) > 0
    g = rc == WD_GONE
    assert np.all(exp["rc"][g] == WD_RUN) and not exp["pos"][g].any() and np.array_equal(exp["ts"], ts)
    # some of them, with values other than 1
    rev = np.where(g & (rng.random(b.n_txn) < 0.5), 0x80, 0).astype(np.uint8)
    check(engine, b, ts, rc, pos, revive=rev)


def test_src_in_given_and_null(engine):
    rng = np.random.default_rng(6)
    b, ts, rc, pos = random_pop(rng, 500)
    src = rng.integers(0, 1 << 32, size=500, dtype=np.uint64).astype(np.uint32)
    f, fts = fresh_of(rng, 30)
    a = check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, base=0xFFFFFFF0)  # the fresh src wraps
    c = check(engine, b, ts, rc, pos, src_in=src, fresh=f, fresh_ts=fts, base=9)
    assert np.array_equal(c["src"][:c["kept"]], src[a["src"][:a["kept"]]])


@BOTH
def test_identity_composes_over_three_carries(engine, dev):
    rng = np.random.default_rng(7)
    b, ts, rc, pos = random_pop(rng, 700)
    ts0, total, src = ts.copy(), 700, None
    for step in range(3):
        f, fts = fresh_of(rng, 100)
        ts0 = np.concatenate([ts0, fts])
        exp = carry(b, ts, rc, pos, None, src, f, fts, total)
        got = run(engine, b, ts, rc, pos, None, src, f, fts, total, dev=dev)
        same(exp, got)
        total += 100
        b, ts, pos, src = as_batch(got), got["ts"], got["pos"], got["src"]
        assert np.array_equal(ts, ts0[src])  # src names the txn of the first population / its arrival
        rc = got["rc"].copy()
        rc[rng.random(rc.size) < 0.3] = WD_GONE


# ------------------------------------------------- seams of the stayers' scatter
@pytest.mark.parametrize("n", [SEL_T - 1, SEL_T, SEL_T + 1, 2 * SEL_T + 1])
def test_txn_count_at_the_tile_size(engine, n):
    rng = np.random.default_rng(n)
    b, ts, rc, pos = random_pop(rng, n)
    f, fts = fresh_of(rng, 20)
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, base=n)


def test_first_or_last_txn_of_a_tile_dropped(engine):
    rng = np.random.default_rng(11)
    n = 2 * SEL_T + 1
    b = csr(rng, rng.integers(1, 7, size=n))
    edges = [0, SEL_T - 1, SEL_T, 2 * SEL_T - 1, 2 * SEL_T]
    for drop in (edges, edges[::2], edges[1::2]):
        rc = np.full(n, RC_ABORT, np.uint8)
        rc[drop] = WD_GONE
        ts, rc, pos = state(rng, b, rc)
        assert check(engine, b, ts, rc, pos)["kept"] == n - len(drop)


def test_longest_txn_last_of_a_tile(engine):
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 4, size=SEL_T + 40)
    lens[SEL_T - 1] = 64
    b = csr(rng, lens)
    ts, rc, pos = state(rng, b, p_gone=0.2)
    rc[SEL_T - 1], pos[SEL_T - 1] = RC_WAIT, 63
    check(engine, b, ts, rc, pos)
    rc[SEL_T - 2] = WD_GONE
    check(engine, b, ts, rc, pos)


@pytest.mark.parametrize("kept_accesses", [SEL_KU * SEL_T - 1, SEL_KU * SEL_T, SEL_KU * SEL_T + 1])
def test_tile_at_the_gather_step(engine, kept_accesses):
    """The first tile keeps kept_accesses accesses (its gather walks SEL_KU *
    SEL_T per step) and drops every eighth txn; a second tile follows."""
    rng = np.random.default_rng(kept_accesses)
    n = SEL_T + 30
    lens = rng.integers(0, 7, size=n)
    rc = np.full(n, WD_RUN, np.uint8)
    rc[7:SEL_T:8] = WD_GONE
    keep = np.nonzero(rc[:SEL_T] != WD_GONE)[0]
    lens[keep] = kept_accesses // keep.size
    lens[keep[:kept_accesses - int(lens[keep].sum())]] += 1
    assert int(lens[keep].sum()) == kept_accesses
    b = csr(rng, lens)
    ts, rc, pos = state(rng, b, rc)
    exp = check(engine, b, ts, rc, pos)
    assert int(exp["offsets"][keep.size]) == kept_accesses


@pytest.mark.parametrize("first", [1, 2, 3])
def test_tile_output_lands_off_the_word(engine, first):
    """The second tile's first output access at 1, 2, 3 mod 4: the head, quad
    and tail paths of the type bytes."""
    rng = np.random.default_rng(20 + first)
    n = 2 * SEL_T + 11
    lens = rng.integers(0, 7, size=n)
    rc = np.where(rng.random(n) < 0.3, WD_GONE, RC_ABORT).astype(np.uint8)
    rc[0] = RC_ABORT
    kept = int(lens[:SEL_T][rc[:SEL_T] != WD_GONE].sum()) - int(lens[0])
    lens[0] = 4 + (first - kept) % 4
    b = csr(rng, lens)
    ts, rc, pos = state(rng, b, rc)
    exp = check(engine, b, ts, rc, pos)
    q = int((rc[:SEL_T] != WD_GONE).sum())
    assert int(exp["offsets"][q]) % 4 == first


# ---------------------------------------------------- seams of the fresh append
def pop_keeping(rng, nnz_kept):
    """A population of 40 txns whose stayers have nnz_kept accesses."""
    lens = rng.integers(1, 5, size=40)
    rc = np.where(np.arange(40) % 3 == 1, WD_GONE, RC_RCOK).astype(np.uint8)
    keep = np.nonzero(rc != WD_GONE)[0]
    lens[keep] = nnz_kept // keep.size
    lens[keep[:nnz_kept - int(lens[keep].sum())]] += 1
    b = csr(rng, lens)
    return (b,) + state(rng, b, rc)


@pytest.mark.parametrize("nnz_kept", [0, 28, 29, 30, 31, 33, 47])
def test_append_base_alignment(engine, nnz_kept):
    """The stayers' accesses at 0 .. 3 mod 4, odd ones included (the keys' 8-byte
    aligned destination) and 15 mod 16 (the longest type-byte head)."""
    rng = np.random.default_rng(100 + nnz_kept)
    b, ts, rc, pos = pop_keeping(rng, nnz_kept)
    f, fts = fresh_of(rng, 90, wide_keys=True)
    exp = check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, base=40)
    assert int(exp["offsets"][exp["kept"]]) == nnz_kept
    f, fts = fresh_of(rng, 90)
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, base=40, run_fresh=compact(f))


@pytest.mark.parametrize("n_fresh", [1, 255, 256, 257])
def test_fresh_count_at_the_workgroup_size(engine, n_fresh):
    rng = np.random.default_rng(n_fresh)
    b, ts, rc, pos = pop_keeping(rng, 21)
    f, fts = fresh_of(rng, n_fresh)
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, base=1000)
    check(engine, EMPTY, *NO_STATE, fresh=f, fresh_ts=fts)


@pytest.mark.parametrize("nnz_fresh", [1, 2, 3, 5, 18, 161, 162, 163])
@pytest.mark.parametrize("nnz_kept", [0, 13, 30])
def test_compact_fresh_with_ragged_tail(engine, nnz_fresh, nnz_kept):
    rng = np.random.default_rng(1000 * nnz_kept + nnz_fresh)
    b, ts, rc, pos = pop_keeping(rng, nnz_kept)
    lens = np.full(9, nnz_fresh // 9)
    lens[:nnz_fresh - int(lens.sum())] += 1
    f = csr(rng, lens)
    assert f.nnz == nnz_fresh
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=np.arange(9, dtype=np.uint64), run_fresh=compact(f))


def test_mixed_forms(engine):
    rng = np.random.default_rng(31)
    b, ts, rc, pos = random_pop(rng, SEL_T + 100)
    f, fts = fresh_of(rng, 120)
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, run_batch=compact(b))
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, run_fresh=compact(f))
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, run_batch=compact(b), run_fresh=compact(f))
    # one form only in each flag
    k32 = d.EpochBatch(f.offsets, np.asarray(f.keys, np.uint32), f.acctype)
    a2 = d.EpochBatch(f.offsets, f.keys, pack_acctype(f.acctype), meta={"acctype_2bit": True})
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, run_fresh=k32)
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, run_fresh=a2)


@pytest.mark.parametrize("shift", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("form", ["wide", "compact"])
def test_fresh_on_unaligned_device_arrays(engine, form, shift):
    """Device arrays sliced so that the keys and the types start `shift` items
    past their allocation: the scalar source paths of the append."""
    rng = np.random.default_rng(40 + shift)
    b, ts, rc, pos = pop_keeping(rng, 30 + shift)
    f, fts = fresh_of(rng, 150)
    g = compact(f) if form == "compact" else f
    kdt = np.asarray(g.keys).dtype.type
    pad = lambda a, dt: t_dev(np.concatenate([np.zeros(shift, dt), np.asarray(a, dt)]), dt)[shift:]
    gd = d.EpochBatch(t_dev(g.offsets, np.uint32), pad(g.keys, kdt), pad(g.acctype, np.uint8), meta=dict(g.meta))
    check(engine, b, ts, rc, pos, fresh=f, fresh_ts=fts, base=5, modes=(True,), run_fresh=gd)


# ------------------------------------------------------------------ rejections
SENTINEL = 0xA5


def sentinel_out(dev, cap_txn, cap_nnz):
    def full(k, dt):
        a = np.full(max(k, 1), SENTINEL, np.uint8).repeat(np.dtype(dt).itemsize).view(dt)
        return t_dev(a, dt) if dev else a.copy()
    out = d.EpochBatch(full(cap_txn + 1, np.uint32), full(cap_nnz, np.uint64), full(cap_nnz, np.uint8))
    out.meta.update(cap=(cap_txn, cap_nnz), ts=full(cap_txn, np.uint64), rc=full(cap_txn, np.uint8),
                    pos=full(cap_txn, np.uint32), src=full(cap_txn, np.uint32))
    return out


def untouched(out):
    arrays = [out.offsets, out.keys, out.acctype] + [out.meta[k] for k in ("ts", "rc", "pos", "src")]
    raw = lambda a: (a if isinstance(a, np.ndarray) else a.cpu().numpy()).view(np.uint8)
    return all(np.all(raw(a) == SENTINEL) for a in arrays)


def rejected(eng, code, dev, b, ts, rc, pos, revive=None, fresh=None, fresh_ts=None, cap=None):
    nf, mf = (fresh.n_txn, fresh.nnz) if fresh is not None else (0, 0)
    cap = cap or (b.n_txn + nf, b.nnz + mf)
    out = sentinel_out(dev, *cap)
    with pytest.raises(d.DccError) as e:
        run(eng, b, ts, rc, pos, revive, None, fresh, fresh_ts, 0, dev=dev, out=out)
    assert e.value.code == code, e.value
    assert untouched(out), "a rejected call wrote to its outputs"
    return e.value, out


def small(rng):
    b = csr(rng, [2, 0, 3, 1, 4, 2] * 60)
    rc = np.asarray([WD_RUN, RC_RCOK, RC_WAIT, RC_ABORT, WD_GONE, RC_WAIT] * 60, np.uint8)
    return (b,) + state(rng, b, rc)


@BOTH
@pytest.mark.parametrize("what", ["rc_byte", "pos_gt_len", "rcok_pos", "wait_pos", "revive_live"])
def test_einval_state(engine, what, dev):
    rng = np.random.default_rng(50)
    b, ts, rc, pos = small(rng)
    rev = None
    i = 300  # a txn of the second tile; i % 6 names its state and length
    if what == "rc_byte":
        rc[i + 3] = 0x12
    elif what == "pos_gt_len":
        pos[i + 3] = 2  # ABORT, len 1
    elif what == "rcok_pos":
        rc[i + 2], pos[i + 2] = RC_RCOK, 2  # len 3
    elif what == "wait_pos":
        pos[i + 2] = 3  # WAIT, len 3
    else:
        rev = np.zeros(b.n_txn, np.uint8)
        rev[i + 4] = 1  # GONE: fine
        rev[i] = 1      # RUN
    f, fts = fresh_of(rng, 10)
    rejected(engine, _abi.DCC_EINVAL, dev, b, ts, rc, pos, rev, f, fts)


@BOTH
@pytest.mark.parametrize("which", ["batch", "fresh"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_einval_offsets(engine, which, where, dev):
    rng = np.random.default_rng(51)
    b, ts, rc, pos = small(rng)
    f, fts = fresh_of(rng, 300, max_len=3)
    t = b if which == "batch" else f
    off = t.offsets.copy()
    if where == "first":
        off[0] = 1
    elif where == "middle":
        off[200] = off[199] - 1
    else:
        off[-1] -= 1
    bad = d.EpochBatch(off, t.keys, t.acctype)
    if which == "batch":
        rejected(engine, _abi.DCC_EINVAL, dev, bad, ts, rc, pos, None, f, fts)
    else:
        rejected(engine, _abi.DCC_EINVAL, dev, b, ts, rc, pos, None, bad, fts)


def raw_args(dev, null=(), fresh_flags=None, txn_base=0, nnz_base=0):
    """The C arguments of a small valid call, with the named pointers NULL."""
    rng = np.random.default_rng(52)
    b, ts, rc, pos = small(rng)
    f, fts = fresh_of(rng, 10)
    out = sentinel_out(dev, b.n_txn + 10, b.nnz + f.nnz)
    if dev:
        b, f = b_dev(b), b_dev(f)
        ts, rc, pos, fts = t_dev(ts, np.uint64), t_dev(rc, np.uint8), t_dev(pos, np.uint32), t_dev(fts, np.uint64)
    ptr = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else int(a.data_ptr())
    cb, cf = b.to_c(), f.to_c()
    if fresh_flags is not None:
        cf.flags = fresh_flags(cb.flags)
    so = _abi.SelectOut(b.n_txn + 10, b.nnz + f.nnz, txn_base, nnz_base, ptr(out.offsets), ptr(out.keys),
                        ptr(out.acctype), None, None, None, ptr(out.meta["src"]))
    v = dict(batch=C.pointer(cb), ts=ptr(ts), rc=ptr(rc), pos=ptr(pos), revive=None, src_in=None,
             fresh=C.pointer(cf), fresh_ts=ptr(fts), fresh_src_base=0, out=C.pointer(so),
             out_ts=ptr(out.meta["ts"]), out_rc=ptr(out.meta["rc"]), out_pos=ptr(out.meta["pos"]))
    for k in null:
        v[k] = None
    return _abi.WaitdieCarryArgs(**v), out, (cb, cf, so, b, f, ts, rc, pos, fts)


@BOTH
@pytest.mark.parametrize("null", ["a", "batch", "out", "ts", "rc", "pos", "out_ts", "out_rc", "out_pos", "fresh_ts"])
def test_einval_null(engine, null, dev):
    a, out, keep = raw_args(dev, () if null == "a" else (null,))
    n = C.c_uint64(99)
    code = _abi.lib.dcc_waitdie_carry(engine.handle, None if null == "a" else C.byref(a), C.byref(n), None, None,
                                      None)
    assert code == _abi.DCC_EINVAL and n.value == 0
    assert untouched(out)


@BOTH
def test_einval_flags_and_bases(engine, dev):
    for kw in (dict(fresh_flags=lambda fl: fl ^ _abi.DEVICE_PTRS), dict(txn_base=1), dict(nnz_base=1)):
        a, out, keep = raw_args(dev, **kw)
        assert _abi.lib.dcc_waitdie_carry(engine.handle, C.byref(a), None, None, None, None) == _abi.DCC_EINVAL
        assert untouched(out)
    a, out, keep = raw_args(dev)  # the same arguments unchanged are accepted
    assert _abi.lib.dcc_waitdie_carry(engine.handle, C.byref(a), None, None, None, None) == _abi.DCC_OK
    assert not untouched(out)


@BOTH
def test_erange_then_exact_capacity(engine, dev):
    rng = np.random.default_rng(53)
    b, ts, rc, pos = random_pop(rng, SEL_T + 50)
    f, fts = fresh_of(rng, 60)
    exp = carry(b, ts, rc, pos, None, None, f, fts, 0)
    n, m, kept = exp["offsets"].size - 1, exp["keys"].size, exp["kept"]
    for cap in ((n - 1, m), (n, m - 1), (f.n_txn - 1, m), (n, f.nnz - 1)):
        e, _ = rejected(engine, _abi.DCC_ERANGE, dev, b, ts, rc, pos, None, f, fts, cap=cap)
        assert e.needed == (n, m, kept)
        with pytest.raises(CarryRange) as r:
            carry(b, ts, rc, pos, None, None, f, fts, 0, cap_txn=cap[0], cap_nnz=cap[1])
        assert r.value.needed == (n, m, kept)
    out = sentinel_out(dev, n, m)
    same(exp, run(engine, b, ts, rc, pos, None, None, f, fts, 0, dev=dev, out=out))


# ------------------------------------------------------ history on the device
@pytest.mark.parametrize("family", ["permuted", "tied"])
def test_history_stays_on_the_device(engine, family):
    """epoch -> release -> carry, six times, on device arrays, ping-ponged.  The
    host gets the counts the calls return and nothing else until the end; the
    masks of the release and of the revival are computed on the device."""
    import torch
    (b0, ts0), steps = carry_history(family)
    cap_n = steps[-1]["batch"].n_txn
    cap_m = steps[-1]["batch"].nnz
    bufs = []
    for _ in range(2):
        o = d.EpochBatch(t_dev(np.zeros(cap_n + 1), np.uint32), t_dev(np.zeros(cap_m), np.uint64),
                         t_dev(np.zeros(cap_m), np.uint8))
        o.meta["cap"] = (cap_n, cap_m)
        bufs.append(o)
    fresh = [(b_dev(s["fresh"]), t_dev(s["fresh_ts"], np.uint64)) for s in steps]
    b, ts = b_dev(b0), t_dev(ts0, np.uint64)
    rc, pos = t_dev(np.full(b0.n_txn, WD_RUN), np.uint8), t_dev(np.zeros(b0.n_txn), np.uint32)
    src = t_dev(np.arange(b0.n_txn), np.uint32)
    seen, kept = [], []
    for e, s in enumerate(steps):
        _, _, conf, _ = engine.waitdie_lock_epoch(b, ts, rc, pos)
        after_epoch = (rc.clone(), pos.clone(), conf.clone())
        died = (rc == RC_ABORT).to(torch.uint8)
        leave = ((rc == RC_RCOK) | (rc == RC_ABORT)).to(torch.uint8)
        left, prom, _ = engine.waitdie_release(b, ts, rc, pos, leave)
        after_release = (rc.clone(), pos.clone(), left, prom)
        nb, ts, rc, pos, nsrc, k, _ = engine.waitdie_carry(b, ts, rc, pos, revive=died, src_in=src, fresh=fresh[e][0],
                                                          fresh_ts=fresh[e][1],
                                                          fresh_src_base=s["fresh_src_base"], out=bufs[e % 2])
        seen.append((src, after_epoch, after_release, (nb, ts.clone(), rc.clone(), pos.clone(), nsrc.clone())))
        kept.append(k)
        b, src = nb, nsrc.clone()  # this buffer is written again by the carry after the next
    torch.cuda.synchronize()
    h32 = lambda a: to_np(a, np.uint32)
    for s, (src, ep, rel, ca) in zip(steps, seen):
        i = h32(src)
        u = s["epoch"]
        assert np.array_equal(to_np(ep[0], np.uint8), u[0][i]) and np.array_equal(h32(ep[1]), u[1][i])
        assert np.array_equal(h32(ep[2]), u[2][i])
        u = s["release"]
        assert np.array_equal(to_np(rel[0], np.uint8), u[0][i]) and np.array_equal(h32(rel[1]), u[1][i])
        assert rel[2:] == u[2:]
        j = h32(ca[4])
        assert np.all(np.diff(j.astype(np.int64)) > 0)
        gone = np.ones(s["batch"].n_txn, bool)
        gone[j] = False
        assert np.all(s["rc"][gone] == WD_GONE)
        assert np.array_equal(to_np(ca[1], np.uint64), s["ts"][j])
        assert np.array_equal(to_np(ca[2], np.uint8), s["rc"][j]) and np.array_equal(h32(ca[3]), s["pos"][j])
    # the last population, access for access
    U, nb, j = steps[-1]["batch"], seen[-1][3][0], h32(seen[-1][3][4])
    pick = np.concatenate([np.arange(U.offsets[i], U.offsets[i + 1]) for i in j]).astype(np.int64)
    assert np.array_equal(to_np(nb.keys, np.uint64), U.keys[pick])
    assert np.array_equal(to_np(nb.acctype, np.uint8), U.acctype[pick])
    assert np.array_equal(np.diff(h32(nb.offsets).astype(np.int64)), np.diff(U.offsets.astype(np.int64))[j])
    assert nb.n_txn < U.n_txn


# ------------------------------------------------------------- smaller cases
def test_reserve_and_repeat(engine):
    rng = np.random.default_rng(60)
    b, ts, rc, pos = random_pop(rng, 3000)
    f, fts = fresh_of(rng, 1000)
    engine.reserve(b.n_txn + f.n_txn, b.nnz + f.nnz)
    exp = carry(b, ts, rc, pos, None, None, f, fts, 3000)
    for dev in (True, False):
        for _ in range(2):
            same(exp, run(engine, b, ts, rc, pos, None, None, f, fts, 3000, dev=dev))


def test_two_rank_multi_context_on_one_device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(61)
    b, ts, rc, pos = random_pop(rng, SEL_T + 77)
    f, fts = fresh_of(rng, 33)
    with d.Engine(devices=[0, 0]) as m:
        check(m, b, ts, rc, pos, revive=(rc == WD_GONE) & (rng.random(b.n_txn) < 0.5), fresh=f, fresh_ts=fts)


def test_stats_and_phases(engine):
    rng = np.random.default_rng(62)
    b, ts, rc, pos = random_pop(rng, 2000)
    f, fts = fresh_of(rng, 500)
    engine.set_profiling(True)
    try:
        got = run(engine, b, ts, rc, pos, None, None, f, fts, 0, dev=True)
    finally:
        engine.set_profiling(False)
    st = got["stats"]
    kept = got["kept"]
    assert st["alg_bytes"] == d.waitdie_carry_alg_bytes(2000, kept, int(got["offsets"][kept]), 500, f.nnz, False, True)
    assert st["device_ms"] > 0 and st["total_ms"] >= st["device_ms"]
    assert all(p > 0 for p in st["phase_ms"]) and sum(st["phase_ms"]) <= st["device_ms"] * 1.5 + 0.1
