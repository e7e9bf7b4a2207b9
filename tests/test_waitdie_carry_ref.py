"""The carry of a WAIT_DIE population (dcc_waitdie_carry) changes no decision:
waitdie_carry_ref.carry plus waitdie_ref's replays on the compacted population
against the same history on the population that is never compacted, compared
through src after every call.  And the algorithmic-bytes formula of the
library against the table of include/dcc.h.  No GPU."""
import numpy as np
import pytest

import deneva_amd as d
from deneva_amd import RC_ABORT, RC_RCOK, RC_WAIT, RD, WD_GONE, WD_RUN, WR
from helpers import make_batch
from waitdie_cases import TS_FAMILIES
from waitdie_carry_ref import CarryRange, alg_bytes, as_batch, carry, carry_history
from waitdie_ref import replay_epoch, replay_release


def same(what, got, exp):
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    assert bad.size == 0, f"{what} differs at {bad[:10]}"


@pytest.mark.parametrize("family", TS_FAMILIES)
def test_carry_changes_no_decision(family):
    (b, ts), steps = carry_history(family)
    rc, pos = np.full(b.n_txn, WD_RUN, np.uint8), np.zeros(b.n_txn, np.uint32)
    src = np.arange(b.n_txn, dtype=np.uint32)
    dec, promoted, revived = [0, 0, 0], 0, 0
    for s in steps:
        # the epoch
        u = s["epoch"]
        e = replay_epoch(b, ts, rc, pos)
        same("rc after the epoch", e[0], u[0][src])
        same("pos after the epoch", e[1], u[1][src])
        same("conflict", e[2], u[2][src])
        assert e[3] == u[3]  # GONE txns decide nothing
        dec = [x + e[3][k] for x, k in zip(dec, ("n_commit", "n_abort", "n_survivors"))]
        # the release of every RCOK and ABORT txn
        u = s["release"]
        leave = np.isin(e[0], [RC_RCOK, RC_ABORT]).astype(np.uint8)
        same("leave", leave, s["leave"][src])
        r = replay_release(b, ts, e[0], e[1], leave)
        same("rc after the release", r[0], u[0][src])
        same("pos after the release", r[1], u[1][src])
        assert r[2:] == u[2:]
        promoted += r[3]
        # the next population
        c = carry(b, ts, r[0], r[1], revive=(e[0] == RC_ABORT), src_in=src, fresh=s["fresh"],
                  fresh_ts=s["fresh_ts"], fresh_src_base=s["fresh_src_base"])
        revived += c["revived"]
        b, ts, rc, pos, src = as_batch(c), c["ts"], c["rc"], c["pos"], c["src"]
        assert np.all(np.diff(src.astype(np.int64)) > 0)  # index order is kept
        gone = np.ones(s["batch"].n_txn, bool)
        gone[src] = False
        assert np.all(s["rc"][gone] == WD_GONE)  # exactly the GONE txns were dropped
        same("ts after the carry", ts, s["ts"][src])
        same("rc after the carry", rc, s["rc"][src])
        same("pos after the carry", pos, s["pos"][src])
        U = s["batch"]
        lens = np.diff(U.offsets.astype(np.int64))
        same("lengths", np.diff(b.offsets.astype(np.int64)), lens[src])
        pick = np.concatenate([np.arange(U.offsets[i], U.offsets[i + 1]) for i in src]).astype(np.int64)
        same("keys", b.keys, U.keys[pick])
        same("access types", b.acctype, U.acctype[pick])
    assert min(dec) > 0, f"an outcome is missing: RCOK / ABORT / WAIT = {dec}"
    assert promoted > 0 and revived > 0
    assert b.n_txn < steps[-1]["batch"].n_txn


def test_reference_rejections():
    b = make_batch([[(1, WR)], [(2, RD), (3, WR)], []])
    ts = np.arange(3, dtype=np.uint64)
    ok = dict(rc=[WD_RUN, RC_WAIT, WD_GONE], pos=[0, 1, 9])
    assert carry(b, ts, **ok)["kept"] == 2
    for rc, pos, rev in (([7, RC_WAIT, WD_GONE], [0, 1, 0], None), ([WD_RUN, RC_WAIT, WD_GONE], [2, 1, 0], None),
                         ([RC_RCOK, RC_WAIT, WD_GONE], [0, 1, 0], None), ([WD_RUN, RC_WAIT, WD_GONE], [0, 2, 0], None),
                         ([WD_RUN, RC_WAIT, WD_GONE], [0, 1, 0], [1, 0, 0])):
        with pytest.raises(ValueError):
            carry(b, ts, rc, pos, revive=rev)
    with pytest.raises(ValueError):
        carry(b, ts, **ok, fresh=b)
    with pytest.raises(ValueError):
        carry(d.EpochBatch(np.asarray([0, 2, 1, 3], np.uint32), b.keys, b.acctype), ts, **ok)
    with pytest.raises(CarryRange) as e:
        carry(b, ts, **ok, fresh=b, fresh_ts=ts, cap_txn=4)
    assert e.value.needed == (5, 6, 2)
    with pytest.raises(CarryRange):
        carry(b, ts, **ok, fresh=b, fresh_ts=ts, cap_nnz=5)
    assert carry(b, ts, **ok, fresh=b, fresh_ts=ts, cap_txn=5, cap_nnz=6)["src"].tolist() == [0, 1, 0, 1, 2]


@pytest.mark.parametrize("args", [(0, 0, 0, 0, 0), (1, 1, 0, 0, 0), (1000, 700, 9001, 0, 0), (0, 0, 0, 257, 4099),
                                  (65536, 40000, 640000, 65536, 1048576), (3, 2, 5, 1, 7)])
@pytest.mark.parametrize("with_revive", [False, True])
@pytest.mark.parametrize("with_src", [False, True])
def test_alg_bytes(args, with_revive, with_src):
    n, nk, mk, nf, mf = args
    want = (4 * (n + 1) + n * (2 if with_revive else 1) + 25 * nk + 18 * mk + 4 * (nf + 1) + 8 * nf + 13 * nf +
            18 * mf + 4 * (nk + nf + 1) + (8 * nk + 4 * nf if with_src else 0))
    assert alg_bytes(*args, with_revive, with_src) == want
    assert d.waitdie_carry_alg_bytes(*args, with_revive=with_revive, with_src=with_src) == want
