"""CPU checks of the MaaT edge-case builders (maat_cases.py): every fact a case
claims -- its round count, the host checks that compact, the prefix's access
count, the filter's survivors, the opposite decisions of the twins -- holds
against the oracle and the round model, the model's decisions and commit
timestamps are the oracle's, the literal replay equals the formula, and the
constants the cases are built on are the engine's."""
import functools
import os
import re

import numpy as np
import pytest

import _oracle as orc
import maat_cases as mc
from deneva_amd import KEY_RESERVED, RD, WR
from helpers import random_batch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva_amd", "csrc")


@functools.lru_cache(maxsize=None)
def solved(name):
    """The case, the oracle's formula results and the model's."""
    b, rows, facts = mc.build(name)
    rk, lr, lw = rows if rows is not None else (None, None, None)
    erc, ects, _ = orc.maat(b, rk, lr, lw)
    m = mc.model_prefix(b, rows) if mc.takes_prefix(b) else mc.model(b, rows)
    return b, rows, facts, erc, ects, m


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_is_well_formed_and_model_equals_oracle(name):
    b, rows, facts, erc, ects, m = solved(name)
    assert np.diff(b.offsets.astype(np.int64)).max() <= mc.MAX_TXN_LEN
    assert not (b.keys == np.uint64(KEY_RESERVED)).any()
    assert b.nnz <= 285000
    if rows is not None:
        assert not (rows[0] == np.uint64(KEY_RESERVED)).any() and np.unique(rows[0]).size == rows[0].size
    assert np.array_equal(m["state"] == mc.COM, erc == 0), "model decisions differ from the oracle's"
    assert np.array_equal(m["state"] == mc.ABO, erc == 2)
    assert np.array_equal(m["cts"], ects), "model commit timestamps differ from the oracle's"
    rk, lr, lw = rows if rows is not None else (None, None, None)
    lrc, lcts, lrows = orc.maat(b, rk, lr, lw, literal=True)
    assert np.array_equal(lrc, erc) and np.array_equal(lcts, ects), "literal replay differs from the formula"
    frows = orc.maat(b, rk, lr, lw)[2]
    assert all(np.array_equal(x, y) for x, y in zip(lrows, frows))
    assert mc.takes_prefix(b) == (b.n_txn > 4 * mc.MT_PREFIX)
    if "rounds" in facts:
        assert not mc.takes_prefix(b) and m["rounds"] == facts["rounds"]


def test_every_family_runs_with_device_pointers_once():
    fam = {n.split("-")[0] for n in mc.CASES}
    assert fam == {n.split("-")[0] for n in mc.DEV_CASES}
    assert set(mc.DEV_CASES) <= set(mc.CASES) and set(mc.RW_ALL_CASES) <= set(mc.CASES)


@pytest.mark.parametrize("c", mc.CHAIN_C)
def test_chain(c):
    b, rows, facts, erc, ects, m = solved(f"chain-{c}")
    assert m["rounds"] == c == b.n_txn
    assert m["und"] == list(range(c - 1, -1, -1)), "one txn decides per round"
    assert erc.tolist() == [0, 2] * (c // 2) + [0] * (c % 2)
    # the ring wraps; the position compaction runs at least twice (both buffer sets)
    assert c >= mc.MT_RING
    assert sum(pc for _, _, pc in m["checks"]) >= 2


def test_chain_seams():
    """73 ends exactly at a host check, 74 one round into a batch; 129 and 300
    wrap the ring twice and four times; 300 compacts the undecided list."""
    assert (73 - 1) % mc.MT_BATCH == 0 and (74 - 1) % mc.MT_BATCH == 1
    assert 64 == mc.MT_RING and 129 > 2 * mc.MT_RING and 300 > 4 * mc.MT_RING
    for c in (129, 300):
        assert any(lc for _, lc, _ in solved(f"chain-{c}")[5]["checks"])


@pytest.mark.parametrize("name", [n for n in mc.CASES if n.startswith("composite")])
def test_composite(name):
    b, rows, facts, erc, ects, m = solved(name)
    c = facts["rounds"]
    n = b.n_txn
    assert n == facts["n"] <= 4 * mc.MT_PREFIX and m["rounds"] == c
    r0, r1 = facts["readers"]
    assert erc[0] == 0 and (erc[r0:r1] == 2).all()
    # the readers wait in round 1 and abort in round 2
    assert m["und"][0] == (r1 - r0) + c - 1 and m["und"][1] == c - 2
    c0, c1 = facts["chain"]
    assert (erc[c0:c1] == 0).any() and (erc[c0:c1] == 2).any()
    assert (erc[c1:] == 0).all()
    # groups of more than one position among the independents
    off = b.offsets.astype(np.int64)
    assert any(np.unique(b.keys[off[t]:off[t + 1]]).size < off[t + 1] - off[t] for t in range(c1, n))
    checks = {r: (lc, pc) for r, lc, pc in m["checks"]}
    # first check: nothing aborted yet, the repeated keys alone drop > 10 %
    assert m["kept"][0] * 10 <= b.nnz * 9 and checks[1] == (False, True)
    # second check: undecided below 30 % of n, the readers' groups gone
    second = 1 + mc.MT_BATCH
    assert m["und"][second - 1] * 10 < n * 3 and checks[second] == (True, True)
    # and again as chain txns abort
    assert sum(pc for r, (lc, pc) in checks.items() if r > second) >= 1
    if rows is not None:
        assert int(ects.max()) >= 1 << 32 and int(rows[2].min()) >= 1 << 32


@pytest.mark.parametrize("kind", mc.WIDE_KINDS)
def test_wide_ts(kind):
    b, rows, facts, erc, ects, m = solved(f"wide_ts-{kind}")
    assert int(ects.max()) >= facts["min_max_cts"] == 1 << 32
    assert 0.2 < (erc == 0).mean() < 0.5
    lo, hi = {"lo32": (1 << 32, (1 << 32) + 50), "hi62": (1 << 62, (1 << 62) + 50), "full": (0, 1 << 62)}[kind]
    for v in rows[1:]:
        assert lo <= int(v.min()) and int(v.max()) < hi
    if kind == "full":
        assert int(rows[2].max()) >= 1 << 61
    # commit timestamps that differ only above bit 31, and only below it
    c = ects[erc == 0]
    assert np.unique(c >> np.uint64(32)).size >= (1 if kind != "full" else 100)
    assert np.unique(c & np.uint64(0xFFFFFFFF)).size > 10


def test_prefix_gate():
    b0, rows0, _, erc0, ects0, m0 = solved("prefix_gate-4096")
    b1, rows1, _, erc1, ects1, m1 = solved("prefix_gate-4097")
    assert b0.n_txn == 4 * mc.MT_PREFIX and b1.n_txn == 4 * mc.MT_PREFIX + 1
    assert not mc.takes_prefix(b0) and mc.takes_prefix(b1)
    assert np.array_equal(b0.keys, b1.keys[:-1]) and np.array_equal(b0.offsets, b1.offsets[:-1])
    assert np.array_equal(erc0, erc1[:-1]) and np.array_equal(ects0, ects1[:-1]) and erc1[-1] == 0
    assert 0 < m1["nsurv"] < 3 * mc.MT_PREFIX + 1 and m1["surv_rounds"] > 1
    assert int(ects1.max()) >= 1 << 32


def test_prefix_small_cap():
    b0, _, f0, erc0, _, m0 = solved("prefix_small_cap-16384")
    b1, _, f1, erc1, _, m1 = solved("prefix_small_cap-16385")
    assert m0["mp"] == f0["mp"] == mc.MS_MAXPOS and m1["mp"] == f1["mp"] == mc.MS_MAXPOS + 1
    for b, erc, m in ((b0, erc0, m0), (b1, erc1, m1)):
        P = mc.MT_PREFIX
        assert b.n_txn == P + 3200
        assert m["prefix_rounds"] > 1 and (erc[:P] == 0).any() and (erc[:P] == 2).any()
        # the filter kills some later txns, the survivors' rounds abort more
        killed = 3200 - m["nsurv"]
        assert killed > 100 and m["surv_rounds"] > 1
        assert int((erc[P:] == 2).sum()) > killed


def test_prefix_chain():
    _, _, _, erc0, _, m0 = solved("prefix_chain-0")
    _, _, _, erc1, _, m1 = solved("prefix_chain-1")
    P = mc.MT_PREFIX
    assert erc0[P - 1] != erc1[P - 1], "the decision of txn 1,023 flips with the shift"
    assert erc0[P - 1] == 2 and erc1[P - 1] == 0
    assert P in m0["survivors"] and P not in m1["survivors"]
    assert m0["prefix_rounds"] == P and m1["prefix_rounds"] == P - 1
    assert m0["surv_rounds"] >= 1200 - P and m1["surv_rounds"] >= 1200 - P - 1
    b, rows, _, erc, ects, m = solved("prefix_chain-1-wide")
    assert m["prefix_rounds"] == P - 1 and m["surv_rounds"] >= 1200 - P - 1
    assert int(ects.max()) >= 1 << 61 and (erc[1:1201] == 2).any()


def test_prefix_two_rows():
    b, rows, facts, erc, ects, m = solved("prefix_two_rows")
    for t, c in facts["cts"].items():
        assert erc[t] == 0 and ects[t] == c
    X, X2 = facts["abort"], facts["commit"]
    assert erc[X] == 2 and erc[X2] == 0 and X >= mc.MT_PREFIX and X2 >= mc.MT_PREFIX
    assert X not in m["survivors"] and X2 in m["survivors"]
    # X with either of its rows alone commits
    off = b.offsets.astype(np.int64)
    for drop in (0, 1):
        keep = np.ones(b.nnz, bool)
        keep[off[X] + drop] = False
        lens = np.diff(off)
        lens[X] -= 1
        o2 = np.zeros(b.n_txn + 1, np.uint32)
        o2[1:] = np.cumsum(lens)
        one = type(b)(o2, b.keys[keep], b.acctype[keep])
        assert orc.maat(one, *rows)[0][X] == 0


def test_prefix_filter_boundary():
    P = mc.MT_PREFIX
    b0, rows0, f0, erc0, ects0, m0 = solved("prefix_filter_boundary-0")
    b1, rows1, f1, erc1, ects1, m1 = solved("prefix_filter_boundary-1")
    for f, erc, ects in ((f0, erc0, ects0), (f1, erc1, ects1)):
        for t, c in f["cts"].items():
            assert t < P and erc[t] == 0 and ects[t] == c
    # L = 11 against U = 11: killed by the filter, no survivor rounds at all
    assert (erc0[P:] == 2).all() and m0["nsurv"] == f0["nsurv"] == 0 and m0["surv_rounds"] == 0
    assert mc.expected_rounds("prefix_filter_boundary-0") == m0["prefix_rounds"] == 1
    # against U = 12: all survive, the first commits at 11
    assert m1["nsurv"] == f1["nsurv"] == b1.n_txn - P and m1["surv_rounds"] >= 2
    assert erc1[P] == 0 and ects1[P] == 11 and (erc1[P + 1:] == 2).all()


def test_prefix_no_survivors():
    b, rows, facts, erc, ects, m = solved("prefix_no_survivors")
    assert (erc[mc.MT_PREFIX:] == 2).all() and (erc[:mc.MT_PREFIX] == 0).all()
    assert m["nsurv"] == facts["nsurv"] == 0 and m["surv_rounds"] == 0


def test_prefix_empty():
    b, rows, facts, erc, ects, m = solved("prefix_empty")
    assert m["mp"] == facts["mp"] == 0 and b.n_txn == 4 * mc.MT_PREFIX + 1
    assert (erc[:mc.MT_PREFIX] == 0).all() and (ects[:mc.MT_PREFIX] == 1).all()
    later = erc[mc.MT_PREFIX:]
    assert (later == 0).any() and (later == 2).any() and m["nsurv"] == later.size and m["surv_rounds"] > 2


def test_prefix_false_positives():
    b, rows, facts, erc, ects, m = solved("prefix_false_positives")
    assert np.unique(b.keys).size == b.nnz == mc.MT_PREFIX * 16 + 3100 * 4
    assert m["mp"] == mc.MS_MAXPOS and m["nsurv"] == facts["nsurv"] == 3100
    assert (erc == 0).all() and (ects == 1).all()
    # 16,384 rows set some 6 % of the 2^18 presence bits
    assert 0.05 < 1 - np.exp(-mc.MS_MAXPOS / float(1 << 18)) < 0.07


def test_long_row():
    b, rows, facts, erc, ects, m = solved("long_row")
    w1, w2 = facts["w1"], facts["w2"]
    assert erc[w1] == 0 and int(ects[w1]) == facts["w1_cts"] == (1 << 33) + 4301
    assert erc[w2] == 2
    after = erc[w1 + 1:w2]
    assert after.size > 50 and (after == after[0]).all()
    i = np.arange(w1)
    assert (erc[:w1] == 0).all() and np.array_equal(ects[:w1], (np.uint64(1 << 33) + i + 1).astype(np.uint64))
    # H's group: one row start, longer than one look-back window of 64 tiles
    hot = b.keys == b.keys[0]
    assert int(hot.sum()) == facts["h_positions"] > 64 * mc.MT_TILE
    assert w1 * 63 >= 66 * mc.MT_TILE


def test_long_row_small_replay():
    """The same shape at 600 txns."""
    b, rows, facts = mc.long_row(600, 500)
    erc, ects, _ = orc.maat(b, *rows)
    lrc, lcts, _ = orc.maat(b, *rows, literal=True)
    assert np.array_equal(erc, lrc) and np.array_equal(ects, lcts)
    assert erc[500] == 0 and int(ects[500]) == (1 << 33) + 501 and erc[599] == 2


def test_random_shaped_batches_stay_below_the_ring():
    """The gap these cases close: batches of test_gpu_maat.test_random's shape
    need far fewer rounds than the MT_RING counters, so the ring's wrap, a
    second batch of rounds and repeated compaction were reached by chance only."""
    rng = np.random.default_rng(7)
    for it in range(3):
        nk = int(rng.integers(1, 1500))
        b = random_batch(rng, int(rng.integers(1000, 2000)), int(rng.integers(1, 64)), nk,
                         p_write=float(rng.random()), types=(RD, WR), unique=bool(it % 2))
        rk = np.arange(nk, dtype=np.uint64)
        rows = (rk, rng.integers(0, 100, size=nk).astype(np.uint64), rng.integers(0, 100, size=nk).astype(np.uint64))
        m = mc.model(b, rows)
        erc, ects, _ = orc.maat(b, *rows)
        assert np.array_equal(m["state"] == mc.COM, erc == 0) and np.array_equal(m["cts"], ects)
        assert m["rounds"] < mc.MT_RING


def _const(text, name):
    m = re.search(r"constexpr\s+uint(?:32|64)_t\s+(?:\w+\s*=\s*[^,;]+,\s*)*" + name + r"\s*=\s*([^,;]+)[,;]", text)
    assert m, f"{name} not found"
    return m.group(1).strip()


def test_constants_match_engine():
    """A retune of the driver moves the seams: the cases must move with it."""
    read = lambda f: open(os.path.join(CSRC, f)).read()
    maat, occ, dev, rowtab = read("maat.hip"), read("occ_kernels.h"), read("dcc_device.h"), read("rowtab.h")
    items = int(_const(maat, "MT_ITEMS"))
    assert _const(maat, "MT_TILE") == "256 * MT_ITEMS" and 256 * items == mc.MT_TILE
    ms_t, ms_items = int(_const(maat, "MS_T")), int(_const(maat, "MS_ITEMS"))
    assert _const(maat, "MS_MAXPOS") == "MS_T * MS_ITEMS" and ms_t * ms_items == mc.MS_MAXPOS
    assert _const(maat, "MS_MAXTXN") == "MS_T" and ms_t == mc.MT_PREFIX
    for name, text in (("MT_PREFIX", maat), ("MT_RING", maat), ("MT_BATCH", maat), ("MAX_TXN_LEN", occ),
                       ("MT_WALK", dev), ("RT_MIN_BITS", rowtab)):
        got = int(_const(text, name))
        assert got == getattr(mc, name), (
            f"{name} is {got} in the engine but {getattr(mc, name)} in maat_cases.py: "
            "rebuild the cases around the new seam")
    assert "n > 4 * prefix" in maat
