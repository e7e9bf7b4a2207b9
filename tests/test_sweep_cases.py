"""CPU checks of the sweep edge-case builders (sweep_cases.py): every fact a
case claims -- |C0|, the positives in front of the deciding txn, the survivor
counts, the opposite decisions of the chained pairs -- holds against the
oracle's serial replay alone, so a case cannot silently stop forcing its
branch; and the constants the cases are built on are the engine's."""
import functools
import os
import re

import numpy as np
import pytest

import _oracle as orc
import sweep_cases as sc
from deneva_amd import KEY_RESERVED, WR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva_amd", "csrc")


@functools.lru_cache(maxsize=None)
def built(name, *args):
    b, facts = getattr(sc, name)(*args)
    return b, facts, orc.occ(b)[0]


def level0(b, erc):
    """From the oracle's decisions alone: C0 (the distinct write keys of the
    committed txns of the serial range), the accesses that touch it, and the
    txns that survive the level-0 filter."""
    n = b.n_txn
    lens = np.diff(b.offsets.astype(np.int64))
    owner = np.repeat(np.arange(n), lens)
    c0 = np.unique(b.keys[(owner < sc.P0) & (b.acctype == WR) & (erc[owner] == 0)])
    hit = np.isin(b.keys, c0)
    touched = np.bincount(owner[hit], minlength=n) > 0
    hasw = np.bincount(owner[b.acctype == WR], minlength=n) > 0
    surv = (np.arange(n) >= sc.P0) & ~touched & (lens > 0)
    return c0, hit, surv, hasw, lens


def check_common(b, facts, erc):
    c0, hit, surv, hasw, lens = level0(b, erc)
    assert b.n_txn >= sc.P0 and int(b.offsets[sc.P0]) <= sc.L0_BUDGET, "the serial range is not 1,024 txns"
    assert (erc[:sc.P0] == 0).all(), "a head txn aborts"
    assert c0.size == facts["c"]
    assert lens.max() <= sc.MAX_LEN
    assert not (b.keys == np.uint64(KEY_RESERVED)).any()
    assert int(surv.sum()) == facts["surv"]
    assert int((surv & ~hasw).sum()) == facts["ro"]
    # killed txns abort, and nothing but the survivors is left to level 1
    body = np.arange(b.n_txn) >= sc.P0
    assert (erc[body & ~surv & (lens > 0)] == 2).all()
    assert (erc[body & (lens == 0)] == 0).all()
    for bk, bc in facts["pairs"]:
        assert surv[bk] and surv[bc]
        assert erc[bk] == 2 and erc[bc] == 0, f"pair ({bk}, {bc}) decided {erc[bk]}, {erc[bc]}"
    return c0, hit, surv, hasw, lens


@pytest.mark.parametrize("c", sc.XCAP_C)
def test_xcap(c):
    b, facts, erc = built("xcap_case", c)
    c0, hit, surv, hasw, lens = check_common(b, facts, erc)
    assert len(facts["pairs"]) >= 16
    owner = np.repeat(np.arange(b.n_txn), lens)
    body_hit = hit & (owner >= sc.P0)
    # every key of C0 is the only reason of some kill, as a first, a middle
    # and a last access, and as a txn's only write
    per_txn = np.bincount(owner[body_hit], minlength=b.n_txn)
    sole = body_hit & (per_txn[owner] == 1)
    assert np.unique(b.keys[sole]).size == c
    assert np.unique(b.keys[sole & hasw[owner]]).size == c, "every key kills a write txn alone"
    assert (sole & ~hasw[owner]).any()
    rel = np.arange(b.nnz) - b.offsets[owner].astype(np.int64)
    assert (sole & (rel == 0) & (lens[owner] > 2)).any()
    assert (sole & (rel == lens[owner] - 1) & (lens[owner] > 2)).any()
    assert (sole & (rel > 0) & (rel < lens[owner] - 1)).any()
    assert (sole & (b.acctype == WR)).any()
    assert (lens[sc.P0:] == 0).any()


def positives_before(b, hit, tile, txn):
    lo = int(b.offsets[sc.P0 + tile * sc.SW_T])
    assert sc.P0 + tile * sc.SW_T <= txn < sc.P0 + (tile + 1) * sc.SW_T
    return int(hit[lo:int(b.offsets[txn])].sum())


@pytest.mark.parametrize("variant,per,c", [(v, 8, c) for v in sc.STASH_VARIANTS for c in (sc.F_XCAP, sc.F_XCAP + 1)]
                         + [("over", 16, sc.F_XCAP)])
def test_stash(variant, per, c):
    b, facts, erc = built("stash_case", variant, per, c)
    c0, hit, surv, hasw, lens = check_common(b, facts, erc)
    d = facts["txn"]
    before = positives_before(b, hit, facts["tile"], d)
    assert before == facts["positives"]
    if variant == "over":
        assert before >= sc.F_STASH + 32
        # a txn's hot accesses lie on both sides of positive 255 / 256
        t = sc.P0
        while positives_before(b, hit, 0, t + 1) <= sc.F_STASH - 1:
            t += 1
        assert positives_before(b, hit, 0, t) < sc.F_STASH - 1 and positives_before(b, hit, 0, t + 1) > sc.F_STASH
    else:
        assert before == {"at256": sc.F_STASH, "at257": sc.F_STASH + 1}[variant]
        assert hit[int(b.offsets[d])], "the deciding txn's first access is the positive"
    assert erc[d] == 2
    # deciding txns behind it: killed at their last access, and survivors
    last = sc.P0 + sc.SW_T
    after = np.arange(d + 1, last)
    assert (surv[after]).any() and len(facts["pairs"]) >= 4
    assert any(hit[int(b.offsets[t + 1]) - 1] and hit[int(b.offsets[t]):int(b.offsets[t + 1])].sum() == 1
               for t in after if lens[t] > 1)
    # the workgroup's next wave: a tile of cold survivors only, > 1,024 accesses
    assert surv[last:last + sc.SW_T].all()
    assert int(b.offsets[last + sc.SW_T]) - int(b.offsets[last]) > sc.ROUND


@pytest.mark.parametrize("c", [sc.F_XCAP, sc.F_XCAP + 1])
def test_wide_tile(c):
    b, facts, erc = built("wide_tile_case", c)
    c0, hit, surv, hasw, lens = check_common(b, facts, erc)
    spans = set()
    for t in facts["tiles"]:
        t0 = sc.P0 + t["tile"] * sc.SW_T
        lo, hi = int(b.offsets[t0]), int(b.offsets[t0 + sc.SW_T])
        assert sc.ROUND < hi - lo <= sc.SW_WA
        spans.add(hi - lo)
        # the hot key sits at the named tile accesses and nowhere else
        assert np.array_equal(np.nonzero(hit[lo:hi])[0], np.sort(np.asarray(t["targets"])))
        assert int(surv[t0:t0 + sc.SW_T].sum()) == sc.SW_T - np.unique(
            np.searchsorted(b.offsets[t0:t0 + sc.SW_T + 1].astype(np.int64) - lo, t["targets"], side="right")).size
    assert sc.SW_WA in spans and min(spans) < sc.ROUND + 64 * 2
    targets = {x for t in facts["tiles"] for x in t["targets"]}
    assert {sc.ROUND - 1, sc.ROUND, sc.SW_WA - 1} <= targets
    # killed txns lying across a 64-access word and across the register round
    off = b.offsets.astype(np.int64)
    across_word = across_round = False
    for t in facts["tiles"]:
        t0 = sc.P0 + t["tile"] * sc.SW_T
        for q in range(t0, t0 + sc.SW_T):
            if surv[q]:
                continue
            s, e = off[q] - off[t0], off[q + 1] - off[t0] - 1
            across_word |= (s >> 6) != (e >> 6)
            across_round |= s < sc.ROUND <= e
    assert across_word and across_round
    assert len(facts["pairs"]) >= 2 * len(facts["tiles"])


@pytest.mark.parametrize("L", sc.LIST_SEAMS)
def test_list_seam(L):
    b, facts, erc = built("list_seam_case", L)
    c0, hit, surv, hasw, lens = check_common(b, facts, erc)
    assert b.n_txn == sc.P0 + L
    assert not surv[sc.P0:].all()
    if L >= 63:
        assert (lens[sc.P0:] == 0).any() and surv.any() and facts["pairs"]
        assert set(range(1, 11)) <= set(lens[sc.P0:].tolist())


@pytest.mark.parametrize("extra", [0, 64])
@pytest.mark.parametrize("n_cu", [4, 256])
def test_grid_seam(n_cu, extra):
    b, facts, erc = built("grid_seam_case", n_cu, extra)
    c0, hit, surv, hasw, lens = check_common(b, facts, erc)
    grid = 4 * n_cu
    n64 = (b.n_txn - sc.P0 + 63) // 64
    assert max(-(-n64 // grid), sc.SW_CHUNK // 64) == (5 if extra else 4)
    assert n64 == 4 * grid + (1 if extra else 0) and (b.n_txn - sc.P0) % 64 == 0
    assert (lens[sc.P0:] == 1).all()
    assert 4 * facts["surv"] <= b.n_txn and len(facts["pairs"]) >= 64
    assert facts["ro"] > 0 and facts["surv"] - facts["ro"] > 0


@pytest.mark.parametrize("split,s", [(sp, s) for sp in (1, 0) for s in sc.TAIL_S[sp]])
def test_tail_seam(s, split):
    b, facts, erc = built("tail_seam_case", s, split)
    c0, hit, surv, hasw, lens = check_common(b, facts, erc)
    assert int((surv & hasw).sum()) == s
    assert (facts["ro"] > 0) == bool(split)
    # level 1 aborts some of the chain, also behind every serial range in use
    w = np.nonzero(surv & hasw)[0]
    assert (erc[w] == 2).any() and (erc[w] == 0).any()
    # far below the level's access budget (16 accesses per txn of its serial
    # range), so the serial pass ends at p_max(1) and not before
    assert int(lens[w].sum()) <= 8 * s


@pytest.mark.parametrize("r", sc.RO_SEAMS)
def test_ro_seam(r):
    b, facts, erc = built("ro_seam_case", r)
    c0, hit, surv, hasw, lens = check_common(b, facts, erc)
    assert int((surv & ~hasw).sum()) == r == facts["r"]
    assert int((surv & hasw).sum()) == 48
    if r >= 63:
        # read-only and write survivors share tiles; both decisions occur
        ro = np.nonzero(surv & ~hasw)[0]
        assert (erc[ro] == 2).any() and (erc[ro] == 0).any()
        tiles_ro = set(((ro - sc.P0) // sc.SW_T).tolist())
        tiles_w = set(((np.nonzero(surv & hasw)[0] - sc.P0) // sc.SW_T).tolist())
        assert len(tiles_ro & tiles_w) >= 2
        assert len(facts["pairs"]) >= 8


def _const(text, name):
    m = re.search(r"(?:constexpr\s+uint32_t|#define)\s+" + name + r"\s*=?\s*(\d+)", text)
    assert m, f"{name} not found"
    return int(m.group(1))


def test_constants_match_engine():
    """A retune of the filter moves the seams: the cases must move with it."""
    with open(os.path.join(CSRC, "occ_sweep.hip")) as f:
        sweep = f.read()
    with open(os.path.join(CSRC, "occ_kernels.h")) as f:
        hdr = f.read()
    for name, text in (("F_STASH", sweep), ("DCC_F_XS", sweep), ("FK", sweep), ("SW_CHUNK", hdr),
                       ("SW_WA", hdr), ("SW_T", hdr), ("SW_PL", hdr)):
        got = _const(text, name)
        assert got == getattr(sc, name), (
            f"{name} is {got} in the engine but {getattr(sc, name)} in sweep_cases.py: "
            "rebuild the cases around the new seam")
