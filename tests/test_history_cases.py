"""CPU checks of the directed history cases (history_cases.py): the plain
predicate and the plain commit rule agree with the literal oracle on every
step of every scenario, the placed keys have the homes and bitmap bits they
claim at every table size the case can meet, the structural claims (which
level holds how many pairs, when a merge happens, how big the tables are and
how often an overflowing one is rebuilt) hold in numbers, and the reads reach
every resolution path of hist_hit with a hit and with a miss."""
import os
import re

import numpy as np
import pytest

import _oracle as orc
import history_cases as hc
import rowtab_cases as rt
from deneva_amd import KEY_RESERVED
from deneva_amd._abi import RC_ABORT, RC_RCOK


def test_constants_and_rules_are_the_engine_s():
    assert hc.HASH_MUL == rt.FIB, "the history's home is no longer ProbeFib's: keys_with_home does not place its keys"
    assert hc.BM_MUL % 2 == 1 and (hc.BM_MUL * hc.BM_MUL_INV) & hc.M64 == 1
    hdr = open(os.path.join(hc.CSRC, "occ_history.h")).read()
    # the three walks that must agree on HIST_WALK slots from home
    assert "for (uint32_t i = 0; i < HIST_WALK; i++)" in hdr          # hist_level_hit
    assert "if (i == HIST_WALK) {" in hdr                              # hist_insert
    hip = open(os.path.join(hc.CSRC, "occ_history.hip")).read()
    assert "if (w == HIST_WALK) atomicOr(over, 1u);" in hip            # k_hist_heads
    assert "for (uint32_t it = 1; it < HIST_WALK; it++)" in open(os.path.join(hc.CSRC, "occ_kernels.hip")).read()
    assert re.search(r"constexpr uint32_t HB = 1024;", hip) and re.search(r"constexpr uint32_t FIN_TXN_WG = 2048;", hip)
    ctx = open(os.path.join(hc.CSRC, "dcc_ctx.hip")).read()
    assert "if (D.m > std::max<uint64_t>(hist_merge_min, B.m / 4)) {" in ctx
    assert "return e && atoi(e) >= 2 ? (uint64_t)atoi(e) : 4ull;" in ctx            # slots per pair
    assert "need = std::max<uint64_t>({need, 65536," in ctx
    assert "4 * (std::max<uint64_t>(hist_merge_min, hs[0].m / 4) + h.last_app)});" in ctx
    assert "if (h.overflowed) need = std::max<uint64_t>(need, 4ull << h.hbits);" in ctx
    assert "h.hbits = 4;" in ctx
    assert hc.base_bits(64) == 8 and hc.base_bits(65) == 9 and hc.base_bits(1) == 4 and hc.base_bits(10) == 6
    assert hc.delta_bits(0, 4096, 0, 64) == 16 and hc.delta_bits(0, 1 << 22, 0, 0) == 24
    assert hc.merges(9, 0, 8) and not hc.merges(8, 0, 8) and hc.merges(26, 100, 8) and not hc.merges(25, 100, 8)


def test_bitmap_keys():
    for bit in (0, 1, 0x1ABCD, (1 << hc.HIST_BM_LOG) - 1):
        k = hc.keys_with_bm_bit(bit, 50, seed=bit + 1)
        assert np.unique(k).size == 50 and all(hc.bm_bit(x) == bit for x in k)
        assert KEY_RESERVED not in k.tolist()
        k2 = hc.keys_with_bm_bit(bit, 5, seed=bit + 1, avoid=k[:5])
        assert not set(k2.tolist()) & set(k[:5].tolist())
    ks = rt.keys_with_home("fib", 77, 16, 30, 18, 2)
    a = hc.key_with_home_and_bit(77, 16, 18, 2, ks, ks)
    assert a not in ks.tolist() and hc.bm_bit(a) in {hc.bm_bit(x) for x in ks}
    assert all(rt.home("fib", a, b) == rt.home("fib", ks[0], b) for b in range(4, 19))


def test_edge_windows_have_the_stated_relations():
    for tns in ([10, 20, 30], [20], [1], [(1 << 33) + 5, (1 << 33) + 6]):
        w = set(hc.edge_windows(tns))
        t0, t1 = min(tns), max(tns)
        for t in tns:
            assert {(t - 1, t - 1), (t - 1, t), (t, t - 1), (t, t)} <= w
        assert any(hi < t0 for lo, hi in w) and any(lo == hi for lo, hi in w) and any(lo > hi for lo, hi in w)
        assert any(lo == t1 and hi > lo for lo, hi in w) and any(lo > t1 for lo, hi in w)
        for a, b in zip(sorted(tns), sorted(tns)[1:]):
            assert (a, b - 1) in w  # opens on one tn, ends below the next
        hit = [any(lo < t <= hi for t in tns) for lo, hi in w]
        assert any(hit) and not all(hit)


def walk(sc, on_step):
    """Run a scenario through the plain model, the level restatement and the
    literal oracle."""
    m, lv = hc.Model(), hc.Levels()
    for i, st in enumerate(sc.steps):
        where = f"{sc.name} step {i} ({type(st).__name__})"
        hk = np.array([k for k, _ in m.pairs], np.uint64)
        ht = np.array([t for _, t in m.pairs], np.uint64)
        new = ()
        if isinstance(st, hc.Reads):
            lv.apply(st)
            reads = m.reads_of(st)
            assert 0 < len(reads) <= 4000, where
            b, top = hc.read_batch(reads)
            want = m.read_rc(reads)
            if st.snapshot:
                got = orc.occ_snapshot(b, np.zeros(b.n_txn + 1, np.uint32), np.zeros(0, np.uint32), top, hk, ht)
            else:
                got, tn, tnc = orc.occ(b, hist_keys=hk, hist_tn=ht, tnc=m.tnc, literal=True)
                assert tnc == m.tnc and not tn.any(), where
            assert np.array_equal(got, want), where
            on_step(st, m, lv, reads, want)
            continue
        if isinstance(st, hc.Write):
            assert 0 < len(st.txns) <= 4000, where
            b = hc.write_batch(st.txns)
            tnc0 = m.tnc
            erc, etn, etnc = orc.occ(b, hist_keys=hk, hist_tn=ht, tnc=tnc0, literal=True)
            rc, tn, new = m.write(st.txns)
            assert np.array_equal(rc, erc) and np.array_equal(tn, etn) and m.tnc == etnc, where
        else:
            m.apply(st)
        lv.apply(st, new)
        assert sorted(lv.B + lv.D) == sorted(m.pairs), where
        on_step(st, m, lv, None, None)
    return m, lv


@pytest.mark.parametrize("name", hc.NAMES)
def test_scenario(name):
    sc = hc.scenario(name)
    seen = {"rc": set(), "expects": 0}

    def on_step(st, m, lv, reads, want):
        if reads is not None:
            seen["rc"] |= set(want.tolist())
        if isinstance(st, hc.Expect):
            seen["expects"] += 1
            have = dict(base=len(lv.B), run=len(lv.run) + len(lv.flat), chain=len(lv.chain), merges=lv.n_merges,
                        bbits=lv.bbits(), dbits=lv.dbits())
            for f, v in have.items():
                assert getattr(st, f) in (None, v), f"{name}: {f} is {v}, the case claims {getattr(st, f)}"
            if st.chain is not None or st.run is not None:
                assert not lv.flat or st.chain is None, f"{name}: pairs await a rebuild"
        if isinstance(st, hc.Write) and not st.defer:
            # a push overflows iff the delta's table then holds a key HIST_WALK from home
            keys = list(dict.fromkeys(k for k, _ in lv.D))
            assert (hc.farthest(keys, lv.dbits()) >= hc.HIST_WALK) == st.overflow, name
            assert lv.merge_min <= 4096 or not st.overflow

    walk(sc, on_step)
    assert seen["rc"] == {RC_ABORT, RC_RCOK}, "both RCs must occur"
    assert seen["expects"] > 0
    keys = {k for st in sc.steps for k in getattr(st, "keys", [])}
    assert KEY_RESERVED not in keys
    for ks, first, sizes in sc.clusters:
        assert len(set(ks)) == len(ks)
        assert hc.rebuild_sizes(ks, first) == sizes, f"{name}: a cluster of {len(ks)} is built at {sizes}"
        assert hc.rebuild_sizes(ks[::-1], first) == sizes
        for seed in range(20):  # whatever the order of arrival
            assert hc.rebuild_sizes([ks[i] for i in np.random.default_rng(seed).permutation(len(ks))], first) == sizes
        for b in range(4, (sizes[-2] if len(sizes) > 1 else first) + 1):
            assert len({rt.home("fib", k, b) for k in ks}) == 1, f"{name}: the homes differ at 2^{b} slots"
        assert (32 << sizes[-1]) <= (32 << 20), "no table above 32 MiB"
    if sc.last_slot:
        assert len(set(sc.last_slot)) == len(sc.last_slot)
        for b in range(4, 21):
            assert {rt.home("fib", k, b) for k in sc.last_slot} == {(1 << b) - 1}


def test_walk_bound_cases_sit_on_the_bound():
    """64 keys of one home fill the walk exactly (the last one HIST_WALK - 1
    from home, found by the probe's last step); the 65th is one past it; an
    absent key of the home passes the bitmap and walks the whole bound."""
    for name, bits in (("walk_push", 16), ("walk_build_delta", 16), ("walk_build_base", 8)):
        sc = hc.scenario(name)
        full, over = sc.clusters[0][0], sc.clusters[1][0]
        assert len(full) == hc.HIST_WALK and len(over) == hc.HIST_WALK + 1 and over[:hc.HIST_WALK] == full
        assert hc.farthest(full, bits) == hc.HIST_WALK - 1
        assert hc.farthest(over, sc.clusters[1][1]) == hc.HIST_WALK
        reads = [st for st in sc.steps if isinstance(st, hc.Reads)]
        absent = [k for k in reads[0].keys if k not in over]
        assert len(absent) == 1
        assert rt.home("fib", absent[0], bits) == rt.home("fib", full[0], bits)
        assert hc.bm_bit(absent[0]) in {hc.bm_bit(k) for k in full}


def test_bitmap_case_shares_bits():
    sc = hc.scenario("bitmap")
    keys = sc.steps[2].keys
    assert len({hc.bm_bit(k) for k in keys[:5]}) == 1 and len(set(keys[:5])) == 5
    assert hc.bm_bit(keys[5]) != hc.bm_bit(keys[0])
    # absent from both levels, in the base only, in the delta only -- at some read of the case
    state = set()

    def on_step(st, m, lv, reads, want):
        if reads is None:
            return
        b, dl = {k for k, _ in lv.B}, {k for k, _ in lv.D}
        for k in keys[:5]:
            others = (b | dl) - {k}
            if any(hc.bm_bit(o) == hc.bm_bit(k) for o in others):
                state.add("absent" if k not in b | dl else "base" if k not in dl else "delta" if k not in b else "both")
    walk(sc, on_step)
    assert {"absent", "base", "delta"} <= state


def test_reads_reach_every_path_with_a_hit_and_a_miss():
    got = set()
    for sc in hc.SCENARIOS:
        if not sc.paths:
            continue

        def on_step(st, m, lv, reads, want):
            if reads is None or st.snapshot:
                return
            for (k, lo, hi), rc in zip(reads, want):
                p = lv.paths(k, lo, hi)
                assert (rc == RC_ABORT) == any(h for _, _, h in p), (sc.name, k, lo, hi, p)
                if hi > lo:  # an empty window is answered before the history is read
                    got.update(p)
        walk(sc, on_step)
    want = {(lv, stage, hit) for lv, stage in (("base", "tmax"), ("base", "run"), ("delta", "tmax"),
                                               ("delta", "chain"), ("delta", "run")) for hit in (False, True)}
    assert want <= got, f"paths never taken: {sorted(want - got)}"
    # the split case has windows that the newer level's tmax does not answer and only the base hits
    sc = hc.scenario("edges_split")
    only_base = []

    def on_step(st, m, lv, reads, want):
        if reads is not None and not st.snapshot:
            for k, lo, hi in reads:
                p = lv.paths(k, lo, hi)
                if len(p) >= 2 and p[0][0] == "delta" and not p[0][2] and p[0][1] != "tmax" and p[-1] == ("base", "tmax", True):
                    only_base.append((lo, hi))
    walk(sc, on_step)
    assert only_base
