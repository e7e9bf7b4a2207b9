"""CPU proofs of the wave walk's directed cases (calvin_wave_cases.py): every
fact the GPU test (test_gpu_calvin_wave_edges.py) relies on holds by the oracle
and the model alone.  For every batch: classify() finds each probe's carrier
and reader in the classes the case was built for, the oracle gives the reader
wave D + 1, the reader's wave drops with the carrier's request removed (the
probed path carries the strict maximum), and the literal Row_lock replay
equals the formula.  The coverage of the grid is asserted, not assumed."""
import numpy as np
import pytest

import _oracle as orc
import calvin_wave_cases as cw
from deneva_amd import GROUP_NONE


@pytest.fixture(scope="module")
def solved():
    """name -> (case, oracle groups, rc, waves, classes), computed once."""
    memo = {}

    def get(name):
        if name not in memo:
            c = cw.build(name)
            g, rc, w = orc.calvin(c.batch)
            memo[name] = (c, g, rc, w, cw.classify(c.batch, g))
        return memo[name]
    return get


def test_plan_geometry():
    # cw_plan at the two slot widths, and the dataflow grid above CW_LMAX
    assert cw.plan(1, 1) == cw.Plan(4, 960, 15360, 1, False)
    assert cw.plan(1, 16).lg == 4 and cw.plan(1, 17) == cw.Plan(5, 384, 12288, 1, False)
    assert cw.plan(7681, 16) == cw.Plan(4, 960, 15360, 9, True)
    assert cw.plan(10, 32).lg == 5 and cw.plan(10, 33) is None and cw.plan(0, 4) is None
    assert cw.plan(10, 0) is None


NCH = {"1": 1, "63": 1, "64": 1, "65": 1, "191": 1, "192": 1, "193": 1, "C-1": 1, "C": 1, "C+1": 2,
       "2C": 2, "2C+1": 3, "3C": 3, "3C+1": 4, "4C+65": 5}
# One probe of every (own, previous) class pair that fits.  One sub-chunk:
# (sub, sub).  65 txns: the second sub-chunk's only txn reads, (sub, chunk) too.
# Three sub-chunks and more: the four same-chunk pairs.  Two chunks: those, two
# with the reader and two with A in the next chunk.  Three: 4 + 4 + the five of
# span two.  Five: all 25 but the three that span five or six chunks.  A last
# chunk of one txn serves as one more reader.
N_PROBES = {"1": 0, "63": 1, "64": 1, "65": 2, "191": 4, "192": 4, "193": 4, "C-1": 4, "C": 4, "C+1": 5,
            "2C": 8, "2C+1": 9, "3C": 13, "3C+1": 14, "4C+65": 22}


@pytest.mark.parametrize("lg", [4, 5])
def test_sizes_plan_and_form(lg, solved):
    assert [s for s, _ in cw.size_list(lg)] == list(NCH)
    for label, n in cw.size_list(lg):
        c, g, rc, w, cl = solved(f"sizes-lg{lg}-{label}")
        lens = np.diff(np.asarray(c.batch.offsets, np.int64))
        assert c.batch.n_txn == n and (17 <= lens.max() <= 32 if lg == 5 else lens.max() <= 16)
        assert (cl.plan.lg, cl.plan.nch, cl.plan.helpers) == (lg, NCH[label], NCH[label] > 2), label
        assert len(c.probes) == N_PROBES[label], label
    # the last size without helper workgroups and the first with them
    C = cw.CHUNK[lg]
    assert not cw.plan(2 * C, 1 << lg).helpers and cw.plan(2 * C + 1, 1 << lg).helpers


@pytest.mark.parametrize("name", list(cw.CASES))
def test_probe_facts(name, solved):
    c, g, rc, w, cl = solved(name)
    b = c.batch
    g2, rc2, w2 = orc.calvin(b, literal=True)
    assert np.array_equal(g, g2) and np.array_equal(rc, rc2) and np.array_equal(w, w2)
    assert len({p.row for p in c.probes}) == len(c.probes)
    ds = [p.D for p in c.probes if "chain" not in p.facts]
    assert len(set(ds)) == len(ds)
    if name != "sizes-lg4-1" and name != "sizes-lg5-1":
        assert c.probes
    for p in c.probes:
        assert g[p.xm] == 0 and g[p.xa] == 0 and g[p.xt] == 1, p.name
        assert w[p.m] == p.D and w[p.t] == p.D + 1 and (p.a == p.m or w[p.a] == 0), p.name
        if cl is not None:
            got = (cw.OWN[cl.own[p.xm]], cl.own_dist[p.xm], cw.PREV[cl.prev[p.xt]], cl.prev_dist[p.xt])
            assert got == (p.own, p.own_dist, p.prev, p.prev_dist), p.name
            # the carrier publishes to the slot the reader reads: A's request
            assert cl.own_code[p.xm] == cl.code[p.xa] == cl.prev_code[p.xt], p.name
        # without the carrier's request the reader's wave falls: the path carries the maximum
        w3 = orc.calvin(cw.without_carrier(c, p))[2]
        assert w3[p.t] < p.D + 1 and w3[p.m] == p.D, p.name


@pytest.mark.parametrize("name", cw.GRID)
def test_grid_coverage(name, solved):
    c, g, rc, w, cl = solved(name)
    assert c.n == 8 * cw.CHUNK[c.lg] + 1 and cl.plan.nch == 9 and cl.plan.lg == c.lg
    got = {(cw.OWN[cl.own[p.xm]], int(cl.own_dist[p.xm]), cw.PREV[cl.prev[p.xt]], int(cl.prev_dist[p.xt]))
           for p in c.probes}
    want = set()
    for own, do in (("sub", 0), ("chunk", 0), ("+1", 1), ("+2", 2), ("far", 3), ("far", 5)):
        for prev, dp in (("sub", 0), ("chunk", 0), ("-1", 1), ("-2", 2), ("far", 3), ("far", 5)):
            if do + dp <= 7 or (do, dp) == (5, 3):  # (3, 5) and (5, 5) need a second txn in the ninth chunk
                want.add((own, do, prev, dp))
    assert got == want and len(want) == 34
    # every pair of classes, whatever the distance
    assert {(o, p) for o, _, p, _ in got} == {(o, p) for o in cw.OWN[1:] for p in cw.PREV[1:]}
    # the last chunk holds one txn, a reader
    seq = np.argsort(cw.seq_positions(c.batch))
    assert int(seq[-1]) in {p.t for p in c.probes}
    if name.endswith("seq"):
        order = np.asarray(c.batch.order)
        assert np.unique(order).size < order.size  # ties
        assert not np.array_equal(cw.seq_positions(c.batch), np.arange(c.n))
    if c.lg == 5:
        assert np.diff(np.asarray(c.batch.offsets, np.int64)).max() == 17


@pytest.mark.parametrize("lg", [4, 5])
def test_edges(lg, solved):
    c, g, rc, w, cl = solved(f"edges-lg{lg}")
    P = cl.plan
    pos = cw.seq_positions(c.batch)
    slots, t_at, roles = set(), set(), set()
    for p in c.probes:
        slot = int(cw.lds_slot(P, cl.own_code[p.xm]))
        if "lds_slot" in p.facts:
            assert slot == p.facts["lds_slot"], p.name
            assert p.prev == "-1" and pos[p.t] // P.C == pos[p.a] // P.C + 1
            slots.add(slot)
            t_at.add(int(pos[p.t] % P.C))
        if "G" in p.facts:
            G = int(pos[p.a] // cw.SUB)
            assert pos[p.a] % cw.SUB == cw.SUB - 1 and pos[p.t] == pos[p.a] + 1 and p.prev == "chunk"
            roles.add(G % 3)
        if "partial" in p.facts:
            assert pos[p.a] // P.C == P.nch - 1 and pos[p.a] // cw.SUB == (c.n - 1) // cw.SUB
            assert c.n % cw.SUB and p.prev == "sub"
    assert {0, P.H - 1, P.H, 2 * P.H - 1} <= slots
    assert {0, P.C - 1} <= t_at and roles == {0, 1, 2}


def test_compact(solved):
    c, g, rc, w, cl = solved("compact")
    seen = {}
    for p in c.probes:
        if "intra" in p.facts:
            assert cl.n_intra[p.t] == p.facts["intra"] and (p.own, p.prev) == ("sub", "sub")
            seen[("intra", int(cl.n_intra[p.t]))] = 1
        if "hot" in p.facts:
            assert cl.n_hot[p.m] == p.facts["hot"] and (p.own, p.prev) == ("sub", "sub")
            seen[("hot", int(cl.n_hot[p.m]))] = 1
        if "chain" in p.facts:  # 64 dependent txns at positions lo .. lo + 63 (index order)
            lo = p.facts["chain"]
            assert np.array_equal(w[lo:lo + 64], np.arange(64)) and p.m == lo + 63
            seen[("chain", lo // cw.SUB == (lo + 63) // cw.SUB, lo // cl.plan.C == (lo + 63) // cl.plan.C)] = 1
        if "dup" in p.facts:
            assert g[p.xm + 1] == GROUP_NONE and g[p.xt + 1] == GROUP_NONE
            seen["dup"] = 1
    assert set(seen) == {("intra", cw.CR_K), ("intra", cw.CR_K + 1), ("hot", cw.CR_K), ("hot", cw.CR_K + 1),
                         ("chain", True, True), ("chain", False, True), ("chain", False, False), "dup"}
    # no other txn overflows the compact record
    assert (cl.n_intra > cw.CR_K).sum() == 1 and (cl.n_hot > cw.CR_K).sum() == 1


def test_shapes(solved):
    C = cw.CHUNK[4]
    lens = {k: np.diff(np.asarray(solved(f"shapes-{k}")[0].batch.offsets, np.int64))
            for k in ("uniform", "empty", "seq", 16, 17, 32, 33)}
    assert (lens["uniform"] == 4).all()
    assert (lens["empty"][[0, C, 2 * C - 1, -1]] == 0).all() and (lens["empty"] == 0).sum() == 4
    assert solved("shapes-empty")[0].batch.order is None
    assert solved("shapes-seq")[0].batch.order is not None and np.unique(lens["seq"]).size > 1
    for k in (16, 17, 32, 33):
        assert lens[k].max() == k and np.unique(lens[k]).size > 1
    assert solved("shapes-16")[4].plan.lg == 4 and solved("shapes-17")[4].plan.lg == 5
    assert solved("shapes-32")[4].plan.lg == 5
    assert solved("shapes-33")[4] is None  # the dataflow grid's epoch
    for k in lens:
        assert len(solved(f"shapes-{k}")[0].probes) == 22


@pytest.mark.parametrize("lg", [4, 5])
def test_spread(lg, solved):
    c, g, rc, w, cl = solved(f"spread-lg{lg}")
    keys = np.asarray(c.batch.keys, np.uint64)
    at_chunk, read_from = set(), set()
    for p in c.probes:
        mem = np.nonzero((keys == np.uint64(p.row)) & (g == 0))[0]
        assert {int(x) for x in cl.code[mem] // cl.plan.H} == set(range(6))
        assert int(cl.code[p.xa] // cl.plan.H) == 5
        # A's slot receives maxima by the walker, both boundary adds and the helpers
        assert {cw.OWN[k] for k in cl.own[mem]} >= {"+1", "+2", "far"}
        assert {cw.OWN[k] for k in cl.own[mem]} & {"sub", "chunk"}
        at_chunk.add(int(cl.code[p.xm] // cl.plan.H))
        read_from.add(int(cl.prev_dist[p.xt]))
    assert at_chunk >= {0, 1, 2, 3} and read_from == {1, 3}
