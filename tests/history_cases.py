"""Directed cases of the device OCC history (csrc/occ_history.h, the hist_*
host code of csrc/dcc_ctx.hip): scenarios of host appends, epochs, trims and
window reads built from keys placed exactly in the levels' tables, with the
plain expected answers and a restatement of where every pair lives.

The history's home slot is hist_hash_slot: ProbeFib's multiplier and top-bits
rule, so rowtab_cases.keys_with_home("fib", ...) places keys in a level's
table (and a home at 2^b slots is the prefix of the home at any bigger size:
a cluster that shares a home at 2^16 slots shares one in every smaller table).
The bitmap hash hist_bm_bit has its own multiplier, inverted here the same way.
HIST_WALK, HIST_BM_LOG and both multipliers are read out of occ_history.h.

Expected answers are a predicate over the list of (key, tn) pairs: a window
(lo, hi) on a key hits iff the key has a pair with lo < tn <= hi.  The read
epochs are one-access RD txns, whose RC is then ABORT iff the predicate holds;
the writing epochs carry no windows, so a txn aborts iff an earlier committed
txn of the epoch wrote one of its keys, and committed writers take tnc+1...

Level sizing (dcc_ctx::hist_build), restated in base_bits / delta_bits: the
base has 4 slots per pair, at least 2^4; the delta at least 65,536 slots, or
4 * (max(merge_min, B.m / 4) + last_app) if larger; a table in which a key
landed HIST_WALK or more slots from its home is rebuilt with 4 x the slots.
The merge (dcc_ctx::hist_prepare, before every epoch that reads or appends):
D.m > max(merge_min, B.m / 4).  The overflow cases keep merge_min at 4,096 or
below, so the delta stays at 2^16 slots until it overflows and no table passes
2^20 slots (32 MiB).

Pure numpy / Python ints: no GPU."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import numpy as np

import rowtab_cases as rt
from deneva_amd import KEY_RESERVED, RD, WR
from deneva_amd._abi import RC_ABORT, RC_RCOK
from helpers import make_batch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva_amd", "csrc")
_HDR = open(os.path.join(CSRC, "occ_history.h")).read()
M64 = rt.M64
HIST_WALK = int(re.search(r"constexpr uint32_t HIST_WALK = (\d+);", _HDR).group(1))
HIST_BM_LOG = int(re.search(r"constexpr uint32_t HIST_BM_LOG = (\d+);", _HDR).group(1))
HASH_MUL = int(re.search(r"hist_hash_slot\(uint64_t key, uint32_t bits\) \{\s*return \(key \* (0x[0-9A-Fa-f]+)ull\) >> "
                         r"\(64 - bits\);", _HDR).group(1), 16)
BM_MUL = int(re.search(r"return \(uint32_t\)\(\(key \* (0x[0-9A-Fa-f]+)ull\) >> \(64 - HIST_BM_LOG\)\);",
                       _HDR).group(1), 16)
BM_MUL_INV = pow(BM_MUL, -1, 1 << 64)
MAX_TXN_LEN = int(re.search(r"constexpr uint32_t MAX_TXN_LEN = (\d+);",
                            open(os.path.join(CSRC, "occ_kernels.h")).read()).group(1))
DEFAULT_MERGE = 65536
DELTA_MIN_SLOTS = 65536


# ---------------------------------------------------------------- placed keys
def bm_bit(key):
    return ((int(key) * BM_MUL) & M64) >> (64 - HIST_BM_LOG)


def keys_with_bm_bit(bit, count, seed=1, avoid=()):
    """`count` distinct keys whose bitmap bit is `bit` (none of `avoid`)."""
    assert 0 <= bit < (1 << HIST_BM_LOG)
    free = 64 - HIST_BM_LOG
    rng = np.random.default_rng(seed)
    out, seen = [], {int(a) for a in avoid} | {KEY_RESERVED}
    while len(out) < count:
        r = int(rng.integers(0, 1 << free))
        key = (((bit << free) | r) * BM_MUL_INV) & M64
        if key not in seen:
            seen.add(key)
            out.append(key)
    return np.asarray(out, np.uint64)


def key_with_home_and_bit(h, bits, shared_bits, ext, bit_of, avoid, seed=1):
    """A key of keys_with_home("fib", h, bits, ..., shared_bits, ext)'s home
    that is none of `avoid` and shares its bitmap bit with one of the keys
    `bit_of`: absent from a history of those keys, it still passes the bitmap
    and its probe walks the cluster."""
    want = {bm_bit(k) for k in bit_of}
    avoid = {int(a) for a in avoid}
    for rnd in range(400):
        cand = rt.keys_with_home("fib", h, bits, 20000, shared_bits, ext, seed=1000 * seed + rnd)
        bitsv = (cand * np.uint64(BM_MUL)) >> np.uint64(64 - HIST_BM_LOG)
        for k in cand[np.isin(bitsv, np.fromiter(want, np.uint64))].tolist():
            if k not in avoid:
                return k
    raise AssertionError("no key of that home shares a bitmap bit")


# ---------------------------------------------------------------- sizing rules
def _bits_for(need):
    b = 4
    while (1 << b) < need:
        b += 1
    return b


def base_bits(m):
    return _bits_for(4 * m)


def delta_bits(m, merge_min, base_m, last_app):
    return _bits_for(max(4 * m, DELTA_MIN_SLOTS, 4 * (max(merge_min, base_m // 4) + last_app)))


def merges(delta_m, base_m, merge_min):
    return delta_m > max(merge_min, base_m // 4)


def farthest(keys, bits):
    """Largest distance from home of any of `keys` in a 2^bits-slot table
    filled by linear probing (the clusters here have one home and nothing
    near them; test_history_cases.py checks that the order of arrival does not
    matter for them)."""
    used, far = set(), 0
    for k in keys:
        s = rt.home("fib", k, bits)
        w = 0
        while s in used:
            s = (s + 1) & ((1 << bits) - 1)
            w += 1
        used.add(s)
        far = max(far, w)
    return far


def rebuild_sizes(keys, bits):
    """The sizes a level of `keys` is built at, from 2^bits slots: 4 x the
    slots while a key sits HIST_WALK or more from its home."""
    out = [bits]
    while farthest(keys, out[-1]) >= HIST_WALK:
        out.append(out[-1] + 2)
    return out


# ---------------------------------------------------------------- windows
def edge_windows(tns):
    """(lo, hi) around every tn of one key: hi and lo each at tn - 1 and tn
    (lo == hi and lo > hi among them), hi below every tn, lo at and above the
    largest, and between consecutive tns."""
    tns = sorted(set(int(t) for t in tns))
    w = set()
    for t in tns:
        w |= {(lo, hi) for lo in (t - 1, t) for hi in (t - 1, t)}
        w |= {(t - 1, t + 1), (t, t + 1)}
    t0, t1 = tns[0], tns[-1]
    w |= {(0, t0 - 1), (0, 0), (t0 - 1, t0 - 1), (max(t0 - 2, 0), t0 - 1)}
    w |= {(t1, t1 + 5), (t1 + 1, t1 + 9), (t1, t1), (t1 + 1, t1 + 1), (t1 - 1, t1 + 5)}
    w |= {(0, t1 + 5), (0, t1 - 1), (0, t1)}
    for a, b in zip(tns, tns[1:]):
        w |= {(a, b - 1), (a - 1, b - 1), (a, b), (a - 1, b)}
        if b - a > 2:
            w.add((a + 1, b - 1))
    return sorted(x for x in w if x[0] >= 0 and x[1] >= 0)


# ---------------------------------------------------------------- steps
@dataclass
class Opt:        # DCC_OPT_HIST_MERGE
    merge_min: int


@dataclass
class Tnc:        # the commit counter, set by the host
    value: int


@dataclass
class Append:     # dcc_occ_history_append
    keys: list
    tns: list


@dataclass
class Trim:
    floor: int


@dataclass
class Clear:
    pass


@dataclass
class Reads:      # an epoch of one-access RD txns with windows; top: through the captured snapshot
    reads: list   # (key, lo, hi), or "auto": the edge windows of `keys`
    keys: list = field(default_factory=list)
    snapshot: bool = False


@dataclass
class Write:      # an epoch without windows that appends its committed write sets
    txns: list    # lists of (key, type)
    defer: bool = False     # numbered and appended by dcc_occ_finish_epoch (k_hist_count / k_hist_emit)
    overflow: bool = False  # claim: a push lands HIST_WALK from home


@dataclass
class Expect:     # where the pairs are now (checked on the CPU against Levels)
    base: int = None
    run: int = None
    chain: int = None
    merges: int = None
    bbits: int = None
    dbits: int = None


@dataclass
class Scenario:
    name: str
    steps: list
    clusters: list = field(default_factory=list)  # (keys, first bits, the sizes the level is built at)
    last_slot: list = field(default_factory=list)  # keys homed on the last slot at 2^4 .. 2^20 slots
    paths: bool = False  # its reads count towards the path coverage


# ---------------------------------------------------------------- the plain model
class Model:
    """The history as a list of pairs, tnc, and the predicate."""

    def __init__(self):
        self.pairs = []
        self.tnc = 0

    def hit(self, key, lo, hi):
        for k, t in self.pairs:
            if k == key and lo < t <= hi:
                return True
        return False

    def tns_of(self, key):
        return sorted(t for k, t in self.pairs if k == key)

    def reads_of(self, step):
        """(key, lo, hi[, top]) of a Reads step against the pairs of now."""
        r = list(step.reads) if step.reads != "auto" else []
        far = max([t for _, t in self.pairs], default=0) + 50
        for k in step.keys:
            t = self.tns_of(k)
            r += [(k, lo, hi) for lo, hi in (edge_windows(t) if t else [(0, far), (0, 1), (far, far + 5)])]
        if step.snapshot:  # the window ends at min(finish_tn, hist_top): the edge on either
            r = [(k, lo, hi + 40, hi) if i % 2 else (k, lo, hi, hi + 40) for i, (k, lo, hi) in enumerate(r)]
        return r

    def read_rc(self, reads):
        return np.array([RC_ABORT if self.hit(r[0], r[1], min(r[2:])) else RC_RCOK for r in reads], np.uint8)

    def write(self, txns):
        """RCs and commit tns of an epoch without windows; the pairs join."""
        rc, tn, wrote, new = [], [], set(), []
        for t in txns:
            if any(k in wrote for k, _ in t):
                rc.append(RC_ABORT)
                tn.append(0)
                continue
            rc.append(RC_RCOK)
            w = [k for k, a in t if a == WR]
            wrote.update(w)
            if w:
                self.tnc += 1
                new += [(k, self.tnc) for k in w]
            tn.append(self.tnc if w else 0)
        self.pairs += new
        return np.array(rc, np.uint8), np.array(tn, np.uint64), new

    def apply(self, step):
        if isinstance(step, Tnc):
            self.tnc = step.value
        elif isinstance(step, Append):
            self.pairs += [(int(k), int(t)) for k, t in zip(step.keys, step.tns)]
        elif isinstance(step, Trim):
            self.pairs = [(k, t) for k, t in self.pairs if t > step.floor]
        elif isinstance(step, Clear):
            self.pairs = []

    def sorted_pairs(self):
        p = sorted(self.pairs)
        return np.array([k for k, _ in p], np.uint64), np.array([t for _, t in p], np.uint64)


def read_batch(reads):
    b = make_batch([[(r[0], RD)] for r in reads], [r[1] for r in reads], [r[2] for r in reads])
    top = np.array([r[3] for r in reads], np.uint64) if reads and len(reads[0]) == 4 else None
    return b, top


def write_batch(txns):
    return make_batch(txns)


# ---------------------------------------------------------------- where the pairs live
class Levels:
    """dcc_ctx's two HistStores restated: which pairs are in the base, in the
    delta's sorted run and on the delta's chains, and how big the tables are."""

    def __init__(self):
        self.B, self.run, self.chain, self.flat = [], [], [], []
        self.merge_min = DEFAULT_MERGE
        self.last_app = 0
        self.n_merges = 0
        self.d_built = False   # a cleared history: the first prepare builds the delta's empty table
        self.cur_dbits = None  # the delta's table as last built
        self.d_over = False    # a push overflowed it: the next build has at least 4 x the slots

    @property
    def D(self):
        return self.run + self.chain + self.flat

    def prepare(self):
        if merges(len(self.D), len(self.B), self.merge_min):
            self.B += self.D
            self.run, self.chain, self.flat = [], [], []
            self.n_merges += 1
            self.d_built = False
        if not self.d_built:  # the rebuild sorts every flat pair into the run
            self.run, self.chain, self.flat = self.D, [], []
            bits = delta_bits(len(self.run), self.merge_min, len(self.B), self.last_app)
            if self.d_over:
                bits = max(bits, self.cur_dbits + 2)
            self.cur_dbits = rebuild_sizes(list(dict.fromkeys(k for k, _ in self.run)), bits)[-1]
            self.d_over = False
            self.d_built = True

    def apply(self, step, new=()):
        if isinstance(step, Opt):
            self.merge_min = step.merge_min
        elif isinstance(step, Append):
            self.flat += [(int(k), int(t)) for k, t in zip(step.keys, step.tns)]
            self.d_built = False
        elif isinstance(step, Trim):
            self.B = [(k, t) for k, t in self.B + self.D if t > step.floor]
            self.run, self.chain, self.flat = [], [], []
            self.d_built = False
        elif isinstance(step, Clear):
            self.B, self.run, self.chain, self.flat = [], [], [], []
            self.d_built = False
        elif isinstance(step, Reads):
            if self.B or self.D:
                self.prepare()
        elif isinstance(step, Write):
            if step.defer:  # validated without the append flag; the finish appends flat pairs
                self.flat += list(new)
                self.d_built = self.d_built and not new
            else:
                self.prepare()
                if new:
                    self.last_app = len(new)
                if step.overflow:
                    self.flat += list(new)
                    self.d_built = False
                    self.d_over = True
                else:
                    self.chain += list(new)

    def bbits(self):
        return base_bits(len(self.B))

    def dbits(self):
        return self.cur_dbits

    def paths(self, key, lo, hi):
        """hist_hit restated: the (level, stage, hit) of every stage that
        answers for this window -- the delta first, the base if it misses."""
        out = []
        for name, run, chain in (("delta", self.run, self.chain), ("base", self.B, [])):
            rt_ = sorted(t for k, t in run if k == key)
            ct = sorted((t for k, t in chain if k == key), reverse=True)
            if not rt_ and not ct:
                continue
            tmax = max(rt_ + ct)
            if tmax <= lo:
                out.append((name, "tmax", False))
                continue
            if tmax <= hi:
                out.append((name, "tmax", True))
                return out
            got = False
            for t in ct:  # newest first, stopping at the first one at or below hi
                if t <= hi:
                    got = t > lo
                    break
            if ct and (got or not rt_):
                out.append((name, "chain", got))
            if got:
                return out
            if rt_:
                got = any(lo < t <= hi for t in rt_)
                out.append((name, "run", got))
                if got:
                    return out
        return out


# ---------------------------------------------------------------- the scenarios
def _w(keys):
    return [[(int(k), WR)] for k in keys]


def _scenarios():
    S = []
    BIG = 1 << 22
    # four keys of one home in the delta's 2^16 slots (and so in every smaller table)
    K1, K2, K3, K4, KX = (int(k) for k in rt.keys_with_home("fib", 0x0BAD, 16, 5, seed=11))
    e_keys = [K1, K2, K3, K4, KX]
    three = Append([K1, K1, K1, K2], [10, 20, 30, 20])
    S.append(Scenario("edges_base", [Opt(1), three, Reads("auto", e_keys), Expect(base=4, run=0, chain=0, merges=1)],
                      paths=True))
    S.append(Scenario("edges_run", [three, Reads("auto", e_keys), Expect(base=0, run=4, chain=0, merges=0)],
                      paths=True))
    chain3 = [Tnc(9), Write(_w([K1])), Tnc(18), Write(_w([K2, K1])), Tnc(29), Write(_w([K1]))]
    S.append(Scenario("edges_chain", chain3 + [Reads("auto", e_keys), Expect(base=0, run=0, chain=4, merges=0)],
                      paths=True))
    S.append(Scenario("edges_chain_snapshot", chain3 + [Reads("auto", e_keys, snapshot=True),
                                                        Expect(base=0, run=0, chain=4, merges=0)]))
    S.append(Scenario("edges_split", [
        Opt(1), Append([K1, K2], [10, 20]), Reads("auto", [K1, KX]), Expect(base=2, run=0, chain=0, merges=1),
        Opt(DEFAULT_MERGE), Append([K1, K3], [20, 20]), Tnc(29), Write(_w([K1, K4])),
        Reads("auto", e_keys), Expect(base=2, run=2, chain=2, merges=1),
        Reads("auto", e_keys, snapshot=True)], paths=True))

    # ---- chain order: five epochs of 20 blind writers of one key, one commit each
    st = []
    for e in range(1, 6):
        st += [Tnc(10 * e), Write(_w([K1] * 20) + _w([K2] if e == 3 else []))]
    S.append(Scenario("chain_order", st + [Reads("auto", [K1, K2, KX]), Expect(base=0, run=0, chain=6, merges=0),
                                           Reads("auto", [K1, K2], snapshot=True)], paths=True))

    # ---- the walk bound, in the delta (2^16 slots; the keys share a home through 2^18, split at 2^20)
    # After a 4 x growth the keys of one home have at most 4 homes, next to each other: still one
    # run of 65 slots, in which the key that arrives last may again sit 64 from its home.  So that
    # the sizes do not depend on the order of arrival, 64 of the keys share the home through 2^20
    # (they fill the walk exactly, at every size) and the 65th leaves them there for a lower slot.
    C = [int(k) for k in rt.keys_with_home("fib", 0x1234, 16, HIST_WALK, 20, 0b0111, seed=21)]
    C += [int(k) for k in rt.keys_with_home("fib", 0x1234, 16, 1, 20, 0b0100, seed=21)]
    CA = key_with_home_and_bit(0x1234, 16, 20, 0b0111, C[:HIST_WALK], C, seed=1)
    t64 = list(range(1, HIST_WALK + 1))
    S.append(Scenario("walk_push", [
        Opt(4096), Write(_w(C[:HIST_WALK])), Reads("auto", C + [CA]), Expect(base=0, run=0, chain=HIST_WALK, dbits=16),
        Write(_w(C[HIST_WALK:]), overflow=True), Reads("auto", C + [CA]),
        Expect(base=0, run=HIST_WALK + 1, chain=0, merges=0),
        Write(_w(C[3:9])), Reads("auto", C + [CA]), Expect(run=HIST_WALK + 1, chain=6)],
        clusters=[(C[:HIST_WALK], 16, [16]), (C, 16, [16, 18, 20])]))
    S.append(Scenario("walk_push_then_trim", [
        Opt(4096), Write(_w(C[:HIST_WALK])), Write(_w(C[HIST_WALK:]), overflow=True), Trim(HIST_WALK // 2),
        Reads("auto", C + [CA]), Expect(base=HIST_WALK // 2 + 1, run=0, chain=0),
        Write(_w(C[:5])), Reads("auto", C + [CA])],
        clusters=[(C, 16, [16, 18, 20])]))
    S.append(Scenario("walk_rebuild_then_trim", [
        Opt(4096), Write(_w(C[:HIST_WALK])), Write(_w(C[HIST_WALK:]), overflow=True), Reads("auto", C[-3:]),
        Trim(HIST_WALK - 1), Reads("auto", C + [CA]), Expect(base=2, run=0, chain=0)],
        clusters=[(C, 16, [16, 18, 20])]))
    S.append(Scenario("walk_build_delta", [
        Opt(4096), Append(C[:HIST_WALK], t64), Reads("auto", C + [CA]), Expect(run=HIST_WALK, chain=0, dbits=16),
        Append(C[HIST_WALK:], [HIST_WALK + 1]), Reads("auto", C + [CA]), Expect(run=HIST_WALK + 1, merges=0),
        Write(_w(C[60:])), Reads("auto", C[55:] + [CA]), Expect(run=HIST_WALK + 1, chain=5)],
        clusters=[(C[:HIST_WALK], 16, [16]), (C, 16, [16, 18, 20])]))
    # ---- ... and in the base: 64 pairs get 2^8 slots, 65 get 2^9; one home through 2^13, split at 2^15
    # (the same construction: 64 keys of one home through 2^15, the 65th with them through 2^13)
    Cb = [int(k) for k in rt.keys_with_home("fib", 0x155, 9, HIST_WALK, 15, (7 << 2) | 3, seed=22)]
    Cb += [int(k) for k in rt.keys_with_home("fib", 0x155, 9, 1, 15, 7 << 2, seed=22)]
    CbA = key_with_home_and_bit(0x155, 9, 15, (7 << 2) | 3, Cb[:HIST_WALK], Cb, seed=2)
    S.append(Scenario("walk_build_base", [
        Opt(1), Append(Cb[:HIST_WALK], t64), Reads("auto", Cb + [CbA]), Expect(base=HIST_WALK, run=0, bbits=8, merges=1),
        Clear(), Append(Cb, t64 + [HIST_WALK + 1]), Reads("auto", Cb + [CbA]),
        Expect(base=HIST_WALK + 1, run=0, bbits=9, merges=2)],
        clusters=[(Cb[:HIST_WALK], 8, [8]), (Cb, 9, [9, 11, 13, 15])]))

    # ---- a cluster homed on the table's last slot wraps to slot 0, at every size reached
    W = [int(k) for k in rt.keys_with_home("fib", 0xFFFF, 16, 12, 20, 0xF, seed=23)]
    WA = key_with_home_and_bit(0xFFFF, 16, 20, 0xF, W[:10], W, seed=3)
    S.append(Scenario("wrap_push", [
        Opt(4096), Write(_w(W[:10])), Reads("auto", W + [WA]), Expect(chain=10, run=0, dbits=16),
        Write(_w(W[8:])), Reads("auto", W + [WA]), Expect(chain=14)], last_slot=W + [WA]))
    S.append(Scenario("wrap_build", [
        Opt(4096), Append(W[:10], list(range(1, 11))), Reads("auto", W + [WA]), Expect(run=10, base=0, dbits=16),
        Opt(1), Reads("auto", W + [WA]), Expect(base=10, run=0, bbits=6, merges=1),
        Append(W[9:], [11, 12, 13]), Reads("auto", W + [WA]), Expect(base=13, bbits=6, merges=2)],
        last_slot=W + [WA]))

    # ---- the key bitmap stays a superset
    Ba, Bb, Bd, Be, Bn = (int(k) for k in keys_with_bm_bit(0x1ABCD, 5, seed=31))
    Xa = int(keys_with_bm_bit(0x00077, 1, seed=32)[0])
    probe = [Ba, Bb, Bd, Be, Bn, Xa, K1]
    S.append(Scenario("bitmap", [
        Opt(1), Append([Ba, Xa], [10, 11]), Reads("auto", probe), Expect(base=2, run=0, merges=1),
        Opt(DEFAULT_MERGE), Append([Bd], [20]), Reads("auto", probe), Expect(base=2, run=1),
        Opt(1), Append([K1], [21]), Reads("auto", probe), Expect(base=4, run=0, merges=2),  # merge: null delta
        Tnc(30), Write(_w([Be])), Reads("auto", probe), Expect(base=4, chain=1),
        Trim(10), Reads("auto", probe), Expect(base=4, run=0, chain=0),   # Ba gone, its bit may stay
        Trim(20), Reads("auto", probe),                                    # Xa, Bd gone
        Clear(), Reads("auto", probe), Append([Bn], [5]), Reads("auto", probe), Expect(base=0, run=1),
        Clear(), Tnc(0), Write(_w([Bb])), Reads("auto", probe), Expect(base=0, chain=1)]))

    # ---- the merge threshold, on both arms of max(merge_min, B.m / 4)
    F = [int(k) for k in np.random.default_rng(41).integers(1, 1 << 62, size=200)]
    S.append(Scenario("merge_at_merge_min", [
        Opt(8), Append(F[:8], list(range(1, 9))), Reads("auto", F[:10] + [K1]), Expect(base=0, run=8, merges=0),
        Append(F[8:9], [9]), Reads("auto", F[:10] + [K1]), Expect(base=9, run=0, merges=1)]))
    S.append(Scenario("merge_at_a_quarter_of_the_base", [
        Opt(1), Append(F[:100], list(range(1, 101))), Reads("auto", F[:3]), Expect(base=100, run=0, merges=1),
        Opt(8), Append(F[100:125], list(range(101, 126))), Reads("auto", F[98:127]), Expect(base=100, run=25, merges=1),
        Tnc(200), Write(_w(F[125:126])), Expect(base=100, run=25, chain=1, merges=1),
        Reads("auto", F[98:127]), Expect(base=126, run=0, chain=0, merges=2)]))

    # ---- appends out of tn order, equal tns, keys with bit 63, tns above 2^32
    H = [int(k) | (1 << 63) for k in np.random.default_rng(42).integers(1, 1 << 62, size=6)]
    T = 1 << 33
    hp = H + [K1]
    S.append(Scenario("non_monotonic", [
        Append([H[0], H[1], H[0], 5], [T + 50, T + 50, T + 60, 3]), Reads("auto", hp + [5]), Expect(run=4),
        Append([H[0], H[2], H[1], 5], [T + 10, 7, T + 50, 3]), Reads("auto", hp + [5]), Expect(run=8, merges=0),
        Tnc(T + 100), Write(_w([H[0], H[3], 5])), Reads("auto", hp + [5]), Expect(run=8, chain=3),
        Opt(1), Reads("auto", hp + [5]), Expect(base=11, run=0, chain=0, merges=1),
        Append([H[4], H[0], H[2]], [9, T + 5, T + 7]), Reads("auto", hp + [5]), Expect(base=14, merges=2),
        Trim(T + 10), Reads("auto", hp + [5]), Expect(base=7),
        Opt(DEFAULT_MERGE), Write(_w([H[5], H[0]])), Reads("auto", hp + [5]), Expect(base=7, chain=2),
        Trim(T + 101), Reads("auto", hp + [5]), Expect(base=4)], paths=True))

    # ---- trim floors, with pairs in both levels
    def both():
        return [Opt(1), Append([K1, K2, K3], [10, 10, 20]), Reads("auto", [K1]), Expect(base=3, merges=1),
                Opt(DEFAULT_MERGE), Append([K1, K2], [20, 30]), Tnc(29), Write(_w([K1, K4])),
                Reads("auto", e_keys), Expect(base=3, run=2, chain=2)]
    for name, floor, kept in (("at_a_tn", 20, 3), ("below_a_tn", 19, 5), ("below_all", 9, 7), ("at_the_top", 31, 0),
                              ("above_all", 1000, 0)):
        S.append(Scenario("trim_" + name, both() + [
            Trim(floor), Expect(base=kept, run=0, chain=0), Reads("auto", e_keys),
            Write([[(K1, RD), (K3, WR)], [(K3, RD)], [(K2, WR)]]), Reads("auto", e_keys), Expect(base=kept, chain=2)]))

    # ---- append seams: 1,024 txns per workgroup of k_hist_count / k_hist_emit, 2,048 of k_fin
    n = 2060
    R = [int(k) for k in np.random.default_rng(43).permutation(1 << 20)[:3 * n + 256] + 1]
    at = (1023, 1024, 2047, 2048)
    sparse = [[(R[i], WR if i in at else RD)] for i in range(n)]
    dense = _w(R[n:2 * n])
    long_ = [[(R[2 * n + i], RD)] for i in range(2050)]
    for i in (1024, 2047):
        ks = R[2 * n + 2050 + MAX_TXN_LEN * (i & 1):][:MAX_TXN_LEN]
        long_[i] = [(k, RD) for k in ks[:-1]] + [(ks[-1], WR)]
    for defer in (False, True):
        watch = [R[i] for i in at] + [R[0], R[1022], R[n], R[n + 1023], R[n + 1024], R[n + 2047], R[n + 2048],
                                      R[2 * n - 1], long_[1024][-1][0], long_[1024][0][0], long_[2047][-1][0]]
        S.append(Scenario("seams_defer" if defer else "seams_fin", [
            Tnc(100), Write(sparse, defer=defer), Reads("auto", watch),
            Write(dense, defer=defer), Reads("auto", watch),
            Write(long_, defer=defer), Reads("auto", watch), Expect(base=0, merges=0)]))
    return S


SCENARIOS = _scenarios()
NAMES = [s.name for s in SCENARIOS]


def scenario(name):
    return SCENARIOS[NAMES.index(name)]
