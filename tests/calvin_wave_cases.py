"""Directed cases for the one-CU Calvin wave walk (csrc/calvin_wave.hip), shared
by the CPU proofs (test_calvin_wave_cases.py) and the GPU parity test
(test_gpu_calvin_wave_edges.py).  No GPU here.

plan() restates cw_plan / cw_run's choice of kernel form from the constants of
calvin_wave.hip / calvin_wave.h, read by regular expression and asserted: a
changed geometry fails here instead of silently moving the seams.

classify() restates k_cw_link's rule from the oracle's groups: a request's slot
code is seqpos(txn) << lg | j, a group's maximum lives at the slot of its
sequence-last member, chunk = code / H, sub-chunk = sequence position / 64.
Per request it gives the class of the previous group's slot (the read) and of
the own group's slot (the publication):

  previous: none | sub (same sub-chunk: F_FLAG, intra) | chunk (same chunk) |
            -1 (previous chunk) | -2 (rec2's p2, LDS) | far (3+: helper gather)
  own:      sub | chunk (both: the walker publishes) | +1 (boundary add from
            `own`) | +2 (from `ownq`) | far (3+: helper fetch_max into mg)

A probe is a row R with group 0 = SH requests of a carrier M, of the group's
sequence-last member A and of any further members, and group 1 = one EX request
of a reader T.  M also ends a private chain of D EX writes on a private key,
so wave(M) = D, every other member of group 0 has wave 0, and wave(T) = D + 1
exactly when M's contribution survives its path to A's slot (M's own class) and
from there to T (T's previous class); lost, T reads 1.  Probes of one batch
have distinct rows, private keys, chain txns and (but for the 64-txn chains of
`compact`) distinct D.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from deneva_amd import GROUP_NONE, RD, WR, EpochBatch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva_amd", "csrc")


def _src(fname):
    with open(os.path.join(CSRC, fname)) as f:
        return f.read()


def _const(name, fname):
    m = re.search(r"constexpr uint32_t [^;]*\b%s = (\d+)[,;]" % name, _src(fname))
    assert m, f"{name} not found in {fname}"
    return int(m.group(1))


CW_T = _const("CW_T", "calvin_wave.hip")
CW_K = _const("CW_K", "calvin_wave.hip")
CR_K = _const("CR_K", "calvin_wave.hip")
CW_CMAX = _const("CW_CMAX", "calvin_wave.h")
CW_LMAX = _const("CW_LMAX", "calvin_wave.h")
_m = re.search(r"/ (\d+)u \* (\d+)u;", _src("calvin_wave.hip"))
assert _m and _m.group(1) == _m.group(2), "cw_plan's chunk rounding not found"
CW_ROUND = int(_m.group(1))  # a chunk is a multiple of three 64-txn sub-chunks
# the forms plan() restates: the staging thread count, the slots per chunk, the
# slot width by the longest txn, the helper form's condition
for _pat in (r"CW_HELP = CW_T - 64;", r"CW_HPLAN = CW_K \* CW_HELP;", r"maxlen <= 16 \? 4u : 5u;",
             r"std::min<uint32_t>\(CW_CMAX, CW_HPLAN >> lg\)", r"a\.nh && a\.rec2 && p\.nch > 2"):
    assert re.search(_pat, _src("calvin_wave.hip")), f"calvin_wave.hip no longer says {_pat!r}"
assert re.search(r"cw && cwp\.nch > 2 \? cw_helpers\(n_cu\)", _src("calvin.hip"))
# the seams below are built on these: a retune of the walk has to move them
assert (CW_T, CW_K, CR_K, CW_CMAX, CW_LMAX, CW_ROUND) == (512, 36, 4, 1024, 32, 192), \
    (CW_T, CW_K, CR_K, CW_CMAX, CW_LMAX, CW_ROUND)
SUB = 64  # txns per sub-chunk: one walker lane each

Plan = namedtuple("Plan", "lg C H nch helpers")


def plan(n, maxlen):
    """cw_plan, and cw_run's kernel form (helpers iff nch > 2).  None: the
    dataflow grid takes the epoch (a txn longer than CW_LMAX, or nothing to do)."""
    if maxlen == 0 or maxlen > CW_LMAX or n == 0:
        return None
    lg = 4 if maxlen <= 16 else 5
    C = min(CW_CMAX, (CW_K * (CW_T - 64)) >> lg) // CW_ROUND * CW_ROUND
    nch = -(-n // C)
    return Plan(lg, C, C << lg, nch, nch > 2)


CHUNK = {4: plan(1, 16).C, 5: plan(1, 17).C}
assert CHUNK == {4: 960, 5: 384}, CHUNK

PREV = ("none", "sub", "chunk", "-1", "-2", "far")
OWN = ("none", "sub", "chunk", "+1", "+2", "far")

Classes = namedtuple("Classes", "plan code prev own prev_code own_code prev_dist own_dist n_intra n_hot")


def seq_positions(b):
    n = b.n_txn
    if b.order is None:
        return np.arange(n, dtype=np.int64)
    seq = np.argsort(np.asarray(b.order, np.uint64), kind="stable")
    pos = np.empty(n, np.int64)
    pos[seq] = np.arange(n, dtype=np.int64)
    return pos


def classify(b, groups):
    """Per request: its slot code, the class index (PREV / OWN) and slot code of
    its previous and own group's maximum, the chunk distances; per txn the
    compact record's counts (k_cw_cr): intra reads and hot publications.
    `groups` are the oracle's (orc.calvin(b)[0]).  None when plan() is."""
    n, nnz = b.n_txn, b.nnz
    off = np.asarray(b.offsets, np.int64)
    lens = np.diff(off)
    p = plan(n, int(lens.max()) if n else 0)
    if p is None:
        return None
    keys = np.asarray(b.keys, np.uint64)
    txn = np.repeat(np.arange(n, dtype=np.int64), lens)
    q = seq_positions(b)[txn]
    code = (q << p.lg) | (np.arange(nnz, dtype=np.int64) - off[txn])
    g = np.asarray(groups).astype(np.int64)
    live = np.nonzero(np.asarray(groups) != GROUP_NONE)[0]
    si = live[np.lexsort((code[live], g[live], keys[live]))]  # by row, group, sequence
    ks, gs, cs = keys[si], g[si], code[si]
    first = np.r_[True, (ks[1:] != ks[:-1]) | (gs[1:] != gs[:-1])]
    gid = np.cumsum(first) - 1
    glast = cs[np.r_[first[1:], True]]  # per (row, group): its sequence-last member's slot
    own_code = np.full(nnz, -1, np.int64)
    prev_code = np.full(nnz, -1, np.int64)
    own_code[si] = glast[gid]
    has = gs > 0
    # a row's groups are dense (0, 1, ...): the previous group is the previous id
    f0 = np.nonzero(first)[0]
    assert (ks[f0][gid[has] - 1] == ks[has]).all() and (gs[f0][gid[has] - 1] == gs[has] - 1).all()
    prev_code[si[has]] = glast[gid[has] - 1]
    c, sub = q // p.C, q // SUB

    def cls(slot, sign):
        ch, sb = slot // p.H, (slot >> p.lg) // SUB
        dist = np.where(slot >= 0, sign * (ch - c), -1)
        k = np.where(dist >= 3, 5, np.where(dist == 2, 4, np.where(dist == 1, 3, np.where(sb == sub, 1, 2))))
        assert (dist[slot >= 0] >= 0).all()
        return np.where(slot >= 0, k, 0), dist

    prev, prev_dist = cls(prev_code, -1)
    own, own_dist = cls(own_code, 1)
    n_intra = np.bincount(txn[prev == 1], minlength=n)
    marked = np.unique(prev_code[prev == 1])  # k_cw_mark
    hot = (own_code >= 0) & (own_dist == 0) & np.isin(own_code, marked)
    n_hot = np.bincount(txn[hot], minlength=n)
    return Classes(p, code, prev, own, prev_code, own_code, prev_dist, own_dist, n_intra, n_hot)


def lds_slot(p, code):
    """The LDS slot of a global slot code (k_cw_link: two chunk regions)."""
    return ((code // p.H) & 1) * p.H + code % p.H


# ------------------------------------------------------------------ the builder
Probe = namedtuple("Probe", "name D row m a t xm xa xt own own_dist prev prev_dist facts")
Case = namedtuple("Case", "name batch probes lg n facts")


class NoRoom(Exception):
    pass


class Layout:
    """n sequence positions; roles claim positions, the rest are fillers (one SH
    request on a private key).  seed: the sequencer order is a fixed
    pseudo-random permutation with `order` keys that include ties; else index
    order."""

    def __init__(self, n, lg, seed=None, maxlen=None, uniform=0):
        self.n, self.lg, self.C = n, lg, CHUNK[lg]
        self.used = np.zeros(n, bool)
        self.seed, self.uniform = seed, uniform
        self.maxlen = maxlen if maxlen is not None else (17 if lg == 5 else 0)
        self.probes, self.empty, self.extra = [], [], []

    # -- positions
    def claim(self, pos):
        if not 0 <= pos < self.n or self.used[pos]:
            raise NoRoom(pos)
        self.used[pos] = True
        return pos

    def take(self, chunk, sub=None, below=None):
        """The highest free position of the chunk (of its sub-chunk) below `below`."""
        lo = chunk * self.C + (0 if sub is None else sub * SUB)
        hi = chunk * self.C + (self.C if sub is None else (sub + 1) * SUB)
        hi = min(hi, self.n, hi if below is None else below)
        for pos in range(hi - 1, lo - 1, -1):
            if not self.used[pos]:
                self.used[pos] = True
                return pos
        raise NoRoom((chunk, sub, below))

    def take_any(self, chunk, sub):
        try:
            return self.take(chunk, sub)
        except NoRoom:
            return self.take(chunk)

    def chain_below(self, m, D):
        """The D nearest free positions below m."""
        out = []
        for pos in range(m - 1, -1, -1):
            if len(out) == D:
                break
            if not self.used[pos]:
                out.append(pos)
        if len(out) < D:
            raise NoRoom(("chain", m, D))
        self.used[out] = True
        return out[::-1]

    def snapshot(self):
        return self.used.copy(), len(self.probes)

    def restore(self, snap):
        self.used[:] = snap[0]
        del self.probes[snap[1]:]

    def next_d(self):
        return 2 + len(self.probes)

    def probe(self, name, m, a, t, D=None, chain=None, members=(), jm=None, ja=None, jt=None,
              dup=False, m_pre=(), t_pre=(), facts=None, want=None):
        """Positions m < a < t already claimed (a None: M is the last member
        itself).  chain: its positions (claimed), default the nearest free ones."""
        D = self.next_d() if D is None else D
        assert m < t and (a is None or m < a < t) and all(x < (t if a is None else a) for x in members)
        chain = self.chain_below(m, D) if chain is None else list(chain)
        assert len(chain) == D and all(x < m for x in chain)
        self.probes.append(dict(name=name, D=D, m=m, a=a, t=t, chain=chain, members=tuple(members),
                                jm=jm, ja=ja, jt=jt, dup=dup, m_pre=tuple(m_pre), t_pre=tuple(t_pre),
                                facts=facts or {}, want=want))
        return self.probes[-1]

    # -- the batch
    def finish(self, name, facts=None):
        n, key = self.n, [0]

        def fresh():
            key[0] += 1
            return key[0]

        fixed = {}   # pos -> {j: (key, type)}
        free = {}    # pos -> [(key, type)]

        def put(pos, k, at, j=None):
            if j is None:
                free.setdefault(pos, []).append((k, at))
            else:
                assert j not in fixed.setdefault(pos, {})
                fixed[pos][j] = (k, at)

        for pr in self.probes:
            R, P = fresh(), fresh()
            pr["row"] = R
            for x in pr["chain"]:
                put(x, P, WR)
            for k, at in pr["m_pre"]:     # requests ahead of M's on R (compact: hot publications)
                put(pr["m"], k, at)
            put(pr["m"], R, RD, pr["jm"])
            if pr["dup"]:                 # M and T name R twice: the second is a duplicate slot
                put(pr["m"], R, WR)
            put(pr["m"], P, WR)
            if pr["a"] is not None:
                put(pr["a"], R, RD, pr["ja"])
            for x in pr["members"]:
                put(x, R, RD)
            for k, at in pr["t_pre"]:     # requests ahead of T's on R (compact: intra reads)
                put(pr["t"], k, at)
            put(pr["t"], R, WR, pr["jt"])
            if pr["dup"]:
                put(pr["t"], R, RD)
        for pos, reqs in self.extra:
            for k, at in reqs:
                put(pos, k, at)
        txns = [None] * n
        pad = {}
        if self.maxlen:  # one filler padded with private keys to the longest length
            pad[int(np.nonzero(~self.used)[0][0])] = self.maxlen
        for pos in range(n):
            if pos in self.empty:
                txns[pos] = []
                continue
            fx, fr = fixed.get(pos, {}), list(free.get(pos, []))
            if not fx and not fr:
                fr = [(fresh(), RD)]
            L = max(max(fx) + 1 if fx else 0, len(fx) + len(fr), pad.get(pos, 0), self.uniform)
            t = []
            for j in range(L):
                t.append(fx[j] if j in fx else fr.pop(0) if fr else (fresh(), RD))
            txns[pos] = t
        # sequence position -> txn index
        if self.seed is None:
            perm, order = np.arange(n), None
        else:
            rng = np.random.default_rng(self.seed)
            perm = rng.permutation(n)
            order = np.zeros(n, np.uint64)
            pos, run = 0, 0
            while pos < n:  # runs of 1..3 positions share an order key: index order inside a run
                ln = int(rng.integers(1, 4))
                perm[pos:pos + ln] = np.sort(perm[pos:pos + ln])
                order[perm[pos:pos + ln]] = run * 7 + 3
                pos, run = pos + ln, run + 1
        by_txn = [None] * n
        for pos in range(n):
            by_txn[perm[pos]] = txns[pos]
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(t) for t in by_txn])
        keys = np.array([k for t in by_txn for k, _ in t], np.uint64)
        at = np.array([a for t in by_txn for _, a in t], np.uint8)
        b = EpochBatch(off, keys, at, order=order)
        assert (plan(n, max(len(t) for t in by_txn)) or Plan(self.lg, 0, 0, 0, 0)).lg == self.lg

        def req(pos, R):  # the first request of the txn at pos on row R
            return int(off[perm[pos]]) + [k for k, _ in txns[pos]].index(R)

        probes = []
        for pr in self.probes:
            a = pr["m"] if pr["a"] is None else pr["a"]
            cm, ca, ct = pr["m"] // self.C, a // self.C, pr["t"] // self.C
            own = OWN[min(ca - cm, 3) + 2] if ca > cm else ("sub" if a // SUB == pr["m"] // SUB else "chunk")
            prev = PREV[min(ct - ca, 3) + 2] if ct > ca else ("sub" if a // SUB == pr["t"] // SUB else "chunk")
            if pr["want"]:  # what place() was asked for
                w = pr["want"]
                assert (own, ca - cm, prev, ct - ca) == (w[0] if w[1] == 0 else OWN[min(w[1], 3) + 2], w[1],
                                                         w[2] if w[3] == 0 else PREV[min(w[3], 3) + 2], w[3]), pr
            probes.append(Probe(pr["name"], pr["D"], pr["row"], int(perm[pr["m"]]), int(perm[a]),
                                int(perm[pr["t"]]), req(pr["m"], pr["row"]), req(a, pr["row"]),
                                req(pr["t"], pr["row"]), own, ca - cm, prev, ct - ca, pr["facts"]))
        return Case(name, b, probes, self.lg, n, facts or {})


def without_carrier(case, pr):
    """The batch with the carrier's request(s) on the probe's row removed."""
    b = case.batch
    off = np.asarray(b.offsets, np.int64)
    keys = np.asarray(b.keys, np.uint64)
    x = np.arange(off[pr.m], off[pr.m + 1])
    drop = x[keys[x] == np.uint64(pr.row)]
    keep = np.ones(b.nnz, bool)
    keep[drop] = False
    off2 = off.copy()
    off2[pr.m + 1:] -= drop.size
    return EpochBatch(off2.astype(np.uint32), keys[keep], np.asarray(b.acctype)[keep], order=b.order)


def place(L, name, own, do, prev, dp, cm, i=0, t_at=None, **kw):
    """One probe: M in chunk cm, A `do` chunks on, T `dp` chunks after A; a
    class "sub" shares the sub-chunk, "chunk" the chunk but not the sub-chunk.
    Tries every choice of sub-chunks, starting at one that i picks."""
    nsub = L.C // SUB
    snap = L.snapshot()
    ca, ct = cm + do, cm + do + dp

    def rot(lo, hi):  # lo .. hi - 1, starting at one that i picks
        return [lo + (i + k) % (hi - lo) for k in range(hi - lo)] if hi > lo else []

    for sa in rot(0, nsub):
        t_subs = [None] if t_at is not None or dp else [sa] if prev == "sub" else rot(sa + 1, nsub)
        m_subs = [None] if do else [sa] if own == "sub" else rot(0, sa)
        for ts in t_subs:
            for ms in m_subs:
                try:
                    if t_at is not None:
                        t = L.claim(t_at)
                    else:
                        t = L.take_any(ct, (5 * i + 3) % nsub) if dp else L.take(ct, ts)
                    a = L.take(ca, sa, below=t)
                    if do:
                        m = L.take_any(cm, max(1, (7 * i + 2) % nsub) if cm == 0 else (7 * i + 2) % nsub)
                    else:
                        m = L.take(cm, ms, below=a)
                    return L.probe(name, m, a, t, want=(own, do, prev, dp), **kw)
                except NoRoom:
                    L.restore(snap)
    raise NoRoom(name)


DIST = (("sub", 0), ("chunk", 0), (1, 1), (2, 2), (3, 3), (5, 5))  # grid: same sub-chunk .. five chunks


def _cname(c, d, sign):
    return c if d == 0 else f"{sign}{d}"


def grid_pairs():
    """(own, do, prev, dp) of the grid: the carrier in chunk >= 0, A `do` chunks
    on, the reader `dp` chunks after A, in 8 chunks plus one txn.  do + dp <= 7
    fits freely; the ninth chunk holds one txn, so one pair with do + dp = 8
    fits too, (5, 3); (3, 5) and (5, 5) do not."""
    out = []
    for own, do in DIST:
        for prev, dp in DIST:
            if do + dp <= 7 or (do, dp) == (5, 3):
                out.append((own, do, prev, dp))
    return out


def build_grid(lg, seq):
    C = CHUNK[lg]
    L = Layout(8 * C + 1, lg, seed=(40 + lg if seq else None))
    pairs = grid_pairs()
    # the pair that needs the last chunk's only txn first
    pairs.sort(key=lambda p: (p[1], p[3]) != (5, 3))
    for i, (own, do, prev, dp) in enumerate(pairs):
        last = (do, dp) == (5, 3)
        cm = 0 if last else i % (8 - do - dp)
        place(L, f"own {_cname(own, do, '+')} prev {_cname(prev, dp, '-')}", own, do, prev, dp, cm, i,
              t_at=8 * C if last else None)
    return L.finish(f"grid-lg{lg}-{'seq' if seq else 'index'}")


def build_edges(lg):
    """A's request in slot 0 and slot Lp - 1 of A, A at a chunk's position 0
    and C - 1, in an odd and an even chunk (LDS slots 0, H - 1, H, 2H - 1); T at
    the next chunk's first and last positions; A / T in adjacent sub-chunks G,
    G + 1 for G mod 3 = 0, 1, 2; A in the last, partial sub-chunk of the last
    chunk."""
    C, Lp = CHUNK[lg], 1 << lg
    n = 7 * C + SUB + 10
    L = Layout(n, lg, maxlen=0)
    H = C << lg
    for ca in (1, 4):  # an odd and an even chunk
        base = (ca & 1) * H
        a0, a1 = L.claim(ca * C), L.claim(ca * C + C - 1)
        nx = (ca + 1) * C
        for a, ja, t, mc, slot in ((a0, 0, nx, ca - 1, base), (a0, Lp - 1, nx + 1, ca - 1, base + Lp - 1),
                                   (a1, 0, nx + C - 2, ca, base + H - Lp), (a1, Lp - 1, nx + C - 1, ca - 1, base + H - 1)):
            m = L.take(mc, None, below=a)
            L.probe(f"A chunk {ca} pos {a - ca * C} slot {ja}", m, a, L.claim(t), ja=ja,
                    facts=dict(lds_slot=slot, t_pos=t - nx))
    for G in (0, 1, 2):  # chunk 6: A last in sub-chunk G, T first in G + 1
        a, t = L.claim(6 * C + SUB * G + SUB - 1), L.claim(6 * C + SUB * (G + 1))
        L.probe(f"A sub-chunk {G} T sub-chunk {G + 1}", L.take(6, G, below=a), a, t, facts=dict(G=(6 * C // SUB + G) % 3))
    # the last chunk: one whole sub-chunk and 10 txns; A and T among the 10
    t = L.claim(n - 1)
    a = L.claim(n - 3)
    L.probe("A in the last partial sub-chunk", L.take(5, None), a, t, facts=dict(partial=True))
    return L.finish(f"edges-lg{lg}")


CLASS5 = (("sub", 0), ("chunk", 0), (1, 1), (2, 2), (3, 3))


def all_classes(L, dist=CLASS5):
    """One probe of every (own, previous) class that fits in L, ending as late
    as it can (the last chunk may be partial)."""
    last = (L.n - 1) // L.C
    i = 0
    # the widest first: a last chunk of one txn goes to a pair that needs it
    for own, do, prev, dp in sorted(((o, a, p, b) for o, a in dist for p, b in dist), key=lambda x: -x[1] - x[3]):
        for cm in range(last - do - dp, -1, -1):
            try:
                place(L, f"own {_cname(own, do, '+')} prev {_cname(prev, dp, '-')}", own, do, prev, dp, cm, i)
                i += 1
                break
            except NoRoom:
                pass
    return L


def size_list(lg):
    C = CHUNK[lg]
    return (("1", 1), ("63", 63), ("64", 64), ("65", 65), ("191", 191), ("192", 192), ("193", 193),
            ("C-1", C - 1), ("C", C), ("C+1", C + 1), ("2C", 2 * C), ("2C+1", 2 * C + 1),
            ("3C", 3 * C), ("3C+1", 3 * C + 1), ("4C+65", 4 * C + 65))


def build_size(lg, n):
    return all_classes(Layout(n, lg)).finish(f"sizes-lg{lg}-n{n}")


def build_compact():
    """lg 4.  Everything of a compact-record probe sits in one sub-chunk, so the
    carrier's wave is not there in the first round and arrives through the
    intra rounds."""
    C = CHUNK[4]
    L = Layout(3 * C, 4)
    key = [1 << 20]  # rows of the padding reads / publications, apart from finish()'s keys

    def rows(k):
        key[0] += k
        return list(range(key[0] - k, key[0]))

    # a reader with exactly k intra reads, the probe's the last: U holds SH on
    # the k - 1 other rows in the same sub-chunk, T takes them EX ahead of R
    for sub, k in ((2, CR_K), (4, CR_K + 1)):
        t = L.take(0, sub)
        a = L.take(0, sub, below=t)
        m = L.take(0, sub, below=a)
        u = L.take(0, sub, below=m)
        qs = rows(k - 1)
        L.extra.append((u, [(q, RD) for q in qs]))
        L.probe(f"{k} intra reads", m, a, t, t_pre=[(q, WR) for q in qs], facts=dict(intra=k))
    # a carrier with exactly k hot publications, the probe's the last: M holds
    # SH on k - 1 other rows that V, of the same sub-chunk, takes EX
    for sub, k in ((6, CR_K), (8, CR_K + 1)):
        t = L.take(0, sub)
        v = L.take(0, sub, below=t)
        m = L.take(0, sub, below=v)
        qs = rows(k - 1)
        L.extra.append((v, [(q, WR) for q in qs]))
        L.probe(f"{k} hot publications", m, None, t, m_pre=[(q, RD) for q in qs], facts=dict(hot=k))
    # 64 dependent txns: one whole sub-chunk, across a sub-chunk seam, across a chunk seam
    for nm, lo in (("chain fills a sub-chunk", SUB * 10), ("chain across a sub-chunk seam", SUB * 12 + 32),
                   ("chain across a chunk seam", C - 32)):
        ch = [L.claim(x) for x in range(lo, lo + 63)]
        m = L.claim(lo + 63)
        a = L.claim(lo + 64)
        L.probe(nm, m, a, L.claim(lo + 65), D=63, chain=ch, facts=dict(chain=lo))
    # a row named twice by the carrier (SH then EX) and by the reader (EX then SH)
    place(L, "duplicate slots", "sub", 0, "sub", 0, 1, 3, dup=True, facts=dict(dup=True))
    place(L, "next to the duplicates", "sub", 0, "sub", 0, 1, 3)
    return L.finish("compact")


def build_shape(kind):
    if kind == "uniform":      # every txn 4 requests: k_cw_link's ulen path
        L = Layout(4 * CHUNK[4] + 65, 4, uniform=4)
    elif kind == "empty":      # zero-length txns at position 0, a chunk's first and last, the last
        L = Layout(4 * CHUNK[4] + 65, 4)
        L.empty = [L.claim(x) for x in (0, CHUNK[4], 2 * CHUNK[4] - 1, L.n - 1)]
    elif kind == "seq":        # ragged in sequencer order: off2
        L = Layout(4 * CHUNK[4] + 65, 4, seed=77)
    else:                      # a txn of exactly `kind` requests
        lg = 4 if kind <= 16 else 5
        L = Layout(4 * CHUNK[lg] + 65, lg, maxlen=kind)
    return all_classes(L).finish(f"shapes-{kind}")


def build_spread(lg):
    """Rows whose group 0 has a member in each of chunks 0..5, A in chunk 5:
    A's slot receives maxima by the walker, the next-chunk add, the two-ahead
    add and the helpers at once.  The carrier sits in chunk 0, 1, 2, 3 (and 4,
    5) in turn.  Read from chunk 6 (the chunk after A); the ninth chunk holds
    one txn, so one row, the chunk-0 carrier's, is read three chunks later."""
    C = CHUNK[lg]
    L = Layout(8 * C + 1, lg)
    for cm in range(6):
        t = L.claim(8 * C) if cm == 0 else L.take(6, cm)
        a = L.take(5, 1 + cm % 4, below=None)
        mem = [L.take(c, None if c == 5 else (c + cm) % 4 + 1, below=a) for c in range(6) if c != cm]
        m = L.take(cm, None, below=a)
        L.probe(f"carrier in chunk {cm} of 0..5", m, a, t, members=mem, facts=dict(spread=cm))
    return L.finish(f"spread-lg{lg}")


def _cases():
    out = {}
    for lg in (4, 5):
        for seq in (False, True):
            out[f"grid-lg{lg}-{'seq' if seq else 'index'}"] = functools.partial(build_grid, lg, seq)
        out[f"edges-lg{lg}"] = functools.partial(build_edges, lg)
        for label, n in size_list(lg):
            out[f"sizes-lg{lg}-{label}"] = functools.partial(build_size, lg, n)
        out[f"spread-lg{lg}"] = functools.partial(build_spread, lg)
    out["compact"] = build_compact
    for kind in ("uniform", "empty", "seq", 16, 17, 32, 33):
        out[f"shapes-{kind}"] = functools.partial(build_shape, kind)
    return out


CASES = _cases()
GRID = tuple(k for k in CASES if k.startswith("grid-"))
DEV_CASES = GRID + tuple(k for k in CASES if k.startswith("spread-"))


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name]()
