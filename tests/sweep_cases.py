"""Constructed epochs that force single branches of the OCC sweep's filter and
compaction (occ_sweep.hip: k_sw_filter, k_sw_apply, k_sw_compact, k_sw_ro) at
the engine's real constants, shared by the CPU check of the builders
(test_sweep_cases.py) and the GPU parity test (test_gpu_sweep_edges.py).
Pure numpy; the expected decisions always come from the oracle.

Every builder returns (EpochBatch, facts) and shares one skeleton:

  head  the first P0 = 1,024 txns, the level-0 serial range: `c` single-WR
        txns of distinct hot keys (one with two writes when c = 1,025), the
        rest single-RD txns of private cold keys.  All commit, so the
        level-0 committed set C0 is exactly the c hot keys.
  body  the filter's list, from three kinds of txn: killed (one hot key at a
        chosen access), survivors (cold keys only) and chained survivors,
        which level 1 decides from exactly the keys and access types the
        compaction moved: A's last access is a WR of cold key x and a later
        B's last access an RD of x, so B aborts; A' (the access an RD, and A'
        a write txn through another key) lets B' commit.

facts: "c" (|C0|), "surv" / "ro" (level-0 survivors, the read-only ones among
them), "pairs" [(B, B')] with opposite decisions, and per case the tile, txn
and count it is meant to force.  Cold keys are distinct draws from
[2^40, 2^41), so false positives of the filter's bitmaps occur by themselves
among a few thousand accesses."""
import numpy as np

from deneva_amd import RD, WR, EpochBatch

# the engine's constants the cases sit on (test_sweep_cases.py compares them
# with occ_sweep.hip / occ_kernels.h)
P0 = 1024          # level-0 serial range (sw_pmax)
L0_BUDGET = 16384  # accesses of the level-0 serial range (sw_budget)
F_STASH = 256      # Bloom-positive keys a filter wave keeps in LDS
DCC_F_XS = 2048    # LDS exact-set slots; exact mode up to F_XCAP keys
F_XCAP = DCC_F_XS // 2
FK = 16            # 64-access rounds of a tile held in registers
SW_CHUNK = 256     # txns per filter workgroup step (4 waves)
SW_WA = 4096       # accesses of one filter wave's tile
SW_T = 64          # txns per tile
SW_PL = 640        # probe entries of a serial tile record
ROUND = 64 * FK    # accesses of one register round of the filter
MAX_LEN = 64       # accesses per txn

XCAP_C = (F_XCAP - 1, F_XCAP, F_XCAP + 1)
STASH_VARIANTS = ("over", "at256", "at257")
LIST_SEAMS = (1, 63, 64, 65, 255, 256, 257, 1025)
# level-1 lists around p_max(1): 3,072 / 8,192 with the read-only split (the
# fixed and the two-level schedule), 2,048 without
TAIL_S = {1: (3071, 3072, 3073, 8191, 8192, 8193), 0: (2047, 2048, 2049)}
RO_SEAMS = (0, 1, 63, 64, 65)

KEY_LO, KEY_HI = 1 << 40, 1 << 41


class _Pool:
    """Distinct keys of [KEY_LO, KEY_HI) in random order, handed out once."""

    def __init__(self, rng, n):
        k = np.unique(rng.integers(KEY_LO, KEY_HI, size=n + n // 8 + 64, dtype=np.uint64))
        rng.shuffle(k)
        self.k, self.i = k, 0

    def take(self, n):
        out = self.k[self.i:self.i + n]
        assert out.size == n, "key pool exhausted"
        self.i += n
        return out

    def one(self):
        return int(self.take(1)[0])


class _Txn:
    __slots__ = ("acc", "tag")

    def __init__(self, acc, tag=None):
        self.acc, self.tag = acc, tag


def _cold(pool, n, at=RD):
    return [(int(k), at) for k in pool.take(n)]


def _killed(pool, hot, length, pos, at=RD):
    acc = _cold(pool, length)
    acc[pos] = (int(hot), at)
    return _Txn(acc, ("killed",))


def _survivor(pool, rng, length, p_write=0.25):
    acc = [(k, WR if rng.random() < p_write else RD) for k, _ in _cold(pool, length)]
    return _Txn(acc, ("surv",))


def _pair(pool, pid, kill, la, lb, b_writes):
    """A (la accesses) then B (lb accesses), chained through the last access
    of each; kill: A writes the key (B aborts), else A reads it and writes
    its first key (B commits)."""
    x = pool.one()
    a, b = _cold(pool, la), _cold(pool, lb)
    if kill:
        a[-1] = (x, WR)
    else:
        a[-1] = (x, RD)
        if la >= 2:
            a[0] = (a[0][0], WR)
    b[-1] = (x, RD)
    if b_writes and lb >= 2:
        b[0] = (b[0][0], WR)
    return _Txn(a, ("A", pid, kill)), _Txn(b, ("B", pid, kill))


def _interleave(rng, items):
    """The items' txns in one random order that keeps each item's own."""
    slots = []
    for it in items:
        slots += list(zip(np.sort(rng.random(len(it))), it))
    slots.sort(key=lambda s: s[0])
    return [t for _, t in slots]


def _head(pool, rng, c):
    assert 0 < c <= 2 * P0
    hot = pool.take(c)
    nw = min(c, P0)
    writer = np.zeros(P0, bool)
    writer[rng.choice(P0, nw, replace=False)] = True
    extra, h, txns = c - nw, 0, []
    for i in range(P0):
        if writer[i]:
            acc = [(int(hot[h]), WR)]
            h += 1
            if extra:  # a second write: C0 one key larger than the serial range
                acc.append((int(hot[h]), WR))
                h += 1
                extra -= 1
        else:
            acc = _cold(pool, 1)
        txns.append(_Txn(acc, ("head",)))
    assert sum(len(t.acc) for t in txns) <= L0_BUDGET
    return txns, hot


def _finish(head, body, facts):
    txns = head + body
    n = len(txns)
    lens = np.fromiter((len(t.acc) for t in txns), np.int64, n)
    assert lens.max() <= MAX_LEN
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    keys = np.array([k for t in txns for k, _ in t.acc], np.uint64)
    at = np.array([a for t in txns for _, a in t.acc], np.uint8)
    pb, surv, ro = {}, 0, 0
    for i, t in enumerate(txns):
        if t.tag[0] == "D":
            facts["txn"] = i
        if t.tag[0] in ("head", "killed", "D") or not t.acc:
            continue
        surv += 1
        ro += all(a != WR for _, a in t.acc)
        if t.tag[0] == "B":
            pb.setdefault(t.tag[1], {})[t.tag[2]] = i
    facts.update(surv=surv, ro=ro, pairs=[(v[True], v[False]) for v in pb.values() if len(v) == 2])
    return EpochBatch(off, keys, at), facts


def _pair_items(pool, rng, n_pairs, first_id=0, max_len=10):
    items = []
    for q in range(n_pairs):
        la, lb = int(rng.integers(1, max_len + 1)), int(rng.integers(1, max_len + 1))
        for kill in (True, False):
            items.append(list(_pair(pool, first_id + q, kill, la, lb, b_writes=bool(q & 1))))
    return items


def xcap_case(c):
    """|C0| = c around F_XCAP: the LDS exact set (c <= 1,024) against the
    Bloom filter with exact checks in the global key table.  Every hot key is
    the only hot key of one killed write txn (first, middle or last access,
    RD or WR), so a key missing from either set shows."""
    rng = np.random.default_rng(0xC0 + c)
    pool = _Pool(rng, 40000)
    head, hot = _head(pool, rng, c)
    items = []
    for i, h in enumerate(hot):
        # a write txn (its hot access or a cold one): were it to survive, it
        # would stay in the level lists and commit at level 1 whatever the split
        length = 1 + i % 10
        pos = (0, length // 2, length - 1)[i % 3]
        hot_wr = i % 4 == 1 or length == 1
        t = _killed(pool, h, length, pos, WR if hot_wr else RD)
        if not hot_wr:
            q = (pos + 1 + i % (length - 1)) % length
            t.acc[q] = (t.acc[q][0], WR)
        items.append([t])
    for i in range(c // 4):  # read-only killed txns
        length = 1 + i % 7
        items.append([_killed(pool, hot[int(rng.integers(c))], length, i % length)])
    for _ in range(c // 8):
        items.append([_survivor(pool, rng, int(rng.integers(1, 11)))])
    items += [[_Txn([], ("empty",))] for _ in range(8)]
    items += _pair_items(pool, rng, 24)
    return _finish(head, _interleave(rng, items), {"c": c})


def stash_case(variant="over", per=8, c=F_XCAP):
    """Body tile 0 has more than F_STASH filter-positive accesses before a
    deciding txn, whose keys are then read back from the batch, not from the
    wave's LDS stash.  "over": 40 txns of `per` hot reads each first;
    "at256" / "at257": exactly that many positives before txn D, whose first
    access is hot.  Body tile 1 (the workgroup's next wave) is all cold
    survivors of 32 accesses, so its own stash fills with false positives."""
    assert variant in STASH_VARIANTS
    rng = np.random.default_rng(0x57A5 + STASH_VARIANTS.index(variant) + 16 * per + c)
    pool = _Pool(rng, 20000)
    head, hot = _head(pool, rng, c)

    def hot_reads(n):
        return _Txn([(int(k), RD) for k in rng.choice(hot, n, replace=False)], ("killed",))

    tile = []
    if variant == "over":
        # the first txn is half as long, so a later one's hot reads straddle
        # positives 255 / 256
        tile.append(hot_reads(per // 2))
        tile += [hot_reads(per) for _ in range(39)]
        before = per // 2 + 39 * per
        d = _killed(pool, hot[0], 6, 5)
    else:
        tile += [hot_reads(8) for _ in range(32)]
        before = 256
        if variant == "at257":
            tile.append(hot_reads(1))
            before = 257
        d = _killed(pool, hot[0], 6, 0)
    d.tag = ("D",)
    tile.append(d)
    rest, pid, step = [], 0, 0
    while len(tile) + sum(len(it) for it in rest) < SW_T - 4:
        q, step = step % 3, step + 1
        if q == 0:
            length = int(rng.integers(1, 11))
            rest.append([_killed(pool, hot[int(rng.integers(c))], length, length - 1)])
        elif q == 1:
            rest.append([_survivor(pool, rng, int(rng.integers(1, 11)))])
        else:
            rest += _pair_items(pool, rng, 1, first_id=pid)
            pid += 1
    tile += _interleave(rng, rest)
    while len(tile) < SW_T:
        tile.append(_survivor(pool, rng, 3))
    cold_tile = _interleave(rng, _pair_items(pool, rng, 8, first_id=100, max_len=1))
    cold_tile = [_Txn(_cold(pool, 31) + t.acc, t.tag) for t in cold_tile]
    cold_tile += [_survivor(pool, rng, 32, p_write=0.1) for _ in range(SW_T - len(cold_tile))]
    tail = [_killed(pool, hot[1], 4, 3), _survivor(pool, rng, 5), _killed(pool, hot[2], 1, 0)]
    return _finish(head, tile + cold_tile + tail, {"c": c, "tile": 0, "positives": before})


def _tile_shapes():
    return {
        "sq": [64] * 64,                   # span 4,096, every txn on a 64-access boundary
        "n17": [17] * 64,                  # span 1,088: just past one register round
        "off": [32] + [64] * 62 + [32],    # span 4,032, every txn across a 64-access boundary
    }


WIDE_TARGETS = {
    "sq": (0, 1023, 1024, 2048, 4095),
    "n17": (51, 63, 64, 67, 1020, 1023, 1024, 1036, 1087),
    "off": (992, 1023, 1024, 1055, 2047, 2048, 4031),
}


def wide_tile_case(c=F_XCAP):
    """Tiles spanning more than one register round of the filter (64 * FK
    accesses): one tile per shape and target, whose only hot key sits at that
    tile access (the last access of the first round, the first of the second,
    the tile's last, and the ends of txns lying across a 64-access word or the
    round boundary), then one tile per shape with every target hot.  The other
    txns survive, eight of each tile chained."""
    rng = np.random.default_rng(0x71DE + c)
    pool = _Pool(rng, 90000)
    head, hot = _head(pool, rng, c)
    body, tiles, pid = [], [], 0
    for shape, lens in _tile_shapes().items():
        starts = np.concatenate([[0], np.cumsum(lens)])
        assert starts[-1] <= SW_WA and starts[-1] > ROUND
        for targets in [(t,) for t in WIDE_TARGETS[shape]] + [WIDE_TARGETS[shape]]:
            tile = [None] * SW_T
            for x in targets:
                t = int(np.searchsorted(starts, x, side="right")) - 1
                if tile[t] is None:
                    tile[t] = _Txn(_cold(pool, lens[t]), ("killed",))
                tile[t].acc[x - starts[t]] = (int(hot[int(rng.integers(c))]), RD)
            free = [t for t in range(SW_T) if tile[t] is None]
            pick = np.sort(rng.choice(free, 8, replace=False))
            for q in range(2):
                for kill, (ia, ib) in ((True, pick[4 * q:4 * q + 2]), (False, pick[4 * q + 2:4 * q + 4])):
                    tile[ia], tile[ib] = _pair(pool, pid + q, kill, lens[ia], lens[ib], b_writes=bool(q))
            pid += 2
            for t in free:
                if tile[t] is None:
                    tile[t] = _survivor(pool, rng, lens[t], p_write=0.05)
            tiles.append({"shape": shape, "tile": len(body) // SW_T, "targets": targets})
            body += tile
    return _finish(head, body, {"c": c, "tiles": tiles})


def _mixed_items(pool, rng, hot, total):
    """`total` txns: the first killed at its last access, then killed txns
    (hot key anywhere, RD or WR), survivors, empty txns and chained pairs, of
    0 to 10 accesses."""
    items, n, pid = [[_killed(pool, hot[0], 3, 2)]], 1, 0
    while n < total:
        u = rng.random()
        if u < 0.12 and total - n >= 4:
            items += _pair_items(pool, rng, 1, first_id=pid)
            pid += 1
            n += 4
            continue
        length = int(rng.integers(0, 11))
        if length == 0:
            items.append([_Txn([], ("empty",))])
        elif u < 0.6:
            items.append([_killed(pool, hot[int(rng.integers(hot.size))], length, int(rng.integers(length)),
                                  WR if rng.random() < 0.3 else RD)])
        else:
            items.append([_survivor(pool, rng, length)])
        n += 1
    return items


def list_seam_case(L, c=F_XCAP):
    """L txns past the serial range: around the wave (63, 64, 65), the filter
    workgroup's four tiles (255, 256, 257) and a fifth workgroup (1,025), with
    a last partial tile, ragged lengths and empty txns."""
    rng = np.random.default_rng(0x115E + L)
    pool = _Pool(rng, 12 * L + 4000)
    head, hot = _head(pool, rng, c)
    body = _interleave(rng, _mixed_items(pool, rng, hot, L))
    assert len(body) == L
    return _finish(head, body, {"c": c, "L": L})


def grid_seam_case(n_cu, extra, c=F_XCAP):
    """A body of 4 tiles for each of the filter's 4 * n_cu workgroups, plus
    `extra` (0 or 64) txns: every workgroup takes four tiles (one per wave),
    or five, so a wave takes a second tile and the compaction a second slot.
    One access per txn; 6 % survive, a few hundred chained."""
    rng = np.random.default_rng(0x961D + 2 * n_cu + extra)
    nb = 4 * (4 * n_cu) * 64 + extra
    pool = _Pool(rng, nb + 4 * P0)
    head, hot = _head(pool, rng, c)
    hb, _ = _finish(head, [], {})
    keys = pool.take(nb).copy()
    at = np.full(nb, RD, np.uint8)
    u = rng.random(nb)
    killed = u >= 0.06
    keys[killed] = hot[rng.integers(0, c, size=int(killed.sum()))]
    at[u < 0.03] = WR  # write survivors; the other survivors are read-only
    n_pairs = 128
    pos = np.sort(rng.choice(nb, size=(2 * n_pairs, 2), replace=False), axis=1)
    x = pool.take(2 * n_pairs)
    kill = np.arange(2 * n_pairs) % 2 == 0       # rows 2q (B aborts) and 2q + 1 (B' commits)
    b_wr = (np.arange(2 * n_pairs) // 2) % 2 == 1  # B a write txn: it stays in the level lists
    keys[pos[:, 0]] = x
    keys[pos[:, 1]] = x
    at[pos[:, 0]] = np.where(kill, WR, RD)
    at[pos[:, 1]] = np.where(b_wr, WR, RD)
    killed[pos.reshape(-1)] = False
    off = np.concatenate([hb.offsets, hb.offsets[-1] + np.arange(1, nb + 1, dtype=np.uint32)]).astype(np.uint32)
    b = EpochBatch(off, np.concatenate([hb.keys, keys]), np.concatenate([hb.acctype, at]))
    surv = ~killed
    facts = {"c": c, "surv": int(surv.sum()), "ro": int((surv & (at != WR)).sum()), "body": nb,
             "pairs": [(int(P0 + pos[2 * q, 1]), int(P0 + pos[2 * q + 1, 1])) for q in range(n_pairs)]}
    assert facts["surv"] <= (P0 + nb) // 4, "level 0 would hand off"
    return b, facts


def tail_seam_case(s, split, c=F_XCAP):
    """Exactly s write txns survive level 0, so the level-1 list is s long
    around p_max(1) whatever the split (with it, read-only survivors are
    sprinkled in and leave the list).  The survivors are chained (k reads what
    k - 1 wrote, restarting every fifth), so level 1 aborts some of them, also
    past its serial range."""
    rng = np.random.default_rng(0x7A11 + 2 * s + split)
    pool = _Pool(rng, 8 * s + 4000)
    head, hot = _head(pool, rng, c)
    chain, prev = [], None
    for k in range(s):
        y = pool.one()
        acc = [(y, WR)] + _cold(pool, int(rng.integers(0, 4)))
        if k % 5 and prev is not None:
            acc.append((prev, RD))
        prev = y
        chain.append(_Txn(acc, ("surv",)))
    items = [chain]
    for _ in range(s // 3):
        length = int(rng.integers(1, 6))
        items.append([_killed(pool, hot[int(rng.integers(c))], length, int(rng.integers(length)))])
    if split:
        items += [[_Txn(_cold(pool, int(rng.integers(1, 4))), ("surv",))] for _ in range(s // 16)]
    b, facts = _finish(head, _interleave(rng, items), {"c": c})
    assert facts["surv"] - facts["ro"] == s
    facts["s"] = s
    return b, facts


def ro_seam_case(r, c=F_XCAP):
    """r read-only survivors among write survivors of the same tiles.  Writer
    W_i commits at level 1 and V_i (which reads what W_i wrote) aborts; a
    read-only txn reading W_i's key after it aborts, one reading V_i's key
    commits, and so does one reading W_i's key before W_i."""
    rng = np.random.default_rng(0x805E + r)
    pool = _Pool(rng, 6000)
    head, hot = _head(pool, rng, c)
    nw = 24
    slots, wk, vk, fw, fv = [], [], [], [], []
    for i in range(nw):
        w, v = pool.one(), pool.one()
        f, g = np.sort(rng.random(2) * 0.7)
        slots.append((f, _Txn([(w, WR)] + _cold(pool, int(rng.integers(0, 4))), ("surv",))))
        slots.append((g, _Txn([(v, WR)] + _cold(pool, int(rng.integers(0, 3))) + [(w, RD)], ("surv",))))
        wk.append(w), vk.append(v), fw.append(f), fv.append(g)
    for q in range(r):
        i, kind = q % nw, q % 4
        acc = _cold(pool, int(rng.integers(0, 4)))
        if kind == 0:    # after its committed writer: aborts
            acc.append((wk[i], RD))
            slots.append((rng.uniform(fw[i], 1.0), _Txn(acc, ("B", q // 4, True))))
        elif kind == 1:  # after a writer that aborts: commits
            acc.append((vk[i], RD))
            slots.append((rng.uniform(fv[i], 1.0), _Txn(acc, ("B", q // 4, False))))
        elif kind == 2:  # before its writer: commits
            acc.append((wk[i], RD))
            slots.append((rng.uniform(0.0, fw[i]), _Txn(acc, ("surv",))))
        else:
            slots.append((rng.random(), _Txn(acc + _cold(pool, 1), ("surv",))))
    for _ in range(3 * SW_T - len(slots) % SW_T + 7):
        length = int(rng.integers(1, 8))
        slots.append((rng.random(), _killed(pool, hot[int(rng.integers(c))], length, int(rng.integers(length)),
                                            WR if rng.random() < 0.3 else RD)))
    slots.sort(key=lambda x: x[0])
    b, facts = _finish(head, [t for _, t in slots], {"c": c})
    assert facts["ro"] == r
    facts["r"] = r
    return b, facts
