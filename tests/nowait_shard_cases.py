"""Directed epochs for the key-sharded NO_WAIT lock epoch, shared by the CPU
test of the model (test_nowait_shard_ref.py) and the GPU test
(test_gpu_nowait_shard.py).  Rows are picked with `key_shard` so that they
land on the shard a case needs; the expected answers are nowait_ref.replay's.
Each case: (name, txns, held) with held a list of (key, acctype) or None."""
from deneva_amd import RD, WR


def keys_on(key_shard, R, shard, count, start=1000):
    """`count` distinct keys >= start that key_shard puts on `shard` of R."""
    out = []
    k = start
    while len(out) < count:
        if key_shard(k, R) == shard:
            out.append(k)
        k += 1
    return out


def self_conflict_and_live_locks(key_shard, R, with_held):
    """Txn 0 names row A twice (RD then WR) on shard x and takes EX on row B on
    shard y != x: only x sees the abort, y has txn 0's round-1 word on B.
    Txn 1 takes EX on B and commits, txn 2 reads B and aborts at its request."""
    x, y = 0, R - 1
    a, = keys_on(key_shard, R, x, 1)
    b, = keys_on(key_shard, R, y, 1, start=5000)
    t0 = [(a, RD), (a, WR), (b, WR)]
    held = None
    if with_held:  # a row held SH on x in front of the pair: txn 0 still aborts at its own second request
        h, = keys_on(key_shard, R, x, 1, start=9000)
        t0 = [(h, RD)] + t0
        held = [(h, RD)]
    return [t0, [(b, WR)], [(7, RD), (b, RD)]], held


def first_conflict_elsewhere(key_shard, R, mirror):
    """A txn of 5 accesses conflicts at ordinals 1 and 3, on two shards: the
    lower one wins whichever rank has it."""
    s1, s3 = (0, R - 1) if mirror else (R - 1, 0)
    k1, = keys_on(key_shard, R, s1, 1)
    k3, = keys_on(key_shard, R, s3, 1, start=5000)
    return [[(k1, WR), (k3, WR)], [(11, RD), (k1, RD), (12, RD), (k3, RD), (13, RD)]], None


def killed_here_blocked_there(key_shard, R):
    """DESIGN.md §8f's case across ranks.  Txn 3 reads Y (request 0, shard a)
    and X (request 1, shard b).  In round 2 it is killed on X (txn 0 committed
    in round 1) while Y is only blocked by txn 2, which is still undecided
    behind txn 1 and commits in round 3: the request txn 3 aborted at is 0."""
    a, b = 0, R - 1
    y, = keys_on(key_shard, R, a, 1)
    x, = keys_on(key_shard, R, b, 1, start=5000)
    h, q = 20001, 20002
    return [[(h, WR), (x, WR)], [(h, RD), (q, WR)], [(q, WR), (y, WR)], [(y, RD), (x, RD)]], None


def one_shard_only(key_shard, R, n_txn=40):
    """Every row on shard 1: the other ranks have no access at all."""
    ks = keys_on(key_shard, R, 1 % R, 6)
    txns = [[(ks[(t + q) % 6], WR if (t + q) % 5 == 0 else RD) for q in range(t % 4)] for t in range(n_txn)]
    return txns, [(ks[0], RD)]


def directed(key_shard, R):
    out = []
    for with_held in (False, True):
        t, h = self_conflict_and_live_locks(key_shard, R, with_held)
        out.append((f"self_conflict_live_locks_held{int(with_held)}", t, h))
    for mirror in (False, True):
        t, h = first_conflict_elsewhere(key_shard, R, mirror)
        out.append((f"first_conflict_elsewhere_mirror{int(mirror)}", t, h))
    t, h = killed_here_blocked_there(key_shard, R)
    out.append(("killed_here_blocked_there", t, h))
    t, h = one_shard_only(key_shard, R)
    out.append(("one_shard_only", t, h))
    out.append(("one_txn", [[(3, WR), (4, RD)]], None))
    out.append(("zero_lengths", [[], [], []], None))
    out.append(("empty", [], None))
    return out
