"""Keys placed exactly in the persistent row table (csrc/rowtab.h): the two
unit-step probe policies of csrc/dcc_device.h restated in Python with their
inverses, so a test can build keys that share one home slot -- at the table's
last slot (the walk wraps with (h + 1) & mask), 256 of them (ProbeFib's walk
bound MT_WALK at its limit), 257 (one past it) -- at every table size the
test can reach.  Pure numpy / Python ints: no GPU."""
from __future__ import annotations

import numpy as np

from deneva_amd import KEY_RESERVED

M64 = (1 << 64) - 1
FIB = 0x9E3779B97F4A7C15          # ProbeFib: the home is the top `bits` bits of key * FIB
FIB_INV = pow(FIB, -1, 1 << 64)   # odd, so invertible mod 2^64
FMIX_M1, FMIX_M2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53  # fmix64; ProbeMix: fmix64(key) & mask
FMIX_M1_INV, FMIX_M2_INV = pow(FMIX_M1, -1, 1 << 64), pow(FMIX_M2, -1, 1 << 64)
MT_WALK = 256
RT_MIN_BITS = 12
POLICIES = ("fib", "mix")  # maat, tso


def fmix64(k):
    k ^= k >> 33
    k = (k * FMIX_M1) & M64
    k ^= k >> 33
    k = (k * FMIX_M2) & M64
    k ^= k >> 33
    return k


def fmix64_inv(h):
    h ^= h >> 33  # x ^= x >> 33 is its own inverse on 64 bits
    h = (h * FMIX_M2_INV) & M64
    h ^= h >> 33
    h = (h * FMIX_M1_INV) & M64
    h ^= h >> 33
    return h


def home(policy, key, bits):
    """The home slot of `key` in a table of 2^bits slots."""
    key = int(key)
    if policy == "fib":
        return ((key * FIB) & M64) >> (64 - bits)
    assert policy == "mix"
    return fmix64(key) & ((1 << bits) - 1)


def shared_home(policy, h, bits, shared_bits, ext, at_bits):
    """The one home at 2^at_bits slots of keys_with_home(policy, h, bits, ...,
    shared_bits, ext)."""
    e = at_bits - bits
    if policy == "fib":
        return (h << e) | (ext >> (shared_bits - at_bits))
    return h | ((ext & ((1 << e) - 1)) << bits)


def keys_with_home(policy, h, bits, count, shared_bits=None, ext=0, seed=1):
    """`count` distinct keys whose home at 2^bits slots is h and who share one
    home at every table size up to 2^shared_bits: `ext` is the shared_bits -
    bits further bits of the hash that a bigger table looks at (the next lower
    ones of the product for fib, the next higher ones of fmix64 for mix)."""
    shared_bits = bits if shared_bits is None else shared_bits
    assert 0 <= h < (1 << bits) and bits <= shared_bits < 64 and 0 <= ext < (1 << (shared_bits - bits))
    free = 64 - shared_bits
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < count:
        r = int(rng.integers(0, 1 << min(free, 62)))
        if r in seen:
            continue
        seen.add(r)
        if policy == "fib":
            top = (h << (shared_bits - bits)) | ext
            key = (((top << free) | r) * FIB_INV) & M64
        else:
            key = fmix64_inv((r << shared_bits) | (ext << bits) | h)
        if key != KEY_RESERVED:
            out.append(key)
    return np.asarray(out, np.uint64)
