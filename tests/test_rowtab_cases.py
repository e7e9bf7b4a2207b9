"""CPU checks of the placed-key builders (rowtab_cases.py): the keys have the
homes they claim at every table size they claim it for, none is reserved, and
the Python home functions are the engine's (their constants and expressions
are read from csrc/dcc_device.h)."""
import os
import re

import numpy as np
import pytest

import rowtab_cases as rc
from deneva_amd import KEY_RESERVED

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deneva_amd", "csrc")


def test_inverses():
    rng = np.random.default_rng(3)
    for x in [0, 1, rc.M64, 1 << 63] + [int(v) for v in rng.integers(0, 1 << 63, size=200)]:
        assert rc.fmix64_inv(rc.fmix64(x)) == x and rc.fmix64(rc.fmix64_inv(x)) == x
        assert (((x * rc.FIB) & rc.M64) * rc.FIB_INV) & rc.M64 == x
    # known values of the murmur3 finaliser
    assert rc.fmix64(0) == 0 and rc.fmix64(1) == 0xB456BCFC34C2CB2C


@pytest.mark.parametrize("policy", rc.POLICIES)
@pytest.mark.parametrize("h,bits,count,shared,ext", [
    (4095, 12, 10, 12, 0),            # the last slot of the minimum table
    (4095, 12, 10, 13, 1),            # ... and still the last slot at 2^13
    (4095, 12, 300, 24, 0xFFF),       # a cluster that no growth up to 2^24 splits
    (4000, 12, 257, 24, 0xABC),       # one home within 255 of the table's end
    (0, 12, 300, 24, 0),
    (77, 12, 300, 31, 12345),
])
def test_keys_have_the_claimed_homes(policy, h, bits, count, shared, ext):
    k = rc.keys_with_home(policy, h, bits, count, shared, ext)
    assert k.size == count and np.unique(k).size == count
    assert not (k == np.uint64(KEY_RESERVED)).any()
    for b in range(bits, shared + 1):
        want = rc.shared_home(policy, h, bits, shared, ext, b)
        assert all(rc.home(policy, x, b) == want for x in k), f"homes differ at 2^{b} slots"
    assert rc.shared_home(policy, h, bits, shared, ext, bits) == h
    if shared < 31:  # a bigger table splits the cluster
        assert len({rc.home(policy, x, shared + 4) for x in k}) > 1
    # other seeds give other keys of the same home
    k2 = rc.keys_with_home(policy, h, bits, count, shared, ext, seed=2)
    assert np.setdiff1d(k2, k).size > 0 and all(rc.home(policy, x, bits) == h for x in k2[:20])


def test_last_slot_stays_last():
    for policy in rc.POLICIES:
        assert rc.shared_home(policy, 4095, 12, 13, 1, 13) == 8191


def test_home_functions_are_the_engine_s():
    src = open(os.path.join(CSRC, "dcc_device.h")).read()
    fib = re.search(r"struct ProbeFib \{.*?\n\};", src, re.S).group(0)
    assert "walk_last = MT_WALK - 1" in fib and "return 1u" in fib
    m = re.search(r"return \(uint32_t\)\(\(key \* (0x[0-9A-Fa-f]+)ull\) >> 32\) >> __builtin_clz\(mask\);", fib)
    assert m, "ProbeFib::home is no longer the top bits of key * constant"
    assert int(m.group(1), 16) == rc.FIB
    mix = re.search(r"struct ProbeMix \{.*?\n\};", src, re.S).group(0)
    assert "walk_last = ~0u" in mix and "return 1u" in mix
    assert "return (uint32_t)fmix64(key) & mask;" in mix
    f = re.search(r"inline uint64_t fmix64\(uint64_t k\) \{(.*?)\n\}", src, re.S).group(1)
    steps = [s.strip() for s in f.strip().split(";") if s.strip()]
    assert steps == ["k ^= k >> 33", "k *= 0x%016xull" % rc.FMIX_M1, "k ^= k >> 33",
                     "k *= 0x%016xull" % rc.FMIX_M2, "k ^= k >> 33", "return k"]
    assert int(re.search(r"constexpr uint32_t MT_WALK = (\d+);", src).group(1)) == rc.MT_WALK
    # the probe loops step with (h + st) & mask and give up after walk_last + 1 slots
    assert src.count("h = (h + st) & mask;") == 2 and src.count("for (uint32_t n = 0; n <= last; n++)") == 2
    rowtab = open(os.path.join(CSRC, "rowtab.h")).read()
    assert int(re.search(r"constexpr uint32_t RT_MIN_BITS = (\d+)", rowtab).group(1)) == rc.RT_MIN_BITS
    # clz(mask) of a 2^bits-slot table is 32 - bits: the home is the product's top `bits` bits
    for bits in (12, 13, 24, 31):
        mask = (1 << bits) - 1
        clz = 32 - mask.bit_length()
        for key in (1, 12345678901234567, rc.M64 - 1):
            assert ((((key * rc.FIB) & rc.M64) >> 32) >> clz) == rc.home("fib", key, bits)
            assert (rc.fmix64(key) & 0xFFFFFFFF) & mask == rc.home("mix", key, bits)
