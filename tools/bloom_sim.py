#!/usr/bin/env python3
"""CPU simulation of the unit kernel's blocked Bloom filters: the fraction of units of DISTINCT ids that raise a (false)
flag, the way profiles/NOTES.md rounds 10 and 12 quote it.  A unit's ids arrive one by one; each ORs its bits into one
64-bit word and is flagged when all of them were set already.

  bits6    round 10: word = top ten bits of table_hash, six positions from a second multiplicative hash of it
  product  round 12: ONE 32 x 32 -> 64 bit product of the folded id: word = top ten bits of its low half, six positions =
           bits 0..29 of its high half
either on table_hash's fold of Snowflake-like ids (timestamp << 22 | worker << 12 | sequence) or on ideal 32-bit values.

usage: bloom_sim.py [units, default 2000] [ids per unit, default 1264] [seed]
"""
import random
import sys

M32 = 0xFFFFFFFF
K1, K2 = 0x9E3779B1, 0x85EBCA6B


def fold(i):
    x = (i ^ (i >> 32)) & M32
    return x ^ (x >> 15)


def bits6(x):
    """-> (word, mask) of round 10's bloom_bits6 on hv = table_hash(id, 32) (what bloom_product replaced)"""
    hv = (x * K1) & M32
    g = (hv * K2) & M32
    g ^= g >> 13
    lo = (1 << ((g >> 2) & 31)) | (1 << ((g >> 7) & 31)) | (1 << ((g >> 12) & 31))
    hi = (1 << ((g >> 17) & 31)) | (1 << ((g >> 22) & 31)) | (1 << (g >> 27))
    return hv >> 22, (hi << 32) | lo


def product(x):
    """-> (word, mask) of csrc/sann_unit.h bloom_product / bloom_product_bits"""
    p = x * K1
    l, h = p & M32, p >> 32
    lo = (1 << (h & 31)) | (1 << ((h >> 5) & 31)) | (1 << ((h >> 10) & 31))
    hi = (1 << ((h >> 15) & 31)) | (1 << ((h >> 20) & 31)) | (1 << ((h >> 25) & 31))
    return l >> 22, (hi << 32) | lo


def snowflake(rng, n):
    t0 = 1_600_000_000_000
    out = set()
    while len(out) < n:
        ms = t0 + rng.randrange(2 * 86_400_000)
        seq = min(int(rng.expovariate(1.5)), 4095)
        out.add((ms << 22) | (rng.randrange(1024) << 12) | seq)
    out = list(out)
    rng.shuffle(out)
    return out


def flagged_fraction(units, n, scheme, ideal, seed):
    rng = random.Random(seed)
    bad = 0
    for _ in range(units):
        xs = rng.sample(range(1 << 32), n) if ideal else [fold(i) for i in snowflake(rng, n)]
        words = {}
        for x in xs:
            w, m = scheme(x)
            old = words.get(w, 0)
            if old & m == m:
                bad += 1
                break
            words[w] = old | m
    return bad / units


def main():
    units = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1264
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 12
    print("%d units of %d distinct ids, 1024 words of 64 bits; units with a false flag:" % (units, n))
    for name, scheme in (("bits6 (round 10)", bits6), ("product (round 12)", product)):
        print("  %-18s ideal 32-bit values %.2f %%   fold of Snowflake-like ids %.2f %%" % (
            name, 100 * flagged_fraction(units, n, scheme, True, seed), 100 * flagged_fraction(units, n, scheme, False, seed + 1)))


if __name__ == "__main__":
    main()
